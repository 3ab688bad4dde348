"""The EDGE SWEEP of the dense int8 GEMM kernels (tests/test_gpu_gemm_edges.py, tests/test_gemm_edges_host.py): tables of shapes, the window reference, the output
buffers and their comparison.  Nothing here needs a GPU.

The window reference.  y[m, n] depends only on row m of A, row n of B, xs[m], ws[n] and bias[n]: ONE problem a[Mmax, Kmax], b[Nmax, Kmax] per tile geometry serves every
shape (M, N) of the sweep — the problem (M, N) is the prefix views a[:M], b[:N], xs[:M], ws[:N], bias[:N], its expected output the top-left window of the full one.  A K
sweep takes a[:, :K], b[:, :K] with lda = ldb = Kmax and one exact product per K.  Two operand patterns (tests/test_gpu_k_rotation.py): "full" — the whole int8 range,
-128 included — and "ktile" — activation codes that grow with the index of the K-tile (for the weight-streaming kernel: of the 64-byte k-step) against positive weights, so
that a skipped or revisited step moves every sum of its row and cannot cancel.

Output placement.  Every output is a window of a larger buffer filled with POISON bits no expected output can hold (a NaN payload for the float kinds, 0x5B5B5B5B for
int32): at least one row above and below, at least 8 elements left and right.  The WHOLE buffer is compared against an expected buffer (poison fill + one slice copy);
first_bad() names the first differing element in window coordinates, the margin included.

The shape tables.  Part 1: every forced tile (TILE: (TM, TN) read from the launchers — launch_gemm_fast<OUT, TM, TN>, launch_gemm_ring128 (128 x 128), launch_gemm_ringt
(64 x 128, 64 x 64, 128 x 160), gemm_s8_generic.hip's GT = 64) and the forms behind PQ_SP256_P3=0, PQ_RING_LC=0, PQ_SP128_LC=0.  Every tile picks its epilogue per wave
QUARTER ((wm0 + TM/2 <= M) && (wn0 + TN/2 <= N) && ...), so the edges sit at multiples of half a tile: edge_set(T) = {1, 15, 16, 17} + {k T/2 + d: k = 1..4, d = -1, 0, 1}
+ {T + 1 .. T + 16} (every residue mod 16 as the size of a last tile).  Part 2: the split-K forms on the 256-tile sets.  Part 3: the weight-streaming kernel's K split.

skinny_plan() / skinny_walk() below RESTATE host and device arithmetic of protoquant_amd/csrc/gemm_s8_skinny.hip.  They are COVERAGE BOOKKEEPING ONLY: they prove that the
tables reach the states they claim to reach, and never produce an expected value."""
import collections
import functools

import numpy as np

from oracle import qspec_numpy as Q

# ---------------------------------------------------------------- kinds, poison, output layouts
Kind = collections.namedtuple("Kind", "name code bias entry")      # entry: "y" pq_qlinear_s8, "acc" pq_gemm_s8s8s32, "yt" pq_qlinear_s8_t (the output is [N, M])
BF16_B, FP16, F32_B, I32, BF16_BT = (Kind("bf16+bias", 0, True, "y"), Kind("fp16", 1, False, "y"), Kind("f32+bias", 2, True, "y"), Kind("int32", None, False, "acc"),
                                     Kind("bf16+bias^T", 0, True, "yt"))
KINDS = (BF16_B, FP16, F32_B, I32, BF16_BT)
ITEM = {0: 2, 1: 2, 2: 4, None: 4}                                  # bytes per output element
# NaN payloads (sign 0, exponent all ones, a mantissa that no arithmetic NaN and no rounding produces) and, for int32, a value beyond |acc| <= 128 * 128 * Kmax
POISON = {0: 0x7FDB, 1: 0x7EDB, 2: 0x7FDB5B5B, None: 0x5B5B5B5B}
OPERAND_POISON = 0x5B                                               # int8 margins of the operands (and every other byte of a test's arena)
MODES = ("contig", "ld8")

Layout = collections.namedtuple("Layout", "rows cols ld offset total")      # in elements: the window [rows, cols] at `offset` of a flat buffer of `total`


def _up8(v):
    return -(-v // 8) * 8


def layout(rows, cols, mode):
    """contig: ldy = cols (rows that are not 16-byte aligned when cols is ragged) at a 16-byte aligned base, a row + 8 elements of margin before and after;
    ld8: ldy a multiple of 8, rows 1 .. rows at column 8 of a [rows + 2, ldy] buffer (16-byte aligned base and rows for 2- and 4-byte elements)"""
    if mode == "contig":
        pre = _up8(cols + 8)
        return Layout(rows, cols, cols, pre, pre + rows * cols + cols + 8)
    assert mode == "ld8"
    ld = _up8(cols) + 16
    return Layout(rows, cols, ld, ld + 8, (rows + 2) * ld)


def bits_dtype(code):
    return np.uint16 if ITEM[code] == 2 else np.uint32


def expected_buffer(window, lay, code):
    """poison fill + one slice copy (numpy; the GPU test builds the same on the device)"""
    assert window.shape == (lay.rows, lay.cols)
    buf = np.full(lay.total, POISON[code], bits_dtype(code))
    np.lib.stride_tricks.as_strided(buf[lay.offset:], (lay.rows, lay.cols), (lay.ld * buf.itemsize, buf.itemsize))[...] = window
    return buf


Bad = collections.namedtuple("Bad", "row col inside got want count")


def first_bad(got, want, lay):
    """None, or the first differing element of the two flat buffers in WINDOW coordinates (row < 0, row >= rows or col >= cols: the margin)"""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape == (lay.total,) and got.dtype == want.dtype
    idx = np.flatnonzero(got != want)
    if idx.size == 0:
        return None
    row, col = divmod(int(idx[0]) - lay.offset, lay.ld)
    return Bad(row, col, 0 <= row < lay.rows and col < lay.cols, int(got[idx[0]]), int(want[idx[0]]), int(idx.size))


def describe(bad, variant, kind, M, N, K, extra=""):
    where = "element" if bad.inside else "MARGIN element"
    return (f"{variant} {kind.name} M={M} N={N} K={K} {extra}: {bad.count} elements of the buffer differ, first at {where} [{bad.row}, {bad.col}]"
            f" (got 0x{bad.got:X}, want 0x{bad.want:X})")


# ---------------------------------------------------------------- the window reference
class Problem:
    def __init__(self, Mmax, Nmax, Kmax, pattern, kstep=128):
        rng = np.random.default_rng([Mmax, Nmax, Kmax, kstep, len(pattern)])
        self.Mmax, self.Nmax, self.Kmax, self.pattern = Mmax, Nmax, Kmax, pattern
        if pattern == "full":
            self.a = rng.integers(-128, 128, (Mmax, Kmax), dtype=np.int8)
            self.b = rng.integers(-128, 128, (Nmax, Kmax), dtype=np.int8)
            self.a[:, 0] = -128          # (column 0 is in every K prefix: every row of every problem holds the code -128 on both sides)
            self.b[:, 0] = -128
        else:
            assert pattern == "ktile"
            k = np.arange(Kmax)
            self.a = ((k // kstep) % 120 + 1 + (np.arange(Mmax) % 7)[:, None]).astype(np.int8)
            self.b = (1 + (np.arange(Nmax)[:, None] + k) % 5).astype(np.int8)
        self.xs = (rng.random(Mmax, dtype=np.float32) * 0.1 + 1e-3).astype(np.float32)
        self.ws = (rng.random(Nmax, dtype=np.float32) * 0.01 + 1e-4).astype(np.float32)
        self.bias = {c: Q.from_f32(rng.standard_normal(Nmax).astype(np.float32), c) for c in (0, 1, 2)}
        self._acc, self._want = {}, {}

    def acc(self, K=None):
        K = K or self.Kmax
        if K not in self._acc:
            self._acc[K] = Q.gemm_s8s8s32(self.a[:, :K], self.b[:, :K])
        return self._acc[K]

    def epilogue(self, acc, kind):
        """the bits of one output kind for a given accumulator, in the orientation of its entry"""
        if kind.code is None:
            return acc.view(np.uint32)
        y = Q.epilogue(acc, self.xs, self.ws, self.bias[kind.code] if kind.bias else None, kind.code)
        y = y.view(np.uint32) if kind.code == 2 else y
        return np.ascontiguousarray(y.T) if kind.entry == "yt" else y

    def want(self, kind, K=None):
        """the full expected output [Mmax, Nmax] ([Nmax, Mmax] for the transposed entry) as bit patterns; the problem (M, N) takes its top-left window"""
        K = K or self.Kmax
        if (kind, K) not in self._want:
            self._want[(kind, K)] = self.epilogue(self.acc(K), kind)
        return self._want[(kind, K)]

    def window(self, kind, M, N, K=None):
        w = self.want(kind, K)
        return w[:N, :M] if kind.entry == "yt" else w[:M, :N]


@functools.lru_cache(maxsize=8)
def problem(Mmax, Nmax, Kmax, pattern, kstep=128):
    return Problem(Mmax, Nmax, Kmax, pattern, kstep)


# ---------------------------------------------------------------- Part 1: every tile, every edge
TILE = {"generic": (64, 64), "sp256_16": (256, 256), "sp128_16": (128, 256), "sp128x128": (128, 128), "ring128": (128, 128), "ring64x128": (64, 128),
        "ring64x64": (64, 64), "ring128x160": (128, 160)}
DISPLAY = {"generic": b"generic64", "sp256_16": b"sp256_16x16x64", "sp128_16": b"sp128x256_16x16x64", "sp128x128": b"sp128x128_16x16x64", "ring128": b"ring128_16x16x64",
           "ring64x128": b"ring64x128_16x16x64", "ring64x64": b"ring64x64_16x16x64", "ring128x160": b"ring128x160_16x16x64", "skinny": b"skinny_16x16x64"}
Form = collections.namedtuple("Form", "id variant switches")
FORMS = tuple(Form(v, v, ()) for v in TILE) + (Form("sp256_16-P3=0", "sp256_16", (("PQ_SP256_P3", "0"),)), Form("ring128-LC=0", "ring128", (("PQ_RING_LC", "0"),)),
                                                Form("sp128_16-LC=0", "sp128_16", (("PQ_SP128_LC", "0"),)))
K_EDGE = 640                                    # five K-tiles: one more than the four-slot rings, more than the 256-tile's 3 / 2-deep split rings
KT_COUNTS = tuple(range(1, 10)) + (13,)        # K = 128 n as K-prefix views of operands with lda = ldb = KT_LD
KT_LD = 1664
# (output mode, PQ_EPI_ANY_ALIGN): contiguous rows, 16-byte aligned rows, and the contiguous rows again where the staged epilogue is confined to aligned ones
OUT_MODES = (("contig", ""), ("ld8", ""), ("contig", "0"))


def half_tile_set(T):
    return sorted({k * T // 2 + d for k in (1, 2, 3, 4) for d in (-1, 0, 1)})


def edge_set(T):
    return sorted({1, 15, 16, 17} | set(half_tile_set(T)) | set(range(T + 1, T + 17)))


def edge_pairs(TM, TN):
    """the required pairs: every M of the set against N in {TN, TN + 5}, every N against M in {TM, TM + 3}, and the corner block (TM + {1, 8, 15}) x (TN + 1 .. 16)"""
    p = {(M, N) for M in edge_set(TM) for N in (TN, TN + 5)} | {(M, N) for N in edge_set(TN) for M in (TM, TM + 3)}
    p |= {(TM + i, TN + j) for i in (1, 8, 15) for j in range(1, 17)}
    return sorted(p)


def kt_shapes(TM, TN):
    """(fully staged, ragged): every wave quarter of every tile inside the output; a last tile of 3 rows and 5 columns on each axis"""
    return ((2 * TM, 2 * TN), (TM + 3, TN + 5))


def edge_extent(TM, TN):
    return 2 * TM + 1, 2 * TN + 1


# ---------------------------------------------------------------- Part 2: the split-K forms (256 x 256 tile; M > 64, forced_variant() == V_AUTO: qlinear_core's `tiled`)
SPLIT_FORMS = (Form("splitk-2", None, (("PQ_FORCE_SPLITK", "2"),)), Form("splitk-4", None, (("PQ_FORCE_SPLITK", "4"),)),
               Form("fsk-2-ticket", None, (("PQ_FSK", "2"),)), Form("fsk-4-ticket", None, (("PQ_FSK", "4"),)),
               Form("fsk-2-symmetric", None, (("PQ_FSK", "2"), ("PQ_FSK_SYMMETRIC", "1"))), Form("fsk-4-symmetric", None, (("PQ_FSK", "4"), ("PQ_FSK_SYMMETRIC", "1"))))
K_SPLIT = 2560                                  # twenty K-tiles: five per slice under PQ_FSK=4
SPLIT_MODES = ("contig", "ld8")


def split_pairs():
    """+-1 around each half-tile multiple of the 256-tile on both axes (against a full tile and a ragged one on the other axis) and the sixteen-residue corner block"""
    h = half_tile_set(256)
    p = {(M, N) for M in h for N in (256, 261)} | {(M, N) for N in h for M in (256, 259)} | {(256 + i, 256 + j) for i in (1, 8, 15) for j in range(1, 17)}
    return sorted(p)


# ---------------------------------------------------------------- Part 3: the weight-streaming kernel
SK_KT = tuple(range(1, 21)) + (43, 86)          # K / 128
SK_KMAX = 86 * 128
SK_M = (1, 9, 17, 33, 49, 64)
SK_N = 37
SK_KS = ("", "1", "2", "4", "8", "16")
SK_RB = ("", "1", "2")
SK_STAGE = ("", "0")
SK_KINDS = (I32, BF16_B)
SK_EDGE_M = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
SK_EDGE_N = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 37)
SK_EDGE_RB = ("", "2")


def token_tiles(M):
    return (M + 15) // 16


# COVERAGE BOOKKEEPING ONLY — a restatement of protoquant_amd/csrc/gemm_s8_skinny.hip, never a source of expected values:
#   sk_batch      line 19          k-steps per batch
#   skinny_plan   lines 224 - 243  (RB, KS) of a launch, PQ_SKINNY_RB / PQ_SKINNY_KS
#   staged        line 253         const bool stage = opt().skinny_stage && M > 1
#   skinny_walk   line 40 (a wave's slice s0 .. s1 of the K / 64 steps), lines 106 - 143 (whole batches; RB == 1: the two-register-set loop whose exits depend on the
#                 parity of the batch count), lines 144 - 154 (the step-by-step tail)
def sk_batch(mt, rb):
    return (4 if mt == 1 else 2) if rb == 1 else (4 if mt * rb == 2 else 2)


def skinny_plan(M, N, K, force_rb=0, force_ks=0):
    mt = token_tiles(M)
    rb, min_ks, target = 1, 1, 4096
    if mt <= 2:
        if M == 1:
            min_ks = 4
        elif N <= 4096:
            target, min_ks = 2048, 2
        elif N < 16384:
            rb, target, min_ks = 2, 768, 2
        else:
            target, min_ks = 1, (4 if M <= 8 else 2)
    if force_rb and mt <= 2:
        rb = force_rb
    blocks, steps = (N + 16 * rb - 1) // (16 * rb), K // 64
    ks = 1
    while ks < 16 and (blocks * ks < target or ks < min_ks) and steps // (ks * 2) >= sk_batch(mt, rb):
        ks <<= 1
    if force_ks > 0:
        ks = 1
        while ks < force_ks and ks < 16 and steps // (ks * 2) >= 1:
            ks <<= 1
    return rb, ks


Walk = collections.namedtuple("Walk", "mt rb ks staged waves")      # waves: (batches, tail steps) of each wave of a workgroup


def skinny_walk(M, N, K, rb_opt="", ks_opt="", stage_opt=""):
    rb, ks = skinny_plan(M, N, K, int(rb_opt or 0), int(ks_opt or 0))
    mt, steps = token_tiles(M), K // 64
    u = sk_batch(mt, rb)
    waves = []
    for w in range(ks):
        s0, s1 = steps * w // ks, steps * (w + 1) // ks
        waves.append(((s1 - s0) // u, (s1 - s0) % u))
    return Walk(mt, rb, ks, stage_opt != "0" and M > 1, tuple(waves))


def batch_class(batches):
    return "tail only" if batches == 0 else "one batch" if batches == 1 else "even >= 2" if batches % 2 == 0 else "odd >= 3"
