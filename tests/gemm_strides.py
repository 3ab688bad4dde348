"""Operand LAYOUTS for the dense int8 GEMM entries (tests/test_gpu_gemm_strides.py, tests/test_gemm_strides_host.py): the same a[M, K], b[N, K] placed in backing buffers
with leading dimensions other than K, at bases that are 16-byte but not 128-byte aligned, and at the two sides of the fast path's bound lda, ldb < 2^23.

Every byte of a backing buffer outside its [rows, K] window holds the POISON code 0x5B (91): a read past K, or of a wrong row, moves the integer sum.  Nothing here
needs a GPU at import; place() builds the buffers on whatever device it is given (the host test uses the CPU for the small layouts and geometry() alone for the large).

| layout    | A                                                             | B                                                                |
| contig    | lda = K                                                       | ldb = K                                                           (the control)
| pad       | lda = K + 16                                                  | ldb = K + 48                      (distinct; neither a multiple of 128)
| window    | rows 2.., columns [48, 48 + K) of an [M + 3, K + 176] buffer  | rows 1.., columns [16, 16 + K) of an [N + 1, 2 K + 16] buffer
| limit_a   | lda = 2^23 - 16 (the largest the MFMA tiles admit)            | ldb = K + 16
| limit_b   | lda = K + 16                                                  | ldb = 2^23 - 16
| beyond_a  | lda = 2^23 (the planner must pick the generic kernel)         | ldb = K + 16
| beyond_b  | lda = K + 16                                                  | ldb = 2^23
| ragged_ld | lda = K + 8 (not a multiple of 16: generic)                   | ldb = K + 16
| odd_base  | columns [1, 1 + K) of an [M, K + 17] buffer (generic)         | as pad

(window, A: column 48, not 32 — with K a multiple of 64 the offset 2 (K + 176) + 32 = 2 K + 384 is a multiple of 128, and the layout exists for a base that is NOT.)

The limit_* / beyond_* buffers are (rows - 1) * ld + K bytes: 2.5 GB for 300 rows, 4.4 GB for 520.  They are for M <= 300 and N <= 520 only (MAX_M, MAX_N): one
torch.empty, one fill_ with the poison, one strided copy of the window."""
import collections

import numpy as np

from oracle import qspec_numpy as Q

POISON = 0x5B
LIMIT = (1 << 23) - 16          # gemm_fast_eligible: lda, ldb < 2^23 and multiples of 16
BEYOND = 1 << 23
MAX_M, MAX_N = 300, 520         # the large layouts are sized for these
SMALL = ("contig", "pad", "window")
FAST = SMALL + ("limit_a", "limit_b")                         # fast-eligible: the MFMA tiles (and the weight-streaming kernel) run
GENERIC = ("beyond_a", "beyond_b", "ragged_ld", "odd_base")   # not eligible: pick_variant returns the generic kernel
LAYOUTS = FAST + GENERIC
LARGE = ("limit_a", "limit_b", "beyond_a", "beyond_b")
CASES = [(code, hb) for code in (0, 1, 2) for hb in (False, True)]
SENTINEL = 7.0                  # what an output buffer holds before the call

Geo = collections.namedtuple("Geo", "nbytes ld offset")        # one operand: bytes of the backing buffer, leading dimension, byte offset of element [0, 0]


def _flat(rows, K, ld, offset=0):
    return Geo(offset + (rows - 1) * ld + K, ld, offset)


def geometry(layout, M, N, K):
    """(Geo of A, Geo of B) — pure arithmetic"""
    if layout in LARGE:
        assert M <= MAX_M and N <= MAX_N, "the 2^23 layouts are a few GB at 300 x 520: not for larger operands"
    pad_a, pad_b = Geo(M * (K + 16), K + 16, 0), Geo(N * (K + 48), K + 48, 0)
    small = Geo(M * (K + 16), K + 16, 0), Geo(N * (K + 16), K + 16, 0)
    return {
        "contig": (Geo(M * K, K, 0), Geo(N * K, K, 0)),
        "pad": (pad_a, pad_b),
        "window": (Geo((M + 3) * (K + 176), K + 176, 2 * (K + 176) + 48), Geo((N + 1) * (2 * K + 16), 2 * K + 16, (2 * K + 16) + 16)),
        "limit_a": (_flat(M, K, LIMIT), small[1]),
        "limit_b": (small[0], _flat(N, K, LIMIT)),
        "beyond_a": (_flat(M, K, BEYOND), small[1]),
        "beyond_b": (small[0], _flat(N, K, BEYOND)),
        "ragged_ld": (Geo(M * (K + 8), K + 8, 0), small[1]),
        "odd_base": (Geo(M * (K + 17), K + 17, 1), pad_b),
    }[layout]


def ldy_of(cols):
    """the leading dimension of an output window [rows, cols] at column offset 8 of a wider buffer: 16-byte aligned rows for 2- and 4-byte elements (the staged epilogue
    still runs), N + 24 for N a multiple of 8"""
    return -(-cols // 8) * 8 + 24


class Problem:
    """build(): full-range codes (-128 included), finite positive scales, a bias per output type, the exact int32 product and the six references"""

    def __init__(self, M, N, K, seed):
        rng = np.random.default_rng(seed)
        self.M, self.N, self.K = M, N, K
        self.a = rng.integers(-128, 128, (M, K), dtype=np.int8)
        self.b = rng.integers(-128, 128, (N, K), dtype=np.int8)
        self.a[0, 0] = self.b[0, 0] = -128
        self.xs = (rng.random(M, dtype=np.float32) * 0.1 + 1e-3).astype(np.float32)
        self.ws = (rng.random(N, dtype=np.float32) * 0.01 + 1e-4).astype(np.float32)
        self.bias = {c: Q.from_f32(rng.standard_normal(N).astype(np.float32), c) for c in (0, 1, 2)}
        self.acc = reference_acc(self.a, self.b)
        self._want = {}

    def want(self, case):
        if case not in self._want:
            code, hb = case
            self._want[case] = Q.epilogue(self.acc, self.xs, self.ws, self.bias[code] if hb else None, code)
        return self._want[case]


def build(M, N, K, seed):
    return Problem(M, N, K, seed)


def reference_acc(a, b):
    """the exact product: float64 BLAS on integers (|acc| <= 128 * 128 * K < 2^53), as the parity tests compute it; a and b may be strided views"""
    assert 128 * 128 * a.shape[1] < 2 ** 53
    return (a.astype(np.float64) @ b.astype(np.float64).T).astype(np.int64).astype(np.int32)


Placed = collections.namedtuple("Placed", "layout a b lda ldb bufs")      # a, b: the views the GEMM is given; lda, ldb: stride(0); bufs: the flat backing buffers


def _place_one(x, geo, device):
    import torch
    rows, K = x.shape
    buf = torch.empty((geo.nbytes,), dtype=torch.int8, device=device)
    buf.fill_(POISON)
    view = torch.as_strided(buf, (rows, K), (geo.ld, 1), geo.offset)
    view.copy_(torch.from_numpy(x).to(device))
    return buf, view


def place(p, layout, device):
    ga, gb = geometry(layout, p.M, p.N, p.K)
    ba, va = _place_one(p.a, ga, device)
    bb, vb = _place_one(p.b, gb, device)
    return Placed(layout, va, vb, ga.ld, gb.ld, (ba, bb))


def out_window(rows, cols, dtype, device):
    """(whole buffer, the [rows, cols] window at column offset 8 with leading dimension ldy_of(cols)), pre-filled with SENTINEL"""
    import torch
    big = torch.full((rows, ldy_of(cols)), SENTINEL, dtype=dtype, device=device)
    return big, big[:, 8:8 + cols]


def untouched_outside(big, cols):
    return bool((big[:, :8] == SENTINEL).all()) and bool((big[:, 8 + cols:] == SENTINEL).all())
