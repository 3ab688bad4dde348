"""-m gpu: ONE TABLE of dense-GEMM paths, each run on STRIDED operands — the layouts of tests/gemm_strides.py: leading dimensions other than K (and distinct for A, B
and y), windows of wider buffers at bases that are 16-byte but not 128-byte aligned, lda or ldb = 2^23 - 16 (the largest the MFMA tiles admit) and, on the other side
of the bound, the operands that must leave the fast path.  Every byte around an operand's window is the poison code 0x5B, so a row taken at `K` instead of `ld`, A's
leading dimension used for B, or a read past K moves the integer sum.

Each row forces its path with the switch and shape the older files use (test_gpu_epilogue_domain.py, test_gpu_parity.py, test_gpu_k_rotation.py,
test_gpu_int8_exchange.py) and asserts, where the library can tell, that the path is reached WITH THE REAL leading dimensions (pq_gemm_variant_name,
pq_qlinear_workspace_bytes, pq_kslabs_way_name, pq_qlinear_kslabs_workspace_bytes_for).  For each layout the row runs pq.qlinear_s8 for bf16, fp16 and f32 with and
without bias, pq.qlinear_s8_t (the swapped problem: lda and ldb change places) and pq.int_mm; every output goes into a window of a wider buffer (a third leading
dimension, ldy_of(N), at column offset 8) that must stay untouched outside [M, N].  All comparisons are on bits: against the numpy reference (exact product +
Q.epilogue) and against the `contig` call under the same switches.  For outputs of more than 2^20 elements (the tail-split and PQ_FAKE_CUS rows) the contiguous call is held against
numpy and the strided calls against the contiguous call's bits on the device — the same statement, without shipping 90 MB per comparison.

The tail split has no query of its own: pq_gemm_variant_name reports "+ sp128 tail" from tail_split_plan(M, N), and reach rests on that plan for the two shapes —
the launch is two sub-problems whose second pointer is a + lead * lda (or b + lead * ldb).

The 2^23 layouts are 2.5 GB (A, 300 rows) and 4.4 GB (B, 520 rows): they run in functions of their own, one per operand side, and are freed at the end of each.
Layouts left out because the smallest shape of the path is too large for them: limit_* on the two tail-split shapes (2048 x 11008 and 11008 x 2048: 17 and 92 GB)
and on the PQ_FAKE_CUS shapes (rows beyond 300 / 520); no others.

Module level (test_modules_on_strided_codes): qlinear.from_qtensor keeps a strided weight view as it is, and qlinear / FusedQLinear / GatedMLP hand a QTensor whose
int_data is a strided view to the GEMM without a copy; FusedQLinear's constructor concatenates its parts' weights, so ITS weight is always a contiguous copy."""
import numpy as np
import pytest
import torch

from oracle import qspec_numpy as Q
from tests import gemm_strides as S
from tests.gpu_util import TD, same, to_gpu

pytestmark = pytest.mark.gpu

SEED = 11
VARIANT_NAME = {"generic": b"generic64", "sp256_16": b"sp256_16x16x64", "sp128_16": b"sp128x256_16x16x64", "sp128x128": b"sp128x128_16x16x64",
                "ring128": b"ring128_16x16x64", "ring64x128": b"ring64x128_16x16x64", "ring64x64": b"ring64x64_16x16x64", "ring128x160": b"ring128x160_16x16x64",
                "auto": b"ring64x64_16x16x64"}           # (auto at 300 x 520 and at 520 x 300: the mid-M planner's 64 x 64 ring tile on a 256-CU device)
TILE_VARIANTS = ["auto", "sp256_16", "sp128_16", "sp128x128", "ring128", "ring64x128", "ring64x64", "ring128x160"]
TILED = (b"sp256_16x16x64", b"sp128x256_16x16x64", b"ring128_16x16x64")          # qlinear_core's `tiled`: the variants whose shapes the split-K forms take over
DIRECT_MAX = 1 << 20            # outputs up to this many elements go to numpy from every layout


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    from protoquant_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    yield protoquant_amd
    _PROBLEMS.clear()          # (the operands and their placed layouts: nothing of this file stays on the device for the rest of the session)
    torch.cuda.empty_cache()


def _L():
    from protoquant_amd import _lib
    return _lib.lib()


def _ld(t):
    from protoquant_amd import _lib
    return _lib.ld(t)


class GpuProblem:
    """S.build() + its vectors on the device and the SMALL layouts, placed once (the 2^23 layouts are placed and freed by the function that runs them)"""

    def __init__(self, M, N, K):
        self.p = S.build(M, N, K, SEED + M + N + K)
        self.M, self.N, self.K = M, N, K
        self.xg, self.wg = torch.from_numpy(self.p.xs).cuda(), torch.from_numpy(self.p.ws).cuda()
        self.bias_g = {c: to_gpu(self.p.bias[c], c) for c in (0, 1, 2)}
        self._placed = {}

    def placed(self, layout):
        if layout in S.LARGE:
            return S.place(self.p, layout, "cuda")
        if layout not in self._placed:
            self._placed[layout] = S.place(self.p, layout, "cuda")
        return self._placed[layout]


_PROBLEMS = {}


def problem(M, N, K):
    if M * N > 1 << 22:
        return GpuProblem(M, N, K)          # (the tail-split shapes: 90 MB accumulators, built by the one function that uses them)
    if (M, N, K) not in _PROBLEMS:
        _PROBLEMS[(M, N, K)] = GpuProblem(M, N, K)
    return _PROBLEMS[(M, N, K)]


def _iv(t):
    t = t.contiguous()
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def launch_all(pq, gp, pl):
    """the three calls on one placed layout -> {key: result}; outputs in windows of wider buffers, nothing written around them"""
    M, N = gp.M, gp.N
    assert pl.a.stride(1) == 1 and pl.b.stride(1) == 1 and (M == 1 or pl.a.stride(0) == pl.lda) and pl.b.stride(0) == pl.ldb
    out = {"acc": pq.int_mm(pl.a, pl.b)}
    for c in S.CASES:
        code, hb = c
        bias = gp.bias_g[code] if hb else None
        big, win = S.out_window(M, N, TD[code], "cuda")
        y = pq.qlinear_s8(pl.a, gp.xg, pl.b, gp.wg, bias, TD[code], out=win)
        assert y.data_ptr() == win.data_ptr() and S.untouched_outside(big, N), f"{pl.layout} {c}: y wrote outside its window"
        out[("y", c)] = win
        bigt, wint = S.out_window(N, M, TD[code], "cuda")
        pq.qlinear_s8_t(pl.a, gp.xg, pl.b, gp.wg, bias, TD[code], out=wint)
        assert S.untouched_outside(bigt, M), f"{pl.layout} {c}: y^T wrote outside its window"
        out[("yt", c)] = wint
    return out


def check(gp, got, ref, what):
    """got: launch_all() of one layout; ref: that of `contig` under the same switches (None: got IS contig).  Bits against numpy and against ref."""
    direct = gp.M * gp.N <= DIRECT_MAX or ref is None
    for key, t in got.items():
        if direct:
            if key == "acc":
                same(t, gp.p.acc, f"{what} int_mm")
            else:
                kind, c = key
                same(t.contiguous() if kind == "y" else t.t().contiguous(), gp.p.want(c), f"{what} {kind} {c}")
        if ref is not None:
            assert torch.equal(_iv(t), _iv(ref[key])), f"{what} {key}: bits differ from the contiguous call"


def reach_names(gp, pl):
    """pq_gemm_variant_name with the leading dimensions the calls pass: of the problem and of the swapped one pq_qlinear_s8_t computes"""
    lda, ldb = _ld(pl.a), _ld(pl.b)
    assert ldb == pl.ldb and (lda == pl.lda or gp.M == 1)
    L = _L()
    return L.pq_gemm_variant_name(gp.M, gp.N, gp.K, lda, ldb), L.pq_gemm_variant_name(gp.N, gp.M, gp.K, ldb, lda)


def run_layouts(pq, gp, layouts, reach, what, reps=1):
    """contig first (the control: held against numpy), then every layout against numpy and contig; reach(pl) asserts the path for THAT layout's leading dimensions"""
    control = gp.placed("contig")
    reach(control)
    ref = launch_all(pq, gp, control)
    check(gp, ref, None, f"{what} contig")
    for layout in layouts:
        if layout == "contig":
            continue
        pl = gp.placed(layout)
        try:
            for buf, geo in zip(pl.bufs, S.geometry(layout, gp.M, gp.N, gp.K)):
                assert buf.numel() == geo.nbytes
            reach(pl)
            for rep in range(reps):
                check(gp, launch_all(pq, gp, pl), ref, f"{what} {layout} rep {rep}")
        finally:
            if layout in S.LARGE:
                del pl
                torch.cuda.empty_cache()


# ---------------------------------------------------------------- the table: one runner per kind of path; each takes the layouts to run
def run_variant(pq, pq_opt, layouts, variant, K, extra=()):
    """a tile kernel forced by name (or the planner's own at 300 x 520), y and the swapped problem of y^T; K = 5 x 128 is the shortest the asm K-loop takes, 10 and 11
    K-tiles leave the rings at other phases"""
    gp = problem(300, 520, K)
    pq_opt("PQ_FORCE_VARIANT", "" if variant == "auto" else variant)
    for name, value in extra:
        pq_opt(name, value)
    assert _L().pq_qlinear_workspace_bytes(gp.M, gp.N, gp.K) == 0 and _L().pq_qlinear_t_workspace_bytes(gp.M, gp.N, gp.K) == 0, "single pass"

    def reach(pl):
        assert reach_names(gp, pl) == (VARIANT_NAME[variant], VARIANT_NAME[variant]), (variant, pl.layout)
    run_layouts(pq, gp, layouts, reach, f"{variant} {extra} K={K}")


def run_splitk(pq, pq_opt, layouts, M, N, K, force):
    """the two-pass split-K: int32 slabs from the 256 x 256 tile's K-slices (a + ks * K/S inside strided rows), then the reduction pass"""
    gp = problem(M, N, K)
    if force:
        pq_opt("PQ_FORCE_SPLITK", str(force))
        assert _L().pq_qlinear_workspace_bytes(M, N, K) == force * M * N * 4
    else:
        assert _L().pq_gemm_variant_name(M, N, K, K, K).startswith(b"ring64") and _L().pq_qlinear_workspace_bytes(M, N, K) == 0
        pq_opt("PQ_NO_MIDM", "1")
        nbytes = _L().pq_qlinear_workspace_bytes(M, N, K)
        assert nbytes > 0 and nbytes % (M * N * 4) == 0 and nbytes // (M * N * 4) >= 2, "planned as the two-pass split-K (whole int32 slabs of the output)"

    def reach(pl):
        assert reach_names(gp, pl)[0] in TILED, pl.layout
    run_layouts(pq, gp, layouts, reach, f"split-K {force or 'planned'} {M}x{N}x{K}")


def run_fsk(pq, pq_opt, layouts, M, N, K, S_, form):
    """the fused split-K: ticket form, the symmetric exchange, and the cooperative launch with its hand-packed argument array; twice on one workspace"""
    gp = problem(M, N, K)
    pq_opt("PQ_FSK", str(S_))
    if form == "symmetric":
        pq_opt("PQ_FSK_SYMMETRIC", "1")
    elif form == "coop":
        pq_opt("PQ_FSK_COOP", "1")
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    assert _L().pq_qlinear_workspace_bytes(M, N, K) == ((tiles * 4 * (4 if S_ == 4 else 2) + 255) // 256) * 256 + tiles * (S_ - 1) * 256 * 256 * 4

    def reach(pl):
        assert reach_names(gp, pl)[0] in TILED, pl.layout
    run_layouts(pq, gp, layouts, reach, f"fused split-K x{S_} {form} {M}x{N}x{K}", reps=2)


def run_tail(pq, pq_opt, layouts, M, N, K, axis):
    """the tail split: a second launch on the trailing tile columns (b + lead * ldb) or rows (a + lead * lda); y^T is the split on the other axis"""
    gp = problem(M, N, K)

    def reach(pl):
        name, name_t = reach_names(gp, pl)
        assert name.endswith(b"tail (" + axis + b")") and b"tail" in name_t, (name, name_t)
    run_layouts(pq, gp, layouts, reach, f"tail split {M}x{N}x{K}")


def run_fake_cus(pq, pq_opt, layouts, cus, M, N, K):
    """plans made for a smaller device: other tiles, other split points, the fused split-K on other grids"""
    gp = problem(M, N, K)
    pq_opt("PQ_FAKE_CUS", str(cus))
    plain = _L().pq_gemm_variant_name(M, N, K, K, K)
    assert plain != b"generic64"

    def reach(pl):
        assert reach_names(gp, pl)[0] == plain, pl.layout
    run_layouts(pq, gp, layouts, reach, f"PQ_FAKE_CUS={cus} {M}x{N}x{K} ({plain.decode()})")


ROT_SHAPE = (300, 520, 12928)           # 101 K-tiles; N * K >= 6 MiB and three m-tiles of 128 rows: the 128-row tiles rotate (test_gpu_k_rotation.py, _walk)


def run_rotation(pq, pq_opt, layouts, variant, switch, chunk):
    """a forced chunk of the rotated K walk with a short last chunk: the rotation adds ktu * 128 to a base that sits in a strided row"""
    M, N, K = ROT_SHAPE
    gp = problem(M, N, K)
    assert N * K >= (6 << 20) and M > 128 and (K // 128) % chunk != 0 and chunk < K // 128
    pq_opt("PQ_FORCE_VARIANT", variant)
    pq_opt(switch, str(chunk))

    def reach(pl):
        assert reach_names(gp, pl)[0] == VARIANT_NAME[variant], pl.layout
    run_layouts(pq, gp, layouts, reach, f"rotation {variant} {switch}={chunk}")


def run_skinny(pq, pq_opt, layouts, M, stage):
    """the weight-streaming kernel (W + nrow * ldw), staged and unstaged; y^T through EPI_STORE_T"""
    gp = problem(M, 520, 1280)
    if not stage:
        assert M > 1, "const bool stage = opt().skinny_stage && M > 1"
        pq_opt("PQ_SKINNY_STAGE", "0")

    def reach(pl):
        assert reach_names(gp, pl)[0] == b"skinny_16x16x64", pl.layout
    run_layouts(pq, gp, layouts, reach, f"skinny M={M} stage={stage}")


def run_generic(pq, pq_opt, layouts, forced):
    """operands that are not fast-eligible: the generic kernel, also when a tile is forced (pick_variant returns V_GENERIC); the bits are the reference's"""
    gp = problem(300, 520, 1280)
    pq_opt("PQ_FORCE_VARIANT", forced)

    def reach(pl):
        want = b"generic64" if pl.layout in S.GENERIC else VARIANT_NAME[forced or "auto"]
        assert reach_names(gp, pl) == (want, want), pl.layout
        if pl.layout == "odd_base":
            assert pl.a.data_ptr() % 16 == 1
    run_layouts(pq, gp, layouts, reach, f"leaving the fast path, forced {forced!r}")


PWL_A, PWL_B, PW = ("pad", "window", "limit_a"), ("pad", "window", "limit_b"), ("pad", "window")
TABLE = (
    # each tile kernel at 300 x 520 (interior and ragged tiles), 10, 5 and 11 K-tiles: all fast-eligible layouts
    [(f"variant-{v}-K{K}", run_variant, (v, K), S.FAST) for K in (1280, 640, 1408) for v in TILE_VARIANTS + ["generic"]]
    + [(f"sp256_16-2deep-ring-K{K}", run_variant, ("sp256_16", K, (("PQ_SP256_P3", "0"),)), S.FAST) for K in (1280, 640, 1408)]
    # two-pass split-K: forced slices on the asm loop (test_forced_splitk_slices_on_the_asm_loop), one planned shape (test_splitk_bit_identical, PQ_NO_MIDM=1)
    + [("splitk-2x5", run_splitk, (300, 520, 2 * 5 * 128, 2), PWL_A), ("splitk-3x7", run_splitk, (257, 256, 3 * 7 * 128, 3), PWL_A),
       ("splitk-planned", run_splitk, (130, 517, 8192, 0), PWL_A)]
    # fused split-K: S = 2 and 4 in the three forms (test_fused_splitk_matches; S = 4 at 300 x 520 too, five K-tiles per slice: the 2^23 layouts are for N <= 520), 3 slices of 17 K-tiles dealt 6 / 6 / 5 (test_fused_splitk_with_uneven_slices)
    + [(f"fsk-{s}-{form}", run_fsk, (M, N, K, s, form), PWL_B) for (M, N, K, s) in ((300, 520, 2 * 5 * 128, 2), (300, 520, 4 * 5 * 128, 4))
       for form in ("ticket", "symmetric", "coop")]
    + [("fsk-3-uneven-ticket", run_fsk, (300, 300, 17 * 128, 3, "ticket"), PWL_B), ("fsk-2-uneven-coop", run_fsk, (300, 300, 17 * 128, 2, "coop"), PWL_B)]
    # tail split on each axis: the smallest shapes that split on a 256-CU device (test_tail_split_bit_identical)
    + [("tail-N", run_tail, (2048, 11008, 128, b"N"), PW), ("tail-M", run_tail, (11008, 2048, 128, b"M"), PW)]
    # plans for fewer CUs (test_plans_made_for_fewer_cus_stay_bit_exact)
    + [(f"fake-cus-{cus}-{M}x{N}x{K}", run_fake_cus, (cus, M, N, K), PW) for cus in (32, 64) for (M, N, K) in ((1000, 1100, 512), (512, 4096, 1024), (3000, 520, 640))]
    # rotated K walk, one forced chunk per loader / consumer tile (test_gpu_k_rotation.py)
    + [(f"rotation-{v}", run_rotation, (v, sw, ch), PWL_B) for (v, sw, ch) in (("ring128", "PQ_RING_ROT", 5), ("sp128_16", "PQ_RING_ROT", 5), ("ring128x160", "PQ_MIDM_CT", 7),
                                                                               ("ring64x128", "PQ_MIDM_CT", 7), ("ring64x64", "PQ_MIDM_CT", 3))]
    # the weight-streaming kernel
    + [(f"skinny-M{M}", run_skinny, (M, True), PWL_B) for M in (1, 17, 48, 64)]
    + [(f"skinny-unstaged-M{M}", run_skinny, (M, False), PWL_B) for M in (17, 48, 64)]
    # leaving the fast path
    + [(f"generic-forced-{f or 'none'}", run_generic, (f,), ("pad",) + S.GENERIC) for f in ("", "sp256_16")]
)
IDS = [r[0] for r in TABLE]
assert len(set(IDS)) == len(IDS)


def _rows(pick):
    """the rows that list one of `pick`, each with exactly those of its layouts"""
    out = [(r[0], r[1], r[2], tuple(l for l in r[3] if l in pick)) for r in TABLE]
    return [r for r in out if r[3]]


SMALL_ROWS = _rows(S.SMALL + ("ragged_ld", "odd_base"))
A_ROWS, B_ROWS = _rows(("limit_a", "beyond_a")), _rows(("limit_b", "beyond_b"))


@pytest.mark.parametrize("row", SMALL_ROWS, ids=[r[0] for r in SMALL_ROWS])
def test_strided_path(pq, pq_opt, row):
    _, runner, args, layouts = row
    runner(pq, pq_opt, layouts, *args)


@pytest.mark.parametrize("row", A_ROWS, ids=[r[0] for r in A_ROWS])
def test_strided_path_lda_at_the_bound(pq, pq_opt, row):
    """lda = 2^23 - 16 (fast path: 255 rows x lda stays below 2^31 in the loaders' 32-bit offsets) and lda = 2^23 (generic)"""
    _, runner, args, layouts = row
    runner(pq, pq_opt, layouts, *args)


@pytest.mark.parametrize("row", B_ROWS, ids=[r[0] for r in B_ROWS])
def test_strided_path_ldb_at_the_bound(pq, pq_opt, row):
    _, runner, args, layouts = row
    runner(pq, pq_opt, layouts, *args)


# ---------------------------------------------------------------- stacked codes with a strided weight, through the C-ABI
KSLABS = {"ring": (300, 520, 1280, 2, None, "in place: ring64x64"),
          "fsk": (300, 300, 4096, 4, ("PQ_FSK", "2"), "in place: fused split-K x2"),
          "layout": (300, 520, 1280, 2, ("PQ_NO_KSLABS", "1"), "layout pass")}


@pytest.mark.parametrize("b_layout", ["pad", "limit_b"])
@pytest.mark.parametrize("way", list(KSLABS))
def test_stacked_codes_with_a_strided_weight(pq, pq_opt, way, b_layout):
    """pq_qlinear_s8_kslabs in its three ways, padded lda and slab_stride as test_gpu_int8_exchange.py builds them, and B at ldb != K"""
    M, N, K, G, switch, want_way = KSLABS[way]
    gp = problem(M, N, K)
    kps = K // G
    lda, stride = kps + 16, (M + 1) * (kps + 16)
    buf = torch.full((G, M + 1, kps + 16), S.POISON, dtype=torch.int8, device="cuda")
    buf[:, :M, :kps] = torch.from_numpy(gp.p.a).cuda().reshape(M, G, kps).permute(1, 0, 2)
    control = gp.placed("contig")
    if switch:
        pq_opt(*switch)
    ref = {c: pq.qlinear_s8(control.a, gp.xg, control.b, gp.wg, gp.bias_g[c[0]] if c[1] else None, TD[c[0]]) for c in S.CASES}
    for c in S.CASES:
        same(ref[c], gp.p.want(c), f"{way}: qlinear_s8 on the row-major codes {c}")
    pl = gp.placed(b_layout)
    try:
        L = _L()
        ldb = _ld(pl.b)
        assert ldb == pl.ldb != K
        need = L.pq_qlinear_kslabs_workspace_bytes_for(buf.data_ptr(), lda, stride, kps, pl.b.data_ptr(), ldb, M, N, K)
        name = L.pq_kslabs_way_name(buf.data_ptr(), lda, stride, kps, pl.b.data_ptr(), ldb, M, N, K, need).decode()
        assert name == want_way and (need == 0) == (way == "ring"), (name, need)
        if way == "layout":
            assert need == ((M * K + 255) // 256) * 256 + L.pq_qlinear_workspace_bytes(M, N, K)
        wsp = torch.empty((need + 256,), dtype=torch.uint8, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        for c in S.CASES:
            code, hb = c
            for rep in range(2):          # (twice on one workspace: the launcher zeroes its tickets itself)
                big, win = S.out_window(M, N, TD[code], "cuda")
                rc = L.pq_qlinear_s8_kslabs(buf.data_ptr(), lda, stride, kps, gp.xg.data_ptr(), pl.b.data_ptr(), ldb, gp.wg.data_ptr(),
                                            gp.bias_g[code].data_ptr() if hb else None, win.data_ptr(), S.ldy_of(N), code, M, N, K, wsp.data_ptr() if need else None, need, st)
                assert rc == 0, L.pq_last_error()
                torch.cuda.synchronize()
                assert S.untouched_outside(big, N)
                same(win.contiguous(), gp.p.want(c), f"{way} {b_layout} {c} rep {rep}")
                assert torch.equal(_iv(win), _iv(ref[c]))
    finally:
        if b_layout in S.LARGE:
            del pl
            torch.cuda.empty_cache()


# ---------------------------------------------------------------- the one-call entry
@pytest.mark.parametrize("M", [300, 17])
def test_qlinear_dyn_on_a_strided_activation_and_weight(pq, M):
    """pq_qlinear_dyn: x in bf16 at ld_x = K + 24 (the padding holds 32768.0: a read past K would raise the row's amax), the weight in the `pad` layout; against the
    two-call path on contiguous copies and against the numpy oracle"""
    N, K = 520, 1280
    gp = problem(M, N, K)
    pl = gp.placed("pad")
    rng = np.random.default_rng(M)
    x = Q.from_f32((rng.standard_normal((M, K)) * 1.5).astype(np.float32), 0)
    xbuf = torch.full((M, K + 24), 32768.0, dtype=torch.bfloat16, device="cuda")
    xv = xbuf[:, :K]
    xv.copy_(to_gpu(x, 0))
    assert xv.stride(0) == K + 24 and not xv.is_contiguous()
    name = _L().pq_gemm_variant_name(M, N, K, K, _ld(pl.b))          # (the codes K1 writes into the workspace have lda = K)
    assert name == (b"skinny_16x16x64" if M == 17 else b"ring64x64_16x16x64")
    for hb in (False, True):
        bias = gp.bias_g[0] if hb else None
        y = pq.qlinear_dyn(xv, pl.b, gp.wg, bias)
        xq = pq.quantize(xv.contiguous())
        y2 = pq.qlinear_s8(xq.int_data, xq.scale, gp.placed("contig").b, gp.wg, bias, torch.bfloat16)
        assert torch.equal(_iv(y), _iv(y2)), f"bias={hb}: differs from the two-call path on contiguous copies"
        want, _, _, _ = Q.qlinear(x, 0, gp.p.b, gp.p.ws, gp.p.bias[0] if hb else None)
        same(y, want, f"qlinear_dyn M={M} bias={hb}")
    assert bool((xbuf[:, K:] == 32768.0).all())


# ---------------------------------------------------------------- module level
def test_modules_on_strided_codes(pq):
    """qlinear.from_qtensor keeps a strided weight view (no copy); qlinear, FusedQLinear and GatedMLP take a QTensor whose int_data is a strided view without copying it
    (reshape(-1, K) of a 2-D tensor is the tensor itself, row_major_2d admits stride(0) > K).  FusedQLinear's constructor concatenates its parts' weights: its own
    weight is always a contiguous copy.  Every result equals the same module on contiguous tensors, and the plain qlinear the numpy reference."""
    from protoquant_amd.qtensor import QTensor
    bf = torch.bfloat16
    gp = problem(300, 520, 1280)
    M, N, K = gp.M, gp.N, gp.K
    pl, ct = gp.placed("pad"), gp.placed("contig")

    def qt(codes, scale):
        return QTensor(codes, scale, 1, bf, torch.Size(tuple(codes.shape)))
    m_s = pq.qlinear.from_qtensor(qt(pl.b, gp.wg), gp.bias_g[0])
    m_c = pq.qlinear.from_qtensor(qt(ct.b, gp.wg), gp.bias_g[0])
    assert m_s.wq.data_ptr() == pl.b.data_ptr() and m_s.wq.stride() == (pl.ldb, 1), "from_qtensor copied the strided weight"
    x_s, x_c = qt(pl.a, gp.xg), qt(ct.a, gp.xg)
    assert x_s.int_data.reshape(-1, K).data_ptr() == pl.a.data_ptr() and x_s.int_data.reshape(-1, K).stride() == (pl.lda, 1), "the module's reshape copies"
    y = m_s(x_s)
    same(y, gp.p.want((0, True)), "qlinear(strided weight)(strided QTensor)")
    for a, b in ((m_s, x_c), (m_c, x_s), (m_c, x_c)):
        assert torch.equal(_iv(a(b)), _iv(y))
    xf = (torch.randn(M, K, generator=torch.Generator().manual_seed(3)) * 1.5).to(bf).cuda()          # a float input: qlinear_dyn with the strided weight
    assert torch.equal(_iv(m_s(xf)), _iv(m_c(xf)))
    # FusedQLinear: two projections that share the input
    f_s = pq.FusedQLinear([pq.qlinear.from_qtensor(qt(pl.b[:256], gp.wg[:256])), pq.qlinear.from_qtensor(qt(pl.b[256:], gp.wg[256:]))])
    assert f_s.wq.is_contiguous() and torch.equal(f_s.wq, ct.b), "FusedQLinear holds a contiguous copy of its parts' weights"
    o_s, o_c = f_s(x_s), f_s(x_c)
    assert all(torch.equal(_iv(s_), _iv(c_)) for s_, c_ in zip(o_s, o_c))
    same(torch.cat(o_s, dim=1), gp.p.want((0, False)), "FusedQLinear(strided QTensor)")
    # GatedMLP: gate / up [384, 256] fused, down [256, 384] as a strided view; the input a strided QTensor [300, 256]
    H, I = 256, 384
    g = torch.Generator().manual_seed(9)
    gu = torch.randint(-128, 128, (2 * I, H), generator=g, dtype=torch.int8).cuda()
    dn = torch.randint(-128, 128, (H, I), generator=g, dtype=torch.int8)
    dbuf = torch.full((H, I + 48), S.POISON, dtype=torch.int8, device="cuda")
    dbuf[:, :I] = dn.cuda()
    s_gu, s_dn = (torch.rand(2 * I, generator=g) * 0.01 + 1e-4).cuda(), (torch.rand(H, generator=g) * 0.01 + 1e-4).cuda()
    gate_up = pq.FusedQLinear([pq.qlinear.from_qtensor(qt(gu[:I], s_gu[:I])), pq.qlinear.from_qtensor(qt(gu[I:], s_gu[I:]))])
    mlp_s = pq.GatedMLP(gate_up, pq.qlinear.from_qtensor(qt(dbuf[:, :I], s_dn)))
    mlp_c = pq.GatedMLP(gate_up, pq.qlinear.from_qtensor(qt(dn.cuda(), s_dn)))
    assert mlp_s.down.wq.stride() == (I + 48, 1)
    xbuf = torch.full((M, H + 16), S.POISON, dtype=torch.int8, device="cuda")
    xq = torch.randint(-128, 128, (M, H), generator=g, dtype=torch.int8).cuda()
    xbuf[:, :H] = xq
    xs = (torch.rand(M, generator=g) * 0.1 + 1e-3).cuda()
    y_s = mlp_s(qt(xbuf[:, :H], xs))
    assert y_s.shape == (M, H) and bool(torch.isfinite(y_s.float()).all())
    assert torch.equal(_iv(y_s), _iv(mlp_c(qt(xq, xs)))) and torch.equal(_iv(y_s), _iv(mlp_s(qt(xq, xs))))
