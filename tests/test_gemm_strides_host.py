"""CPU: the operand layouts of tests/gemm_strides.py are what their table says before a kernel sees them; the planner's side of the leading-dimension contract
(include/pq_hip.h, "Operands of the dense GEMM entries") with PQ_FAKE_CUS=256 set, so that no device is asked; and the dense entries refuse lda < K, ldb < K and
ldy < N with PQ_ERR_BAD_ARG and their own name in pq_last_error() before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch

from tests import gemm_strides as S

SHAPES = [(5, 7, 128), (33, 18, 256), (1, 20, 128)]
PQ_ERR_BAD_ARG = 1


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def problem(request):
    return S.build(*request.param, seed=3)


# ---------------------------------------------------------------- the layout builder
def test_builder_is_deterministic_and_full_range(problem):
    q = S.build(problem.M, problem.N, problem.K, seed=3)
    assert np.array_equal(q.a, problem.a) and np.array_equal(q.b, problem.b) and np.array_equal(q.xs.view(np.uint32), problem.xs.view(np.uint32))
    assert problem.a.min() == -128 and problem.b.min() == -128
    assert (problem.xs > 0).all() and (problem.ws > 0).all() and np.isfinite(problem.xs).all() and np.isfinite(problem.ws).all()
    assert np.array_equal(problem.acc.astype(np.int64), problem.a.astype(np.int64) @ problem.b.astype(np.int64).T)


@pytest.mark.parametrize("layout", [l for l in S.LAYOUTS if l not in S.LARGE])
def test_window_holds_the_operands_and_everything_else_is_poison(problem, layout):
    p = problem
    pl = S.place(p, layout, "cpu")
    ga, gb = S.geometry(layout, p.M, p.N, p.K)
    for x, view, buf, geo, ld in ((p.a, pl.a, pl.bufs[0], ga, pl.lda), (p.b, pl.b, pl.bufs[1], gb, pl.ldb)):
        rows, K = x.shape
        assert buf.numel() == geo.nbytes and ld == geo.ld and view.stride() == (ld, 1) and view.shape == (rows, K)
        assert view.data_ptr() - buf.data_ptr() == geo.offset and geo.offset + (rows - 1) * ld + K <= geo.nbytes
        assert np.array_equal(view.numpy(), x)
        flat = buf.numpy().copy()
        mask = np.ones(flat.shape, bool)
        for r in range(rows):
            mask[geo.offset + r * ld: geo.offset + r * ld + K] = False
        assert (flat[mask] == S.POISON).all() and int(mask.sum()) == geo.nbytes - rows * K
        if layout != "contig":
            assert mask.any(), "a strided layout has bytes outside its window"
    # the reference on the strided numpy views equals the reference on the contiguous copies
    assert np.array_equal(S.reference_acc(pl.a.numpy(), pl.b.numpy()), p.acc)
    # the poison can tell: the same window read with K for the leading dimension (rows > 1), or one column late, is another matrix with another product
    if layout != "contig":
        flat = pl.bufs[0].numpy()
        late = np.lib.stride_tricks.as_strided(flat[ga.offset + 1:], (p.M, p.K), (ga.ld, 1))
        assert not np.array_equal(S.reference_acc(late, p.b), p.acc)
        if p.M > 1:
            wrong_ld = np.lib.stride_tricks.as_strided(flat[ga.offset:], (p.M, p.K), (p.K, 1))
            assert not np.array_equal(S.reference_acc(wrong_ld, p.b), p.acc)


@pytest.mark.parametrize("M,N,K", [(300, 520, 1280), (300, 520, 640), (300, 520, 12928), (64, 520, 1280), (1, 520, 1280), (130, 517, 8192)])
def test_geometry_table(M, N, K):
    """the alignment and leading dimensions the table promises, the limit layouts by arithmetic alone"""
    g = {l: S.geometry(l, M, N, K) for l in S.LAYOUTS}
    ldy = S.ldy_of(N)
    assert (ldy * 2) % 16 == 0 and (8 * 2) % 16 == 0 and ldy >= N + 8
    if N % 8 == 0:
        assert ldy == N + 24
    for l, (a, b) in g.items():
        assert a.offset + (M - 1) * a.ld + K <= a.nbytes and b.offset + (N - 1) * b.ld + K <= b.nbytes, l
        assert a.ld >= K and b.ld >= K
        if l != "contig":
            assert len({a.ld, b.ld, ldy}) == 3, (l, a.ld, b.ld, ldy)
    assert g["contig"][0][1:] == (K, 0) and g["contig"][1][1:] == (K, 0)
    assert (g["pad"][0].ld, g["pad"][1].ld) == (K + 16, K + 48) and g["pad"][0].ld % 128 != 0 and g["pad"][1].ld % 128 != 0
    wa, wb = g["window"]
    assert (wa.ld, wb.ld) == (K + 176, 2 * K + 16) and wa.nbytes == (M + 3) * (K + 176) and wb.nbytes == (N + 1) * (2 * K + 16)
    assert wa.offset == 2 * wa.ld + 48 and wb.offset == wb.ld + 16
    for geo in (wa, wb):          # (the caching allocator's blocks are 512-byte aligned: the base's alignment is the offset's)
        assert geo.offset % 16 == 0 and geo.offset % 128 != 0 and geo.ld % 16 == 0
    for side, other in ((0, 1), (1, 0)):
        rows = (M, N)[side]
        lim, bey = g[("limit_a", "limit_b")[side]], g[("beyond_a", "beyond_b")[side]]
        assert lim[side].ld == (1 << 23) - 16 and lim[side].ld % 16 == 0 and lim[side].ld < 1 << 23 and lim[other].ld == K + 16
        assert bey[side].ld == 1 << 23 and bey[other].ld == K + 16
        assert lim[side].nbytes == (rows - 1) * lim[side].ld + K and bey[side].nbytes == (rows - 1) * (1 << 23) + K
        assert 255 * lim[side].ld + 7 * 16 + K < 1 << 31, "the loaders' 32-bit staging offset: 255 rows x ld + the chunk + the K walk stays below 2^31"
    if (M, N) == (300, 520):
        assert 2.5e9 < g["limit_a"][0].nbytes < 2.6e9 and 4.3e9 < g["limit_b"][1].nbytes < 4.4e9
        assert g["beyond_a"][0].nbytes + g["beyond_a"][1].nbytes < 7e9 and g["beyond_b"][0].nbytes + g["beyond_b"][1].nbytes < 7e9
    assert (g["ragged_ld"][0].ld, g["ragged_ld"][1].ld) == (K + 8, K + 16) and g["ragged_ld"][0].ld % 16 == 8
    assert g["odd_base"][0].ld == K + 17 and g["odd_base"][0].offset == 1 and g["odd_base"][1] == g["pad"][1]


def test_large_layouts_are_refused_for_larger_operands():
    with pytest.raises(AssertionError):
        S.geometry("limit_a", 301, 520, 1280)
    with pytest.raises(AssertionError):
        S.geometry("beyond_b", 300, 521, 1280)


def test_output_window_and_its_check():
    big, win = S.out_window(5, 13, torch.float32, "cpu")
    assert win.shape == (5, 13) and win.stride() == (S.ldy_of(13), 1) and (win.data_ptr() - big.data_ptr()) == 8 * 4
    win.zero_()
    assert S.untouched_outside(big, 13)
    big[2, 8 + 13] = 0.0
    assert not S.untouched_outside(big, 13)


# ---------------------------------------------------------------- the table of tests/test_gpu_gemm_strides.py (read here, where no GPU is needed)
def test_every_row_lists_the_layouts_its_path_is_held_to():
    from tests import test_gpu_gemm_strides as T
    IDS, TABLE, SMALL_ROWS, A_ROWS, B_ROWS = T.IDS, T.TABLE, T.SMALL_ROWS, T.A_ROWS, T.B_ROWS
    by = {r[0]: set(r[3]) for r in TABLE}
    assert all(set(S.FAST) <= by[i] for i in IDS if i.startswith(("variant-", "sp256_16-2deep")))
    assert all({"pad", "window", "limit_a"} <= by[i] for i in IDS if i.startswith("splitk-"))
    assert all({"pad", "window", "limit_b"} <= by[i] for i in IDS if i.startswith(("fsk-", "rotation-", "skinny-")))
    assert all({"pad", "window"} <= by[i] for i in IDS if i.startswith(("tail-", "fake-cus-")))
    assert all(set(S.GENERIC) <= by[i] for i in IDS if i.startswith("generic-"))
    assert {r[0] for r in SMALL_ROWS} == set(IDS), "every row runs its small layouts"
    assert all(set(r[3]) <= {"limit_a", "beyond_a"} for r in A_ROWS) and all(set(r[3]) <= {"limit_b", "beyond_b"} for r in B_ROWS), "one operand side per function"
    ran = {i: set() for i in IDS}
    for rows in (SMALL_ROWS, A_ROWS, B_ROWS):
        for r in rows:
            ran[r[0]] |= set(r[3])
    assert ran == by, "the three functions together run every layout a row lists"
    for r in TABLE:          # the 2^23 layouts only at shapes they are sized for
        if set(r[3]) & set(S.LARGE):
            shape = {T.run_variant: (300, 520), T.run_generic: (300, 520), T.run_rotation: T.ROT_SHAPE[:2], T.run_skinny: (r[2][0], 520)}.get(r[1], r[2][:2])
            assert shape[0] <= S.MAX_M and shape[1] <= S.MAX_N, r[0]


# ---------------------------------------------------------------- the planner's side of the contract (no device is asked: PQ_FAKE_CUS=256)
@pytest.fixture
def L(pq_opt):
    from protoquant_amd import _lib
    pq_opt("PQ_FAKE_CUS", "256")
    return _lib.lib()


def test_planner_keeps_its_tile_for_strided_operands_up_to_the_bound(L, pq_opt):
    M, N, K = 300, 520, 1280
    lim = (1 << 23) - 16
    name = L.pq_gemm_variant_name(M, N, K, K, K)
    assert name == b"ring64x64_16x16x64"
    for lda, ldb in ((K + 16, K + 48), (K + 176, 2 * K + 16), (lim, K + 16), (K + 16, lim), (lim, lim)):
        assert L.pq_gemm_variant_name(M, N, K, lda, ldb) == name, (lda, ldb)
    assert L.pq_gemm_variant_name(17, N, K, K + 16, lim) == b"skinny_16x16x64"
    for forced, want in (("sp256_16", b"sp256_16x16x64"), ("ring128", b"ring128_16x16x64"), ("generic", b"generic64")):
        pq_opt("PQ_FORCE_VARIANT", forced)
        assert L.pq_gemm_variant_name(M, N, K, lim, K + 16) == want and L.pq_gemm_variant_name(M, N, K, K + 16, lim) == want


@pytest.mark.parametrize("forced", ["", "sp256_16", "ring64x64", "skinny"])
def test_planner_leaves_the_fast_path_beyond_the_bound(L, pq_opt, forced):
    """2^23 on either side, a leading dimension that is not a multiple of 16 (K + 8; K + 17, the odd_base layout): the generic kernel, also when a tile is forced
    (pick_variant returns V_GENERIC for operands that are not eligible)"""
    M, N, K = 300, 520, 1280
    pq_opt("PQ_FORCE_VARIANT", forced)
    for m in (M, 17):
        for lda, ldb in ((1 << 23, K + 16), (K + 16, 1 << 23), (K + 8, K + 16), (K + 16, K + 8), (K + 17, K + 48), (K + 16, K + 17), ((1 << 23) + 16, K)):
            assert L.pq_gemm_variant_name(m, N, K, lda, ldb) == b"generic64", (m, lda, ldb)
    assert L.pq_gemm_variant_name(M, N, K + 64, K + 64, K + 64) == b"generic64", "K is not a multiple of 128"


# ---------------------------------------------------------------- argument checks that need no device
def _host(nbytes=64):
    """a non-null pointer (host memory: nothing dereferences it before the checks), so that the leading dimension is the only bad argument"""
    buf = ctypes.create_string_buffer(nbytes)
    return buf, ctypes.addressof(buf)


M_, N_, K_ = 4, 8, 16
BAD = [("lda", dict(lda=K_ - 1)), ("ldb", dict(ldb=K_ - 1)), ("ldy", dict(ldy=N_ - 1))]


def _call(L, entry, lda=K_, ldb=K_, ldy=N_, ldyt=M_):
    keep, p = _host()
    if entry == "pq_qlinear_s8":
        return L.pq_qlinear_s8(p, lda, p, p, ldb, p, None, p, ldy, 0, M_, N_, K_, None, 0, None)
    if entry == "pq_qlinear_s8_t":      # (its output is yt[N, M]: the leading dimension is held against M)
        return L.pq_qlinear_s8_t(p, lda, p, p, ldb, p, None, p, ldyt if ldy == N_ else M_ - 1, 0, M_, N_, K_, None, 0, None)
    if entry == "pq_gemm_s8s8s32":
        return L.pq_gemm_s8s8s32(p, lda, p, ldb, p, ldy, M_, N_, K_, None)
    if entry == "pq_qlinear_s8_kslabs":      # two slabs of K / 2 columns: lda is held against k_per_slab
        kps = K_ // 2
        return L.pq_qlinear_s8_kslabs(p, kps if lda == K_ else kps - 1, M_ * kps, kps, p, p, ldb, p, None, p, ldy, 0, M_, N_, K_, None, 0, None)
    if entry == "pq_qlinear_dyn":
        return L.pq_qlinear_dyn(p, 0, lda, p, ldb, p, None, p, ldy, M_, N_, K_, p, 1 << 30, None)
    raise AssertionError(entry)


@pytest.mark.parametrize("which,bad", BAD, ids=[b[0] for b in BAD])
@pytest.mark.parametrize("entry", ["pq_qlinear_s8", "pq_qlinear_s8_t", "pq_gemm_s8s8s32", "pq_qlinear_s8_kslabs", "pq_qlinear_dyn"])
def test_a_leading_dimension_below_the_row_length_is_refused(entry, which, bad):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert L.pq_set_option(b"PQ_FAKE_CUS", b"") == 0          # (any successful call: pq_last_error() below is this test's)
    assert _call(L, entry, **bad) == PQ_ERR_BAD_ARG, (entry, which)
    msg = L.pq_last_error().decode()
    assert msg.startswith(entry + ":"), msg
    value = {"lda": K_ // 2 - 1 if entry == "pq_qlinear_s8_kslabs" else K_ - 1, "ldb": K_ - 1, "ldy": M_ - 1 if entry == "pq_qlinear_s8_t" else N_ - 1}[which]
    assert f"={value}" in msg, f"the message shows the offending leading dimension: {msg}"


def test_null_operands_are_refused_by_the_one_call_entry_too():
    """pq_qlinear_dyn used to check only the sizes' signs itself: a short ldw or ldy was found by pq_qlinear_s8 AFTER K1 had been launched, a short ld_x under K1's name"""
    from protoquant_amd import _lib
    L = _lib.lib()
    keep, p = _host()
    assert L.pq_qlinear_dyn(None, 0, K_, p, K_, p, None, p, N_, M_, N_, K_, p, 1 << 30, None) == PQ_ERR_BAD_ARG and L.pq_last_error().startswith(b"pq_qlinear_dyn:")
    assert L.pq_qlinear_dyn(p, 0, K_, p, K_, None, None, p, N_, M_, N_, K_, p, 1 << 30, None) == PQ_ERR_BAD_ARG and L.pq_last_error().startswith(b"pq_qlinear_dyn:")
    assert L.pq_qlinear_dyn(p, 0, K_, p, K_, p, None, p, N_, 0, N_, K_, None, 0, None) == 0, "empty stays a no-op"
    assert L.pq_qlinear_dyn(p, 7, K_, p, K_, p, None, p, N_, M_, N_, K_, p, 1 << 30, None) == PQ_ERR_BAD_ARG and b"dtype" in L.pq_last_error()
