"""CPU: the tables of tests/gemm_edges.py are what they claim to be before any kernel sees them — the window property of the reference, the poison, the coverage of the
three parts (the weight-streaming kernel's through the restatement of skinny_plan, which is coverage bookkeeping only), the planner's answers for every Part 1 shape with
PQ_FAKE_CUS=256 (no device is asked), and the buffer comparison itself: fed with shifted windows, a touched margin and products with a K-tile dropped or doubled, it names
the right element."""
import itertools

import numpy as np
import pytest

from oracle import qspec_numpy as Q
from tests import gemm_edges as E

GEOMETRIES = sorted(set(E.TILE.values()))


# ---------------------------------------------------------------- the window property
@pytest.mark.parametrize("pattern", ["full", "ktile"])
def test_sliced_operands_give_the_window_of_the_full_output(pattern):
    p = E.problem(137, 101, 5 * 128, pattern)
    assert np.array_equal(p.acc().astype(np.int64), p.a.astype(np.int64) @ p.b.astype(np.int64).T), "the exact product agrees with an int64 matmul"
    if pattern == "full":
        assert (p.a[:, 0] == -128).all() and (p.b[:, 0] == -128).all() and p.a.max() == 127
    else:
        assert p.a.min() >= 1 and p.b.min() >= 1, "ktile: every product is positive — a dropped or repeated step moves every sum"
    assert (p.xs > 0).all() and (p.ws > 0).all() and np.isfinite(p.xs).all() and np.isfinite(p.ws).all()
    for (M, N, K) in ((1, 1, 128), (1, 101, 640), (137, 1, 256), (17, 33, 384), (64, 65, 640), (137, 101, 128), (100, 37, 512)):
        a, b = p.a[:M, :K], p.b[:N, :K]
        acc = Q.gemm_s8s8s32(a, b)
        assert np.array_equal(acc.astype(np.int64), a.astype(np.int64) @ b.astype(np.int64).T)
        assert np.array_equal(acc, p.acc(K)[:M, :N])
        for kind in E.KINDS:
            if kind.code is None:
                own = acc.view(np.uint32)
            else:
                own = Q.epilogue(acc, p.xs[:M], p.ws[:N], p.bias[kind.code][:N] if kind.bias else None, kind.code)
                own = own.view(np.uint32) if kind.code == 2 else own
                own = own.T if kind.entry == "yt" else own
            win = p.window(kind, M, N, K)
            assert win.dtype == E.bits_dtype(kind.code) and np.array_equal(win, own), (kind.name, M, N, K)


def test_step_pattern_of_the_streaming_kernel_is_indexed_by_the_64_byte_step():
    p = E.problem(4, 3, 86 * 128, "ktile", 64)
    steps = p.a[0].reshape(-1, 64)
    assert (steps == steps[:, :1]).all() and (np.diff(steps[:120, 0].astype(int)) == 1).all(), "one value per 64-byte step, growing"
    assert p.a.max() <= 126 and p.a.min() >= 1 and p.b.min() >= 1


# ---------------------------------------------------------------- the poison
def _all_problems():
    for (TM, TN) in GEOMETRIES:
        Mx, Nx = E.edge_extent(TM, TN)
        yield E.problem(Mx, Nx, E.K_EDGE, "full"), (None,)
        for pattern in ("full", "ktile"):
            yield E.problem(2 * TM, 2 * TN, E.KT_LD, pattern), tuple(128 * n for n in E.KT_COUNTS)
    yield E.problem(513, 513, E.K_SPLIT, "full"), (None,)
    for pattern in ("full", "ktile"):
        yield E.problem(64, E.SK_N, E.SK_KMAX, pattern, 64), tuple(128 * n for n in E.SK_KT)


def test_no_expected_output_holds_the_poison():
    for code, bits in E.POISON.items():
        if code is not None:      # a NaN whose payload is not the quiet bit alone
            f = Q.to_f32(np.array([bits], E.bits_dtype(code)).view(np.float32 if code == 2 else np.uint16), code)
            assert np.isnan(f).all()
    assert E.POISON[None] > 128 * 128 * E.SK_KMAX
    for p, Ks in _all_problems():
        for K in Ks:
            for kind in E.KINDS:
                w = p.want(kind, K)
                assert not (w == E.POISON[kind.code]).any(), (p.Mmax, p.Nmax, K, kind.name)
                if kind.code is not None:
                    assert np.isfinite(Q.to_f32(w.view(np.float32) if kind.code == 2 else w, kind.code)).all()


def test_output_layouts():
    for rows, cols in ((1, 1), (1, 37), (5, 13), (64, 1), (257, 261), (513, 513)):
        c, l = E.layout(rows, cols, "contig"), E.layout(rows, cols, "ld8")
        assert c.ld == cols and c.offset % 8 == 0 and c.offset >= cols + 8 and c.total - (c.offset + rows * cols) >= cols + 8
        assert l.ld % 8 == 0 and l.ld >= cols + 16 and l.offset == l.ld + 8 and l.total == (rows + 2) * l.ld
        for lay in (c, l):          # a row above and below, eight elements left and right
            assert lay.offset - lay.ld - 8 >= 0 and lay.offset + rows * lay.ld + cols + 7 < lay.total, "elements [-1, -8] and [rows, cols + 7] exist"


# ---------------------------------------------------------------- Part 1 and 2: coverage
@pytest.mark.parametrize("TM,TN", GEOMETRIES)
def test_edge_pairs_cover_every_residue_and_every_half_tile(TM, TN):
    pairs = E.edge_pairs(TM, TN)
    for axis, T, other in ((0, TM, (TN, TN + 5)), (1, TN, (TM, TM + 3))):
        sizes = {p[axis] for p in pairs}
        assert {s - T for s in sizes if T < s <= T + 16} == set(range(1, 17)), "every residue mod 16 is the size of a last tile"
        assert all(any(((s, o) if axis == 0 else (o, s)) in pairs for o in other) for s in range(T + 1, T + 17))
        for k in (1, 2, 3, 4):
            for d in (-1, 0, 1):
                s = k * T // 2 + d
                assert all(((s, o) if axis == 0 else (o, s)) in pairs for o in other), (T, k, d)
        assert {1, 15, 16, 17} <= sizes
    assert {(TM + i, TN + j) for i in (1, 8, 15) for j in range(1, 17)} <= set(pairs)
    Mx, Nx = E.edge_extent(TM, TN)
    assert max(p[0] for p in pairs) <= Mx and max(p[1] for p in pairs) <= Nx
    full, ragged = E.kt_shapes(TM, TN)
    assert full[0] % TM == 0 and full[1] % TN == 0 and ragged[0] % (TM // 2) != 0 and ragged[1] % (TN // 2) != 0
    assert set(range(1, 10)) <= set(E.KT_COUNTS) and max(E.KT_COUNTS) * 128 == E.KT_LD


def test_every_variant_and_switch_is_in_the_table():
    assert {f.variant for f in E.FORMS} == set(E.TILE) == {"generic", "sp256_16", "sp128_16", "sp128x128", "ring128", "ring64x128", "ring64x64", "ring128x160"}
    assert {f.switches for f in E.FORMS if f.switches} == {(("PQ_SP256_P3", "0"),), (("PQ_RING_LC", "0"),), (("PQ_SP128_LC", "0"),)}
    assert E.K_EDGE == 5 * 128 and ("contig", "0") in E.OUT_MODES and ("contig", "") in E.OUT_MODES and ("ld8", "") in E.OUT_MODES
    assert E.KINDS == (E.BF16_B, E.FP16, E.F32_B, E.I32, E.BF16_BT)
    h = set(E.half_tile_set(256))
    assert h == {127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513}
    sp = set(E.split_pairs())
    assert all((M, 256) in sp and (M, 261) in sp and (256, M) in sp and (259, M) in sp for M in h) and all(M > 64 and M * N >= 128 * 128 for M, N in sp)
    assert {(256 + i, 256 + j) for i in (1, 8, 15) for j in range(1, 17)} <= sp and E.K_SPLIT // 128 == 20


@pytest.fixture
def L(pq_opt):
    from protoquant_amd import _lib
    pq_opt("PQ_FAKE_CUS", "256")
    return _lib.lib()


@pytest.mark.parametrize("form", E.FORMS, ids=[f.id for f in E.FORMS])
def test_planner_reports_the_forced_variant_single_pass_for_every_part1_shape(L, pq_opt, form):
    pq_opt("PQ_FORCE_VARIANT", form.variant)
    for name, value in form.switches:
        pq_opt(name, value)
    TM, TN = E.TILE[form.variant]
    want = E.DISPLAY[form.variant]
    shapes = [(M, N, E.K_EDGE, E.K_EDGE) for M, N in E.edge_pairs(TM, TN)] + [(M, N, 128 * n, E.KT_LD) for M, N in E.kt_shapes(TM, TN) for n in E.KT_COUNTS]
    for M, N, K, ld in shapes:
        lda = K if M == 1 else ld          # (one row: the entries are given K for its leading dimension)
        assert L.pq_gemm_variant_name(M, N, K, lda, ld) == want and L.pq_gemm_variant_name(N, M, K, ld, lda) == want, (M, N, K)
        assert L.pq_qlinear_workspace_bytes(M, N, K) == 0 and L.pq_qlinear_t_workspace_bytes(M, N, K) == 0, (M, N, K)


@pytest.mark.parametrize("form", E.SPLIT_FORMS, ids=[f.id for f in E.SPLIT_FORMS])
def test_planner_hands_every_part2_shape_to_its_split_k_form(L, pq_opt, form):
    for name, value in form.switches:
        pq_opt(name, value)
    S = int(form.switches[0][1])
    for M, N in E.split_pairs():
        tiles = ((M + 255) // 256) * ((N + 255) // 256)
        if form.id.startswith("splitk"):
            want = S * M * N * 4
        else:
            want = ((tiles * 4 * (4 if S == 4 else 2) + 255) // 256) * 256 + tiles * (S - 1) * 256 * 256 * 4
        assert L.pq_qlinear_workspace_bytes(M, N, E.K_SPLIT) == want and L.pq_qlinear_t_workspace_bytes(M, N, E.K_SPLIT) == L.pq_qlinear_workspace_bytes(N, M, E.K_SPLIT) > 0
        assert L.pq_gemm_variant_name(M, N, E.K_SPLIT, E.K_SPLIT, E.K_SPLIT) in (E.DISPLAY["sp256_16"], E.DISPLAY["sp128_16"], E.DISPLAY["ring128"]), "qlinear_core's `tiled`"


# ---------------------------------------------------------------- Part 3: coverage (skinny_plan restated: bookkeeping only)
def test_streaming_plan_agrees_with_the_library_where_it_can_be_asked(L, pq_opt):
    """the restatement never yields an expected value; what CAN be held is that every case is one the planner sends to the weight-streaming kernel"""
    pq_opt("PQ_FORCE_VARIANT", "skinny")
    for M in set(E.SK_M) | set(E.SK_EDGE_M):
        for N in set(E.SK_EDGE_N):
            assert L.pq_gemm_variant_name(M, N, E.K_EDGE, E.K_EDGE, E.K_EDGE) == E.DISPLAY["skinny"]
        for n in E.SK_KT:
            assert L.pq_gemm_variant_name(M, E.SK_N, 128 * n, E.SK_KMAX, E.SK_KMAX) == E.DISPLAY["skinny"]


def _walks(mt, rb, staged):
    for M in E.SK_M:
        for n, rbo, kso, sto in itertools.product(E.SK_KT, E.SK_RB, E.SK_KS, E.SK_STAGE):
            w = E.skinny_walk(M, E.SK_N, 128 * n, rbo, kso, sto)
            if (w.mt, w.rb, w.staged) == (mt, rb, staged):
                yield w


@pytest.mark.parametrize("mt,rb,staged", [(mt, rb, st) for mt in (1, 2, 3, 4) for rb in ((1, 2) if mt <= 2 else (1,)) for st in (True, False)])
def test_k_sweep_reaches_every_state_of_a_wave(mt, rb, staged):
    """per (token tiles, weight blocks per wave, staged): some wave's slice with no full batch (its tail is then never empty: the K split is clamped to the steps), with
    exactly one batch, an even count >= 2 and an odd count >= 3, each with an empty and with a non-empty tail; unequal slices within a workgroup; every K split"""
    seen, uneven, splits = set(), False, set()
    for w in _walks(mt, rb, staged):
        splits.add(w.ks)
        uneven |= len({b * E.sk_batch(mt, rb) + t for b, t in w.waves}) > 1
        assert all(b > 0 or t > 0 for b, t in w.waves), "no wave has an empty slice"
        seen |= {(E.batch_class(b), t > 0) for b, t in w.waves}
    want = {(c, t) for c in ("one batch", "even >= 2", "odd >= 3") for t in (False, True)} | {("tail only", True)}
    assert seen == want, want - seen
    assert uneven and splits == {1, 2, 4, 8, 16}


def test_edge_sweep_of_the_streaming_kernel():
    assert set(map(E.token_tiles, E.SK_EDGE_M)) == {1, 2, 3, 4}
    assert {n % 4 for n in E.SK_EDGE_N} == {0, 1, 3} | {E.SK_N % 4} and {n % 16 for n in E.SK_EDGE_N} >= {0, 1, 15} and {1, 17, 33} <= set(E.SK_EDGE_N)
    for M in E.SK_EDGE_M:          # the default plan and PQ_SKINNY_RB=2: both block counts per wave where the kernel has them
        rbs = {E.skinny_walk(M, 37, E.K_EDGE, rbo).rb for rbo in E.SK_EDGE_RB}
        assert rbs == ({1, 2} if E.token_tiles(M) <= 2 else {1})


# ---------------------------------------------------------------- the checker checks
KIND_IDS = [k.name for k in E.KINDS]


@pytest.fixture(scope="module")
def small():
    return E.problem(40, 29, 3 * 128, "full"), E.problem(40, 29, 3 * 128, "ktile")


@pytest.mark.parametrize("mode", E.MODES)
@pytest.mark.parametrize("kind", E.KINDS, ids=KIND_IDS)
def test_the_comparison_names_the_right_element(small, kind, mode):
    full, ktile = small
    M, N = 23, 17
    rows, cols = (N, M) if kind.entry == "yt" else (M, N)
    lay = E.layout(rows, cols, mode)
    win = full.window(kind, M, N)
    want = E.expected_buffer(win, lay, kind.code)
    assert E.first_bad(want.copy(), want, lay) is None
    assert (want != E.POISON[kind.code]).sum() == rows * cols, "the window and nothing else"

    def placed(offset):
        return E.expected_buffer(win, lay._replace(offset=offset), kind.code)
    # the window one row down: slot [0, 0] still holds the poison
    bad = E.first_bad(placed(lay.offset + lay.ld), want, lay)
    assert (bad.row, bad.col, bad.inside, bad.got) == (0, 0, True, E.POISON[kind.code])
    # one row up: the first element written lies in the margin, a row above [0, 0]
    bad = E.first_bad(placed(lay.offset - lay.ld), want, lay)
    assert (bad.row, bad.col, bad.inside, bad.want) == (-1, 0, False, E.POISON[kind.code])
    # one column to the right, one to the left
    bad = E.first_bad(placed(lay.offset + 1), want, lay)
    assert (bad.row, bad.col, bad.inside) == (0, 0, True)
    bad = E.first_bad(placed(lay.offset - 1), want, lay)
    assert (bad.row, bad.col, bad.inside) == (-1, lay.ld - 1, False)
    # one element of the margin: right before the window, right after the end of a row (contiguous rows: of the last one), eight elements further
    end = lay.offset + (rows - 1) * lay.ld + cols
    for at in (lay.offset - 1, end, end + 7) + ((lay.offset + 5 * lay.ld + cols, lay.offset + 6 * lay.ld - 1) if mode == "ld8" else ()):
        got = want.copy()
        got[at] = win[0, 0]
        bad = E.first_bad(got, want, lay)
        assert (bad.count, bad.inside, bad.want) == (1, False, E.POISON[kind.code])
        assert lay.offset + bad.row * lay.ld + bad.col == at
    got = want.copy()
    got[-1] ^= 1
    bad = E.first_bad(got, want, lay)
    assert bad.count == 1 and not bad.inside and lay.offset + bad.row * lay.ld + bad.col == lay.total - 1
    # a product with one K-tile dropped, and with one doubled: both patterns; under "ktile" every sum moves
    for p in (full, ktile):
        w = p.window(kind, M, N)
        wbuf = E.expected_buffer(w, lay, kind.code)
        t = p.a[:, 128:256].astype(np.int64) @ p.b[:, 128:256].astype(np.int64).T
        for sign in (-1, +1):
            mut = p.epilogue((p.acc() + sign * t).astype(np.int32), kind)
            mut = mut[:N, :M] if kind.entry == "yt" else mut[:M, :N]
            first = np.argwhere(mut != w)[0]
            bad = E.first_bad(E.expected_buffer(mut, lay, kind.code), wbuf, lay)
            assert bad.inside and (bad.row, bad.col) == tuple(first) and bad.got == int(mut[tuple(first)]) and bad.want == int(w[tuple(first)])
            if p is ktile and kind.code is None:
                assert bad.count == rows * cols and (bad.row, bad.col) == (0, 0)
            text = E.describe(bad, "ring128", kind, M, N, 384)
            assert f"M={M} N={N} K=384" in text and f"[{bad.row}, {bad.col}]" in text and kind.name in text and "ring128" in text
