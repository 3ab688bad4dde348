"""CPU: the designed operands of tests/amax_design.py do what they claim before any kernel sees them.

  - the restated dispatches reach exactly the (TPR, VPT) their sources instantiate, and the designed widths reach EVERY one of them, per form and dtype;
  - per layout the planted positions cover what the module's docstring promises (every column; or every lane in its first and last live slot, every slot at the wave edges,
    the last vectors), every planted position with a finite value of each sign, every planted (lane, slot) once with NaN and once with Inf (where a norm leaves them visible);
  - on the reference alone, every row's strict maximum of |h| is at its planted position, a finite one a factor of 4 above the runner-up, and the scale depends on it
    (narrow and generic cases here; tests/test_gpu_amax_positions.py asserts the same on every case before it compares);
  - the shortcut reference of the elementwise forms equals form.ref on the whole operands;
  - the tail-slot widths leave the three classes of dead slots in every norm layout class, every special value lands in an element of its own in the last (first)
    vector, the six row classes are populated, and the numpy specification and the C oracle agree on those operands where both exist (K1n)."""
import numpy as np
import pytest

from oracle import c_oracle as C
from oracle import qspec_numpy as Q
from tests import amax_design as D
from tests.row_forms import BY_NAME, FORMS, compare, eps_values

AMAX_FORMS = [f.name for f in FORMS if not f.custom and (f.nq or f.amax) and f.name != "K2"]
TAIL_FORMS = [f.name for f in FORMS if not f.custom and f.vecs]
CODES = [0, 1, 2]

# what the sources instantiate and a width can reach (quant_kernels.hip launch_rowwise_vec, rowmap_kernels.h rowmap_dispatch, rownorm_kernels.h rownorm_dispatch)
K1_SET = {(64, 1, ""), (64, 2, ""), (64, 4, ""), (64, 8, ""), (256, 4, ""), (256, 8, ""), (256, 16, ""), (256, 32, ""),
          (64, 1, "rpw2"), (64, 2, "rpw2"), (64, 4, "rpw2"), (64, 8, "rpw2")}
K1_ST16 = {(64, 2, "st16"), (64, 4, "st16"), (64, 8, "st16")}                       # 16-bit storage only
ROWMAP_SET = {(64, 1, ""), (64, 2, ""), (64, 4, ""), (256, 2, ""), (256, 4, ""), (256, 8, ""), (256, 16, "")}
ROWMAP_WIDE = {(512, 3, ""), (256, 8, "tpr256")}
ROWNORM_SET = {(64, 1, ""), (64, 2, ""), (64, 4, ""), (64, 8, ""), (256, 1, ""), (256, 2, ""), (256, 4, ""), (256, 8, ""), (256, 16, "")}


def test_the_table_has_the_forms_with_a_code_or_an_amax_output():
    assert len(AMAX_FORMS) == 22 and {"K1", "K1_amax_halves", "K1s_amax_halves", "K1n", "K1a", "K1pl_two_groups", "K1l2", "K1pang", "K1oq"} <= set(AMAX_FORMS)
    assert set(TAIL_FORMS) == {"K1n", "K1a", "K1l_bias", "K1l_nobias", "K1al", "K1pl_one_group", "K1pl_two_groups", "K1l2", "K1ng", "K1ang", "K1pang", "K1pa", "K1oq", "K1oa",
                               "K1on"}


def test_restated_dispatches_at_known_widths():
    assert str(D.k1_layout(0, 4096)) == "k1:64x8" and str(D.k1_layout(0, 4104)) == "k1:256x4" and str(D.k1_layout(2, 32768)) == "k1:256x32"
    assert str(D.k1_layout(0, 4096, rpw=2)) == "k1:64x8:rpw2" and str(D.k1_layout(0, 4096, st16=1)) == "k1:64x8:st16" and str(D.k1_layout(0, 520, st16=1)) == "k1:64x2"
    assert str(D.k1_layout(2, 1024, st16=1)) == "k1:64x4" and str(D.k1_layout(0, 333)) == "k1:generic" and str(D.k1_layout(0, 8 * 8193)) == "k1:generic"
    assert str(D.rowmap_layout(0, 2048, True)) == "rowmap:64x4" and str(D.rowmap_layout(0, 2056, True)) == "rowmap:256x2"
    assert str(D.rowmap_layout(0, 11008, True)) == "rowmap:512x3" and str(D.rowmap_layout(0, 11008, False)) == "rowmap:256x8"
    assert str(D.rowmap_layout(0, 11008, True, silu_tpr=256)) == "rowmap:256x8:tpr256" and str(D.rowmap_layout(0, 8 * 1537, True)) == "rowmap:256x8"
    assert str(D.rownorm_layout(0, 2048)) == "rownorm:64x4" and str(D.rownorm_layout(0, 4096)) == "rownorm:256x2" and str(D.rownorm_layout(0, 4096, 512)) == "rownorm:64x8"
    assert str(D.rownorm_layout(0, 512, 0)) == "rownorm:256x1" and str(D.rownorm_layout(2, 16384)) == "rownorm:256x16" and str(D.rownorm_layout(0, 8 * 4097)) == "rownorm:generic"


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("name", AMAX_FORMS)
def test_designed_widths_reach_every_instantiated_layout(name, code):
    form = BY_NAME[name]
    fam = D.family(form)
    want = {"k1": K1_SET | (K1_ST16 if code != 2 else set()), "rowmap": ROWMAP_SET | (ROWMAP_WIDE if form.wide else set()), "rownorm": ROWNORM_SET}[fam]
    reach = D.reachable(form, code)
    assert {(l.tpr, l.vpt, l.variant) for l in reach} == want, (name, code)
    cs = D.cases(form, code)
    assert {(c.layout.tpr, c.layout.vpt, c.layout.variant) for c in cs if c.layout.tpr} == want, "a layout that no designed width reaches"
    assert sorted(c.cols for c in cs if not c.layout.tpr) == list(D.GENERIC_WIDTHS)
    for c in cs:
        assert D.layout_of(form, code, c.cols, dict(c.switches)) == c.layout, c.id           # the restated dispatch sends the width there under those switches
        assert c.cols >= D.min_cols(form, code) and (c.mode == "all") == (c.cols <= D.ALL_COLUMNS_MAX)
    assert len({c.id for c in cs}) == len(cs)


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("name", AMAX_FORMS)
def test_planted_positions_cover_each_layout(name, code):
    form, epv = BY_NAME[name], D.EPV[code]
    signs = {"+"} if D.positive_only(form) else {"+", "-"}
    for c in D.cases(form, code):
        rows = D.planted_rows(form, code, c)
        lay, nvec = c.layout, -(-c.cols // epv)
        assert all(0 <= col < c.cols for col, _ in rows) and len(set(rows)) == len(rows), c.id
        by_col = {}
        for col, k in rows:
            if k in "+-":
                by_col.setdefault(col, set()).add(k)
        assert all(v == signs for v in by_col.values()), (c.id, "a planted position without a finite value of each sign")
        vec_of = lambda kinds: {col // epv for col, k in rows if k in kinds}                  # noqa: E731
        planted = {col // epv for col in by_col}
        # once with Inf and once with NaN per planted (lane, slot), where the arithmetic leaves the position visible: no NaN in a norm, nothing in a LayerNorm
        assert D.is_layernorm(form) or vec_of(("+inf", "-inf")) == planted, c.id
        assert D.is_norm(form) or vec_of(("nan",)) == planted, c.id
        assert not D.is_layernorm(form) or not vec_of(("nan", "+inf", "-inf")), c.id
        if c.mode == "all":
            assert sorted(by_col) == list(range(c.cols)) and planted == set(range(nvec)), c.id      # every column
            continue
        for t in range(lay.tpr):
            ls = D.live_slots(lay, nvec, t)
            assert ls and ls[0] * lay.tpr + t in planted and ls[-1] * lay.tpr + t in planted, (c.id, t)
        for s in range(lay.vpt):
            live = [t for t in range(lay.tpr) if s * lay.tpr + t < nvec]
            assert live or lay.variant == "tpr256", (c.id, s, "the wide width keeps every slot index live")
            for w in range(lay.tpr // 64):
                lw = [t for t in live if t // 64 == w]
                assert not lw or (s * lay.tpr + lw[0] in planted and s * lay.tpr + lw[-1] in planted), (c.id, s, w)
        assert {nvec - 1, nvec - 2} <= planted, c.id
        assert D.dead_slot_classes(lay, nvec) >= {"part of a wave"}, c.id


def test_positions_name_lane_slot_and_element():
    lay = D.Layout("rownorm", 256, 4)
    assert D.position(lay, 0, 8 * (2 * 256 + 70) + 5) == dict(col=8 * 582 + 5, vector=582, elem=5, lane=6, wave=1, slot=2)
    assert D.position(D.Layout("k1", 64, 8), 2, 4 * 100 + 3) == dict(col=403, vector=100, elem=3, lane=36, wave=0, slot=1)
    assert "wave 1 lane 6 slot 2" in D.describe(lay, 0, 8 * 582 + 5)
    assert D.position(D.Layout("rowmap", 0), 0, 700)["wave"] == (700 % 256) // 64


def _narrow(form, code):
    return [c for c in D.cases(form, code) if c.cols <= 528]


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("name", AMAX_FORMS)
def test_reference_maximum_is_at_the_planted_position(name, code):
    form = BY_NAME[name]
    cs = _narrow(form, code)
    assert len(cs) >= 3
    seen = set()
    for c in cs:
        if (c.cols, c.mode) in seen:
            continue
        seen.add((c.cols, c.mode))
        inp, rows = D.planted_inputs(form, code, c)
        want = D.reference(form, inp, rows, code)
        top = D.check_planted(form, inp, rows, want, code, f"{name} {D.DT[code]} {c.id}")
        kinds = {k for _, k in rows}
        assert kinds >= ({"+", "+inf"} if D.positive_only(form) else {"+", "-"} if D.is_layernorm(form) else {"+", "-", "+inf", "-inf"} if c.cols > D.EPV[code] else {"+"}), (c.id, kinds)
        if not D.is_norm(form) and not name.startswith("K1g"):                                  # (the clamped gates clamp an infinite u: a finite maximum)
            nan_rows = [i for i, (_, k) in enumerate(rows) if k == "nan"]
            assert nan_rows and (top[nan_rows] > 0x7F800000).all(), c.id
        if D.elementwise_with_h(form):
            full = form.ref(inp, code)
            for n in ("q", "sc", "h"):
                compare(n, want[n], full[n], code, f"{name} {c.id}: shortcut reference against form.ref")


# ---------------------------------------------------------------------------------------------------------------- tail slots
@pytest.mark.parametrize("code", CODES)
def test_tail_widths_leave_every_class_of_dead_slot(code):
    got = set()
    for nvec in D.TAIL_NVEC:
        lay = D.rownorm_layout(code, nvec * D.EPV[code])
        assert lay.tpr and D.dead_slot_classes(lay, nvec) == D.TAIL_CLASSES[nvec], (nvec, lay)
        got |= D.dead_slot_classes(lay, nvec)
        assert (nvec * D.EPV[code] + D.PAD) % D.EPV[code] == 0                               # the padded buffer keeps the vector path
    assert got == {"part of a wave", "whole waves", "slot"}
    assert {str(D.rownorm_layout(code, n * D.EPV[code])) for n in D.TAIL_NVEC} == {"rownorm:64x2", "rownorm:256x2", "rownorm:256x4"}


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("name", TAIL_FORMS)
def test_tail_cases_and_row_classes(name, code):
    form, epv = BY_NAME[name], D.EPV[code]
    cs = D.tail_cases(form, code)
    assert len(cs) == len(D.TAIL_NVEC) * len(form.vecs) * 2 * 7
    for nvec in D.TAIL_NVEC:
        for p in form.vecs:
            for where in ("last", "first"):
                mine = [c for c in cs if c[:3] == (nvec, p, where)]
                assert [c[3] for c in mine] == ["+inf", "-inf", "nan", "+0", "-0", "max", "subnormal"]
                assert len({c[4] for c in mine}) == min(7, epv), "each special in an element of its own (f32: four elements, walked in turn)"
    # one case in full: the special is where it should be and is what it should be; the row classes are populated
    for (nvec, p, where, sname, elem) in [c for c in cs if c[0] == 325 and c[1] == form.vecs[-1]]:
        inp, c_sp, cls = D.tail_inputs(form, code, nvec, p, where, sname, elem)
        cols = nvec * epv
        assert c_sp == (cols - epv + elem if where == "last" else elem) and sorted(set(cls)) == list(range(6)) and cls.count(0) == D.ROWS_PER_CLASS
        v = Q.to_f32(inp[p], code)
        want = dict(D.special_values(code))[sname]
        assert (np.isnan(v[c_sp]) if sname == "nan" else (v[c_sp] == want and np.signbit(v[c_sp]) == np.signbit(np.float32(want)))), (sname, v[c_sp])
        if sname == "subnormal":
            b = np.asarray(inp[p]).reshape(-1)[c_sp:c_sp + 1]
            assert v[c_sp] != 0 and ((b.view(np.uint32) & 0x7F800000) == 0 if code == 2 else (b & (0x7F80 if code == 0 else 0x7C00)) == 0)
        if sname == "max":
            with np.errstate(over="ignore"):
                assert np.isfinite(v[c_sp]) and np.isinf(Q.to_f32(Q.from_f32(np.array([v[c_sp]], np.float64) * 1.01, code), code)).all()
        others = np.delete(v, c_sp)
        assert np.isfinite(others).all() and (others != 0).all()
        prim = Q.to_f32(inp[D.plant_operand(form)], code)
        rows_of = lambda k: [i for i, c in enumerate(cls) if c == k]                          # noqa: E731
        assert all((Q.to_f32(inp[n], code)[rows_of(1), c_sp] == 0).all() and not Q.to_f32(inp[n], code)[rows_of(2)].any() for n in form.mats)
        assert all((Q.to_f32(inp[n], code)[rows_of(5), cols - epv:] == 0).all() for n in form.mats)
        assert np.isnan(Q.to_f32(inp[form.mats[0]], code)[rows_of(3)]).any(axis=1).all() and not np.isnan(prim[rows_of(0)]).any()
        assert (np.abs(prim[rows_of(4)]).argmax(axis=1) >= cols - epv).all()
    pad = Q.to_f32(D.pad_values(code, 4), code)
    assert np.isnan(pad[:, 0::2]).all() and (np.abs(pad[:, 1::2]) > 5e4).all() and pad.shape == (4, D.PAD)


@pytest.mark.parametrize("code", CODES)
def test_numpy_specification_and_c_oracle_agree_on_the_tail_operands(code):
    """K1n has both; eps = 0, so that the all-zero rows have rs = Inf; all three widths that the GPU test uses"""
    form = BY_NAME["K1n"]
    with eps_values(0.0, 0.0, 0.0):
        for (nvec, p, where, sname, elem) in D.tail_cases(form, code):
            inp, c_sp, cls = D.tail_inputs(form, code, nvec, p, where, sname, elem)
            want = form.ref(inp, code)                                                       # the C oracle
            q, sc, h = Q.rmsnorm_quantize(inp["x"], inp["w"], 0.0, code)[:3]
            for n, got in (("q", q), ("sc", sc), ("h", h)):
                compare(n, got, want[n], code, f"K1n {D.DT[code]} {p} {where} {sname}: numpy specification against the C oracle")
            if sname in ("+inf", "-inf"):                                                    # what the issue's reading rests on: the specification's scale is Inf, not NaN
                ordinary = [i for i, c in enumerate(cls) if c == 0]
                assert np.isinf(want["sc"][ordinary]).all()
                zeroed = [i for i, c in enumerate(cls) if c == 1]
                assert np.isnan(want["sc"][zeroed]).all()                                     # Inf * 0: a NaN the specification DOES ask for


# ---------------------------------------------------------------------------------------------------------------- K2
K2_CASES = [(path, code) for path in ("vec", "scalar") for code in CODES]


def _k2_shape(path):
    s = D.K2_VEC if path == "vec" else D.K2_SCALAR
    return s["rows"], s["cols"]


@pytest.mark.parametrize("path,code", K2_CASES)
def test_k2_plans_give_short_last_blocks_and_second_iterations(path, code):
    rows, cols = _k2_shape(path)
    batch = 8 * D.K2_AMAX_WAVES * D.K2_AMAX_UNROLL if path == "vec" else 4 * D.K2_COL_UNROLL
    plans = [D.k2_plan(code, rows, cols, a, e) for a, e in D.K2_SWITCHES[path]]
    assert all(p[0] == (path == "vec") for p in plans)
    assert any(-(-rows // p[1]) >= 3 and rows % p[1] and rows % p[1] < batch for p in plans), "three amax row blocks at least, the last one shorter than one iteration"
    assert any(p[1] >= 2 * batch and min(rows, p[1]) > batch for p in plans), "a second loop iteration inside one block"
    assert len({p[1] for p in plans}) >= 2 and len({p[2] for p in plans}) >= 2
    epv = D.EPV[code]
    if path == "vec":
        assert cols % epv == 0 and (cols // epv) % 8 and (cols // epv) % 64, "the clamped strips of both passes are live"
    else:
        assert cols % 8 and cols % 64


@pytest.mark.parametrize("path,code", K2_CASES)
def test_k2_every_position_class_holds_a_column_maximum(path, code):
    rows, cols = _k2_shape(path)
    holds = {D.k2_max_row(c, rows) for c in range(cols) if D.k2_kind(c) != "zero"}
    for a, e in D.K2_SWITCHES[path]:
        vec, rpb_a, rpb_e = D.k2_plan(code, rows, cols, a, e)
        seen = {}
        for r in range(rows):
            p = D.k2_position(code, rows, cols, r, 0, a, e)
            seen.setdefault((p["block"], p["iteration"]), set()).update({(p["wave"], p["row_group"], p["unroll"])} if r in holds else set())
        full = (D.K2_AMAX_WAVES * 8 * D.K2_AMAX_UNROLL) if vec else 4 * D.K2_COL_UNROLL
        whole = [k for k in seen if min(rows, (k[0] + 1) * rpb_a) - k[0] * rpb_a >= (k[1] + 1) * full]
        assert whole and all(len(seen[k]) == full for k in whole), "a (wave, row group, unroll slot) of a whole iteration without a column maximum"
        for rpb in (rpb_a, rpb_e):
            edges = {b * rpb for b in range(-(-rows // rpb))} | {min(rows, (b + 1) * rpb) - 1 for b in range(-(-rows // rpb))} | {rows - 1}
            assert edges <= holds, sorted(edges - holds)
    for s in range(cols // 64):
        kinds = {D.k2_kind(c) for c in range(64 * s, 64 * s + 64)}
        assert kinds == set(D.K2_KINDS), (s, kinds)


@pytest.mark.parametrize("path,code", K2_CASES)
def test_k2_reference_maxima_are_on_the_diagonal(path, code):
    rows, cols = _k2_shape(path)
    x = D.k2_matrix(code, rows, cols)
    assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(D.k2_matrix(code, rows, cols)).view(np.uint8))
    q, sc = C.quant_colwise(x, code)
    qn, sn = Q.quantize(x, code, 0)
    assert np.array_equal(q, qn) and np.array_equal(sc.view(np.uint32), sn.view(np.uint32)), "numpy specification and C oracle differ on the K2 operands"
    b = np.abs(Q.to_f32(x, code)).view(np.uint32) & np.uint32(0x7FFFFFFF)
    kinds = np.array([D.k2_kind(c) for c in range(cols)])
    live = kinds != "zero"
    want_row = np.array([D.k2_max_row(c, rows) for c in range(cols)])
    assert np.array_equal(b.argmax(axis=0)[live], want_row[live]) and not b[:, ~live].any()
    top = b[want_row, np.arange(cols)].copy()
    b[want_row, np.arange(cols)] = 0
    second = b.max(axis=0)
    assert (top[live] > second[live]).all()
    fin = live & (top < 0x7F800000)
    assert (top[fin].view(np.float32) >= 4 * second[fin].view(np.float32)).all()
    s_of = lambda bits_: Q.quantize_rows_with_amax(np.zeros((cols, 1), np.float32), 2, bits_)[1].view(np.uint32)                # noqa: E731
    assert (s_of(top)[live] != s_of(second)[live]).all(), "a column whose scale does not depend on its diagonal element"
    u = sc.view(np.uint32)
    assert (u[kinds == "nan"] == 0x7FC00000).all() and (u[kinds == "inf"] == 0x7F800000).all() and (sc[kinds == "zero"] == 1.0).all()
    e = u >> 23
    slow = (e < 67) | (e > 187) | ((u & 0x7FFFFF) == 0x7FFFFF)                                    # scale_fast_ok restated
    assert not slow[kinds == "ordinary"].any() and (code == 1 or (slow[kinds == "subnormal"].all() and slow[kinds == "huge"].all()))
    assert (u[kinds == "allones"] == 0x3FFFFFFF).all() if code == 2 else not slow[kinds == "allones"].any()


@pytest.mark.parametrize("code", [0, 1])
def test_no_16_bit_amax_has_a_scale_with_an_all_ones_significand(code):
    """why K2's "allones" column kind exists for f32 only: every finite positive bf16 / fp16 magnitude enumerated"""
    b = np.arange(1, 0x7F80 if code == 0 else 0x7C00, dtype=np.uint16)
    s = (Q.to_f32(b, code) / np.float32(127)).astype(np.float32).view(np.uint32)
    assert not ((s & 0x7FFFFF) == 0x7FFFFF).any()
    a = np.array([D.K2_ALLONES_F32], np.uint32).view(np.float32)
    assert (a / np.float32(127)).astype(np.float32).view(np.uint32)[0] == 0x3FFFFFFF
