"""GPU: every quantising row kernel sees every position of its row layout (tests/amax_design.py).

One case per (form, dtype, layout, width): the C-ABI entry runs on operands whose row i has its strict maximum of |h| at one designed position p(i) — a lane, a slot, an
element of the 16-byte vector — and every output is compared with the CPU specification: codes, scales and the amax vector bit for bit, h / s with NaNs as a class.  A lane,
a vector slot, a wave's partial or a clamped tail slot that is left out of the maximum changes the scale of exactly the rows planted there, and the failure names them.
Before the kernel runs, the case asserts on the reference alone that the maximum IS at p(i), a factor of 4 above the runner-up, and that the scale depends on it
(amax_design.check_planted): that is what makes a passing comparison mean "position p(i) was seen".  Each case also states the layout the restated dispatch sends it to.

K2 (per-channel columns) takes square-ish matrices with a dominant diagonal — column c has its maximum at row c mod rows, the column kinds (ordinary, all zero, NaN, +-Inf, a
subnormal and the largest finite amax and, for f32, an amax whose scale has an all-ones significand) alternate inside every 64-lane strip, so col_encode takes its
true-division path in every strip (the division-free encode is held by the Gaussian K2 tests of tests/test_gpu_parity.py) — on the vector and on the scalar path under several PQ_K2_BLOCKS_A / PQ_K2_BLOCKS_E, so that
col_amax runs three row blocks with a short last one and, in another case, three loop iterations inside one block; a column that differs is named by row block, iteration,
unroll slot, wave and row group.

Switches set here, by name (tests/test_switch_coverage.py): PQ_K1_RPW, PQ_K1_ST16, PQ_SILU_TPR, PQ_RMS_WAVE_MAX, PQ_K2_BLOCKS_A, PQ_K2_BLOCKS_E."""
from functools import lru_cache

import pytest

from tests import amax_design as D
from tests.row_forms import BY_NAME, FORMS, launch, mismatch_rows

SWITCHES_SET = ("PQ_K1_RPW", "PQ_K1_ST16", "PQ_SILU_TPR", "PQ_RMS_WAVE_MAX")
AMAX_FORMS = [f.name for f in FORMS if not f.custom and (f.nq or f.amax) and f.name != "K2"]
CASES = [(name, code, case) for name in AMAX_FORMS for code in (0, 1, 2) for case in sorted(D.cases(BY_NAME[name], code), key=lambda c: (c.cols, c.mode, str(c.layout)))]


@lru_cache(maxsize=1)
def _design(name, code, cols, mode, tpr, vpt):
    """operands and reference, built once per (form, dtype, width) and shared by the switch values that run on them (the cases of one width are neighbours)"""
    form = BY_NAME[name]
    case = next(c for c in D.cases(form, code) if (c.cols, c.mode) == (cols, mode) and (mode == "all" or (c.layout.tpr, c.layout.vpt) == (tpr, vpt)))
    inp, rows = D.planted_inputs(form, code, case)
    want = D.reference(form, inp, rows, code)
    D.check_planted(form, inp, rows, want, code, f"{name} {D.DT[code]} cols={cols}")
    return inp, rows, want


def test_cases_name_only_listed_switches():
    assert {n for _, _, c in CASES for n, _ in c.switches} == set(SWITCHES_SET)
    assert len({(n, code, c.id) for n, code, c in CASES}) == len(CASES) > 800


@pytest.mark.gpu
@pytest.mark.parametrize("name,code,case", CASES, ids=[f"{n}-{D.DT[code]}-{c.id}" for n, code, c in CASES])
def test_planted_maximum_is_seen(name, code, case):
    from protoquant_amd import _lib
    form = BY_NAME[name]
    assert D.layout_of(form, code, case.cols, dict(case.switches)) == case.layout                  # dense operands, aligned bases: the restated dispatch decides
    wide = case.mode == "wide"
    inp, rows, want = _design(name, code, case.cols, case.mode, case.layout.tpr if wide else 0, case.layout.vpt if wide else 0)
    try:
        for n, v in case.switches:
            _lib.set_option(n, v)
        got = launch(form, code, inp)
    finally:
        for n, _ in case.switches:
            _lib.set_option(n, "")
    assert set(want) >= set(got), (sorted(want), sorted(got))
    bad = {n: mismatch_rows(n, got[n], want[n], code) for n in sorted(got)}
    bad = {n: r for n, r in bad.items() if r}
    if bad:
        first = sorted({i for r in bad.values() for i in r})
        raise AssertionError(f"{name} {D.DT[code]} {case.id}: " + ", ".join(f"{n}: {len(r)} of {len(rows)} rows differ" for n, r in bad.items())
                             + " -- " + D.explain(form, code, case, rows, first))


# ---------------------------------------------------------------------------------------------------------------- K2: column maxima on a dominant diagonal
@lru_cache(maxsize=1)
def _k2_design(path, code):
    import numpy as np
    from oracle import c_oracle as C
    s = D.K2_VEC if path == "vec" else D.K2_SCALAR
    x = D.k2_matrix(code, s["rows"], s["cols"])
    return x, dict(zip(("q", "sc"), C.quant_colwise(x, code))), dict(zip(("q", "sc"), C.quant_rowwise(np.ascontiguousarray(x), code)))


K2_RUNS = [(path, code, a, e) for path in ("vec", "scalar") for code in (0, 1, 2) for a, e in D.K2_SWITCHES[path]]


@pytest.mark.gpu
@pytest.mark.parametrize("path,code,blocks_a,blocks_e", K2_RUNS, ids=[f"{p}-{D.DT[c]}-PQ_K2_BLOCKS_A={a}-PQ_K2_BLOCKS_E={e}" for p, c, a, e in K2_RUNS])
def test_k2_column_maxima_are_seen(path, code, blocks_a, blocks_e):
    """col_amax's row blocks, loop iterations, unroll slots, waves and row groups, the LDS merge and the atomics, and col_encode's clamped batches, under several
    PQ_K2_BLOCKS_A / PQ_K2_BLOCKS_E; the same matrix by rows through K1"""
    import numpy as np
    from protoquant_amd import _lib
    x, want, want_rows = _k2_design(path, code)
    rows, cols = x.shape
    assert D.k2_plan(code, rows, cols, blocks_a, blocks_e)[0] == (path == "vec")
    try:
        _lib.set_option("PQ_K2_BLOCKS_A", blocks_a or "")
        _lib.set_option("PQ_K2_BLOCKS_E", blocks_e or "")
        got = launch(BY_NAME["K2"], code, dict(x=x))
    finally:
        _lib.set_option("PQ_K2_BLOCKS_A", "")
        _lib.set_option("PQ_K2_BLOCKS_E", "")
    bad_sc = np.flatnonzero(got["sc"] != want["sc"].view(np.uint32))
    bad_q = np.flatnonzero((got["q"] != want["q"]).any(axis=0))
    if len(bad_sc) or len(bad_q):
        first = sorted(set(bad_sc.tolist()) | set(bad_q.tolist()))[:4]
        raise AssertionError(f"K2 {D.DT[code]} {rows} x {cols} PQ_K2_BLOCKS_A={blocks_a} PQ_K2_BLOCKS_E={blocks_e}: {len(bad_sc)} scales and {len(bad_q)} code columns differ -- "
                             + "; ".join(f"{D.k2_kind(c)} " + D.k2_describe(code, rows, cols, D.k2_max_row(c, rows), c, blocks_a, blocks_e) for c in first))
    if (blocks_a, blocks_e) == (0, 0):
        got1 = launch(BY_NAME["K1"], code, dict(x=x))
        for n in ("q", "sc"):
            r = mismatch_rows(n, got1[n], want_rows[n], code)
            assert not r, f"K1 on the K2 matrix, {D.DT[code]} {rows} x {cols}: {n} differs in rows {r[:5]}"
