"""GPU: a dead slot's h is zero, whatever the parameters hold.

The vector layouts of the norm kernels load CLAMPED DUPLICATES into the slots past a row's end — of the row's last vector and of the last vector of every [cols]
parameter — and must keep them out of the result.  Here the last 16-byte vector of one parameter (weight, bias, post-weight; either group of K1pl / K1l2) holds, in turn,
+Inf, -Inf, NaN, +0, -0, the largest finite value and a subnormal, each in an element of its own, at widths that leave part of a wave, whole waves and a whole slot index
dead (tests/amax_design.py: 67, 325 and 600 vectors); the same values in the FIRST vector are the control.  Six row classes cross them: an ordinary row; a row that is zero
exactly under the special element (Inf * 0 is a NaN the specification DOES ask for); an all-zero row with eps = 0 (rs = Inf); a NaN row; a row whose last live vector
holds the maximum; a row whose last live vector is all zeros.  The matrix inputs are column blocks of wider buffers whose next columns hold NaN and huge values: a slot
that reads past the row instead of clamping shows up too.  Every output against the CPU specification: codes and scales bit for bit, h / s with NaNs as a class.

A kernel that multiplies a dead slot's zero by the duplicated Inf puts a NaN into the row maximum: scale = NaN where the specification has Inf."""
import pytest

from tests import amax_design as D
from tests.row_forms import BY_NAME, FORMS, eps_values, launch, mismatch_rows

TAIL_FORMS = [f.name for f in FORMS if not f.custom and f.vecs]


def _dead(lay, nvec):
    dead = [(t // 64, t % 64, s) for s in range(lay.vpt) for t in range(lay.tpr) if s * lay.tpr + t >= nvec]
    return f"{len(dead)} dead slots, from wave {dead[0][0]} lane {dead[0][1]} slot {dead[0][2]} on, duplicate vector {nvec - 1}"


@pytest.mark.gpu
@pytest.mark.parametrize("nvec", D.TAIL_NVEC)
@pytest.mark.parametrize("code", [0, 1, 2], ids=D.DT)
@pytest.mark.parametrize("name", TAIL_FORMS)
def test_parameters_in_dead_slots_stay_out(name, code, nvec):
    form, epv = BY_NAME[name], D.EPV[code]
    cols = nvec * epv
    lay = D.rownorm_layout(code, cols)
    assert lay.tpr and D.dead_slot_classes(lay, nvec) == D.TAIL_CLASSES[nvec] and (cols + D.PAD) % epv == 0
    failures = []
    with eps_values(0.0, 0.0, 0.0):
        for (_, pname, where, sname, elem) in [c for c in D.tail_cases(form, code) if c[0] == nvec]:
            inp, c_sp, cls = D.tail_inputs(form, code, nvec, pname, where, sname, elem)
            want = form.ref(inp, code)
            got = launch(form, code, inp, pad=D.pad_values(code, len(cls)))
            assert set(want) >= set(got), (sorted(want), sorted(got))
            for n in sorted(got):
                rows = mismatch_rows(n, got[n], want[n], code)
                if rows:
                    i = rows[0]
                    g, w = got[n][i], want[n][i]
                    shown = f"got {g.ravel()[:1].view('uint32')[0]:#010x} want {w.ravel()[:1].view('uint32')[0]:#010x}" if n.startswith("sc") else f"{len(rows)} rows"
                    failures.append(f"{pname}[{where} vector, element {elem}] = {sname}: {n} differs in row {i} ({D.ROW_CLASSES[cls[i]]}; {shown})")
    assert not failures, (f"{name} {D.DT[code]} {lay} at {nvec} vectors ({_dead(lay, nvec)}; the special sits in {D.describe(lay, code, cols - epv)} or in vector 0): "
                          + "; ".join(failures[:6]) + (f" ... {len(failures)} in all" if len(failures) > 6 else ""))
