"""-m gpu: K1ma / K1mo, pq_scaled_add_rmsnorm_quant_rows / scaled_add_rmsnorm_quantize / scaled_add — the scaled residual add of the Granite decoders fused into RMSNorm
+ per-token int8 quantisation.  Codes, scales, the stored sum and h against the CPU specification (tests/scaled_addnorm_spec.py: S1 in numpy, A1 by torch on the CPU,
N1-N6 / Q1-Q6 by the C oracle) and against K1a run on the product computed by torch on the GPU, bit for bit (NaNs as a class where an operand holds one).

WHY THIS FILE DOES NOT GO THROUGH THE TABLE.  The entry is named `..._rows`: tests/row_forms.py lists every export matching pq_\\w+_rowwise and, with the form counts that
tests/test_amax_design_host.py pins, is a yardstick that stays as it is.  The coverage the table gives the other row entries is brought here for this one: the two forms
below are `row_forms.Form` rows of this file's own, driven through row_forms.launch / compare, tests/amax_design.py (planted maxima, tail slots; restated dispatch) and
the far-strided arena of tests/test_gpu_row_addressing.py.  The guarded buffers restate tests/guarded_workspace.py's idea (sentinel margins checked as a whole) for
matrix operands, which that module's allocator patch does not cover.

Switch set here, by name (tests/test_switch_coverage.py): PQ_RMS_WAVE_MAX."""
import numpy as np
import pytest
import torch

from oracle import qspec_numpy as Q
from protoquant_amd.qtensor import scaled_add, scaled_add_rmsnorm_quantize  # noqa: F401  (the ops this file is about)
from tests import addnorm_spec as A
from tests import amax_design as D
from tests import row_forms as RF
from tests import scaled_addnorm_spec as S
from tests.gpu_util import TD, bits, to_gpu
from tests.row_forms import D as LD_OF
from tests.row_forms import Form, P, T, compare, eps_values, launch, mismatch_rows

pytestmark = pytest.mark.gpu

SYM = "pq_scaled_add_rmsnorm_quant_rows"
MULT = [0.22]                     # the multiplier every call and reference below reads


def _call(L, o, c, R, N, st):
    return getattr(L, SYM)(P(o.x), LD_OF(o.x), P(o.r), LD_OF(o.r), MULT[0], P(o.s), LD_OF(o.s), P(o.w), RF.EPS, c, R, N, P(o.q), LD_OF(o.q), P(o.sc), P(o.h), LD_OF(o.h), st)


def _ref_ma(i, c):
    q, sc, s, h = S.scaled_add_rmsnorm_quantize(T(i["x"], c), T(i["r"], c), MULT[0], T(i["w"], c), RF.EPS)
    return dict(q=q, sc=sc, s=s, h=h)


K1MA = Form("K1ma", mats=("x", "r"), vecs=("w",), outs=("s", "h"), alias=("s", "x"), calls=((SYM, _call),), ref=_ref_ma)
K1MO = Form("K1mo", mats=("x", "r"), outs=("s",), nq=0, alias=("s", "x"), calls=((SYM, _call),),
            ref=lambda i, c: dict(s=A.to_bits(S.scaled_add(T(i["x"], c), T(i["r"], c), MULT[0]))))


@pytest.fixture(autouse=True)
def _default_multiplier():
    MULT[0] = 0.22
    yield
    MULT[0] = 0.22


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    from protoquant_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return protoquant_amd


# ---------------------------------------------------------------------------------------------------------------- guarded operands
PADC, PADR = 64, 1                # columns (a multiple of 16 bytes in every dtype: the vector layouts stay reachable) and rows of sentinel around every matrix operand
SENT = {0: 0x5A5B, 1: 0x5A5B, 2: 0x5A5B5A5B}          # finite in every dtype
SENT_Q = 0x5B


class Guard:
    """a matrix operand as a column block of a wider, taller sentinel-filled buffer"""

    def __init__(self, code, rows, cols, dtype=None):
        self.q = dtype is torch.int8
        self.sent = SENT_Q if self.q else SENT[code]
        it = torch.int8 if self.q else (torch.int32 if code == 2 else torch.int16)
        self.raw = torch.full((rows + 2 * PADR, cols + 2 * PADC), self.sent, dtype=it, device="cuda")
        self.win_raw = self.raw[PADR:PADR + rows, PADC:PADC + cols]
        self.view = self.win_raw if self.q else self.raw.view(TD[code])[PADR:PADR + rows, PADC:PADC + cols]

    def margins_clean(self):
        """the whole buffer outside the window still holds the sentinel (the window is overwritten with it first)"""
        keep = self.win_raw.clone()
        self.win_raw.fill_(self.sent)
        ok = bool((self.raw == self.sent).all())
        self.win_raw.copy_(keep)
        return ok


def _guarded_vec(n):
    t = torch.full((n + 32,), SENT[2], dtype=torch.int32, device="cuda")
    return t, t[16:16 + n].view(torch.float32)


def run_guarded(code, inp, m, out_mode="none", with_h=True, quant=True, what=""):
    """one raw C-ABI call on guarded operands; returns the outputs as `compare` takes them after checking every margin and every input that must stay unwritten"""
    from protoquant_amd import _lib
    L = _lib.lib()
    rows, cols = inp["x"].shape
    g = {n: Guard(code, rows, cols) for n in ("x", "r")}
    for n in ("x", "r"):
        g[n].view.copy_(to_gpu(inp[n], code))
    if out_mode == "none":
        g["s"] = Guard(code, rows, cols)
    else:
        g["s"] = g[out_mode]
    o = RF.Ops(x=g["x"].view, r=g["r"].view, s=g["s"].view)
    sc_guard = None
    if quant:
        o["w"] = to_gpu(inp["w"], code)
        g["q"] = Guard(code, rows, cols, torch.int8)
        o["q"] = g["q"].view
        sc_guard, o["sc"] = _guarded_vec(rows)
        if with_h:
            g["h"] = Guard(code, rows, cols)
            o["h"] = g["h"].view
    MULT[0] = m
    _lib.check(_call(L, o, code, rows, cols, torch.cuda.current_stream().cuda_stream), SYM)
    torch.cuda.synchronize()
    got = dict(s=bits(o.s))
    if quant:
        got["q"], got["sc"] = o.q.contiguous().cpu().numpy(), bits(o.sc)
        if with_h:
            got["h"] = bits(o.h)
        assert bool((sc_guard[:16] == SENT[2]).all()) and bool((sc_guard[16 + rows:] == SENT[2]).all()), f"{what}: the scale vector was written outside its {rows} elements"
    for n, gd in g.items():
        assert gd.margins_clean(), f"{what}: the margin around {n} was written"
    for n in ("x", "r"):
        if out_mode != n:
            assert np.array_equal(bits(g[n].view), np.asarray(inp[n]).view(np.uint32) if code == 2 else inp[n]), f"{what}: {n} was written"
    return got


def _inputs(code, rows, cols, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, cols)) * 4.0).astype(np.float32)          # (a sublayer output a few times the stream: the product x * 0.22 is of the stream's order)
    r = rng.standard_normal((rows, cols)).astype(np.float32)
    w = (1.0 + 0.25 * rng.standard_normal(cols)).astype(np.float32)
    return dict(x=Q.from_f32(x, code), r=Q.from_f32(r, code), w=Q.from_f32(w, code))


def _check_all(pq, code, inp, m, out_mode, what, k1a=True):
    """K1ma with and without h_out and K1mo on the same operands: against the specification, and K1ma against K1a on the product computed by torch on the GPU"""
    MULT[0] = m
    want = _ref_ma(inp, code)
    for with_h in (True, False):
        got = run_guarded(code, inp, m, out_mode, with_h, True, what)
        for n in sorted(got):
            compare(n, got[n], want[n], code, f"{what} (K1ma{'' if with_h else ', no h_out'})")
    got = run_guarded(code, inp, m, out_mode, False, False, what)
    compare("s", got["s"], want["s"], code, f"{what} (K1mo)")
    if k1a:
        xd, rd, wd = (to_gpu(inp[n], code) for n in ("x", "r", "w"))
        with torch.no_grad():
            qa, sa, ha = pq.add_rmsnorm_quantize(xd * m, rd, wd, RF.EPS, return_h=True)          # p by torch eager, then K1a
            qt, sm, hm = pq.scaled_add_rmsnorm_quantize(xd, rd, m, wd, RF.EPS, return_h=True)
            so = pq.scaled_add(xd, rd, m)
        for name, a, b in (("codes", qt.int_data, qa.int_data), ("scales", qt.scale, qa.scale), ("summed", sm, sa), ("h", hm, ha), ("summed (K1mo)", so, sa)):
            assert torch.equal(a, b), f"{what}: {name} differ from K1a on torch's product"


# ---------------------------------------------------------------------------------------------------------------- every layout
def _layout_cases():
    out = []
    for code in (0, 1, 2):
        for lay, (sw, lo, hi) in sorted(D.reachable(K1MA, code).items(), key=lambda kv: (kv[0].tpr, kv[0].vpt)):
            out.append((code, lay, sw, lo * D.EPV[code]))          # the smallest width that reaches the layout
    return out


LAYOUTS = _layout_cases()


def test_the_cases_reach_every_layout_of_the_dispatch():
    for code in (0, 1, 2):
        assert {(l.tpr, l.vpt) for c, l, _, _ in LAYOUTS if c == code} == {(64, v) for v in (1, 2, 4, 8)} | {(256, v) for v in (1, 2, 4, 8, 16)}


@pytest.mark.parametrize("code,lay,sw,cols", LAYOUTS, ids=[f"{D.DT[c]}-{l.tpr}x{l.vpt}-{n}" for c, l, _, n in LAYOUTS])
def test_every_vector_layout_matches_the_spec_and_k1a(pq, pq_opt, code, lay, sw, cols):
    assert D.rownorm_layout(code, cols, dict(sw).get("PQ_RMS_WAVE_MAX", 256)) == lay
    for n, v in sw:
        pq_opt(n, v)
    for k, rows in enumerate((1, 3, 4, 5)):                       # four rows per block in the wave layout: full, partial and a second block
        m = S.MULTIPLIERS[(k + lay.vpt + code) % len(S.MULTIPLIERS)]
        _check_all(pq, code, _inputs(code, rows, cols, 1000 * code + cols + rows), m, ("none", "x", "r")[(k + lay.vpt) % 3], f"{D.DT[code]} {lay} {rows}x{cols} m={m}")


@pytest.mark.parametrize("code", [0, 1, 2], ids=D.DT)
@pytest.mark.parametrize("cols", D.GENERIC_WIDTHS)
def test_ragged_widths_take_the_generic_kernel(pq, code, cols):
    assert not D.rownorm_layout(code, cols).tpr
    for k, rows in enumerate((1, 3, 4, 5)):
        m = S.MULTIPLIERS[(k + code) % len(S.MULTIPLIERS)]
        _check_all(pq, code, _inputs(code, rows, cols, 77 * code + cols + rows), m, ("none", "x", "r")[k % 3], f"{D.DT[code]} generic {rows}x{cols} m={m}")


@pytest.mark.parametrize("code", [0, 1, 2], ids=D.DT)
def test_every_multiplier_and_the_identity(pq, code):
    """the host test's multipliers on one wave layout, one 256-thread layout and the generic kernel; multiplier = 1.0 is K1a, bit for bit"""
    for cols in (64 * D.EPV[code], 300 * D.EPV[code], 333):
        inp = _inputs(code, 5, cols, 31 * code + cols)
        for j, m in enumerate(S.MULTIPLIERS):
            _check_all(pq, code, inp, m, ("none", "x", "r")[j % 3], f"{D.DT[code]} 5x{cols} m={m}")
        xd, rd, wd = (to_gpu(inp[n], code) for n in ("x", "r", "w"))
        qa, sa, ha = pq.add_rmsnorm_quantize(xd, rd, wd, RF.EPS, return_h=True)
        for one in (1.0, 1):
            qt, sm, hm = pq.scaled_add_rmsnorm_quantize(xd, rd, one, wd, RF.EPS, return_h=True)
            assert torch.equal(qt.int_data, qa.int_data) and torch.equal(qt.scale, qa.scale) and torch.equal(sm, sa) and torch.equal(hm, ha)
            assert torch.equal(pq.scaled_add(xd, rd, one), rd + xd)


# ---------------------------------------------------------------------------------------------------------------- f32: two roundings, never the FMA
def _fma_telling_f32(rows, cols, m, seed):
    """f32 x and r in which EVERY element tells fma(x, m, r) from the two-rounding chain: per element the first of 24 seeded candidate pairs that does"""
    rng = np.random.default_rng(seed)
    x = np.zeros((rows, cols), np.float32)
    r = np.zeros((rows, cols), np.float32)
    todo = np.ones((rows, cols), bool)
    for _ in range(24):
        cx = (rng.standard_normal((rows, cols)) * 4.0).astype(np.float32)
        cr = rng.standard_normal((rows, cols)).astype(np.float32)
        two = (cr + (cx * np.float32(m)).astype(np.float32)).astype(np.float32)
        tells = S.fma_single_rounding(cx, m, cr).view(np.uint32) != two.view(np.uint32)
        take = todo & tells
        x[take], r[take] = cx[take], cr[take]
        todo &= ~tells
    x[todo], r[todo] = cx[todo], cr[todo]
    return x, r


@pytest.mark.parametrize("lay", [(64, 4), (256, 2), (256, 16), (0, 0)], ids=["64x4", "256x2", "256x16", "generic"])
def test_f32_rows_round_the_product_on_its_own(pq, lay):
    """designed so that every (lane, slot) holds at least one element where FMA and two roundings differ — asserted on the reference before the launch"""
    tpr, vpt = lay
    nvec = tpr * vpt if tpr else 0
    cols = nvec * 4 if tpr else 1003
    if tpr:
        assert D.rownorm_layout(2, cols) == D.Layout("rownorm", tpr, vpt)
    for m in (0.22, 1.0 / 3.0):
        x, r = _fma_telling_f32(5, cols, m, 4242 + cols)
        inp = dict(x=x, r=r, w=_inputs(2, 1, cols, 5)["w"])
        MULT[0] = m
        want = _ref_ma(inp, 2)
        fma = S.fma_single_rounding(x, m, r)
        differs = fma.view(np.uint32) != want["s"].view(np.uint32)
        per_vector = differs[:, :cols // 4 * 4].reshape(5, -1, 4).any(axis=2)
        assert per_vector.all(), "the operands do not tell the FMA from two roundings in every (lane, slot)"
        assert np.array_equal(want["s"].view(np.uint32), (torch.from_numpy(r) + torch.from_numpy(x) * m).numpy().view(np.uint32))          # torch eager on the CPU
        _check_all(pq, 2, inp, m, "none", f"f32 {lay} m={m}: FMA-telling operands")


# ---------------------------------------------------------------------------------------------------------------- special values
@pytest.mark.parametrize("code", [0, 1, 2], ids=D.DT)
@pytest.mark.parametrize("cols", [256, 4096, 333])
def test_special_values(pq, code, cols):
    """NaN, +-Inf, +-0, subnormals and the largest finite value under |m| > 1, in x and in the residual"""
    rows = 12
    i = _inputs(code, rows, cols, 555 + cols + code)
    x, r = Q.to_f32(i["x"], code).copy(), Q.to_f32(i["r"], code).copy()
    sv = dict(D.special_values(code))
    big, sub = sv["max"], sv["subnormal"]
    x[0, 3] = np.nan
    r[1, 5] = np.nan
    x[2, 1], r[2, 2] = np.inf, -np.inf
    x[3, 7], r[3, 7] = np.inf, -np.inf                     # Inf * m - Inf: a NaN made by the add (for m > 0)
    x[4], r[4] = 0.0, 0.0
    x[5], r[5] = -0.0, -0.0                                # -0 * m: the sign of m decides
    x[6], r[6] = 0.0, -0.0
    x[7, :] = big                                          # overflows under |m| > 1 in the product itself
    x[8, 0], r[8, 0] = big, -big
    x[9], r[9] = x[9] * 0 + sub, r[9] * 0 - sub            # subnormals of the storage dtype: the product rounds inside the subnormal range
    x[10, ::2], r[10, 1::2] = -big, big
    x[11, 4], r[11, 4] = -np.inf, 1.0
    inp = dict(x=Q.from_f32(x, code), r=Q.from_f32(r, code), w=i["w"])
    for j, m in enumerate((S.OVERFLOWING, 0.22, -0.5, -S.OVERFLOWING)):
        _check_all(pq, code, inp, m, ("none", "x", "r")[j % 3], f"{D.DT[code]} special values, {cols} columns, m={m}", k1a=False)
    MULT[0] = S.OVERFLOWING
    s = Q.to_f32(_ref_ma(inp, code)["s"], code)
    assert np.isinf(s[7]).all() and np.isnan(s[3, 7])


# ---------------------------------------------------------------------------------------------------------------- dead slots (as tests/test_gpu_tail_slots.py)
@pytest.mark.parametrize("nvec", D.TAIL_NVEC)
@pytest.mark.parametrize("code", [0, 1, 2], ids=D.DT)
def test_parameters_in_dead_slots_stay_out(code, nvec):
    """+-Inf / NaN / +-0 / max / a subnormal in the last live weight vector (the control: in the first), NaN and huge values in the columns beyond the row, six row
    classes, eps = 0; K1mo on the same operands (its dead slots must stay out of the stores)"""
    epv = D.EPV[code]
    cols = nvec * epv
    lay = D.rownorm_layout(code, cols)
    assert lay.tpr and D.dead_slot_classes(lay, nvec) == D.TAIL_CLASSES[nvec] and (cols + D.PAD) % epv == 0
    failures = []
    with eps_values(0.0, 0.0, 0.0):
        for (_, pname, where, sname, elem) in [c for c in D.tail_cases(K1MA, code) if c[0] == nvec]:
            inp, c_sp, cls = D.tail_inputs(K1MA, code, nvec, pname, where, sname, elem)
            want = K1MA.ref(inp, code)
            pad = D.pad_values(code, len(cls))
            got = launch(K1MA, code, inp, pad=pad)
            if (where, sname) == ("last", "nan"):
                got["s (K1mo)"] = launch(K1MO, code, inp, pad=pad)["s"]
                want["s (K1mo)"] = want["s"]
            for n in sorted(got):
                rows = mismatch_rows("s" if n.startswith("s ") else n, got[n], want[n], code)
                if rows:
                    failures.append(f"{pname}[{where} vector, element {elem}] = {sname}: {n} differs in row {rows[0]} ({D.ROW_CLASSES[cls[rows[0]]]}; {len(rows)} rows)")
    assert not failures, f"K1ma {D.DT[code]} {lay} at {nvec} vectors: " + "; ".join(failures[:6]) + (f" ... {len(failures)} in all" if len(failures) > 6 else "")


# ---------------------------------------------------------------------------------------------------------------- planted maxima (as tests/test_gpu_amax_positions.py)
AMAX_CASES = [(code, case) for code in (0, 1, 2) for case in sorted(D.cases(K1MA, code), key=lambda c: (c.cols, c.mode, str(c.layout)))]


@pytest.mark.parametrize("code,case", AMAX_CASES, ids=[f"{D.DT[code]}-{c.id}" for code, c in AMAX_CASES])
def test_planted_maximum_is_seen(pq_opt, code, case):
    """the row maximum of |h| at one designed position per row — every column of the narrow layouts; every lane's first and last live slot, every slot's edge lanes and
    the last vectors of the wide ones.  The condition 'the planted element is the strict maximum, four times the runner-up' is checked on the reference alone."""
    assert D.layout_of(K1MA, code, case.cols, dict(case.switches)) == case.layout
    inp, rows = D.planted_inputs(K1MA, code, case)
    want = D.reference(K1MA, inp, rows, code)
    D.check_planted(K1MA, inp, rows, want, code, f"K1ma {D.DT[code]} cols={case.cols}")
    for n, v in case.switches:
        pq_opt(n, v)
    got = launch(K1MA, code, inp)
    bad = {n: mismatch_rows(n, got[n], want[n], code) for n in sorted(got)}
    bad = {n: r for n, r in bad.items() if r}
    if bad:
        first = sorted({i for r in bad.values() for i in r})
        raise AssertionError(f"K1ma {D.DT[code]} {case.id}: " + ", ".join(f"{n}: {len(r)} of {len(rows)} rows differ" for n, r in bad.items())
                             + " -- " + D.explain(K1MA, code, case, rows, first))


# ---------------------------------------------------------------------------------------------------------------- addressing past 2^31 elements (as tests/test_gpu_row_addressing.py)
FAR = {0: 512, 1: 4096, 2: 333}          # one layout per dtype: one wave per row / 256 threads per row / the generic kernel


@pytest.fixture(scope="module", params=[0, 1, 2], ids=D.DT)
def far_arena(request):
    """tests/test_gpu_row_addressing.py's arena — column blocks of one flat sentinel-filled buffer at a pitch of 2^30 + 64 elements — with six rows in every dtype"""
    from protoquant_amd import _lib
    from tests import test_gpu_row_addressing as R
    _lib.lib()
    code, rows = request.param, 6
    a = R.Arena.__new__(R.Arena)
    a.code, a.rows = code, rows
    ns, nq = R.buf_elems(code, rows), R.FRONT_Q + (rows - 1) * R.LD + R.NBLK * R.BLK + R.TAIL
    R._need(ns * R.ESIZE[code] + nq)
    a.s = torch.empty(ns, dtype=TD[code], device="cuda")
    a.si = a.s.view(torch.int32 if code == 2 else torch.int16)
    a.q = torch.empty(nq, dtype=torch.int8, device="cuda")
    a.used = []
    a.refill()
    yield a
    a.s = a.si = a.q = None
    a.used = []
    del a
    torch.cuda.empty_cache()


@pytest.mark.parametrize("alias", [False, True], ids=["fresh", "sum_out-is-x"])
def test_row_offsets_past_2g(far_arena, alias):
    from tests import test_gpu_row_addressing as R
    assert R.LD == (1 << 30) + 64 and far_arena.rows == 6
    cols = FAR[far_arena.code]
    R.run_case(far_arena, K1MA, cols, alias=alias)
    R.run_case(far_arena, K1MO, cols, alias=alias)


# ---------------------------------------------------------------------------------------------------------------- the Python entries
def test_batch_shapes_out_and_refusals(pq):
    from protoquant_amd import _lib
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 7, 512, generator=g).to(torch.bfloat16).cuda()
    r = torch.randn(2, 7, 512, generator=g).to(torch.bfloat16).cuda()
    w = torch.ones(512, dtype=torch.bfloat16, device="cuda")
    qt, s = pq.scaled_add_rmsnorm_quantize(x, r, 0.22, w)
    ref = pq.rmsnorm_quantize(r + x * 0.22, w)
    assert s.shape == x.shape and qt.int_data.shape == x.shape and qt.scale.shape == (14,)
    assert torch.equal(s, r + x * 0.22) and torch.equal(qt.int_data, ref.int_data) and torch.equal(qt.scale, ref.scale)
    assert torch.equal(pq.scaled_add(x, r, 0.22), s)
    out = torch.empty_like(x)
    assert pq.scaled_add(x, r, 0.22, out=out) is out and torch.equal(out, s)
    xc = x.clone()
    assert pq.scaled_add_rmsnorm_quantize(xc, r, 0.22, w, out=xc)[1] is xc and torch.equal(xc, s)
    e = torch.empty(0, 512, dtype=torch.bfloat16, device="cuda")
    qe, se = pq.scaled_add_rmsnorm_quantize(e, e, 0.22, w)
    assert se.shape == (0, 512) and qe.int_data.shape == (0, 512) and pq.scaled_add(e, e, 0.22).shape == (0, 512)
    buf = torch.zeros(9, 512, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_lib.PQError, match="sum_out overlaps x"):
        pq.scaled_add(buf[:8], r.reshape(14, 512)[:8], 0.22, out=buf[1:9])
    with pytest.raises(TypeError, match="multiplier"):
        pq.scaled_add(x, r, torch.tensor(0.22, device="cuda"))
