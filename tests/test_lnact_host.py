"""CPU: the host side of K1l (pq_layernorm_quant_rowwise / layernorm_quantize) and K1u (pq_act_quant_rowwise / act_quantize): the symbols are declared, exported and
bound; every bad argument is refused and named before any HIP call; empty problems are no-ops; the Python entries have no CPU path; the code objects hold every row
layout without scratch; and the specifications (tests/lnorm_spec.py, tests/act_spec.py) meet their written bars — relu is torch's bit for bit, both GELUs are within
1 ulp of the exact value on every 16-bit pattern and miss the correctly rounded value less often than torch's eager kernels do."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import qspec_numpy as Q
from tests import act_spec as AS
from tests import lnorm_spec as LS
from tests.code_objects import kernels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN, ACT = "pq_layernorm_quant_rowwise", "pq_act_quant_rowwise"


def test_symbols_declared_exported_and_bound():
    from protoquant_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pq_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for sym, nargs in ((LN, 14), (ACT, 12)):
        assert re.search(r"\b%s\s*\(" % sym, hdr), f"pq_hip.h does not declare {sym}"
        assert hasattr(L, sym) and sym in _lib.EXPORTS and len(getattr(L, sym).argtypes) == nargs
    for name, val in (("PQ_ACT_RELU", 0), ("PQ_ACT_GELU_TANH", 1), ("PQ_ACT_GELU_ERF", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr)
    assert _lib.ACT_KINDS == {"relu": 0, "gelu_tanh": 1, "gelu_erf": 2}
    assert L.pq_version() == 1                                          # additions: the ABI version stays
    import protoquant_amd as pq
    for n in ("layernorm_quantize", "act_quantize", "LayerNormQuant", "ActQuant", "fuse_layernorm_layers"):
        assert n in pq.__all__ and callable(getattr(pq, n))


def _ln(L, **kw):
    a = dict(x=0x10000, ldx=128, w=0x40000, b=0x48000, eps=1e-5, dtype=0, rows=4, cols=128, q=0x50000, ldq=128, scale=0x60000, h=None, ldh=0)
    a.update(kw)
    return L.pq_layernorm_quant_rowwise(a["x"], a["ldx"], a["w"], a["b"], a["eps"], a["dtype"], a["rows"], a["cols"], a["q"], a["ldq"], a["scale"], a["h"], a["ldh"], None)


def _act(L, **kw):
    a = dict(x=0x10000, ldx=128, dtype=0, rows=4, cols=128, kind=1, q=0x50000, ldq=128, scale=0x60000, h=None, ldh=0)
    a.update(kw)
    return L.pq_act_quant_rowwise(a["x"], a["ldx"], a["dtype"], a["rows"], a["cols"], a["kind"], a["q"], a["ldq"], a["scale"], a["h"], a["ldh"], None)


@pytest.mark.parametrize("kw,named", [
    (dict(x=None), b"x is null"), (dict(w=None), b"weight is null"), (dict(q=None), b"q is null"), (dict(scale=None), b"scale is null"),
    (dict(dtype=3), b"dtype"), (dict(dtype=-1), b"dtype"), (dict(rows=-1), b"rows"), (dict(cols=-1), b"cols"), (dict(cols=1 << 24, ldx=1 << 24, ldq=1 << 24), b"cols"),
    (dict(ldx=64), b"ld_x"), (dict(ldq=64), b"ld_q"), (dict(h=0x70000, ldh=64), b"ld_h"),
    (dict(eps=float("nan")), b"eps"), (dict(eps=float("inf")), b"eps"), (dict(eps=-1e-6), b"eps"),
    (dict(q=0x10000), b"q overlaps x"), (dict(q=0x40000 + 8), b"q overlaps weight"), (dict(q=0x48000 + 8), b"q overlaps bias"), (dict(scale=0x10000 + 4), b"scale overlaps x"),
    (dict(scale=0x50000 + 128), b"q overlaps scale"), (dict(h=0x10000, ldh=128), b"h_out overlaps x"), (dict(h=0x40000, ldh=128), b"h_out overlaps weight"),
    (dict(h=0x50000 + 256, ldh=128), b"q overlaps h_out"), (dict(h=0x60000 - 64, ldh=128), b"scale overlaps h_out"),
])
def test_layernorm_bad_arguments_are_named_without_a_gpu(kw, named):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _ln(L, **kw) == 1, kw
    err = L.pq_last_error()
    assert LN.encode() in err and named in err, (kw, err)


@pytest.mark.parametrize("kw,named", [
    (dict(x=None), b"x is null"), (dict(q=None), b"q is null"), (dict(scale=None), b"scale is null"), (dict(dtype=3), b"dtype"), (dict(dtype=-1), b"dtype"),
    (dict(kind=3), b"kind"), (dict(kind=-1), b"kind"), (dict(rows=-1), b"rows"), (dict(cols=-1), b"cols"), (dict(ldx=64), b"ld_x"), (dict(ldq=64), b"ld_q"),
    (dict(h=0x70000, ldh=64), b"ld_h"), (dict(q=0x10000 + 64), b"q overlaps x"), (dict(scale=0x10000), b"scale overlaps x"), (dict(h=0x10000, ldh=128), b"h_out overlaps x"),
    (dict(h=0x50000, ldh=128), b"q overlaps h_out"), (dict(scale=0x50000), b"q overlaps scale"),
])
def test_act_bad_arguments_are_named_without_a_gpu(kw, named):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _act(L, **kw) == 1, kw
    err = L.pq_last_error()
    assert ACT.encode() in err and named in err, (kw, err)


def test_empty_problems_are_no_ops_without_a_gpu():
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _ln(L, rows=0) == 0 and _ln(L, cols=0, ldx=0, ldq=0) == 0 and _ln(L, rows=0, x=None, w=None, b=None, q=None, scale=None) == 0
    assert _act(L, rows=0) == 0 and _act(L, cols=0, ldx=0, ldq=0) == 0 and _act(L, rows=0, x=None, q=None, scale=None) == 0
    if not torch.cuda.is_available():          # a column block and a null bias get PAST the checks: the launch then fails for want of a device (status 3, not 1)
        for st in (_ln(L, b=None), _ln(L, ldx=256), _act(L, ldx=512), _act(L, kind=0), _act(L, kind=2)):
            assert st == 3 and b"overlaps" not in L.pq_last_error()


def test_python_entries_have_no_cpu_fallback_and_check_their_operands():
    import protoquant_amd as pq
    from protoquant_amd import _lib
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    w = torch.ones(64, dtype=torch.bfloat16)
    with pytest.raises(_lib.PQError):
        pq.layernorm_quantize(x, w, None)
    with pytest.raises(_lib.PQError):
        pq.act_quantize(x, "relu")
    with pytest.raises(_lib.PQError):
        pq.LayerNormQuant(w, w.clone(), 1e-5)(x)
    with pytest.raises(_lib.PQError):
        pq.ActQuant("gelu_tanh")(x)
    assert list(inspect.signature(pq.layernorm_quantize).parameters) == ["x", "weight", "bias", "eps", "return_h"]
    assert inspect.signature(pq.layernorm_quantize).parameters["eps"].default == 1e-5
    assert list(inspect.signature(pq.act_quantize).parameters) == ["x", "kind", "return_h"]
    assert list(inspect.signature(pq.fuse_layernorm_layers).parameters) == ["model", "fuse_norms", "fuse_act"]
    orig = _lib.require_gpu
    _lib.require_gpu = lambda t, name: None
    try:
        for bad in (dict(weight=None), dict(weight=torch.ones(32, dtype=torch.bfloat16)), dict(weight=torch.ones(64, dtype=torch.float32)),
                    dict(bias=torch.ones(32, dtype=torch.bfloat16)), dict(bias=torch.ones(64, dtype=torch.float16))):
            a = dict(x=x, weight=w, bias=None)
            a.update(bad)
            with pytest.raises(ValueError):
                pq.layernorm_quantize(**a)
        for kind in ("silu", "quick_gelu", "gelu", None):
            with pytest.raises(ValueError):
                pq.act_quantize(x, kind)
    finally:
        _lib.require_gpu = orig
    with pytest.raises(ValueError):
        pq.LayerNormQuant(None, None, 1e-5)
    assert set(pq.LayerNormQuant(w, None, 1e-5).state_dict()) == {"weight"} and set(pq.LayerNormQuant(w, w, 1e-5).state_dict()) == {"weight", "bias"}


def _kernels_of(objname):
    return kernels_of(objname, disassembly=True)


FORBIDDEN = re.compile(r"\bs_\w*(store|atomic|dcache)\w*|\bscratch_", re.I)          # no scalar instruction that writes memory or touches the scalar data cache, no scratch


def test_code_objects_have_every_layout_and_no_scratch():
    kl, dl = _kernels_of("layernorm_kernels")
    for dt in range(3):
        assert len([k for k in kl if re.search(r"\d+layernorm_quant_rowsILi%dELi\d+ELi64ELb[01]ELb0EE" % dt, k)]) == 4 * 2, dt          # 1, 2, 4, 8 vectors per lane, with / without h_out
        assert len([k for k in kl if re.search(r"\d+layernorm_quant_rowsILi%dELi\d+ELi256ELb[01]ELb0EE" % dt, k)]) == 5 * 2, dt           # 1 .. 16 vectors per thread
        assert len([k for k in kl if re.search(r"\d+layernorm_quant_genericILi%dELb0EE" % dt, k)]) == 1, dt
    assert len(kl) == 3 * (8 + 10 + 1)
    ka, da = _kernels_of("act_kernels")
    for dt in range(3):
        for kind in range(3):
            # wave per row x 1 / 2 / 4, 512 threads x 3, 256 threads x 1 .. 16, each with / without h_out; one generic kernel
            assert len([k for k in ka if re.search(r"rowmap_quant_rowsINS_5ActOpILi%dEEELi%dE" % (kind, dt), k)]) == (3 + 1 + 5) * 2, (dt, kind)
            assert len([k for k in ka if re.search(r"rowmap_quant_genericINS_5ActOpILi%dEEELi%dE" % (kind, dt), k)]) == 1, (dt, kind)
    assert len(ka) == 9 * 19
    for k, v in list(kl.items()) + list(ka.items()):
        assert v.get("private_segment_fixed_size", 1) == 0 and v.get("vgpr_spill_count", 1) == 0 and v.get("sgpr_spill_count", 1) == 0, (k, v)
    for dis in (dl, da):
        assert "global_load_dwordx4" in dis and "global_store_dwordx4" in dis and not FORBIDDEN.search(dis)
    assert "v_pk_fma_f32" in da and "v_pk_mul_f32" in dl


# ---------------------------------------------------------------------------------------------------------------- the specifications
PATS = np.arange(65536, dtype=np.uint16)
TDT = {0: torch.bfloat16, 1: torch.float16}


def _key(u):
    u = u.astype(np.int32)
    return np.where(u & 0x8000, -(u & 0x7FFF), u & 0x7FFF)


def _round_f64(ref: np.ndarray, code: int) -> np.ndarray:
    """float64 -> the nearest bf16 / fp16 pattern, ties to even, in ONE rounding (no detour through binary32); finite inputs that stay finite"""
    near = Q.from_f32(ref.astype(np.float32), code).astype(np.int32)
    best, bestd = near.copy(), None
    for delta in (0, -1, 1):
        cand = np.clip(_key(near.astype(np.uint16)) + delta, -0x7FFF, 0x7FFF)
        pat = np.where(cand < 0, 0x8000 | (-cand), cand).astype(np.uint16)
        pat = np.where((cand == 0) & (np.signbit(ref)), 0x8000, pat).astype(np.uint16)
        val = Q.to_f32(pat, code).astype(np.float64)
        d = np.abs(val - ref)
        if bestd is None:
            best, bestd = pat, d
        else:
            take = (d < bestd) | ((d == bestd) & ((pat & 1) == 0) & ((best & 1) == 1))
            best, bestd = np.where(take, pat, best).astype(np.uint16), np.where(take, d, bestd)
    return best


def test_relu_is_torchs_on_every_16_bit_pattern():
    for code, tdt in TDT.items():
        x = torch.from_numpy(PATS.view(np.int16).copy()).view(tdt)
        want = torch.relu(x).view(torch.int16).numpy().view(np.uint16)
        got = AS.act(PATS, code, "relu")
        nan = np.isnan(Q.to_f32(PATS, code))
        assert np.array_equal(got[~nan], want[~nan]) and np.isnan(Q.to_f32(got, code))[nan].all()
        zero = 0x8000          # -0 stays -0 (torch.relu keeps it); every other negative value, -Inf included, becomes +0
        assert got[zero] == 0x8000 and got[0] == 0 and (got[(PATS > 0x8000) & ~nan] == 0).all()


# (kind, dtype code) -> (patterns that miss the correctly rounded float64 value, patterns that differ from torch's eager kernel): measured and
# asserted from above; the misses are also held below torch eager's own count on the machine the test runs on
MEASURED = {("gelu_tanh", 0): (5, 160), ("gelu_erf", 0): (24, 840), ("gelu_tanh", 1): (2, 290), ("gelu_erf", 1): (4, 600)}
FLOOR = 2.0 ** -96          # exact values smaller than this may come out as a zero of the right sign (the deep negative tail)


@pytest.mark.parametrize("kind,approx", [("gelu_tanh", "tanh"), ("gelu_erf", "none")])
@pytest.mark.parametrize("code", [0, 1], ids=["bf16", "fp16"])
def test_gelu_bars_on_every_16_bit_pattern(kind, approx, code):
    xf = Q.to_f32(PATS, code)
    fin = np.isfinite(xf)
    got = AS.act(PATS, code, kind)
    ref = AS.act_f64(xf.astype(np.float64), kind)
    want = _round_f64(np.where(fin, ref, 0.0), code)
    eager = torch.nn.functional.gelu(torch.from_numpy(PATS.view(np.int16).copy()).view(TDT[code]), approximate=approx).view(torch.int16).numpy().view(np.uint16)
    small = np.abs(ref) < FLOOR
    ulp = np.abs(_key(got) - _key(want))
    # (a) within 1 ulp of the storage type of the exact value; below the floor: a zero of the exact value's sign, or within 1 ulp
    assert ulp[fin & ~small].max() <= 1
    tail = fin & small & (ulp > 1)
    assert ((got[tail] & 0x7FFF) == 0).all() and ((got[tail] >> 15) == np.signbit(ref[tail])).all()
    # no difference in the sign of a zero result anywhere
    z = fin & ((got & 0x7FFF) == 0) & ((want & 0x7FFF) == 0)
    assert np.array_equal(got[z], want[z])
    # (b) misses of the correctly rounded value: bounded, and no more than torch eager's
    miss, miss_eager, vs_eager = int(((got != want) & fin).sum()), int(((eager != want) & fin).sum()), int(((got != eager) & fin).sum())
    assert miss <= MEASURED[(kind, code)][0] and miss <= miss_eager, (miss, miss_eager)
    # (c) the distance to torch's eager kernel
    assert vs_eager <= MEASURED[(kind, code)][1], vs_eager
    # (d) NaN -> NaN, +Inf -> +Inf, -Inf and the deep negative tail -> -0 (torch's eager tail is -0 too; its -Inf is NaN)
    gf = Q.to_f32(got, code)
    assert np.isnan(gf[np.isnan(xf)]).all() and (gf[xf == np.inf] == np.inf).all()
    deep = fin & (xf < -14.0)
    assert (got[deep] == 0x8000).all() and (got[xf == -np.inf] == 0x8000).all() and (eager[deep] == 0x8000).all()


@pytest.mark.parametrize("kind,bounds", [("gelu_tanh", ((-12.0, -4.0, 160.0), (-4.0, -1.0, 20.0), (-1.0, 12.0, 3.0))), ("gelu_erf", ((-12.0, 12.0, 10.0),))])
def test_gelu_f32_bound_against_float64(kind, bounds):
    """f32 rows: error in ulp of the exact value over a dense sweep of [-12, 12] and random bit patterns (exact values below 2^-96: absolute error below 2^-96).
    The tanh form loses accuracy in its negative tail because the rounding error of its exponent a (up to 80 in magnitude) is amplified by the exponential."""
    rng = np.random.default_rng(0)
    x = np.concatenate([np.linspace(-12, 12, 400_001).astype(np.float32), rng.integers(0, 2 ** 32, 400_000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    x = x[np.isfinite(x)]
    got = AS._FN[AS.kind_code(kind)](x).astype(np.float64)
    ref = AS.act_f64(x.astype(np.float64), kind)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref) / np.spacing(np.abs(ref.astype(np.float32))).astype(np.float64)
    big = np.abs(ref) >= FLOOR
    assert np.abs(got - ref)[~big].max() < FLOOR
    lo_all, hi_all = bounds[0][0], bounds[-1][1]
    for lo, hi, bound in bounds:
        m = big & (x >= lo) & (x < hi)
        assert err[m].max() <= bound, (kind, lo, hi, err[m].max())
    out = big & ((x < lo_all) | (x >= hi_all))
    assert err[out].max() <= 2.0          # beyond the sweep: h = x (or a zero) up to rounding


def test_layernorm_spec_against_float64_and_eager():
    """lnorm_spec against a float64 LayerNorm: within 1 ulp of the storage type everywhere (the f64 value rounded once); against torch's eager CPU layer_norm: the
    fraction of stored h that differ is small and never more than 1 ulp (the measured distance on 10^7 elements is in DESIGN.md section 2; this is a small sample)."""
    g = torch.Generator().manual_seed(3)
    for code, tdt in TDT.items():
        x = (torch.randn(64, 768, generator=g) * 2 + 0.3).to(tdt)
        w = (1 + 0.2 * torch.randn(768, generator=g)).to(tdt)
        b = (0.2 * torch.randn(768, generator=g)).to(tdt)
        st = lambda t: t.view(torch.int16).numpy().view(np.uint16)          # noqa: E731
        h, _, _ = LS.layernorm(st(x), st(w), st(b), 1e-5, code)
        ref = LS.layernorm_f64(x.double().numpy(), w.double().numpy(), b.double().numpy(), float(np.float32(1e-5)))
        want = _round_f64(ref, code)
        assert np.abs(_key(h) - _key(want)).max() <= 1 and (h != want).mean() < 2e-3
        eager = st(torch.nn.functional.layer_norm(x, (768,), w, b, 1e-5))
        assert np.abs(_key(h) - _key(eager)).max() <= 1 and (h != eager).mean() < 5e-3
        h2, _, _ = LS.layernorm(st(x), st(w), None, 1e-5, code)
        eager2 = st(torch.nn.functional.layer_norm(x, (768,), w, None, 1e-5))
        assert np.abs(_key(h2) - _key(eager2)).max() <= 1
    xf = torch.randn(16, 100, generator=g) * 3
    h32, _, _ = LS.layernorm(xf.numpy(), np.ones(100, np.float32), None, 1e-5, 2)
    assert np.allclose(h32, torch.nn.functional.layer_norm(xf, (100,)).numpy(), rtol=0, atol=2e-6)


def test_pinned_sum_is_layout_independent():
    """the same rows dealt as 1, 4, 16 vectors per lane of 256 lanes, and as one wave per row at 1 .. 8 vectors per lane, give one result (L2 and L3)"""
    rng = np.random.default_rng(1)
    for epv in (8, 4):
        for nvec in (1, 37, 64, 100, 256, 300, 512):
            v = (rng.standard_normal((5, nvec * epv)) * 3 + 0.7).astype(np.float32)
            for square in (False, True):
                want = LS.pinned_sum(v, epv, square)
                if square:
                    assert np.array_equal(want.view(np.uint32), Q.rms_sumsq(v, epv).view(np.uint32))          # L3's order IS N1-N3
                # more slots than needed (a 4- or 16-vector layout on a short row) only add zeros
                for slots in (4, 16):
                    wide = np.zeros((5, slots * 256 * epv), np.float32)
                    wide[:, :v.shape[1]] = v
                    assert np.array_equal(LS.pinned_sum(wide, epv, square).view(np.uint32), want.view(np.uint32))
                for vpl in (1, 2, 4, 8):
                    if nvec <= 64 * vpl:
                        assert np.array_equal(LS.pinned_sum_wave(v, epv, square, vpl).view(np.uint32), want.view(np.uint32)), (epv, nvec, square, vpl)
    # and the order matters: a plain numpy sum of the same row gives other bits somewhere
    v = (rng.standard_normal((64, 4096)) * 3).astype(np.float32)
    assert not np.array_equal(LS.pinned_sum(v, 8, False), v.sum(axis=1, dtype=np.float32))
