"""CPU: the host side of K1ma / K1mo (pq_scaled_add_rmsnorm_quant_rows / scaled_add_rmsnorm_quantize / scaled_add): QSPEC S1 in numpy (tests/scaled_addnorm_spec.py) is
what torch's `x * python_float` stores; S1 + A1 is two roundings and differs from the single-rounding FMA; the symbol is declared, exported and bound; every bad argument is
refused and named before any HIP call; empty problems are no-ops; the Python entries have no CPU path; the code object holds every row layout without scratch.

The entry is named `..._rows`, not `..._rowwise`: tests/row_forms.py (a yardstick, with tests/test_gpu_row_addressing.py's table check and the form count pinned by
tests/test_amax_design_host.py) lists every export matching pq_\\w+_rowwise and stays as it is; the coverage those tables give the other row entries is brought for this
one by tests/test_gpu_scaled_addnorm.py, with the helpers of tests/amax_design.py, tests/row_forms.py and tests/guarded_workspace.py."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from protoquant_amd.qtensor import scaled_add, scaled_add_rmsnorm_quantize  # noqa: F401  (the ops this file is about)
from tests import addnorm_spec as A
from tests import scaled_addnorm_spec as S
from tests.code_objects import kernels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "pq_scaled_add_rmsnorm_quant_rows"
ARGS = ["x", "ld_x", "residual", "ld_r", "multiplier", "sum_out", "ld_s", "weight", "eps", "dtype", "rows", "cols", "q", "ld_q", "scale", "h_out", "ld_h", "stream"]


# ---------------------------------------------------------------------------------------------------------------- S1 and the two roundings
@pytest.mark.parametrize("dt,code", [(torch.bfloat16, 0), (torch.float16, 1)], ids=["bf16", "fp16"])
def test_s1_is_what_torch_stores_for_every_16_bit_pattern(dt, code):
    pats = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    x = pats.view(dt)
    xb = pats.numpy().view(np.uint16)
    big = torch.finfo(dt).max
    for m in S.MULTIPLIERS:
        want = x * m                                                     # torch eager on the CPU: the Python scalar rounded once to binary32, one product, one rounding
        nan = torch.isnan(want.float())
        spelled = (x.float() * torch.tensor(m, dtype=torch.float32)).to(dt)          # the same, spelled out
        assert torch.equal(spelled.view(torch.int16)[~nan], want.view(torch.int16)[~nan]) and torch.equal(torch.isnan(spelled.float()), nan), (dt, m)
        got = torch.from_numpy(S.scale_s1(xb, m, code).view(np.int16).copy()).view(dt)
        assert torch.equal(torch.isnan(got.float()), nan), (dt, m)
        assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]), (dt, m)
    top = torch.tensor([big, -big], dtype=dt)
    got = S.scale_s1(A.to_bits(top), S.OVERFLOWING, code)
    assert bool(torch.isinf(torch.from_numpy(got.view(np.int16).copy()).view(dt).float()).all())          # the largest finite value overflows to Inf


def _f32_pairs():
    g = torch.Generator().manual_seed(20240611)
    x = torch.randn(1 << 16, generator=g)
    r = torch.randn(1 << 16, generator=g) * 3.0
    return x, r


def test_f32_composition_is_two_roundings_and_not_the_fma():
    x, r = _f32_pairs()
    for m in S.MULTIPLIERS:
        want = r + x * m                                                 # torch eager: the product is a tensor of its own
        got = S.scaled_add(x, r, m)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), m
        if m in (1.0, -0.5, 0.0625, 4.0):
            continue                                                     # a power of two: the product is exact, both forms coincide
        fma = S.fma_single_rounding(x.numpy(), m, r.numpy())
        share = float(np.mean(fma.view(np.uint32) != got.numpy().view(np.uint32)))
        assert share >= 0.05, (m, share)                                 # a condition on the INPUTS: they tell the two forms apart (about 15 % here)


def test_spec_is_s1_then_the_add_then_the_oracle():
    from oracle import c_oracle as C
    g = torch.Generator().manual_seed(2)
    for dt, code in ((torch.bfloat16, 0), (torch.float16, 1), (torch.float32, 2)):
        x = (torch.randn(5, 96, generator=g) * 4).to(dt)
        r = torch.randn(5, 96, generator=g).to(dt)
        w = (1 + 0.1 * torch.randn(96, generator=g)).to(dt)
        for m in S.MULTIPLIERS:
            s = S.scaled_add(x, r, m)
            assert torch.equal(s, r + x * m)
            q, sc, sb, h = S.scaled_add_rmsnorm_quantize(x, r, m, w, 1e-5)
            q2, sc2, sb2, h2 = A.add_rmsnorm_quantize(x * m, r, w, 1e-5)             # K1a's specification on p computed by torch: what the kernel is held to
            assert np.array_equal(q, q2) and np.array_equal(sc, sc2) and np.array_equal(sb, sb2) and np.array_equal(h, h2)
            q3, sc3, h3, _ = C.rmsnorm_quant_rowwise(A.to_bits(s), A.to_bits(w), 1e-5, code)
            assert np.array_equal(q, q3) and np.array_equal(sc, sc3) and np.array_equal(h, h3)


# ---------------------------------------------------------------------------------------------------------------- the symbol
def test_symbol_declared_exported_and_bound():
    import ctypes

    from protoquant_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pq_hip.h")).read(), flags=re.S)
    m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % SYM, hdr)
    assert m, f"pq_hip.h does not declare {SYM}"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ARGS
    assert params[4] == "float multiplier"
    ma = re.search(r"int32_t\s+pq_add_rmsnorm_quant_rowwise\s*\(([^)]*)\)\s*;", hdr)
    k1a = [p.strip() for p in ma.group(1).split(",")]
    assert params[:4] + params[5:] == k1a                               # K1a's arguments, with `float multiplier` after ld_r
    L = _lib.lib()
    fn = getattr(L, SYM)
    assert SYM in _lib.EXPORTS and len(fn.argtypes) == 18 and fn.argtypes[4] is ctypes.c_float and fn.restype is ctypes.c_int32
    assert fn.argtypes[:4] + fn.argtypes[5:] == L.pq_add_rmsnorm_quant_rowwise.argtypes
    assert not re.fullmatch(r"pq_\w+_rowwise", SYM)                       # not a row of tests/row_forms.py: this file's docstring says where its coverage is
    assert L.pq_version() == 1                                            # an addition: the ABI version stays
    import protoquant_amd as pq
    for name in ("scaled_add_rmsnorm_quantize", "scaled_add", "fuse_granite_residual", "residual_flow_is_scaled", "ScaledResidualFusedLayer"):
        assert name in pq.__all__ and callable(getattr(pq, name))
    assert SYM in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _call(L, **kw):
    """the entry with plausible (never dereferenced) operands, bf16 4 x 128, some arguments overridden"""
    a = dict(x=0x10000, ldx=128, r=0x20000, ldr=128, m=0.22, s=0x30000, lds=128, w=0x40000, eps=1e-6, dtype=0, rows=4, cols=128, q=0x50000, ldq=128, scale=0x60000, h=None,
             ldh=0)
    a.update(kw)
    return getattr(L, SYM)(a["x"], a["ldx"], a["r"], a["ldr"], a["m"], a["s"], a["lds"], a["w"], a["eps"], a["dtype"], a["rows"], a["cols"], a["q"], a["ldq"], a["scale"],
                           a["h"], a["ldh"], None)


ROW = 128 * 2          # bytes of one bf16 row
ADD_ONLY = dict(w=None, q=None, scale=None, h=None)

BAD = [
    (dict(s=None), b"sum_out is null"), (dict(x=None), b"x is null"), (dict(r=None), b"residual is null"), (dict(dtype=3), b"dtype"), (dict(dtype=-1), b"dtype"),
    (dict(rows=-1), b"rows"), (dict(cols=-1), b"cols"), (dict(cols=1 << 24, ldx=1 << 24, ldr=1 << 24, lds=1 << 24, ldq=1 << 24), b"cols"),
    (dict(ldx=64), b"ld_x"), (dict(ldr=64), b"ld_r"), (dict(lds=64), b"ld_s"), (dict(ldq=64), b"ld_q"), (dict(h=0x70000, ldh=64), b"ld_h"),
    (dict(eps=float("nan")), b"eps"), (dict(eps=float("inf")), b"eps"), (dict(eps=-1e-6), b"eps"),
    (dict(m=float("nan")), b"multiplier"), (dict(m=float("inf")), b"multiplier"), (dict(m=float("-inf")), b"multiplier"),
    # the quantisation group goes together: a null weight with a non-null q, and every other partly-null group
    (dict(w=None), b"weight is null"), (dict(q=None), b"q is null"), (dict(scale=None), b"scale is null"), (dict(w=None, scale=None), b"weight is null"),
    (dict(w=None, q=None, scale=None, h=0x70000, ldh=128), b"weight is null"), (dict(q=None, scale=None), b"q is null"),
    # sum_out: exactly x / residual is fine (below); anything else that overlaps them is not — one element of overlap included
    (dict(s=0x10000 + 16), b"sum_out overlaps x"), (dict(s=0x10000 + ROW), b"sum_out overlaps x"), (dict(s=0x10000 - ROW), b"sum_out overlaps x"),
    (dict(s=0x10000 + 4 * ROW - 2), b"sum_out overlaps x"), (dict(s=0x10000 - 4 * ROW + 2), b"sum_out overlaps x"),
    (dict(s=0x20000 + 4 * ROW - 2), b"sum_out overlaps residual"), (dict(s=0x20000 - 4 * ROW + 2), b"sum_out overlaps residual"),
    (dict(s=0x10000, lds=256, ldx=128), b"sum_out overlaps x"),                      # the same pointer, another leading dimension
    (dict(s=0x20000 + 2 * ROW), b"sum_out overlaps residual"), (dict(s=0x40000), b"sum_out overlaps weight"), (dict(s=0x40000 - 4 * ROW + 2), b"sum_out overlaps weight"),
    # q, scale, h_out: nothing may overlap them
    (dict(q=0x10000), b"q overlaps x"), (dict(q=0x20000 + 100), b"q overlaps residual"), (dict(q=0x40000 + 8), b"q overlaps weight"), (dict(q=0x30000 + 64), b"q overlaps sum_out"),
    (dict(scale=0x10000 + 4), b"scale overlaps x"), (dict(scale=0x30000), b"scale overlaps sum_out"), (dict(scale=0x50000 + 128), b"q overlaps scale"),
    (dict(h=0x10000, ldh=128), b"h_out overlaps x"), (dict(h=0x20000 + ROW, ldh=128), b"h_out overlaps residual"), (dict(h=0x30000, ldh=128), b"h_out overlaps sum_out"),
    (dict(h=0x50000 + 256, ldh=128), b"q overlaps h_out"), (dict(h=0x60000 - 64, ldh=128), b"scale overlaps h_out"),
    # the add-only form keeps the checks of what it still has
    (dict(ADD_ONLY, s=None), b"sum_out is null"), (dict(ADD_ONLY, x=None), b"x is null"), (dict(ADD_ONLY, r=None), b"residual is null"), (dict(ADD_ONLY, lds=64), b"ld_s"),
    (dict(ADD_ONLY, s=0x10000 + 4 * ROW - 2), b"sum_out overlaps x"), (dict(ADD_ONLY, s=0x20000 + 16), b"sum_out overlaps residual"), (dict(ADD_ONLY, m=float("nan")), b"multiplier"),
    (dict(ADD_ONLY, cols=1 << 24, ldx=1 << 24, ldr=1 << 24, lds=1 << 24), b"cols"),
]


@pytest.mark.parametrize("kw,named", BAD)
def test_bad_arguments_are_named_without_a_gpu(kw, named):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _call(L, **kw) == 1, kw
    err = L.pq_last_error()
    assert SYM.encode() in err and named in err, (kw, err)


def test_allowed_aliases_and_the_add_only_form_pass_the_checks():
    """sum_out == x, sum_out == residual (same pointer and leading dimension), disjoint column blocks of one buffer and the add-only form (eps not read: a NaN eps passes)
    get PAST the argument checks: on a machine without a GPU the launch then fails (status 3, not 1).  On one with a GPU these never-dereferenced addresses must not be
    launched, so there the test checks nothing and returns (the GPU tests run the same forms on real memory)."""
    from protoquant_amd import _lib
    L = _lib.lib()
    if torch.cuda.is_available():
        return
    for kw in (dict(s=0x10000), dict(s=0x20000), dict(x=0x10000, ldx=256, s=0x10000 + ROW, lds=256), dict(x=0x10000, ldx=256, s=0x10000, lds=256), ADD_ONLY,
               dict(ADD_ONLY, eps=float("nan")), dict(ADD_ONLY, s=0x20000), dict(m=-0.5), dict(m=3.0e38)):
        st = _call(L, **kw)
        assert st == 3 and b"overlaps" not in L.pq_last_error() and b"null" not in L.pq_last_error(), (kw, st, L.pq_last_error())


def test_empty_problems_are_no_ops_without_a_gpu():
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _call(L, rows=0) == 0
    assert _call(L, cols=0, ldx=0, ldr=0, lds=0, ldq=0) == 0
    assert _call(L, rows=0, x=None, r=None, s=None, w=None, q=None, scale=None) == 0
    assert _call(L, rows=0, **ADD_ONLY) == 0 and _call(L, cols=0, ldx=0, ldr=0, lds=0, **ADD_ONLY) == 0


# ---------------------------------------------------------------------------------------------------------------- the Python entries
def test_python_entries_have_no_cpu_path_and_fixed_signatures():
    import protoquant_amd as pq
    from protoquant_amd import _lib
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    w = torch.ones(64, dtype=torch.bfloat16)
    with pytest.raises(_lib.PQError):
        pq.scaled_add_rmsnorm_quantize(x, x.clone(), 0.22, w)
    with pytest.raises(_lib.PQError):
        pq.scaled_add(x, x.clone(), 0.22)
    sig = inspect.signature(pq.scaled_add_rmsnorm_quantize)
    assert list(sig.parameters) == ["x", "residual", "multiplier", "weight", "eps", "out", "return_h"]
    assert sig.parameters["eps"].default == 1e-6 and sig.parameters["out"].default is None and sig.parameters["return_h"].default is False
    assert list(inspect.signature(pq.scaled_add).parameters) == ["x", "residual", "multiplier", "out"]


def test_python_entries_refuse_a_multiplier_that_is_no_python_number():
    """before anything else, the device check included: a tensor (a value the kernel cannot take as an argument) is a TypeError that names the argument"""
    import protoquant_amd as pq
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    w = torch.ones(64, dtype=torch.bfloat16)
    for bad in (torch.tensor(0.22), torch.tensor([0.22]), np.float32(0.22), "0.22", None, True):
        with pytest.raises(TypeError, match="multiplier"):
            pq.scaled_add_rmsnorm_quantize(x, x.clone(), bad, w)
        with pytest.raises(TypeError, match="multiplier"):
            pq.scaled_add(x, x.clone(), bad)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="multiplier"):
            pq.scaled_add(x, x.clone(), bad)


def test_python_entries_refuse_mismatched_operands():
    """the shape / dtype / layout checks, which come after the device check: played on CPU tensors with the device check stubbed out (every case raises before any call
    into the library)"""
    import protoquant_amd as pq
    from protoquant_amd import _lib, qtensor
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    w = torch.ones(64, dtype=torch.bfloat16)
    orig = _lib.require_gpu
    _lib.require_gpu = lambda t, name: None
    try:
        for bad in (dict(residual=torch.zeros(4, 32, dtype=torch.bfloat16)), dict(residual=torch.zeros(4, 64, dtype=torch.float16)), dict(weight=torch.ones(32, dtype=torch.bfloat16)),
                    dict(weight=torch.ones(64, dtype=torch.float32)), dict(out=torch.zeros(4, 32, dtype=torch.bfloat16)), dict(out=torch.zeros(4, 64, dtype=torch.float16)),
                    dict(out=torch.zeros(64, 4, dtype=torch.bfloat16).t())):
            a = dict(x=x, residual=x.clone(), multiplier=0.22, weight=w)
            a.update(bad)
            with pytest.raises(ValueError):
                pq.scaled_add_rmsnorm_quantize(**a)
            if "weight" not in bad:
                a.pop("weight")
                with pytest.raises(ValueError):
                    pq.scaled_add(**a)
    finally:
        _lib.require_gpu = orig
    assert qtensor.L.require_gpu is orig


# ---------------------------------------------------------------------------------------------------------------- the code object
def test_code_object_has_every_layout_and_no_scratch():
    """as tests/test_addnorm_host.py reads K1a's object: rmsnorm_quant_rows<.., 64 | 256, WRITE_H, ADD = true, LlamaGain, QUANT, float> / rmsnorm_quant_generic<.., true, LlamaGain, QUANT,
    float> (the instantiations that take the multiplier) for all three dtypes — K1ma with and without h_out, K1mo without — none with scratch or spills, and no single-rounding fp16 convert"""
    kernels, dis = kernels_of("scaled_addnorm_kernels", disassembly=True)
    for dt in range(3):
        # wave: 1, 2, 4, 8 vectors per lane; 256 threads: 1, 2, 4, 8, 16 per thread; K1ma with and without h_out, K1mo without; one generic kernel each
        assert len([k for k in kernels if re.search(r"\d+rmsnorm_quant_rowsILi%dELi\d+ELi64ELb[01]ELb1ENS_9LlamaGainELb1EJfEEE" % dt, k)]) == 4 * 2, dt
        assert len([k for k in kernels if re.search(r"\d+rmsnorm_quant_rowsILi%dELi\d+ELi256ELb[01]ELb1ENS_9LlamaGainELb1EJfEEE" % dt, k)]) == 5 * 2, dt
        assert len([k for k in kernels if re.search(r"\d+rmsnorm_quant_rowsILi%dELi\d+ELi(64|256)ELb0ELb1ENS_9LlamaGainELb0EJfEEE" % dt, k)]) == 4 + 5, dt
        assert len([k for k in kernels if re.search(r"\d+rmsnorm_quant_genericILi%dELb1ENS_9LlamaGainELb[01]EJfEEE" % dt, k)]) == 2, dt
    assert len(kernels) == 3 * (8 + 10 + 9 + 2)
    for k, v in kernels.items():
        assert v.get("private_segment_fixed_size", 1) == 0 and v.get("vgpr_spill_count", 1) == 0 and v.get("sgpr_spill_count", 1) == 0, (k, v)
    assert "global_load_dwordx4" in dis and "global_store_dwordx4" in dis and "v_pk_mul_f32" in dis and "v_pk_add_f32" in dis and "scratch_" not in dis
    assert "v_fma_mixlo" not in dis and "v_fma_mixhi" not in dis and "v_mad_mixlo" not in dis
