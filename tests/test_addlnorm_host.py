"""CPU: the host side of K1al (pq_add_layernorm_quant_rowwise / add_layernorm_quantize): the symbol is declared, exported and bound with its argument list; every
bad argument is refused and named before any HIP call; the allowed aliases pass; empty problems are no-ops; the Python entry has no CPU path; the code object of
addlayernorm_kernels.hip holds every row layout for all three dtypes without scratch, spills or a forbidden instruction; the specification is the add, then the
LayerNorm specification on the stored sum."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import addlnorm_spec as AL
from tests import lnorm_spec as LS
from tests.code_objects import kernels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "pq_add_layernorm_quant_rowwise"
ARGS = ["x", "ld_x", "residual", "ld_r", "sum_out", "ld_s", "weight", "bias", "eps", "dtype", "rows", "cols", "q", "ld_q", "scale", "h_out", "ld_h", "stream"]


def test_symbol_declared_exported_and_bound():
    from protoquant_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pq_hip.h")).read(), flags=re.S)
    m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % SYM, hdr)
    assert m, f"pq_hip.h does not declare {SYM}"
    names = [re.split(r"[\s*]+", a.strip())[-1] for a in m.group(1).split(",")]
    assert names == ARGS                                                 # pq_add_rmsnorm_quant_rowwise's order with `bias` after `weight`
    ma = re.search(r"int32_t\s+pq_add_rmsnorm_quant_rowwise\s*\(([^)]*)\)\s*;", hdr)
    assert [re.split(r"[\s*]+", a.strip())[-1] for a in ma.group(1).split(",")] == [a for a in ARGS if a != "bias"]
    L = _lib.lib()
    assert hasattr(L, SYM) and SYM in _lib.EXPORTS and len(getattr(L, SYM).argtypes) == 18
    assert L.pq_version() == 1                                          # an addition: the ABI version stays
    import protoquant_amd as pq
    assert "add_layernorm_quantize" in pq.__all__ and callable(pq.add_layernorm_quantize)


def _call(L, **kw):
    """the entry with plausible (never dereferenced) operands, bf16 4 x 128, some arguments overridden"""
    a = dict(x=0x10000, ldx=128, r=0x20000, ldr=128, s=0x30000, lds=128, w=0x40000, b=0x48000, eps=1e-5, dtype=0, rows=4, cols=128, q=0x50000, ldq=128, scale=0x60000,
             h=None, ldh=0)
    a.update(kw)
    return L.pq_add_layernorm_quant_rowwise(a["x"], a["ldx"], a["r"], a["ldr"], a["s"], a["lds"], a["w"], a["b"], a["eps"], a["dtype"], a["rows"], a["cols"], a["q"],
                                            a["ldq"], a["scale"], a["h"], a["ldh"], None)


ROW = 128 * 2          # bytes of one bf16 row


@pytest.mark.parametrize("kw,named", [
    (dict(s=None), b"sum_out is null"), (dict(x=None), b"x is null"), (dict(r=None), b"residual is null"), (dict(w=None), b"weight is null"), (dict(q=None), b"q is null"),
    (dict(scale=None), b"scale is null"), (dict(dtype=3), b"dtype"), (dict(dtype=-1), b"dtype"), (dict(rows=-1), b"rows"), (dict(cols=-1), b"cols"),
    (dict(cols=1 << 24, ldx=1 << 24, ldr=1 << 24, lds=1 << 24, ldq=1 << 24), b"cols"),
    (dict(ldx=64), b"ld_x"), (dict(ldr=64), b"ld_r"), (dict(lds=64), b"ld_s"), (dict(ldq=64), b"ld_q"), (dict(h=0x70000, ldh=64), b"ld_h"),
    (dict(eps=float("nan")), b"eps"), (dict(eps=float("inf")), b"eps"), (dict(eps=-1e-6), b"eps"),
    # sum_out: exactly x / residual is fine (below); anything else that overlaps them is not
    (dict(s=0x10000 + 16), b"sum_out overlaps x"), (dict(s=0x10000 + ROW), b"sum_out overlaps x"), (dict(s=0x10000 - ROW), b"sum_out overlaps x"),
    (dict(s=0x10000, lds=256, ldx=128), b"sum_out overlaps x"),                      # the same pointer, another leading dimension
    (dict(s=0x20000 + 2 * ROW), b"sum_out overlaps residual"), (dict(s=0x40000), b"sum_out overlaps weight"), (dict(s=0x48000 - ROW), b"sum_out overlaps bias"),
    # q, scale, h_out: nothing may overlap them
    (dict(q=0x10000), b"q overlaps x"), (dict(q=0x20000 + 100), b"q overlaps residual"), (dict(q=0x40000 + 8), b"q overlaps weight"), (dict(q=0x48000 + 8), b"q overlaps bias"),
    (dict(q=0x30000 + 64), b"q overlaps sum_out"),
    (dict(scale=0x10000 + 4), b"scale overlaps x"), (dict(scale=0x30000), b"scale overlaps sum_out"), (dict(scale=0x48000), b"scale overlaps bias"),
    (dict(scale=0x50000 + 128), b"q overlaps scale"),
    (dict(h=0x10000, ldh=128), b"h_out overlaps x"), (dict(h=0x20000 + ROW, ldh=128), b"h_out overlaps residual"), (dict(h=0x30000, ldh=128), b"h_out overlaps sum_out"),
    (dict(h=0x40000, ldh=128), b"h_out overlaps weight"), (dict(h=0x48000, ldh=128), b"h_out overlaps bias"),
    (dict(h=0x50000 + 256, ldh=128), b"q overlaps h_out"), (dict(h=0x60000 - 64, ldh=128), b"scale overlaps h_out"),
])
def test_bad_arguments_are_named_without_a_gpu(kw, named):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _call(L, **kw) == 1, kw
    err = L.pq_last_error()
    assert SYM.encode() in err and named in err, (kw, err)


@pytest.mark.skipif(torch.cuda.is_available(), reason="argument-check-only test: needs a machine without a GPU (the operands are not real memory)")
def test_allowed_aliases_null_bias_and_column_blocks_pass_the_checks():
    """sum_out == x, sum_out == residual (same pointer and leading dimension), a null bias and disjoint column blocks of one buffer get PAST the argument checks: on a
    machine without a GPU the launch then fails (status 3, not 1)"""
    from protoquant_amd import _lib
    L = _lib.lib()
    for kw in (dict(s=0x10000), dict(s=0x20000), dict(b=None), dict(b=None, s=0x10000), dict(x=0x10000, ldx=256, s=0x10000 + ROW, lds=256),
               dict(x=0x10000, ldx=256, s=0x10000, lds=256), dict(h=0x70000, ldh=128)):
        st = _call(L, **kw)
        assert st == 3 and b"overlaps" not in L.pq_last_error(), (kw, st, L.pq_last_error())


def test_empty_problems_are_no_ops_without_a_gpu():
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _call(L, rows=0) == 0
    assert _call(L, cols=0, ldx=0, ldr=0, lds=0, ldq=0) == 0
    assert _call(L, rows=0, x=None, r=None, s=None, w=None, b=None, q=None, scale=None) == 0


def test_python_entry_has_no_cpu_fallback_and_checks_its_operands():
    import protoquant_amd as pq
    from protoquant_amd import _lib, qtensor
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    w = torch.ones(64, dtype=torch.bfloat16)
    with pytest.raises(_lib.PQError):
        pq.add_layernorm_quantize(x, x.clone(), w, None)
    with pytest.raises(_lib.PQError):
        pq.LayerNormQuant(w, w.clone(), 1e-5)(x, residual=x.clone())
    sig = inspect.signature(pq.add_layernorm_quantize)
    assert list(sig.parameters) == ["x", "residual", "weight", "bias", "eps", "out", "return_h"]
    assert sig.parameters["eps"].default == 1e-5 and sig.parameters["out"].default is None and sig.parameters["return_h"].default is False
    assert list(inspect.signature(pq.LayerNormQuant.forward).parameters) == ["self", "x", "residual"]
    assert inspect.signature(pq.LayerNormQuant.forward).parameters["residual"].default is None
    orig = _lib.require_gpu
    _lib.require_gpu = lambda t, name: None
    try:
        for bad in (dict(residual=torch.zeros(4, 32, dtype=torch.bfloat16)), dict(residual=torch.zeros(4, 64, dtype=torch.float16)), dict(weight=None),
                    dict(weight=torch.ones(32, dtype=torch.bfloat16)), dict(weight=torch.ones(64, dtype=torch.float32)), dict(bias=torch.ones(32, dtype=torch.bfloat16)),
                    dict(bias=torch.ones(64, dtype=torch.float16)), dict(out=torch.zeros(4, 32, dtype=torch.bfloat16)), dict(out=torch.zeros(4, 64, dtype=torch.float16)),
                    dict(out=torch.zeros(64, 4, dtype=torch.bfloat16).t())):
            a = dict(x=x, residual=x.clone(), weight=w, bias=None)
            a.update(bad)
            with pytest.raises(ValueError):
                pq.add_layernorm_quantize(**a)
    finally:
        _lib.require_gpu = orig
    assert qtensor.L.require_gpu is orig


def test_spec_is_the_add_then_the_layernorm_spec():
    """tests/addlnorm_spec.py composes and adds nothing: A1 is the value torch's eager add stores, the rest is tests/lnorm_spec on the stored sum"""
    g = torch.Generator().manual_seed(1)
    for dt, code in ((torch.bfloat16, 0), (torch.float16, 1), (torch.float32, 2)):
        x = torch.randn(5, 96, generator=g).to(dt)
        r = (torch.randn(5, 96, generator=g) * 4).to(dt)
        w = (1 + 0.1 * torch.randn(96, generator=g)).to(dt)
        b = (0.1 * torch.randn(96, generator=g)).to(dt)
        for bias in (b, None):
            q, sc, sb, h = AL.add_layernorm_quantize(x, r, w, bias, 1e-5)
            assert np.array_equal(sb, AL.to_bits(r + x))
            q2, sc2, h2 = LS.layernorm_quantize(AL.to_bits(r + x), AL.to_bits(w), None if bias is None else AL.to_bits(bias), 1e-5, code)
            assert np.array_equal(q, q2) and np.array_equal(sc, sc2) and np.array_equal(h, h2)


def _kernels_of(objname):
    return kernels_of(objname, disassembly=True)


FORBIDDEN = re.compile(r"\bs_\w*(store|atomic|dcache)\w*|\bscratch_", re.I)          # no scalar instruction that writes memory or touches the scalar data cache, no scratch


def test_code_object_has_every_layout_and_no_scratch():
    k, dis = _kernels_of("addlayernorm_kernels")
    for dt in range(3):
        for wh in "01":
            for v in (1, 2, 4, 8):          # one wave per row: 1, 2, 4, 8 vectors per lane
                assert len([n for n in k if re.search(r"\d+layernorm_quant_rowsILi%dELi%dELi64ELb%sELb1EE" % (dt, v, wh), n)]) == 1, (dt, v, wh)
            for v in (1, 2, 4, 8, 16):      # 256 threads per row: 1 .. 16 vectors per thread
                assert len([n for n in k if re.search(r"\d+layernorm_quant_rowsILi%dELi%dELi256ELb%sELb1EE" % (dt, v, wh), n)]) == 1, (dt, v, wh)
        assert len([n for n in k if re.search(r"\d+layernorm_quant_genericILi%dELb1EE" % dt, n)]) == 1, dt
    assert len(k) == 3 * (8 + 10 + 1)
    for n, v in k.items():
        assert v.get("private_segment_fixed_size", 1) == 0 and v.get("vgpr_spill_count", 1) == 0 and v.get("sgpr_spill_count", 1) == 0, (n, v)
        assert v["vgpr_count"] <= 512, (n, v)          # (the unified count: VGPRs and AGPRs)
    assert "global_load_dwordx4" in dis and "global_store_dwordx4" in dis and "v_pk_add_f32" in dis and "v_pk_mul_f32" in dis and not FORBIDDEN.search(dis)


def test_the_new_kernels_are_in_an_object_of_their_own():
    """the pre-existing producer objects keep their kernels: nothing of K1al is instantiated in layernorm_kernels.o or addnorm_kernels.o"""
    for obj in ("layernorm_kernels", "addnorm_kernels"):
        k, _ = _kernels_of(obj)
        assert len(k) == 57 and not [n for n in k if re.search(r"\d+layernorm_quant_(rowsILi\d+ELi\d+ELi\d+ELb[01]|genericILi\d+)ELb1EE", n)], obj
