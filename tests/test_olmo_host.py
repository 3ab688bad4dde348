"""CPU: the host side of K1oq / K1oa / K1on (pq_olmo_postnorm_add_quant_rowwise): the symbol declared, exported and bound with its arguments in order; every bad
argument refused and named before any HIP call, in each of the three forms; the empty problems no-ops; no CPU path behind the Python entries, and their shape, dtype
and alias errors; and the new code object holding every row layout of the three forms without scratch or spills."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "pq_olmo_postnorm_add_quant_rowwise"
ARGS = ["x", "ld_x", "post_weight", "post_eps", "residual", "ld_r", "sum_out", "ld_s", "dtype", "rows", "cols", "q", "ld_q", "scale", "stream"]


def test_symbol_declared_exported_and_bound():
    from protoquant_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pq_hip.h")).read(), flags=re.S)
    m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % SYM, hdr)
    assert m, f"pq_hip.h does not declare {SYM}"
    assert [re.split(r"[\s*]+", a.strip())[-1] for a in m.group(1).split(",")] == ARGS
    L = _lib.lib()
    assert hasattr(L, SYM) and SYM in _lib.EXPORTS and len(getattr(L, SYM).argtypes) == len(ARGS)
    assert L.pq_version() == 1                                          # an addition: the ABI version stays
    assert SYM in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    import protoquant_amd as pq
    for name in ("olmo_postnorm_add_quantize", "olmo_postnorm_add", "olmo_rmsnorm", "OlmoRMSNorm", "PostNormFusedLayer", "fuse_olmo_layers", "is_olmo_rmsnorm",
                 "residual_flow_is_postnorm"):
        assert name in pq.__all__ and callable(getattr(pq, name)), name


ROW = 128 * 2          # bytes of one bf16 row


def _call(L, **kw):
    a = dict(x=0x10000, ldx=128, pw=0x80000, post_eps=1e-6, r=0x20000, ldr=128, s=0x30000, lds=128, dtype=0, rows=4, cols=128, q=0x50000, ldq=128, scale=0x60000)
    a.update(kw)
    return getattr(L, SYM)(a["x"], a["ldx"], a["pw"], a["post_eps"], a["r"], a["ldr"], a["s"], a["lds"], a["dtype"], a["rows"], a["cols"], a["q"], a["ldq"], a["scale"], None)


ADD_ONLY = dict(q=None, scale=None)                     # K1oa
NORM_ONLY = dict(r=None, ldr=0, q=None, scale=None)     # K1on (ld_r is not read)
BIG = dict(cols=1 << 24, ldx=1 << 24, ldr=1 << 24, lds=1 << 24, ldq=1 << 24)
BAD = [
    # a null operand, in each form
    (dict(x=None), b"x is null"), (dict(pw=None), b"post_weight is null"), (dict(s=None), b"sum_out is null"),
    (dict(ADD_ONLY, x=None), b"x is null"), (dict(ADD_ONLY, pw=None), b"post_weight is null"), (dict(ADD_ONLY, s=None), b"sum_out is null"),
    (dict(NORM_ONLY, x=None), b"x is null"), (dict(NORM_ONLY, pw=None), b"post_weight is null"), (dict(NORM_ONLY, s=None), b"sum_out is null"),
    # a partly-null q / scale group
    (dict(q=None), b"q is null"), (dict(scale=None), b"scale is null"),
    # q given without residual
    (dict(r=None), b"residual is null"), (dict(r=None, scale=None), b"residual is null"), (dict(r=None, q=None), b"residual is null"),
    # a leading dimension below cols
    (dict(ldx=64), b"ld_x"), (dict(ldr=64), b"ld_r"), (dict(lds=64), b"ld_s"), (dict(ldq=64), b"ld_q"), (dict(ADD_ONLY, ldx=64), b"ld_x"), (dict(ADD_ONLY, ldr=127), b"ld_r"),
    (dict(ADD_ONLY, lds=127), b"ld_s"), (dict(NORM_ONLY, ldx=64), b"ld_x"), (dict(NORM_ONLY, lds=127), b"ld_s"),
    # post_eps: negative, NaN, infinite
    (dict(post_eps=-1e-6), b"post_eps"), (dict(post_eps=float("nan")), b"post_eps"), (dict(post_eps=float("inf")), b"post_eps"),
    (dict(ADD_ONLY, post_eps=float("nan")), b"post_eps"), (dict(NORM_ONLY, post_eps=-1.0), b"post_eps"), (dict(NORM_ONLY, post_eps=float("inf")), b"post_eps"),
    # the shape and the dtype
    (BIG, b"cols"), (dict(ADD_ONLY, **BIG), b"cols"), (dict(NORM_ONLY, cols=1 << 24, ldx=1 << 24, lds=1 << 24), b"cols"), (dict(rows=-1), b"rows"), (dict(cols=-1), b"cols"),
    (dict(dtype=3), b"dtype"), (dict(dtype=-1), b"dtype"), (dict(NORM_ONLY, dtype=3), b"dtype"),
    # sum_out overlapping an input other than exactly
    (dict(s=0x10000 + 16), b"sum_out overlaps x"), (dict(s=0x10000 + ROW), b"sum_out overlaps x"), (dict(s=0x10000 - ROW), b"sum_out overlaps x"),
    (dict(s=0x10000, lds=256, ldx=128), b"sum_out overlaps x"), (dict(s=0x20000 + 2 * ROW), b"sum_out overlaps residual"),
    (dict(s=0x20000, lds=256), b"sum_out overlaps residual"), (dict(s=0x80000), b"sum_out overlaps post_weight"),
    (dict(s=0x80000 - 3 * ROW - 16), b"sum_out overlaps post_weight"), (dict(ADD_ONLY, s=0x10000 + 16), b"sum_out overlaps x"),
    (dict(ADD_ONLY, s=0x20000 + ROW), b"sum_out overlaps residual"), (dict(ADD_ONLY, s=0x80000), b"sum_out overlaps post_weight"),
    (dict(NORM_ONLY, s=0x10000 + 16), b"sum_out overlaps x"), (dict(NORM_ONLY, s=0x10000, lds=256), b"sum_out overlaps x"), (dict(NORM_ONLY, s=0x80000), b"sum_out overlaps post_weight"),
    # the outputs overlap nothing
    (dict(q=0x10000), b"q overlaps x"), (dict(q=0x80000 + 8), b"q overlaps post_weight"), (dict(q=0x20000 + 100), b"q overlaps residual"),
    (dict(q=0x30000 + 64), b"q overlaps sum_out"), (dict(scale=0x30000), b"scale overlaps sum_out"), (dict(scale=0x80000 + 4), b"scale overlaps post_weight"),
    (dict(scale=0x10000 + 4), b"scale overlaps x"), (dict(scale=0x50000 + 128), b"q overlaps scale"),
]


@pytest.mark.parametrize("kw,named", BAD, ids=[f"{i}-{n.decode().replace(' ', '_')}" for i, (_, n) in enumerate(BAD)])
def test_bad_arguments_are_named_without_a_gpu(kw, named):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _call(L, **kw) == 1, kw
    err = L.pq_last_error()
    assert SYM.encode() in err and named in err, (kw, err)


def test_the_permitted_aliases_pass_the_checks_of_an_empty_problem_and_empty_problems_are_no_ops():
    """rows == 0 or cols == 0 returns PQ_OK and touches nothing, in every form (the pointers are looked at after the empty problem, as in the neighbouring entry
    points); post_eps and the dtype are checked before it"""
    from protoquant_amd import _lib
    L = _lib.lib()
    for form in ({}, ADD_ONLY, NORM_ONLY):
        assert _call(L, rows=0, **form) == 0
        assert _call(L, **dict(dict(cols=0, ldx=0, ldr=0, lds=0, ldq=0), **form)) == 0
        assert _call(L, **dict(form, rows=0, x=None, pw=None, s=None)) == 0
        assert _call(L, rows=0, post_eps=-1.0, **form) == 1 and _call(L, **dict(form, rows=0, dtype=7)) == 1
    assert _call(L, rows=0, x=None, pw=None, r=None, s=None, q=None, scale=None) == 0
    assert _call(L, rows=0, q=None) == 0


def test_python_entries_have_no_cpu_fallback_and_check_their_operands():
    import protoquant_amd as pq
    from protoquant_amd import _lib, qtensor
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    w = torch.ones(64, dtype=torch.bfloat16)
    for call in (lambda: pq.olmo_postnorm_add_quantize(x, w, x.clone()), lambda: pq.olmo_postnorm_add(x, w, x.clone()), lambda: pq.olmo_rmsnorm(x, w),
                 lambda: pq.OlmoRMSNorm(w, 1e-6)(x)):
        with pytest.raises(_lib.PQError):
            call()
    sig = inspect.signature(pq.olmo_postnorm_add_quantize)
    assert list(sig.parameters) == ["x", "post_weight", "residual", "post_eps", "out"] and sig.parameters["post_eps"].default == 1e-6 and sig.parameters["out"].default is None
    assert str(inspect.signature(pq.olmo_postnorm_add)).split(" ->")[0] == str(sig).split(" ->")[0]
    sig = inspect.signature(pq.olmo_rmsnorm)
    assert list(sig.parameters) == ["x", "weight", "eps", "out"] and sig.parameters["eps"].default == 1e-6 and sig.parameters["out"].default is None
    mod = pq.OlmoRMSNorm(torch.nn.Parameter(w.clone()), 1e-5)
    assert list(mod.state_dict()) == ["weight"] and mod.variance_epsilon == 1e-5
    orig = _lib.require_gpu
    _lib.require_gpu = lambda t, name: None
    try:
        short, half = torch.ones(32, dtype=torch.bfloat16), w.half()
        for call in (lambda: pq.olmo_postnorm_add_quantize(x, short, x.clone()), lambda: pq.olmo_postnorm_add_quantize(x, half, x.clone()),
                     lambda: pq.olmo_postnorm_add_quantize(x, w, torch.zeros(4, 32, dtype=torch.bfloat16)), lambda: pq.olmo_postnorm_add_quantize(x, w, x.clone().half()),
                     lambda: pq.olmo_postnorm_add_quantize(x, w, x.clone(), out=torch.zeros(4, 32, dtype=torch.bfloat16)),
                     lambda: pq.olmo_postnorm_add_quantize(x, w, x.clone(), out=torch.zeros(64, 4, dtype=torch.bfloat16).t()),
                     lambda: pq.olmo_postnorm_add(x, short, x.clone()), lambda: pq.olmo_postnorm_add(x, w, x.clone().half()),
                     lambda: pq.olmo_postnorm_add(x, w, x.clone(), out=torch.zeros(64, 4, dtype=torch.bfloat16).t()),
                     lambda: pq.olmo_rmsnorm(x, short), lambda: pq.olmo_rmsnorm(x, half), lambda: pq.olmo_rmsnorm(x, w, out=torch.zeros(4, 32, dtype=torch.bfloat16)),
                     lambda: pq.olmo_rmsnorm(x, w, out=x.half()), lambda: pq.olmo_rmsnorm(x, w, out=torch.zeros(64, 4, dtype=torch.bfloat16).t())):
            with pytest.raises(ValueError):
                call()
        with pytest.raises(TypeError):
            pq.olmo_rmsnorm(x.double(), w.double())
    finally:
        _lib.require_gpu = orig
    assert qtensor.L.require_gpu is orig


def test_olmo_object_holds_every_layout_without_scratch():
    """every instantiation the dispatch can launch is in olmo_postnorm_kernels.o — K1oq, K1oa and K1on at every row layout, and the three generic kernels per dtype — and
    none uses scratch or spills; the objects of the Gemma post-norm and of the Llama add-norm hold none of them"""
    from tests.code_objects import kernels_of
    from tests.test_gemma_spec_host import _no_scratch_no_spills
    k = kernels_of("olmo_postnorm_kernels", must_be_built=True)
    for dt in range(3):
        for form in ("11", "10", "00"):            # (ADD, QUANT)
            for v in (1, 2, 4, 8):                 # one wave per row: 1, 2, 4, 8 vectors per lane
                assert len([n for n in k if re.search(r"\d+olmo_postnorm_rowsILi%dELi%dELi64ELb%sELb%sEE" % (dt, v, form[0], form[1]), n)]) == 1, (dt, v, form)
            for v in (1, 2, 4, 8, 16):             # 256 threads per row: 1 .. 16 vectors per thread
                assert len([n for n in k if re.search(r"\d+olmo_postnorm_rowsILi%dELi%dELi256ELb%sELb%sEE" % (dt, v, form[0], form[1]), n)]) == 1, (dt, v, form)
            assert len([n for n in k if re.search(r"\d+olmo_postnorm_genericILi%dELb%sELb%sEE" % (dt, form[0], form[1]), n)]) == 1, (dt, form)
    assert len(k) == 3 * 3 * (9 + 1)
    _no_scratch_no_spills(k)
    for obj in ("gemma_postnorm_kernels", "addnorm_kernels"):
        assert not [n for n in kernels_of(obj, must_be_built=True) if "olmo" in n], obj
