"""CPU: the host side of K1pl / K1l2 (pq_parallel_layernorm_quant_rowwise / add2_layernorm_quantize / layernorm_quantize2): the symbol is declared, exported and bound
with its argument list; every bad argument is refused and named before any HIP call; the allowed aliases pass; empty problems are no-ops; the Python entries have no
CPU path; the code object of parallel_layernorm_kernels.hip holds every row layout of the three forms for all three dtypes without scratch; the specification is A1
twice and then the LayerNorm specification on the stored sum — and its association is visible on the inputs the GPU test uses."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import add2lnorm_spec as A2
from tests import lnorm_spec as LS
from tests.addnorm_spec import add_a1
from tests.code_objects import kernels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "pq_parallel_layernorm_quant_rowwise"
ARGS = ["a", "ld_a", "b", "ld_b", "c", "ld_c", "sum_out", "ld_s", "weight1", "bias1", "eps1", "weight2", "bias2", "eps2", "dtype", "rows", "cols",
        "q1", "ld_q1", "scale1", "h1", "ld_h1", "q2", "ld_q2", "scale2", "h2", "ld_h2", "stream"]


def test_symbol_declared_exported_and_bound():
    from protoquant_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pq_hip.h")).read(), flags=re.S)
    m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % SYM, hdr)
    assert m, f"pq_hip.h does not declare {SYM}"
    assert [re.split(r"[\s*]+", a.strip())[-1] for a in m.group(1).split(",")] == ARGS
    L = _lib.lib()
    assert hasattr(L, SYM) and SYM in _lib.EXPORTS and len(getattr(L, SYM).argtypes) == len(ARGS) == 28
    assert L.pq_version() == 1                                          # an addition: the ABI version stays
    import protoquant_amd as pq
    for name in ("add2_layernorm_quantize", "layernorm_quantize2", "fuse_parallel_residual", "parallel_fused_blocks"):
        assert name in pq.__all__ and callable(getattr(pq, name))


def _call(L, **kw):
    """the entry with plausible (never dereferenced) operands, bf16 4 x 128, K1pl with two norms, some arguments overridden"""
    a = dict(a=0x10000, lda=128, b=0x20000, ldb=128, c=0x28000, ldc=128, s=0x30000, lds=128, w1=0x40000, b1=0x48000, eps1=1e-5, w2=0x41000, b2=0x49000, eps2=1e-6, dtype=0,
             rows=4, cols=128, q1=0x50000, ldq1=128, sc1=0x60000, h1=None, ldh1=0, q2=0x58000, ldq2=128, sc2=0x68000, h2=None, ldh2=0)
    a.update(kw)
    return L.pq_parallel_layernorm_quant_rowwise(a["a"], a["lda"], a["b"], a["ldb"], a["c"], a["ldc"], a["s"], a["lds"], a["w1"], a["b1"], a["eps1"], a["w2"], a["b2"],
                                                 a["eps2"], a["dtype"], a["rows"], a["cols"], a["q1"], a["ldq1"], a["sc1"], a["h1"], a["ldh1"], a["q2"], a["ldq2"], a["sc2"],
                                                 a["h2"], a["ldh2"], None)


ROW = 128 * 2          # bytes of one bf16 row
NO_ADD = dict(a=None, b=None, s=None)
ONE = dict(w2=None, b2=None, q2=None, sc2=None)


@pytest.mark.parametrize("kw,named", [
    (dict(s=None), b"sum_out is null"), (dict(c=None), b"c is null"), (dict(w1=None), b"weight1 is null"), (dict(q1=None), b"q1 is null"), (dict(sc1=None), b"scale1 is null"),
    (dict(q2=None), b"q2 is null"), (dict(sc2=None), b"scale2 is null"),
    (dict(a=None), b"a is null and b is not"), (dict(b=None), b"b is null and a is not"),                      # exactly one of a, b
    (dict(a=None, b=None), b"sum_out must be null"),                                                          # no add: nothing is stored
    (dict(**NO_ADD, **ONE), b"pq_layernorm_quant_rowwise"),                                                   # no add and one norm: another entry's job
    (dict(w2=None), b"bias2 must be null"), (dict(w2=None, b2=None), b"q2 must be null"), (dict(w2=None, b2=None, q2=None), b"scale2 must be null"),
    (dict(**ONE, h2=0x70000, ldh2=128), b"h2 must be null"),
    (dict(dtype=3), b"dtype"), (dict(dtype=-1), b"dtype"), (dict(rows=-1), b"rows"), (dict(cols=-1), b"cols"),
    (dict(cols=1 << 24, lda=1 << 24, ldb=1 << 24, ldc=1 << 24, lds=1 << 24, ldq1=1 << 24, ldq2=1 << 24), b"cols"),
    (dict(lda=64), b"ld_a"), (dict(ldb=64), b"ld_b"), (dict(ldc=64), b"ld_c"), (dict(lds=64), b"ld_s"), (dict(ldq1=64), b"ld_q1"), (dict(ldq2=64), b"ld_q2"),
    (dict(h1=0x70000, ldh1=64), b"ld_h1"), (dict(h2=0x78000, ldh2=64), b"ld_h2"),
    (dict(eps1=float("nan")), b"eps"), (dict(eps1=float("inf")), b"eps"), (dict(eps1=-1e-6), b"eps"),
    (dict(eps2=float("nan")), b"eps2"), (dict(eps2=float("inf")), b"eps2"), (dict(eps2=-1e-6), b"eps2"),
    # sum_out: exactly a / b / c is fine (below); anything else that overlaps them is not
    (dict(s=0x10000 + 16), b"sum_out overlaps a"), (dict(s=0x10000 + ROW), b"sum_out overlaps a"), (dict(s=0x10000 - ROW), b"sum_out overlaps a"),
    (dict(s=0x10000, lds=256, lda=128), b"sum_out overlaps a"),                      # the same pointer, another leading dimension
    (dict(s=0x20000 + 2 * ROW), b"sum_out overlaps b"), (dict(s=0x28000 + ROW), b"sum_out overlaps c"), (dict(s=0x40000), b"sum_out overlaps weight1"),
    (dict(s=0x48000 - ROW), b"sum_out overlaps bias1"), (dict(s=0x41000), b"sum_out overlaps weight2"), (dict(s=0x49000 - ROW), b"sum_out overlaps bias2"),
    # q, scale, h of either group: nothing may overlap them
    (dict(q1=0x10000), b"q1 overlaps a"), (dict(q1=0x20000 + 100), b"q1 overlaps b"), (dict(q2=0x28000 + 8), b"q2 overlaps c"), (dict(q1=0x40000 + 8), b"q1 overlaps weight1"),
    (dict(q2=0x49000 + 8), b"q2 overlaps bias2"), (dict(q1=0x30000 + 64), b"q1 overlaps sum_out"), (dict(q2=0x30000 + 64), b"q2 overlaps sum_out"),
    (dict(q2=0x50000 + 256), b"q1 overlaps q2"), (dict(sc2=0x60000 + 8), b"scale1 overlaps scale2"), (dict(sc1=0x58000 + 128), b"scale1 overlaps q2"),
    (dict(sc1=0x10000 + 4), b"scale1 overlaps a"), (dict(sc2=0x30000), b"scale2 overlaps sum_out"), (dict(sc2=0x48000), b"scale2 overlaps bias1"),
    (dict(h1=0x10000, ldh1=128), b"h1 overlaps a"), (dict(h2=0x28000 + ROW, ldh2=128), b"h2 overlaps c"), (dict(h1=0x30000, ldh1=128), b"h1 overlaps sum_out"),
    (dict(h2=0x41000, ldh2=128), b"h2 overlaps weight2"), (dict(h1=0x50000 + 256, ldh1=128), b"q1 overlaps h1"), (dict(h1=0x58000, ldh1=128), b"h1 overlaps q2"),
    (dict(h1=0x70000, ldh1=128, h2=0x70000 + ROW, ldh2=128), b"h1 overlaps h2"), (dict(h2=0x68000 - 64, ldh2=128), b"scale2 overlaps h2"),
    # the form without the add: c is the only matrix input
    (dict(**NO_ADD, q1=0x28000), b"q1 overlaps c"), (dict(**NO_ADD, c=None), b"c is null"), (dict(**NO_ADD, h2=0x28000, ldh2=128), b"h2 overlaps c"),
])
def test_bad_arguments_are_named_without_a_gpu(kw, named):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _call(L, **kw) == 1, kw
    err = L.pq_last_error()
    assert SYM.encode() in err and named in err, (kw, err)


@pytest.mark.skipif(torch.cuda.is_available(), reason="argument-check-only test: needs a machine without a GPU (the operands are not real memory)")
def test_allowed_aliases_null_biases_and_the_three_forms_pass_the_checks():
    """sum_out == a / b / c (same pointer and leading dimension), a == b, null biases, one norm, the form without the add and disjoint column blocks of one buffer get
    PAST the argument checks: on a machine without a GPU the launch then fails (status 3, not 1)"""
    from protoquant_amd import _lib
    L = _lib.lib()
    for kw in (dict(), dict(s=0x10000), dict(s=0x20000), dict(s=0x28000), dict(b=0x10000, s=0x10000), dict(b1=None), dict(b2=None, s=0x28000), ONE, dict(**ONE, b1=None, s=0x20000),
               NO_ADD, dict(**NO_ADD, b1=None, b2=None), dict(a=0x10000, lda=256, s=0x10000 + ROW, lds=256), dict(c=0x28000, ldc=256, s=0x28000, lds=256),
               dict(h1=0x70000, ldh1=128), dict(h1=0x70000, ldh1=128, h2=0x78000, ldh2=128), dict(h2=0x78000, ldh2=128)):
        st = _call(L, **kw)
        assert st == 3 and b"overlaps" not in L.pq_last_error(), (kw, st, L.pq_last_error())


def test_empty_problems_are_no_ops_without_a_gpu():
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _call(L, rows=0) == 0
    assert _call(L, cols=0, lda=0, ldb=0, ldc=0, lds=0, ldq1=0, ldq2=0) == 0
    assert _call(L, rows=0, a=None, b=None, c=None, s=None, w1=None, b1=None, w2=None, b2=None, q1=None, sc1=None, q2=None, sc2=None) == 0
    assert _call(L, rows=0, a=None) == 0          # an empty problem reads no pointer: which form it would have been is not asked


def test_python_entries_have_no_cpu_fallback_and_check_their_operands():
    import protoquant_amd as pq
    from protoquant_amd import _lib, qtensor
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    w = torch.ones(64, dtype=torch.bfloat16)
    with pytest.raises(_lib.PQError):
        pq.add2_layernorm_quantize(x, x.clone(), x.clone(), w, None)
    with pytest.raises(_lib.PQError):
        pq.layernorm_quantize2(x, w, None, w.clone(), None)
    sig = inspect.signature(pq.add2_layernorm_quantize)
    assert list(sig.parameters) == ["a", "b", "c", "weight", "bias", "eps", "weight2", "bias2", "eps2", "out", "return_h"]
    assert sig.parameters["eps"].default == 1e-5 and all(sig.parameters[n].default is None for n in ("weight2", "bias2", "eps2", "out")) and sig.parameters["return_h"].default is False
    sig2 = inspect.signature(pq.layernorm_quantize2)
    assert list(sig2.parameters) == ["x", "weight", "bias", "weight2", "bias2", "eps", "eps2", "return_h"]
    assert sig2.parameters["eps"].default == 1e-5 and sig2.parameters["eps2"].default is None and sig2.parameters["return_h"].default is False
    orig = _lib.require_gpu
    _lib.require_gpu = lambda t, name: None
    try:
        bf, hf = torch.bfloat16, torch.float16
        for bad in (dict(b=torch.zeros(4, 32, dtype=bf)), dict(b=torch.zeros(4, 64, dtype=hf)), dict(c=torch.zeros(4, 32, dtype=bf)), dict(c=torch.zeros(4, 64, dtype=hf)),
                    dict(weight=None), dict(weight=torch.ones(32, dtype=bf)), dict(weight=torch.ones(64, dtype=torch.float32)), dict(bias=torch.ones(32, dtype=bf)),
                    dict(bias=torch.ones(64, dtype=hf)), dict(weight2=torch.ones(32, dtype=bf)), dict(weight2=torch.ones(64, dtype=hf)),
                    dict(weight2=w.clone(), bias2=torch.ones(32, dtype=bf)), dict(bias2=torch.ones(64, dtype=bf)), dict(eps2=1e-6),
                    dict(out=torch.zeros(4, 32, dtype=bf)), dict(out=torch.zeros(4, 64, dtype=hf)), dict(out=torch.zeros(64, 4, dtype=bf).t())):
            a = dict(a=x, b=x.clone(), c=x.clone(), weight=w, bias=None)
            a.update(bad)
            with pytest.raises(ValueError):
                pq.add2_layernorm_quantize(**a)
        for bad in (dict(weight=None), dict(weight2=None), dict(weight2=torch.ones(32, dtype=bf)), dict(bias=torch.ones(64, dtype=hf)), dict(bias2=torch.ones(32, dtype=bf))):
            a = dict(x=x, weight=w, bias=None, weight2=w.clone(), bias2=None)
            a.update(bad)
            with pytest.raises(ValueError):
                pq.layernorm_quantize2(**a)
    finally:
        _lib.require_gpu = orig
    assert qtensor.L.require_gpu is orig


def test_spec_is_a1_twice_then_the_layernorm_spec_per_group():
    """tests/add2lnorm_spec.py composes and adds nothing: A2 is what two eager torch adds store, the rest is tests/lnorm_spec on the stored sum, once per group"""
    for dt, code in ((torch.bfloat16, 0), (torch.float16, 1), (torch.float32, 2)):
        a, b, c, w1, b1, w2, b2 = A2.inputs(5, 96, dt, 1)
        s_bits, gs = A2.add2_layernorm_quantize(a, b, c, [(w1, b1, 1e-5), (w2, None, 1e-3)])
        assert np.array_equal(s_bits, A2.to_bits((a + b) + c)) and np.array_equal(s_bits, A2.to_bits(add_a1(add_a1(a, b), c))) and len(gs) == 2
        for (q, sc, h), (w, bias, eps) in zip(gs, ((w1, b1, 1e-5), (w2, None, 1e-3))):
            q2, sc2, h2 = LS.layernorm_quantize(s_bits, A2.to_bits(w), None if bias is None else A2.to_bits(bias), eps, code)
            assert np.array_equal(q, q2) and np.array_equal(sc, sc2) and np.array_equal(h, h2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "f32"])
def test_the_association_is_visible_on_the_gpu_tests_inputs(dtype):
    """a test that could not tell (a + b) + c from the other groupings would hold an order-insensitive kernel to nothing: on the seeded inputs of
    tests/test_gpu_parallel_norm.py the specification's sum differs from each of the two other associations in at least 10 % of the elements"""
    epv = 4 if dtype == torch.float32 else 8
    for rows, cols, seed in ((9, 64 * epv, 100 + 64 + 9), (5, 1024 * epv, 100 + 1024 + 5), (9, 333, 300 + 333 + 9), (300, 2560, 2560)):
        a, b, c = A2.inputs(rows, cols, dtype, seed)[:3]
        s = A2.to_bits(A2.add_a2(a, b, c))
        for name, other in (("a + (b + c)", add_a1(a, add_a1(b, c))), ("(a + c) + b", add_a1(add_a1(a, c), b))):
            frac = float(np.mean(s != A2.to_bits(other)))
            assert frac >= 0.10, (dtype, rows, cols, name, frac)




def test_code_object_has_every_layout_of_the_three_forms_and_no_scratch():
    k = kernels_of("parallel_layernorm_kernels")
    forms = (("b1", 1), ("b1", 2), ("b0", 2))          # (ADD2, NORMS): K1pl with one norm, with two, K1l2 — and never the plain K1l
    for dt in range(3):
        for add, norms in forms:
            for wh in "01":
                for tpr, vs in ((64, (1, 2, 4, 8)), (256, (1, 2, 4, 8, 16))):
                    for v in vs:
                        pat = r"\d+parallel_layernorm_quant_rowsILi%dELi%dELi%dELb%sEL%sELi%dEE" % (dt, v, tpr, wh, add, norms)
                        assert len([n for n in k if re.search(pat, n)]) == 1, (dt, v, tpr, wh, add, norms)
            assert len([n for n in k if re.search(r"\d+parallel_layernorm_quant_genericILi%dEL%sELi%dEE" % (dt, add, norms), n)]) == 1, (dt, add, norms)
    assert len(k) == 3 * 3 * (18 + 1)
    assert not [n for n in k if re.search(r"ELb0ELi1EE", n)]          # no add and one norm is K1l: not instantiated again
    for n, v in k.items():
        assert v.get("private_segment_fixed_size", 1) == 0 and v.get("vgpr_spill_count", 1) == 0, (n, v)          # no scratch, no VGPR spilled
        assert v["vgpr_count"] <= 512, (n, v)          # (the unified count: VGPRs and AGPRs)
