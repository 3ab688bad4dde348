"""CPU: the specification and the host side of K1pang / K1pa (pq_gemma_postnorm_add_rmsnorm_quant_rowwise): the symbol declared, exported and bound with its
arguments in order; every bad argument refused and named before any HIP call; the empty problems no-ops; the specification (tests/gemma_postnorm_spec.py) on one
hand-computed row and against its parts; no CPU path behind the Python entries; and the new code object holding every row layout without scratch or spills."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import gemma_postnorm_spec as P
from tests import gemma_spec as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "pq_gemma_postnorm_add_rmsnorm_quant_rowwise"
ARGS = ["x", "ld_x", "post_weight", "post_eps", "residual", "ld_r", "sum_out", "ld_s", "weight", "eps", "dtype", "rows", "cols", "q", "ld_q", "scale", "h_out", "ld_h",
        "stream"]


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
    for name in ("gemma_postnorm_add_rmsnorm_quantize", "gemma_postnorm_add", "SandwichFusedLayer", "fuse_gemma_postnorm_residual", "residual_flow_is_sandwich"):
        assert name in pq.__all__ and callable(getattr(pq, name)), name


ROW = 128 * 2          # bytes of one bf16 row


def _call(L, **kw):
    a = dict(x=0x10000, ldx=128, pw=0x80000, post_eps=1e-6, r=0x20000, ldr=128, s=0x30000, lds=128, w=0x40000, eps=1e-6, dtype=0, rows=4, cols=128, q=0x50000, ldq=128,
             scale=0x60000, h=None, ldh=0)
    a.update(kw)
    return getattr(L, SYM)(a["x"], a["ldx"], a["pw"], a["post_eps"], a["r"], a["ldr"], a["s"], a["lds"], a["w"], a["eps"], a["dtype"], a["rows"], a["cols"], a["q"], a["ldq"],
                           a["scale"], a["h"], a["ldh"], None)


ADD_ONLY = dict(w=None, q=None, scale=None, h=None)
BIG = dict(cols=1 << 24, ldx=1 << 24, ldr=1 << 24, lds=1 << 24, ldq=1 << 24)
BAD = [
    # a null operand
    (dict(x=None), b"x is null"), (dict(pw=None), b"post_weight is null"), (dict(r=None), b"residual is null"), (dict(s=None), b"sum_out is null"),
    (dict(ADD_ONLY, x=None), b"x is null"), (dict(ADD_ONLY, pw=None), b"post_weight is null"), (dict(ADD_ONLY, r=None), b"residual is null"),
    (dict(ADD_ONLY, s=None), b"sum_out is null"),
    # a partly-null quantisation group
    (dict(w=None), b"weight is null"), (dict(q=None), b"q is null"), (dict(scale=None), b"scale is null"), (dict(w=None, q=None), b"weight is null"),
    (dict(q=None, scale=None), b"q is null"), (dict(w=None, q=None, scale=None, h=0x70000, ldh=128), b"weight is null"), (dict(w=None, scale=None), b"weight is null"),
    # a leading dimension below cols
    (dict(ldx=64), b"ld_x"), (dict(ldr=64), b"ld_r"), (dict(lds=64), b"ld_s"), (dict(ldq=64), b"ld_q"), (dict(h=0x70000, ldh=64), b"ld_h"),
    (dict(ADD_ONLY, ldx=64), b"ld_x"), (dict(ADD_ONLY, lds=127), b"ld_s"),
    # eps and post_eps: negative, NaN, infinite
    (dict(eps=-1e-6), b"eps must"), (dict(eps=float("nan")), b"eps must"), (dict(eps=float("inf")), b"eps must"),
    (dict(post_eps=-1e-6), b"post_eps"), (dict(post_eps=float("nan")), b"post_eps"), (dict(post_eps=float("inf")), b"post_eps"),
    (dict(ADD_ONLY, post_eps=float("nan")), b"post_eps"), (dict(ADD_ONLY, post_eps=-1.0), b"post_eps"),
    # the shape and the dtype
    (BIG, b"cols"), (dict(ADD_ONLY, **BIG), b"cols"), (dict(rows=-1), b"rows"), (dict(cols=-1), b"cols"), (dict(dtype=3), b"dtype"), (dict(dtype=-1), b"dtype"),
    # sum_out overlapping an input other than exactly
    (dict(s=0x10000 + 16), b"sum_out overlaps x"), (dict(s=0x10000 + ROW), b"sum_out overlaps x"), (dict(s=0x10000 - ROW), b"sum_out overlaps x"),
    (dict(s=0x10000, lds=256, ldx=128), b"sum_out overlaps x"), (dict(s=0x20000 + 2 * ROW), b"sum_out overlaps residual"),
    (dict(s=0x20000, lds=256), b"sum_out overlaps residual"), (dict(s=0x40000), b"sum_out overlaps weight"), (dict(s=0x80000), b"sum_out overlaps post_weight"),
    (dict(s=0x80000 - 3 * ROW - 16), b"sum_out overlaps post_weight"), (dict(ADD_ONLY, s=0x10000 + 16), b"sum_out overlaps x"),
    (dict(ADD_ONLY, s=0x80000), b"sum_out overlaps post_weight"),
    # the outputs overlap nothing
    (dict(q=0x10000), b"q overlaps x"), (dict(q=0x80000 + 8), b"q overlaps post_weight"), (dict(q=0x20000 + 100), b"q overlaps residual"),
    (dict(q=0x40000 + 8), b"q overlaps weight"), (dict(q=0x30000 + 64), b"q overlaps sum_out"), (dict(scale=0x30000), b"scale overlaps sum_out"),
    (dict(scale=0x80000 + 4), b"scale overlaps post_weight"), (dict(scale=0x50000 + 128), b"q overlaps scale"), (dict(h=0x10000, ldh=128), b"h_out overlaps x"),
    (dict(h=0x80000, ldh=128), b"h_out overlaps post_weight"), (dict(h=0x30000, ldh=128), b"h_out overlaps sum_out"), (dict(h=0x50000 + 256, ldh=128), b"q overlaps h_out"),
]


@pytest.mark.parametrize("kw,named", BAD, ids=[f"{i}-{n.decode().replace(' ', '_')}" for i, (_, n) in enumerate(BAD)])
def test_bad_arguments_are_named_without_a_gpu(kw, named):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _call(L, **kw) == 1, kw
    err = L.pq_last_error()
    assert SYM.encode() in err and named in err, (kw, err)


def test_empty_problems_are_no_ops_without_a_gpu():
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _call(L, rows=0) == 0 and _call(L, cols=0, ldx=0, ldr=0, lds=0, ldq=0) == 0
    assert _call(L, rows=0, x=None, pw=None, r=None, s=None, w=None, q=None, scale=None) == 0
    assert _call(L, rows=0, **ADD_ONLY) == 0 and _call(L, cols=0, ldx=0, ldr=0, lds=0, ldq=0, **ADD_ONLY) == 0
    assert _call(L, rows=0, q=None) == 0                                # (the pointers are looked at after the empty problem, as in the neighbouring entry points)
    assert _call(L, rows=0, post_eps=-1.0) == 1 and _call(L, rows=0, dtype=7) == 1          # eps, post_eps and the dtype before it


# ---------------------------------------------------------------------------------------------------------------- the specification
def test_spec_on_one_hand_computed_row():
    """x = 2 2 2 2, post_eps = 0: mean(x^2) = 4, rs_p = 1/2;  post_weight = 0 1 -.5 .5  ->  p = 1 2 .5 1.5;  residual = 1 0 1.5 .5  ->  s = 2 2 2 2;  eps = 0: rs = 1/2;
    weight = 0 2 -.5 3  ->  h = 1 3 .5 4;  amax 4, scale = 4/127, codes = rne(h * 127/4) = rne(31.75 95.25 15.875 127) = 32 95 16 127"""
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        x = torch.tensor([[2.0, 2.0, 2.0, 2.0]], dtype=dt)
        pw = torch.tensor([0.0, 1.0, -0.5, 0.5], dtype=dt)
        r = torch.tensor([[1.0, 0.0, 1.5, 0.5]], dtype=dt)
        w = torch.tensor([0.0, 2.0, -0.5, 3.0], dtype=dt)
        assert P.postnorm(x, pw, 0.0).float().tolist() == [[1.0, 2.0, 0.5, 1.5]]
        assert P.postnorm_add(x, pw, r, 0.0).float().tolist() == [[2.0, 2.0, 2.0, 2.0]]
        q, sc, s, h = P.postnorm_add_rmsnorm_quantize(x, pw, r, w, 0.0, 0.0)
        assert G.as_tensor(s, dt).float().tolist() == [[2.0, 2.0, 2.0, 2.0]] and G.as_tensor(h, dt).float().tolist() == [[1.0, 3.0, 0.5, 4.0]]
        assert q.tolist() == [[32, 95, 16, 127]] and sc.dtype == np.float32 and sc.tolist() == [float(np.float32(4.0) / np.float32(127.0))]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "f32"])
def test_spec_is_its_three_parts_and_rounds_p(dt):
    """the composition of the docstrings, part by part; distinct eps / post_eps and weights are told apart; the rounding of p changes stored sums in the 16-bit dtypes and
    nothing in f32"""
    g = torch.Generator().manual_seed(19)
    x = (torch.randn(5, 520, generator=g) * torch.tensor([[0.05], [1.0], [20.0], [3.0], [0.3]])).to(dt)
    r = (torch.randn(5, 520, generator=g) * 2).to(dt)
    pw, w = (0.3 * torch.randn(520, generator=g)).to(dt), (0.3 * torch.randn(520, generator=g)).to(dt)
    post_eps, eps = 1e-5, 1e-6
    q, sc, s, h = P.postnorm_add_rmsnorm_quantize(x, pw, r, w, eps, post_eps)
    p = G.as_tensor(G.gemma_rmsnorm_quantize_t(x, pw, post_eps)[2], dt)
    assert torch.equal(P.postnorm(x, pw, post_eps), p)
    summed = (r.float() + p.float()).to(dt)
    assert np.array_equal(s, G.to_bits(summed))
    q2, sc2, h2 = G.gemma_rmsnorm_quantize_t(summed, w, eps)
    assert np.array_equal(q, q2) and np.array_equal(sc, sc2) and np.array_equal(h, h2)
    assert not np.array_equal(P.postnorm_add_rmsnorm_quantize(x, w, r, pw, eps, post_eps)[2], s)                 # the two weights are not interchangeable
    x_small = (x.float() * 1e-3).to(dt)
    assert not torch.equal(P.postnorm(x_small, pw, 1e-5), P.postnorm(x_small, pw, 1e-6))                         # nor the two eps
    # p as the eager module computes it: on these operands the specified post-norm is the eager formula in the 16-bit dtypes (the sums differ only below the rounding)
    xf = x.float()
    eager = ((xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + post_eps)) * (1.0 + pw.float())).to(dt)
    if dt != torch.float32:
        assert torch.equal(eager, p)
    pu = torch.from_numpy(P.unrounded_p(x, pw, post_eps))
    assert torch.equal(pu.to(dt), p)                                                                             # p IS the rounding of that binary32 value
    su = P.unrounded_sum(x, pw, r, post_eps)
    assert torch.equal(su, summed) == (dt == torch.float32)


def test_python_entries_have_no_cpu_fallback_and_check_their_operands():
    import protoquant_amd as pq
    from protoquant_amd import _lib, qtensor
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    w = torch.ones(64, dtype=torch.bfloat16)
    norm = pq.GemmaSandwichNormQuant(w, 1e-6)
    post = pq.GemmaRMSNormQuant(w, 1e-6)          # (anything with a weight and an eps)
    for call in (lambda: pq.gemma_postnorm_add_rmsnorm_quantize(x, w, x.clone(), w), lambda: pq.gemma_postnorm_add(x, w, x.clone()),
                 lambda: norm(x, residual=x.clone(), post_norm=post), lambda: norm(x), lambda: norm(x, residual=x.clone())):
        with pytest.raises(_lib.PQError):
            call()
    with pytest.raises(ValueError):
        norm(x, post_norm=post)
    sig = inspect.signature(pq.gemma_postnorm_add_rmsnorm_quantize)
    assert list(sig.parameters) == ["x", "post_weight", "residual", "weight", "eps", "post_eps", "out", "return_h"]
    assert [sig.parameters[n].default for n in ("eps", "post_eps", "out", "return_h")] == [1e-6, 1e-6, None, False]
    sig = inspect.signature(pq.gemma_postnorm_add)
    assert list(sig.parameters) == ["x", "post_weight", "residual", "post_eps", "out"] and sig.parameters["post_eps"].default == 1e-6 and sig.parameters["out"].default is None
    assert list(inspect.signature(pq.GemmaSandwichNormQuant.forward).parameters) == ["self", "x", "residual", "post_norm"]
    assert issubclass(pq.GemmaSandwichNormQuant, pq.GemmaRMSNormQuant)
    orig = _lib.require_gpu
    _lib.require_gpu = lambda t, name: None
    try:
        short, half = torch.ones(32, dtype=torch.bfloat16), w.half()
        for call in (lambda: pq.gemma_postnorm_add_rmsnorm_quantize(x, short, x.clone(), w), lambda: pq.gemma_postnorm_add_rmsnorm_quantize(x, w, x.clone(), short),
                     lambda: pq.gemma_postnorm_add_rmsnorm_quantize(x, half, x.clone(), w), lambda: pq.gemma_postnorm_add_rmsnorm_quantize(x, w, x.clone(), half),
                     lambda: pq.gemma_postnorm_add_rmsnorm_quantize(x, w, torch.zeros(4, 32, dtype=torch.bfloat16), w),
                     lambda: pq.gemma_postnorm_add_rmsnorm_quantize(x, w, x.clone().half(), w),
                     lambda: pq.gemma_postnorm_add_rmsnorm_quantize(x, w, x.clone(), w, out=torch.zeros(4, 32, dtype=torch.bfloat16)),
                     lambda: pq.gemma_postnorm_add_rmsnorm_quantize(x, w, x.clone(), w, out=torch.zeros(64, 4, dtype=torch.bfloat16).t()),
                     lambda: pq.gemma_postnorm_add(x, short, x.clone()), lambda: pq.gemma_postnorm_add(x, w, x.clone().half()),
                     lambda: pq.gemma_postnorm_add(x, w, x.clone(), out=torch.zeros(64, 4, dtype=torch.bfloat16).t())):
            with pytest.raises(ValueError):
                call()
    finally:
        _lib.require_gpu = orig
    assert qtensor.L.require_gpu is orig


# ---------------------------------------------------------------------------------------------------------------- the code object
def test_postnorm_object_holds_every_layout_without_scratch():
    """every instantiation the dispatch can launch is in gemma_postnorm_kernels.o — K1pang with and without h_out and K1pa, at every row layout, and the two generic
    kernels per dtype — and none uses scratch or spills; the objects of the existing Gemma norm kernels hold none of them"""
    from tests.code_objects import kernels_of
    from tests.test_gemma_spec_host import _no_scratch_no_spills
    k = kernels_of("gemma_postnorm_kernels", must_be_built=True)
    for dt in range(3):
        for wh, qn in ("01", "11", "00"):          # (WRITE_H, QUANT)
            for v in (1, 2, 4, 8):                 # one wave per row: 1, 2, 4, 8 vectors per lane
                assert len([n for n in k if re.search(r"\d+gemma_postnorm_add_rowsILi%dELi%dELi64ELb%sELb%sEE" % (dt, v, wh, qn), n)]) == 1, (dt, v, wh, qn)
            for v in (1, 2, 4, 8, 16):             # 256 threads per row: 1 .. 16 vectors per thread
                assert len([n for n in k if re.search(r"\d+gemma_postnorm_add_rowsILi%dELi%dELi256ELb%sELb%sEE" % (dt, v, wh, qn), n)]) == 1, (dt, v, wh, qn)
        for qn in "01":
            assert len([n for n in k if re.search(r"\d+gemma_postnorm_add_genericILi%dELb%sEE" % (dt, qn), n)]) == 1, (dt, qn)
    assert len(k) == 3 * (3 * 9 + 2)
    _no_scratch_no_spills(k)
    for obj in ("gemma_norm_kernels", "add_gemma_norm_kernels"):
        assert not [n for n in kernels_of(obj, must_be_built=True) if "postnorm" in n], obj
