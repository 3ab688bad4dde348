"""CPU: the specification and the host side of the Gemma kernels (K1ng pq_gemma_rmsnorm_quant_rowwise, K1ang pq_add_gemma_rmsnorm_quant_rowwise, K1gg
pq_gelu_mul_quant_rowwise): tests/gemma_spec.py against transformers' GemmaRMSNorm and against torch's act_fn(g) * u on every 16-bit pattern; the three symbols
declared, exported and bound; every bad argument refused and named before any HIP call; empty problems no-ops; no CPU path behind the Python entries; the three new
code objects hold every row layout they dispatch to without scratch or spills, and the objects that existed before hold none of the new kernels."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import act_spec as U
from tests import gemma_spec as G
from tests.code_objects import kernels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"pq_gemma_rmsnorm_quant_rowwise": ["x", "ld_x", "weight", "eps", "dtype", "rows", "cols", "q", "ld_q", "scale", "h_out", "ld_h", "stream"],
        "pq_add_gemma_rmsnorm_quant_rowwise": ["x", "ld_x", "residual", "ld_r", "sum_out", "ld_s", "weight", "eps", "dtype", "rows", "cols", "q", "ld_q", "scale", "h_out",
                                               "ld_h", "stream"],
        "pq_gelu_mul_quant_rowwise": ["g", "ld_g", "u", "ld_u", "dtype", "rows", "cols", "kind", "q", "ld_q", "scale", "h_out", "ld_h", "stream"]}


# ---------------------------------------------------------------------------------------------------------------- the specification
def _gemma_inputs(rows, H, dtype, seed):
    """rows scaled log-uniformly over 0.05 .. 20, weight 0.3 randn"""
    g = torch.Generator().manual_seed(seed)
    scale = torch.exp(torch.empty(rows, 1).uniform_(float(np.log(0.05)), float(np.log(20.0)), generator=g))
    x = (torch.randn(rows, H, generator=g) * scale).to(dtype)
    w = (0.3 * torch.randn(H, generator=g)).to(dtype)
    return x, w


def test_ng_spec_against_transformers_gemma_rmsnorm():
    """10^6 bf16 elements through transformers' GemmaRMSNorm and through NG1-NG6: they differ only by the pinned summation order — identical row scales, and no
    stored value more than 2 ulp apart"""
    g1 = pytest.importorskip("transformers.models.gemma.modeling_gemma")
    rows, H, eps = 435, 2304, 1e-6
    assert rows * H >= 10 ** 6
    x, w = _gemma_inputs(rows, H, torch.bfloat16, 11)
    norm = g1.GemmaRMSNorm(H, eps=eps).to(torch.bfloat16)
    with torch.no_grad():
        norm.weight.copy_(w)
        want = norm(x)
    q, sc, h = G.gemma_rmsnorm_quantize_t(x, w, eps)
    got = G.as_tensor(h, torch.bfloat16)
    d = G.ulp_distance(got, want)
    q_e, sc_e = G.Q.quantize(G.to_bits(want), 0, 1)
    print(f"NG vs GemmaRMSNorm, {rows} x {H} bf16: stored values differing {float((d > 0).float().mean()):.3g}, max {int(d.max())} ulp, "
          f"codes differing {float((q != q_e).mean()):.3g}, scales differing {int((sc != sc_e).sum())}")
    assert int(d.max()) <= 2
    assert np.array_equal(sc, sc_e)


def test_ng_is_not_the_llama_form_with_a_folded_weight():
    """why K1n cannot serve: N5 on the weight 1 + w (rounded to bf16, and two storage roundings) stores other values than NG5"""
    from oracle import qspec_numpy as Q
    x, w = _gemma_inputs(64, 512, torch.bfloat16, 5)
    folded = (1.0 + w.float()).to(torch.bfloat16)
    h_n = Q.rmsnorm_quantize(G.to_bits(x), G.to_bits(folded), 1e-6, 0)[2]
    h_g = G.gemma_rmsnorm_quantize_t(x, w, 1e-6)[2]
    assert (h_n != h_g).mean() > 0.01


def test_add_spec_is_the_add_then_ng():
    g = torch.Generator().manual_seed(1)
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        x = torch.randn(5, 96, generator=g).to(dt)
        r = (torch.randn(5, 96, generator=g) * 4).to(dt)
        w = (0.3 * torch.randn(96, generator=g)).to(dt)
        q, sc, sb, h = G.add_gemma_rmsnorm_quantize(x, r, w, 1e-6)
        assert np.array_equal(sb, G.to_bits(r + x))
        q2, sc2, h2 = G.gemma_rmsnorm_quantize_t(r + x, w, 1e-6)
        assert np.array_equal(q, q2) and np.array_equal(sc, sc2) and np.array_equal(h, h2)


U_VALUES = (1.0, -1.0, 0.5, -2.0, 3.140625, 0.333251953125, 1e-3, 300.0, -0.0751953125, 0.0, 1.0e4, float("inf"))


@pytest.mark.parametrize("dtype,code", [(torch.bfloat16, 0), (torch.float16, 1)], ids=["bf16", "fp16"])
def test_gg_spec_on_every_pattern_against_torch(dtype, code):
    """all 65 536 patterns of g against 12 values of u: wherever the stored U2 value equals torch's stored gelu, h equals torch's act_fn(g) * u bit for bit (the
    product of two 16-bit values is exact in binary32 and is rounded once, as torch rounds it); NaNs compare as a class"""
    assert len(U_VALUES) == 12
    pats = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    g = pats.view(dtype)
    gb = pats.numpy().view(np.uint16)
    a_spec = G.as_tensor(U.act(gb, code, U.GELU_TANH), dtype)
    a_torch = torch.nn.functional.gelu(g, approximate="tanh")
    nan_t, nan_s = torch.isnan(a_torch.float()), torch.isnan(a_spec.float())
    same = ((a_spec.view(torch.int16) == a_torch.view(torch.int16)) & ~nan_t & ~nan_s) | (nan_t & nan_s)          # (-Inf: U2 stores -0, torch a NaN)
    n_diff = int((~same).sum())
    print(f"{dtype}: the stored U2 value differs from torch's stored gelu on {n_diff} patterns")
    assert n_diff == {0: 151, 1: 275}[code]                 # a documented property of U2 (its -Inf and tail rules among them), not of this change
    for uv in U_VALUES:
        u = torch.full_like(g, uv)
        h = G.as_tensor(G.gelu_mul(gb, G.to_bits(u), code), dtype)
        want = a_torch * u
        nan = torch.isnan(want.float())
        assert torch.equal(torch.isnan(h.float())[same], nan[same]), (dtype, uv)
        ok = same & ~nan
        assert torch.equal(h.view(torch.int16)[ok], want.view(torch.int16)[ok]), (dtype, uv)
        # and on every pattern, GG2 is the product of the stored U2 value
        mine = (a_spec.float() * u.float()).to(dtype)
        nan2 = torch.isnan(mine.float())
        assert torch.equal(torch.isnan(h.float()), nan2) and torch.equal(h.view(torch.int16)[~nan2], mine.view(torch.int16)[~nan2]), (dtype, uv)


# ---------------------------------------------------------------------------------------------------------------- the C-ABI
def test_symbols_declared_exported_and_bound():
    from protoquant_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pq_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for sym, args in SYMS.items():
        m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % sym, hdr)
        assert m, f"pq_hip.h does not declare {sym}"
        assert [re.split(r"[\s*]+", a.strip())[-1] for a in m.group(1).split(",")] == args
        assert hasattr(L, sym) and sym in _lib.EXPORTS and len(getattr(L, sym).argtypes) == len(args)
    # the argument lists of the entry points they are modelled on
    for new, old in (("pq_gemma_rmsnorm_quant_rowwise", "pq_rmsnorm_quant_rowwise"), ("pq_add_gemma_rmsnorm_quant_rowwise", "pq_add_rmsnorm_quant_rowwise")):
        mo = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % old, hdr)
        assert [re.split(r"[\s*]+", a.strip())[-1] for a in mo.group(1).split(",")] == SYMS[new]
    assert L.pq_version() == 1                                          # additions: the ABI version stays
    import protoquant_amd as pq
    for name in ("gemma_rmsnorm_quantize", "add_gemma_rmsnorm_quantize", "gelu_mul_quantize", "GemmaRMSNormQuant", "fuse_gemma_layers", "is_gemma_rmsnorm"):
        assert name in pq.__all__ and callable(getattr(pq, name)), name


ROW = 128 * 2          # bytes of one bf16 row


def _norm(L, **kw):
    a = dict(x=0x10000, ldx=128, w=0x40000, eps=1e-6, dtype=0, rows=4, cols=128, q=0x50000, ldq=128, scale=0x60000, h=None, ldh=0)
    a.update(kw)
    return L.pq_gemma_rmsnorm_quant_rowwise(a["x"], a["ldx"], a["w"], a["eps"], a["dtype"], a["rows"], a["cols"], a["q"], a["ldq"], a["scale"], a["h"], a["ldh"], None)


def _addnorm(L, **kw):
    a = dict(x=0x10000, ldx=128, r=0x20000, ldr=128, s=0x30000, lds=128, w=0x40000, eps=1e-6, dtype=0, rows=4, cols=128, q=0x50000, ldq=128, scale=0x60000, h=None, ldh=0)
    a.update(kw)
    return L.pq_add_gemma_rmsnorm_quant_rowwise(a["x"], a["ldx"], a["r"], a["ldr"], a["s"], a["lds"], a["w"], a["eps"], a["dtype"], a["rows"], a["cols"], a["q"], a["ldq"],
                                                a["scale"], a["h"], a["ldh"], None)


def _geglu(L, **kw):
    a = dict(g=0x10000, ldg=128, u=0x20000, ldu=128, dtype=0, rows=4, cols=128, kind=1, q=0x50000, ldq=128, scale=0x60000, h=None, ldh=0)
    a.update(kw)
    return L.pq_gelu_mul_quant_rowwise(a["g"], a["ldg"], a["u"], a["ldu"], a["dtype"], a["rows"], a["cols"], a["kind"], a["q"], a["ldq"], a["scale"], a["h"], a["ldh"], None)


COMMON_BAD = [(dict(q=None), b"q is null"), (dict(scale=None), b"scale is null"), (dict(dtype=3), b"dtype"), (dict(dtype=-1), b"dtype"), (dict(rows=-1), b"rows"),
              (dict(cols=-1), b"cols"), (dict(ldq=64), b"ld_q"), (dict(h=0x70000, ldh=64), b"ld_h"), (dict(scale=0x50000 + 128), b"q overlaps scale"),
              (dict(h=0x50000 + 256, ldh=128), b"q overlaps h_out"), (dict(h=0x60000 - 64, ldh=128), b"scale overlaps h_out")]
NORM_BAD = [(dict(x=None), b"x is null"), (dict(w=None), b"weight is null"), (dict(ldx=64), b"ld_x"), (dict(eps=float("nan")), b"eps"), (dict(eps=float("inf")), b"eps"),
            (dict(eps=-1e-6), b"eps"), (dict(q=0x10000), b"q overlaps x"), (dict(q=0x40000 + 8), b"q overlaps weight"), (dict(scale=0x10000 + 4), b"scale overlaps x"),
            (dict(h=0x10000, ldh=128), b"h_out overlaps x"), (dict(h=0x40000, ldh=128), b"h_out overlaps weight")]
ADD_BAD = [(dict(s=None), b"sum_out is null"), (dict(r=None), b"residual is null"), (dict(ldr=64), b"ld_r"), (dict(lds=64), b"ld_s"),
           (dict(cols=1 << 24, ldx=1 << 24, ldr=1 << 24, lds=1 << 24, ldq=1 << 24), b"cols"),
           (dict(s=0x10000 + 16), b"sum_out overlaps x"), (dict(s=0x10000 + ROW), b"sum_out overlaps x"), (dict(s=0x10000 - ROW), b"sum_out overlaps x"),
           (dict(s=0x10000, lds=256, ldx=128), b"sum_out overlaps x"), (dict(s=0x20000 + 2 * ROW), b"sum_out overlaps residual"), (dict(s=0x40000), b"sum_out overlaps weight"),
           (dict(q=0x20000 + 100), b"q overlaps residual"), (dict(q=0x30000 + 64), b"q overlaps sum_out"), (dict(scale=0x30000), b"scale overlaps sum_out"),
           (dict(h=0x20000 + ROW, ldh=128), b"h_out overlaps residual"), (dict(h=0x30000, ldh=128), b"h_out overlaps sum_out")]
GEGLU_BAD = [(dict(g=None), b"g is null"), (dict(u=None), b"u is null"), (dict(ldg=64), b"ld_g"), (dict(ldu=64), b"ld_u"), (dict(kind=0), b"kind"), (dict(kind=2), b"kind"),
             (dict(kind=-1), b"kind"), (dict(kind=3), b"kind"), (dict(q=0x10000), b"q overlaps g"), (dict(q=0x20000 + 100), b"q overlaps u"),
             (dict(scale=0x20000 + 4), b"scale overlaps u"), (dict(h=0x10000, ldh=128), b"h_out overlaps g"), (dict(h=0x20000 + ROW, ldh=128), b"h_out overlaps u")]
CASES = ([("pq_gemma_rmsnorm_quant_rowwise", _norm, kw, named) for kw, named in COMMON_BAD + NORM_BAD + [(dict(cols=1 << 24, ldx=1 << 24, ldq=1 << 24), b"cols")]]
         + [("pq_add_gemma_rmsnorm_quant_rowwise", _addnorm, kw, named) for kw, named in COMMON_BAD + NORM_BAD + ADD_BAD]
         + [("pq_gelu_mul_quant_rowwise", _geglu, kw, named) for kw, named in COMMON_BAD + GEGLU_BAD])


@pytest.mark.parametrize("sym,call,kw,named", CASES, ids=[f"{c[0][3:-14]}-{i}" for i, c in enumerate(CASES)])
def test_bad_arguments_are_named_without_a_gpu(sym, call, kw, named):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert call(L, **kw) == 1, kw
    err = L.pq_last_error()
    assert sym.encode() in err and named in err, (kw, err)


def test_empty_problems_are_no_ops_without_a_gpu():
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _norm(L, rows=0) == 0 and _norm(L, cols=0, ldx=0, ldq=0) == 0 and _norm(L, rows=0, x=None, w=None, q=None, scale=None) == 0
    assert _addnorm(L, rows=0) == 0 and _addnorm(L, cols=0, ldx=0, ldr=0, lds=0, ldq=0) == 0
    assert _addnorm(L, rows=0, x=None, r=None, s=None, w=None, q=None, scale=None) == 0
    assert _geglu(L, rows=0) == 0 and _geglu(L, cols=0, ldg=0, ldu=0, ldq=0) == 0 and _geglu(L, rows=0, g=None, u=None, q=None, scale=None) == 0
    assert _geglu(L, rows=0, kind=0) == 1                               # the kind is checked before the shape


def test_python_entries_have_no_cpu_fallback_and_check_their_operands():
    import protoquant_amd as pq
    from protoquant_amd import _lib, qtensor
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    w = torch.ones(64, dtype=torch.bfloat16)
    for call in (lambda: pq.gemma_rmsnorm_quantize(x, w), lambda: pq.add_gemma_rmsnorm_quantize(x, x.clone(), w), lambda: pq.gelu_mul_quantize(x, x.clone()),
                 lambda: pq.GemmaRMSNormQuant(w, 1e-6)(x), lambda: pq.GemmaRMSNormQuant(w, 1e-6)(x, residual=x.clone())):
        with pytest.raises(_lib.PQError):
            call()
    for new, old in ((pq.gemma_rmsnorm_quantize, pq.rmsnorm_quantize), (pq.add_gemma_rmsnorm_quantize, pq.add_rmsnorm_quantize)):
        assert str(inspect.signature(new)) == str(inspect.signature(old))
    sig = inspect.signature(pq.gelu_mul_quantize)
    assert list(sig.parameters) == ["g", "u", "kind", "return_h"] and sig.parameters["kind"].default == "gelu_tanh" and sig.parameters["return_h"].default is False
    assert list(inspect.signature(pq.GemmaRMSNormQuant.forward).parameters) == ["self", "x", "residual"]
    assert inspect.signature(pq.GatedMLP.__init__).parameters["act"].default == "silu"
    orig = _lib.require_gpu
    _lib.require_gpu = lambda t, name: None
    try:
        for call in (lambda: pq.gemma_rmsnorm_quantize(x, torch.ones(32, dtype=torch.bfloat16)), lambda: pq.gemma_rmsnorm_quantize(x, w.float()),
                     lambda: pq.add_gemma_rmsnorm_quantize(x, torch.zeros(4, 32, dtype=torch.bfloat16), w), lambda: pq.add_gemma_rmsnorm_quantize(x, x.clone().half(), w),
                     lambda: pq.add_gemma_rmsnorm_quantize(x, x.clone(), w, out=torch.zeros(4, 32, dtype=torch.bfloat16)),
                     lambda: pq.add_gemma_rmsnorm_quantize(x, x.clone(), w, out=torch.zeros(64, 4, dtype=torch.bfloat16).t()),
                     lambda: pq.gelu_mul_quantize(x, torch.zeros(4, 32, dtype=torch.bfloat16)), lambda: pq.gelu_mul_quantize(x, x.clone().half()),
                     lambda: pq.gelu_mul_quantize(x, x.clone(), kind="gelu_erf"), lambda: pq.gelu_mul_quantize(x, x.clone(), kind="silu")):
            with pytest.raises(ValueError):
                call()
    finally:
        _lib.require_gpu = orig
    assert qtensor.L.require_gpu is orig


# ---------------------------------------------------------------------------------------------------------------- the code objects
def _kernels_of(objname):
    return kernels_of(objname, must_be_built=True)


def _no_scratch_no_spills(kernels):
    for n, v in kernels.items():
        assert v.get("private_segment_fixed_size", 1) == 0 and v.get("vgpr_spill_count", 1) == 0 and v.get("sgpr_spill_count", 1) == 0, (n, v)
        assert v["vgpr_count"] <= 512, (n, v)


@pytest.mark.parametrize("obj,add", [("gemma_norm_kernels", 0), ("add_gemma_norm_kernels", 1)])
def test_norm_objects_hold_every_layout_without_scratch(obj, add):
    k = _kernels_of(obj)
    for dt in range(3):
        for wh in "01":
            for v in (1, 2, 4, 8):          # one wave per row: 1, 2, 4, 8 vectors per lane
                assert len([n for n in k if re.search(r"\d+rmsnorm_quant_rowsILi%dELi%dELi64ELb%sELb%dENS_9GemmaGainELb1EJEEE" % (dt, v, wh, add), n)]) == 1, (dt, v, wh)
            for v in (1, 2, 4, 8, 16):      # 256 threads per row: 1 .. 16 vectors per thread
                assert len([n for n in k if re.search(r"\d+rmsnorm_quant_rowsILi%dELi%dELi256ELb%sELb%dENS_9GemmaGainELb1EJEEE" % (dt, v, wh, add), n)]) == 1, (dt, v, wh)
        assert len([n for n in k if re.search(r"\d+rmsnorm_quant_genericILi%dELb%dENS_9GemmaGainELb1EJEEE" % (dt, add), n)]) == 1, dt
    assert len(k) == 3 * (8 + 10 + 1)
    _no_scratch_no_spills(k)


def test_geglu_object_holds_every_layout_without_scratch():
    k = _kernels_of("geglu_kernels")
    for dt in range(3):
        for wh in "01":
            for v, tpr in ((1, 64), (2, 64), (4, 64), (3, 512), (1, 256), (2, 256), (4, 256), (8, 256), (16, 256)):
                assert len([n for n in k if re.search(r"\d+rowmap_quant_rowsINS_7GegluOpELi%dELi%dELi%dELb%sELi0EEE" % (dt, v, tpr, wh), n)]) == 1, (dt, v, tpr, wh)
        assert len([n for n in k if re.search(r"\d+rowmap_quant_genericINS_7GegluOpELi%dELi0EEE" % dt, n)]) == 1, dt
    assert len(k) == 3 * (2 * 9 + 1)
    _no_scratch_no_spills(k)


def test_k1s_object_holds_exactly_the_layouts_of_the_dispatchers_ladder():
    """K1s and its split halves (producer_kernels.o): per dtype, MODE 0 with and without h_out, MODE 1 and MODE 2 of silu * u, and the two identity modes, each at the
    (threads per row, vectors per thread) pairs of rowmap_dispatch's ladder and no others; the identity never takes 512 threads per row.  The ladder's (256, 1) is
    instantiated but no width reaches it (rows of up to 256 vectors take a wave): it is held here as it is in the counts of K1g, K1gg and K1u."""
    k = {n: v for n, v in _kernels_of("producer_kernels").items() if "rowmap_quant_" in n}
    ladder = ((64, 1), (64, 2), (64, 4), (512, 3), (256, 1), (256, 2), (256, 4), (256, 8), (256, 16))
    forms = (("9SiluMulOp", 0, "01"), ("9SiluMulOp", 1, "0"), ("9SiluMulOp", 2, "0"), ("7IdentOp", 1, "0"), ("7IdentOp", 2, "0"))
    want = set()
    for dt in range(3):
        for op, mode, whs in forms:
            for wh in whs:
                for tpr, v in ladder:
                    if not (op == "7IdentOp" and tpr == 512):
                        want.add("rowsINS_%sELi%dELi%dELi%dELb%sELi%dEEE" % (op, dt, v, tpr, wh, mode))
            want.add("genericINS_%sELi%dELi%dEEE" % (op, dt, mode))
    got = {re.search(r"rowmap_quant_(\w+?EEE)v", n).group(1) for n in k}
    assert got == want, (sorted(got - want), sorted(want - got))
    assert len(k) == len(want) == 3 * (4 * 9 + 2 * 8 + 5)
    _no_scratch_no_spills(k)


@pytest.mark.parametrize("obj,count", [("producer_kernels", None), ("addnorm_kernels", 57), ("act_kernels", None), ("glu_kernels", None)])
def test_the_existing_objects_hold_no_kernel_of_the_new_family(obj, count):
    k = _kernels_of(obj)
    assert k and not [n for n in k if re.search(r"GemmaGain|gelu_mul_quant|GegluOp", n)], obj
    if count is not None:
        assert len(k) == count
