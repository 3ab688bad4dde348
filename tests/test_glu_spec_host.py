"""CPU: QSPEC G1-G6 (tests/glu_spec.py, the restatement the GPU kernel is held to) against what model code computes — transformers' GptOssExperts._apply_gate and
DeepseekV4Experts._apply_gate run by torch's eager CPU kernels: the same stored value on every 16-bit pattern of the gate and of the up projection, bf16 and fp16, at a
limit that is a value of the storage dtype and at one that is not; f32 rows within a few ulp.  And the host side of pq_glu_quant_rowwise: declared, exported, bound,
every bad argument refused and named before any HIP call, and a code object without scratch."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import qspec_numpy as Q
from tests import glu_spec as G
from tests.code_objects import kernels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = {0: torch.bfloat16, 1: torch.float16, 2: torch.float32}
GPT_OSS = pytest.importorskip("transformers.models.gpt_oss.modeling_gpt_oss").GptOssExperts
DEEPSEEK_V4 = pytest.importorskip("transformers.models.deepseek_v4.modeling_deepseek_v4").DeepseekV4Experts


class _Holder:
    """what the two _apply_gate methods read from `self`"""

    def __init__(self, limit, alpha):
        self.limit, self.alpha, self.act_fn = limit, alpha, F.silu


def torch_gate(kind, g: torch.Tensor, u: torch.Tensor, limit, alpha):
    """the model's own gate on CPU tensors g, u [rows, cols]: GPT-OSS reads gate / up from alternating columns, DeepSeek-V4 from the two halves"""
    o = _Holder(limit, alpha)
    if kind == G.ALPHA_SIGMOID:
        return GPT_OSS._apply_gate(o, torch.stack([g, u], -1).reshape(g.shape[0], -1))
    return DEEPSEEK_V4._apply_gate(o, torch.cat([g, u], -1))


def _t(bits_, code):
    return torch.from_numpy(np.ascontiguousarray(bits_).view(np.int16).copy()).view(TD[code])


def _b(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def _differing(want, got, code):
    wf, gf = Q.to_f32(want, code), Q.to_f32(got, code)
    return (want != got) & ~(np.isnan(wf) & np.isnan(gf))            # a NaN is compared as a class: QSPEC leaves payload and sign of a produced NaN open


PATTERNS = np.arange(65536, dtype=np.uint16)                         # every value, NaNs, +-Inf, +-0 and the subnormals included
FIXED = (1.0, -0.5, 3.140625, 6.96875, 7.0, 9.0, -100.0, 0.0, -0.0, float("inf"), float("-inf"), float("nan"))
CASES = [(G.ALPHA_SIGMOID, 7.0, 1.702), (G.CLAMPED_SILU, 7.0, 0.0), (G.ALPHA_SIGMOID, 7.03, 1.702), (G.CLAMPED_SILU, 7.03, 0.0), (G.CLAMPED_SILU, 10.0, 0.0)]


@pytest.mark.parametrize("code", [0, 1], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind,limit,alpha", CASES, ids=lambda v: str(v))
def test_spec_stores_what_torch_eager_stores_on_every_16_bit_pattern(code, kind, limit, alpha):
    """all 65 536 patterns of the gate x a handful of up values, and all 65 536 patterns of up x the same handful as the gate: zero differing stored values.
    limit 7.03 is no value of either dtype: torch.clamp rounds the scalar to the tensor's dtype (7.03125), and so does G1."""
    fixed = Q.from_f32(np.array(FIXED, np.float32), code)
    sweep = np.broadcast_to(PATTERNS, (len(FIXED), 65536))
    other = np.broadcast_to(fixed[:, None], (len(FIXED), 65536))
    for what, gb, ub in (("gate", sweep, other), ("up", other, sweep)):
        want = G.glu(gb, ub, code, kind, limit, alpha)
        got = _b(torch_gate(kind, _t(gb, code), _t(ub, code), limit, alpha))
        bad = _differing(want, got, code)
        assert not bad.any(), f"{G.KIND_NAMES[kind]} limit {limit}: {int(bad.sum())} stored values differ sweeping {what} (first at {np.argwhere(bad)[:3].tolist()})"


def test_limit_is_rounded_to_the_storage_dtype():
    assert float(G.limit_in_dtype(7.03, 0)) == 7.03125 and float(G.limit_in_dtype(7.03, 1)) == 7.03125
    assert float(G.limit_in_dtype(7.03, 2)) == float(np.float32(7.03))
    x = torch.tensor([10.0, -10.0], dtype=torch.bfloat16)
    assert x.clamp(min=-7.03, max=7.03).tolist() == [7.03125, -7.03125]          # torch's behaviour, which G1 adopts


F32_ULP_BOUND = 4


@pytest.mark.parametrize("kind,limit,alpha", CASES[:2], ids=lambda v: str(v))
def test_spec_f32_rows_stay_within_a_few_ulp_of_torch(kind, limit, alpha):
    """binary32 rows: torch's exp is not the specified one, so the contract is the spec and the distance to torch is measured — at most F32_ULP_BOUND ulp of h"""
    rng = np.random.default_rng(5)
    g = (rng.standard_normal((64, 1024)) * 4).astype(np.float32)
    u = (rng.standard_normal((64, 1024)) * 4).astype(np.float32)
    g[0, :8] = (0.0, -0.0, 7.0, 7.5, -20.0, 1e-30, -1e-30, 80.0)
    want = G.glu(g, u, 2, kind, limit, alpha)
    got = torch_gate(kind, torch.from_numpy(g), torch.from_numpy(u), limit, alpha).numpy()
    ulp = np.abs(want.view(np.int32).astype(np.int64) - got.view(np.int32).astype(np.int64))
    same_sign = np.signbit(want) == np.signbit(got)
    assert same_sign.all() and int(ulp.max()) <= F32_ULP_BOUND, f"max distance {int(ulp.max())} ulp"
    print(f"\n  {G.KIND_NAMES[kind]} f32: max distance to torch eager {int(ulp.max())} ulp")


def test_spec_quantises_the_rows_of_h():
    rng = np.random.default_rng(6)
    g = Q.from_f32((rng.standard_normal((5, 64)) * 5).astype(np.float32), 0)
    u = Q.from_f32((rng.standard_normal((5, 64)) * 5).astype(np.float32), 0)
    q, s, h = G.glu_quantize(g, u, 0, G.ALPHA_SIGMOID, 7.0, 1.702)
    q2, s2 = Q.quantize(h, 0, 1)
    assert np.array_equal(q, q2) and np.array_equal(s, s2) and np.abs(q).max() == 127
    f = G.glu_f64(Q.to_f32(g, 0), Q.to_f32(u, 0), G.ALPHA_SIGMOID, 7.0, 1.702)
    assert np.allclose(Q.to_f32(h, 0), f, rtol=2e-2, atol=1e-3)                       # the float64 restatement is the same function, up to bf16 roundings


# ---------------------------------------------------------------------------------------------------------------- the C entry point, without a GPU
SYMS = ("pq_glu_quant_rowwise", "pq_selftest_glu_short")


def test_symbols_declared_exported_and_bound():
    from protoquant_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pq_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, hdr), f"pq_hip.h does not declare {s}"
        assert hasattr(L, s), f"libpq_hip.so does not export {s}"
        assert s in _lib.EXPORTS
        assert getattr(L, s).argtypes, f"{s} has no ctypes signature"
    assert L.pq_version() == 1                                          # additions only
    assert _lib.GLU_KINDS == {"clamped_silu": 0, "alpha_sigmoid": 1}


def _glu(L, **kw):
    """pq_glu_quant_rowwise with plausible (never dereferenced) operands, one argument overridden"""
    a = dict(g=0x1000, ldg=256, u=0x1100, ldu=256, dtype=0, rows=4, cols=128, kind=1, limit=7.0, alpha=1.702, q=0x3000, ldq=128, scale=0x4000, h=None, ldh=0)
    a.update(kw)
    return L.pq_glu_quant_rowwise(a["g"], a["ldg"], a["u"], a["ldu"], a["dtype"], a["rows"], a["cols"], a["kind"], a["limit"], a["alpha"], a["q"], a["ldq"], a["scale"],
                                  a["h"], a["ldh"], None)


@pytest.mark.parametrize("kw,named", [
    (dict(kind=2), b"kind"), (dict(kind=-1), b"kind"), (dict(dtype=3), b"dtype"), (dict(dtype=-1), b"dtype"), (dict(limit=0.0), b"limit"), (dict(limit=-7.0), b"limit"),
    (dict(limit=float("inf")), b"limit"), (dict(limit=float("nan")), b"limit"), (dict(limit=1e-9, dtype=1), b"rounds to zero"), (dict(alpha=float("nan")), b"alpha"),
    (dict(alpha=float("inf")), b"alpha"), (dict(g=None), b"bad matrix"), (dict(u=None), b"bad matrix"), (dict(q=None), b"bad matrix"), (dict(scale=None), b"bad matrix"),
    (dict(ldg=64), b"bad matrix"), (dict(ldu=64), b"bad matrix"), (dict(ldq=64), b"bad matrix"), (dict(rows=-1), b"bad matrix"), (dict(cols=-1), b"bad matrix"),
    (dict(h=0x5000, ldh=64), b"bad matrix"),
])
def test_bad_arguments_are_named_without_a_gpu(kw, named):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _glu(L, **kw) == 1, kw
    err = L.pq_last_error()
    assert b"pq_glu_quant_rowwise" in err and named in err, (kw, err)


def test_empty_problems_are_no_ops_without_a_gpu():
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _glu(L, rows=0) == 0
    assert _glu(L, cols=0, ldg=0, ldu=0, ldq=0) == 0
    assert L.pq_selftest_glu_short(2, 0, 7.0, 0.0, 0x1000, None) == 1 and b"pq_selftest_glu_short" in L.pq_last_error()
    assert L.pq_selftest_glu_short(0, 5, 7.0, 0.0, 0x1000, None) == 1


def test_python_entry_point_has_no_cpu_fallback():
    import protoquant_amd as pq
    from protoquant_amd import _lib
    g = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(_lib.PQError):
        pq.glu_quantize(g, g, "alpha_sigmoid", 7.0, 1.702)


def test_glu_code_object_has_no_scratch_and_the_expected_kernels():
    """as `make spillcheck` reads the GEMM objects: no scratch, no VGPR / SGPR spill in any kernel of glu_kernels.o, every row layout of both kinds is there"""
    kernels, dis = kernels_of("glu_kernels", disassembly=True)
    # 3 dtypes x 2 kinds x with / without h_out x (one wave per row: 1, 2, 4 vectors | 256 threads: 1, 2, 4, 8, 16 | 512 threads: 3)
    assert len([k for k in kernels if "rowmap_quant_rowsINS_5GluOp" in k]) == 3 * 2 * 2 * 9
    assert len([k for k in kernels if "rowmap_quant_genericINS_5GluOp" in k]) == 3 * 2
    assert len([k for k in kernels if "glu_short_check" in k]) == 2 * 2
    for k, v in kernels.items():
        assert v.get("private_segment_fixed_size", 1) == 0 and v.get("vgpr_spill_count", 1) == 0 and v.get("sgpr_spill_count", 1) == 0, (k, v)
    assert "global_load_dwordx4" in dis and "v_med3_f32" in dis and "v_cmp_u_f32" in dis and "v_rcp_f32" in dis and "v_div_scale_f32" in dis
