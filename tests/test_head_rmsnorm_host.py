"""CPU: the host side of K1hn (pq_head_rmsnorm / pq.head_rmsnorm): the symbol declared, exported and bound with its arguments in order; every bad argument refused
and named before any HIP call; the empty problems no-ops; the stride-collapsing helper of the Python entry on the real views of Qwen3 and Gemma-3 and on views that
need a copy; and, from the metadata of the built code object alone, every instantiation of the kernel without scratch or spilled registers."""
import ctypes
import os
import re

import pytest
import torch

from tests import code_objects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "pq_head_rmsnorm"
ARGS = ["x", "ld_xo", "ld_xi", "weight", "eps", "gain", "dtype", "n_outer", "n_inner", "cols", "out", "ld_oo", "ld_oi", "stream"]


def test_symbol_declared_exported_and_bound():
    from protoquant_amd import _lib
    src = open(os.path.join(ROOT, "include", "pq_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % SYM, hdr)
    assert m, f"pq_hip.h does not declare {SYM}"
    assert [re.split(r"[\s*]+", a.strip())[-1] for a in m.group(1).split(",")] == ARGS
    assert re.search(r"#define\s+PQ_GAIN_LLAMA\s+0\b", src) and re.search(r"#define\s+PQ_GAIN_GEMMA\s+1\b", src)
    L = _lib.lib()
    i32, i64, vp, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float
    assert hasattr(L, SYM) and SYM in _lib.EXPORTS
    assert list(getattr(L, SYM).argtypes) == [vp, i64, i64, vp, f32, i32, i32, i64, i64, i64, vp, i64, i64, vp] and getattr(L, SYM).restype is i32
    assert _lib.GAIN_KINDS == {"llama": 0, "gemma": 1}
    assert L.pq_version() == 1                                          # an addition: the ABI version stays
    assert not re.search(r"_rowwise$|_rowamax$|^pq_quant_", SYM)          # not a row entry: its far-addressing case lives in tests/test_gpu_head_rmsnorm.py
    assert SYM in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    import protoquant_amd as pq
    for name in ("head_rmsnorm", "HeadRMSNorm", "fuse_qk_norms", "head_norm_kind"):
        assert name in pq.__all__ and callable(getattr(pq, name)), name


HEAD = 128 * 2          # bytes of one bf16 head


def _call(L, **kw):
    """4 tokens x 8 heads of 128 bf16: x a column slice of a [4, 2048] buffer, out dense; addresses that are never dereferenced"""
    a = dict(x=0x100000, ldxo=2048, ldxi=128, w=0x400000, eps=1e-6, gain=0, dtype=0, n_outer=4, n_inner=8, cols=128, out=0x200000, ldoo=1024, ldoi=128)
    a.update(kw)
    return getattr(L, SYM)(a["x"], a["ldxo"], a["ldxi"], a["w"], a["eps"], a["gain"], a["dtype"], a["n_outer"], a["n_inner"], a["cols"], a["out"], a["ldoo"], a["ldoi"], None)


X_END = 0x100000 + (3 * 2048 + 7 * 128 + 128) * 2          # one byte past the last head of x
BAD = [
    # a null operand
    (dict(x=None), b"x is null"), (dict(w=None), b"weight is null"), (dict(out=None), b"out is null"),
    # the shape
    (dict(cols=1 << 24, ldxi=1 << 24, ldoi=1 << 24, ldxo=1 << 28, ldoo=1 << 28), b"cols"), (dict(cols=-1), b"cols"), (dict(n_outer=-1), b"n_outer"),
    (dict(n_inner=-1), b"n_inner"), (dict(n_outer=1 << 20, n_inner=1 << 11), b"n_outer * n_inner"),
    # the strides
    (dict(ldxi=127), b"ld_xi"), (dict(ldoi=127), b"ld_oi"), (dict(ldxi=0), b"ld_xi"), (dict(ldxo=-1), b"ld_xo"), (dict(ldxi=-128), b"ld_xi"), (dict(ldoo=-1), b"ld_oo"),
    (dict(ldoi=-128), b"ld_oi"), (dict(ldxo=1 << 62), b"strides"),
    # the rows of out overlap each other
    (dict(ldoo=1023), b"rows of out overlap"), (dict(ldoo=128), b"rows of out overlap"), (dict(ldoo=0), b"rows of out overlap"),
    (dict(ldoo=128, ldoi=512 - 1), b"rows of out overlap"), (dict(n_inner=1, ldoi=0, ldoo=127), b"rows of out overlap"),
    # out overlaps an input: there is no in-place form
    (dict(out=0x100000), b"out overlaps x"), (dict(out=X_END - 2), b"out overlaps x"), (dict(out=0x100000 - (3 * 1024 + 1024) * 2 + 2), b"out overlaps x"),
    (dict(out=0x100000 + 1024 * 2), b"out overlaps x"), (dict(out=0x400000), b"out overlaps weight"), (dict(out=0x400000 + HEAD - 2), b"out overlaps weight"),
    (dict(w=0x200000 + 2), b"out overlaps weight"),
    # eps: negative, NaN, infinite
    (dict(eps=-1e-6), b"eps must"), (dict(eps=float("nan")), b"eps must"), (dict(eps=float("inf")), b"eps must"),
    # gain and dtype
    (dict(gain=2), b"gain"), (dict(gain=-1), b"gain"), (dict(dtype=3), b"dtype"), (dict(dtype=-1), b"dtype"),
]


@pytest.mark.parametrize("kw,named", BAD, ids=[f"{i}-{n.decode().replace(' ', '_')}" for i, (_, n) in enumerate(BAD)])
def test_bad_arguments_are_named_before_any_hip_call(kw, named):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _call(L, **kw) == 1, kw                                      # PQ_ERR_BAD_ARG; a call that reached the launch answers 3 on a machine without a GPU
    err = L.pq_last_error()
    assert SYM.encode() in err and named in err, (kw, err)


def test_good_arguments_get_past_the_checks():
    """status 3 (the launch fails) on a machine without a GPU, never 1; on one with a GPU these addresses must not be launched"""
    from protoquant_amd import _lib
    L = _lib.lib()
    if torch.cuda.is_available():
        pytest.skip("argument-check-only test: needs a machine without a GPU (the operands are not real memory)")
    good = [dict(), dict(out=X_END), dict(out=0x100000 - 4 * 1024 * 2), dict(n_inner=1, ldxi=0, ldoi=0), dict(n_outer=1, ldxo=0, ldoo=0), dict(eps=0.0), dict(gain=1, dtype=2),
            dict(ldoo=128, ldoi=512), dict(cols=(1 << 24) - 1, ldxi=1 << 24, ldoi=1 << 24, ldxo=1 << 28, ldoo=1 << 28, out=0x7000_0000_0000)]
    for kw in good:
        st = _call(L, **kw)
        assert st == 3, (kw, st, L.pq_last_error())


def test_empty_problems_are_no_ops():
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _call(L, n_outer=0) == 0 and _call(L, n_inner=0) == 0 and _call(L, cols=0) == 0
    assert _call(L, n_outer=0, x=None, w=None, out=None) == 0 and _call(L, cols=0, x=None, w=None, out=None) == 0
    assert _call(L, n_outer=0, eps=-1.0) == 1 and _call(L, n_outer=0, dtype=7) == 1 and _call(L, cols=0, gain=5) == 1          # eps, the dtype and the gain before it


# ---------------------------------------------------------------------------------------------------------------- the stride-collapsing helper
def test_collapse_of_the_real_views():
    from protoquant_amd.qtensor import _collapse_heads, _dense_head_strides
    B, T, Hq, Hkv, D = 2, 5, 8, 2, 64
    width = (Hq + 2 * Hkv) * D
    qkv = torch.zeros(B, T, width, dtype=torch.bfloat16)
    for lo, H in ((0, Hq), (Hq * D, Hkv)):
        q = qkv[..., lo:lo + H * D].view(B, T, H, D)          # Qwen3: q_proj(x).view(B, T, H, D) on a column slice of the fused output
        assert _collapse_heads(q.shape, q.stride()) == (B * T, width, H, D)
        assert _dense_head_strides(q.shape, q.stride()) == (T * H * D, H * D, D, 1)
        qt = q.transpose(1, 2)                                 # Gemma-3
        assert _collapse_heads(qt.shape, qt.stride()) == (B * T, width, H, D)
        assert _dense_head_strides(qt.shape, qt.stride()) == (T * H * D, D, H * D, 1) == (qt.float() * 1.0).stride()
    c = torch.zeros(B, T, Hq, D)                              # a plain contiguous tensor: ONE axis
    assert _collapse_heads(c.shape, c.stride()) == (B * T * Hq, D, 1, D)
    ct = c.transpose(1, 2)
    assert _collapse_heads(ct.shape, ct.stride()) == (B * T * Hq, D, 1, D) and _dense_head_strides(ct.shape, ct.stride()) == ct.stride()
    assert _collapse_heads((D,), (1,)) == (1, D, 1, D) and _collapse_heads((1, 1, D), (7, 3, 1)) == (1, D, 1, D)
    one_token = qkv[:1, :1, :Hq * D].view(1, 1, Hq, D)         # decode: axes of one index are dropped
    assert _collapse_heads(one_token.shape, one_token.stride()) == (Hq, D, 1, D)
    two_d = qkv[0, :, :D]                                      # a [T, D] column slice
    assert _collapse_heads(two_d.shape, two_d.stride()) == (T, width, 1, D)


def test_views_that_need_a_copy():
    from protoquant_amd.qtensor import _collapse_heads
    B, T, H, D = 2, 5, 6, 64
    big = torch.zeros(B, T, H, D)
    assert _collapse_heads(*(lambda v: (v.shape, v.stride()))(big[:, :T - 1, :H - 1])) is None          # three strided axes are left
    assert _collapse_heads(*(lambda v: (v.shape, v.stride()))(big[..., ::2])) is None                   # the last stride is not 1
    assert _collapse_heads(*(lambda v: (v.shape, v.stride()))(big[:, :, :1].expand(B, T, H, D))) is None          # an expanded axis: rows that overlap
    assert _collapse_heads(*(lambda v: (v.shape, v.stride()))(big.transpose(2, 3))) is None             # D is not the innermost axis
    v = big[:, :T - 1]                                                                                   # two axes are left: (B, T * H * D) x ((T - 1) * H, D)
    assert _collapse_heads(v.shape, v.stride()) == (B, T * H * D, (T - 1) * H, D)


def test_cpu_tensors_and_bad_weights_are_refused():
    import protoquant_amd as pq
    from protoquant_amd._lib import PQError
    x, w = torch.zeros(2, 3, 64, dtype=torch.bfloat16), torch.ones(64, dtype=torch.bfloat16)
    with pytest.raises(PQError, match="no\\s+CPU fallback"):
        pq.head_rmsnorm(x, w)
    with pytest.raises(PQError):
        pq.HeadRMSNorm(w, 1e-6, "llama")(x)
    with pytest.raises(ValueError):
        pq.HeadRMSNorm(w, 1e-6, "olmo")


# ---------------------------------------------------------------------------------------------------------------- the code object
def test_every_instantiation_without_scratch_or_spills():
    """bf16 / fp16 / f32 x LlamaGain / GemmaGain x (G in 4 .. 64, and the generic form): 36 kernels, from the notes of the code object"""
    kernels = code_objects.kernels_of("head_norm_kernels", must_be_built=True)
    vec = [k for k in kernels if "head_rmsnorm_vec" in k]
    gen = [k for k in kernels if "head_rmsnorm_generic" in k]
    assert len(vec) == 3 * 2 * 5 and len(gen) == 3 * 2 and len(kernels) == len(vec) + len(gen), sorted(kernels)
    assert not [k for k in kernels if "OlmoGain" in k or "OneRoundingGainILb0" in k], "OlmoGain is not instantiated: no decoder applies it per head"
    for name, notes in kernels.items():
        assert notes["private_segment_fixed_size"] == 0 and notes["vgpr_spill_count"] == 0 and notes["sgpr_spill_count"] == 0, (name, notes)
        assert notes["vgpr_count"] <= 64, (name, notes)          # eight waves per SIMD
