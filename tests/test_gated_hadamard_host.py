"""CPU: the host side of K1gh (pq_gated_hadamard_quant_rows / gated_hadamard_quantize / rotate_gated_mlps): the symbol is declared, exported and bound; every bad argument
is refused and named before any HIP call; empty problems are no-ops; the Python entry checks its block and has no CPU path; rotate_gated_mlps refuses a CPU model."""
import ctypes
import os

import pytest
import torch
from torch import nn

SYM = "pq_gated_hadamard_quant_rows"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _call(L, **kw):
    """the entry with plausible (never dereferenced) operands, bf16 4 x 128 in blocks of 64, some arguments overridden"""
    a = dict(g=0x10000, ldg=128, u=0x20000, ldu=128, dtype=0, rows=4, cols=128, act=0, block=64, q=0x50000, ldq=128, scale=0x60000, h=None, ldh=0)
    a.update(kw)
    return getattr(L, SYM)(a["g"], a["ldg"], a["u"], a["ldu"], a["dtype"], a["rows"], a["cols"], a["act"], a["block"], a["q"], a["ldq"], a["scale"], a["h"], a["ldh"], None)


BAD = [(dict(dtype=3), b"dtype"), (dict(act=2), b"act"), (dict(act=-1), b"act"), (dict(block=48), b"power of two"), (dict(block=1), b"power of two"),
       (dict(block=8192, cols=8192, ldg=8192, ldu=8192, ldq=8192), b"power of two"), (dict(block=256), b"does not divide"), (dict(cols=96, block=64), b"does not divide"),
       (dict(g=None), b"g is null"), (dict(u=None), b"u is null"), (dict(q=None), b"q is null"), (dict(scale=None), b"scale is null"), (dict(q=None, scale=None), b"q is null"),
       (dict(rows=-1), b"rows"), (dict(cols=-64), b"cols"), (dict(rows=1 << 31), b"rows"), (dict(ldg=64), b"ld_g"), (dict(ldu=64), b"ld_u"), (dict(ldq=64), b"ld_q"),
       (dict(h=0x70000, ldh=64), b"ld_h"), (dict(q=0x10000), b"q overlaps g"), (dict(q=0x20000 + 4 * 256 - 1), b"q overlaps u"), (dict(scale=0x20000 + 8), b"scale overlaps u"),
       (dict(h=0x10000 + 2, ldh=128), b"h_out overlaps g"), (dict(h=0x20000, ldh=128), b"h_out overlaps u"), (dict(h=0x50000 + 64, ldh=128), b"q overlaps h_out"),
       (dict(scale=0x50000 + 4), b"q overlaps scale")]


@pytest.mark.parametrize("kw,named", BAD)
def test_bad_arguments_are_named_without_a_gpu(kw, named):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _call(L, **kw) == 1, kw
    err = L.pq_last_error()
    assert SYM.encode() in err and named in err, (kw, err)
    assert _call(L, rows=0) == 0 and _call(L, cols=0, ldg=0, ldu=0, ldq=0) == 0          # empty problems are no-ops


def test_symbol_is_declared_exported_and_bound():
    from protoquant_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pq_hip.h")).read()
    assert f"int32_t {SYM}(const void* g, int64_t ld_g, const void* u, int64_t ld_u, int32_t dtype," in hdr and "#define PQ_GATE_GELU_TANH 1" in hdr
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    fn = getattr(_lib.lib(), SYM)
    assert SYM in _lib.EXPORTS and fn.restype is i32 and fn.argtypes == [vp, i64, vp, i64, i32, i64, i64, i32, i32, vp, i64, vp, vp, i64, vp]


def test_python_entries_check_their_arguments_and_have_no_cpu_path():
    import protoquant_amd as pq
    from protoquant_amd import _lib
    g, u = torch.zeros(4, 96, dtype=torch.bfloat16), torch.zeros(4, 96, dtype=torch.bfloat16)
    with pytest.raises(_lib.PQError):
        pq.gated_hadamard_quantize(g, u)
    orig = _lib.require_gpu
    _lib.require_gpu = lambda t, name: None
    try:
        for bad in (48, 64, 8, 8192):          # no power of two; does not divide 96; below 16; above 4096
            with pytest.raises(ValueError, match="block"):
                pq.gated_hadamard_quantize(g, u, "silu", bad)
        with pytest.raises(ValueError, match="block"):
            pq.gated_hadamard_quantize(torch.zeros(4, 72, dtype=torch.bfloat16), torch.zeros(4, 72, dtype=torch.bfloat16))          # the default for 72 columns is 8
        with pytest.raises(ValueError, match="act"):
            pq.gated_hadamard_quantize(g, u, "relu")
        for other in (torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(4, 96, dtype=torch.float16)):
            with pytest.raises(ValueError, match="must match"):
                pq.gated_hadamard_quantize(g, other)
    finally:
        _lib.require_gpu = orig
    assert all(n in pq.__all__ and callable(getattr(pq, n)) for n in ("gated_hadamard_quantize", "rotate_gated_mlps"))
    rot = pq.RotatedQLinear(64, 8)
    with pytest.raises(TypeError, match="QTensor"):
        rot.forward_rotated(torch.zeros(2, 64))
    with pytest.raises(TypeError, match="QTensor"):          # forward keeps refusing codes
        rot(pq.QTensor(torch.zeros(2, 64, dtype=torch.int8), torch.ones(2), 1, torch.bfloat16, torch.Size((2, 64))))


def test_rotate_gated_mlps_refuses_a_cpu_model_and_leaves_it_unchanged():
    import protoquant_amd as pq
    from protoquant_amd import _lib

    class MLP(nn.Module):
        def __init__(self, inter):
            super().__init__()
            self.gate_proj, self.up_proj, self.down_proj, self.act_fn = nn.Linear(32, inter, bias=False), nn.Linear(32, inter, bias=False), nn.Linear(inter, 32), nn.SiLU()
    model = nn.Sequential(MLP(64))
    before = list(model.modules())
    with pytest.raises(_lib.PQError, match="down_proj"):
        pq.rotate_gated_mlps(model)
    ragged = nn.Sequential(MLP(24))          # the largest power-of-two divisor is 8: no legal block, nothing is asked of the GPU
    assert pq.rotate_gated_mlps(ragged) == 0 and pq.rotate_gated_mlps(model, lambda name, mod: False) == 0
    assert all(a is b for a, b in zip(before, model.modules())) and isinstance(ragged[0].down_proj, nn.Linear)
