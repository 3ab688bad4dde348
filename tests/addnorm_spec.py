"""TEST INFRASTRUCTURE — the test-side statement of QSPEC A1 composed with the existing oracle's N1-N6 / Q1-Q6: the residual add fused into RMSNorm +
per-token quantisation.  A1 is torch on the CPU — one binary32 add and one storage rounding per element, (x.float() + r.float()).to(dtype) — and the rows of the sum AS
STORED go through oracle.c_oracle.rmsnorm_quant_rowwise.  Half types travel as uint16 bit patterns with a dtype code, as in oracle.qspec_numpy."""
import numpy as np
import torch

from oracle import c_oracle as C

TD = {0: torch.bfloat16, 1: torch.float16, 2: torch.float32}


def to_bits(t: torch.Tensor) -> np.ndarray:
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.float32:
        return t.numpy().copy()
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def add_a1(x: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """A1 on CPU tensors of the storage dtype: s = cast_rne(f32(r) + f32(x))"""
    x, r = x.detach().cpu(), r.detach().cpu()
    assert x.dtype == r.dtype and x.shape == r.shape
    return (r.float() + x.float()).to(x.dtype)


def add_rmsnorm_quantize(x: torch.Tensor, r: torch.Tensor, w: torch.Tensor, eps: float):
    """(q int8 [rows, cols], scale f32 [rows], s bits, h bits) of the specification for 2-D x, r and 1-D w (any device; computed on the CPU)"""
    code = {v: k for k, v in TD.items()}[x.dtype]
    s = add_a1(x, r)
    q, sc, h, _ = C.rmsnorm_quant_rowwise(to_bits(s), to_bits(w), float(eps), code)
    return q, sc, to_bits(s), h
