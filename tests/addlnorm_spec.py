"""TEST INFRASTRUCTURE — the test-side statement of the residual add fused into LayerNorm + per-token quantisation (K1al): QSPEC A1 as
tests/addnorm_spec.py states it (torch on the CPU: one binary32 add and one storage rounding per element), and the rows of the sum AS STORED through
tests/lnorm_spec.layernorm_quantize (L1-L6, Q1-Q6).  No arithmetic of its own.  Half types travel as uint16 bit patterns, as in oracle.qspec_numpy."""
import torch

from tests import lnorm_spec as LS
from tests.addnorm_spec import add_a1, to_bits

CODE = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}


def add_layernorm_quantize(x: torch.Tensor, r: torch.Tensor, w: torch.Tensor, b, eps: float):
    """(q int8 [rows, cols], scale f32 [rows], s bits, h bits) of the specification for 2-D x, r and 1-D w, b (b may be None; any device; computed on the CPU)"""
    s = add_a1(x, r)
    q, sc, h = LS.layernorm_quantize(to_bits(s), to_bits(w), None if b is None else to_bits(b), float(eps), CODE[x.dtype])
    return q, sc, to_bits(s), h
