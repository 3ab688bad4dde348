"""TEST INFRASTRUCTURE — the test-side statement of the parallel residual fused into LayerNorm + per-token quantisation (K1pl / K1l2): QSPEC A2 is
tests.addnorm_spec.add_a1 applied twice, in the association (a + b) + c, and the rows of the sum AS STORED go through tests.lnorm_spec.layernorm_quantize once per
norm group (L1-L6, Q1-Q6).  No arithmetic of its own.  Half types travel as uint16 bit patterns, as in oracle.qspec_numpy.  Also the seeded inputs that the GPU test
and the host test (which shows that the three associations differ on them) share."""
import torch

from tests import lnorm_spec as LS
from tests.addnorm_spec import add_a1, to_bits

CODE = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}


def add_a2(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """A2 on CPU tensors of the storage dtype: t = cast_rne(f32(a) + f32(b)); s = cast_rne(f32(t) + f32(c))"""
    return add_a1(add_a1(a, b), c)


def layernorm_quantize_groups(s: torch.Tensor, groups):
    """[(q int8 [rows, cols], scale f32 [rows], h bits)] — one entry per group (w, b or None, eps) — for the 2-D stored sum s"""
    return [LS.layernorm_quantize(to_bits(s), to_bits(w), None if b is None else to_bits(b), float(eps), CODE[s.dtype]) for w, b, eps in groups]


def add2_layernorm_quantize(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, groups):
    """(s bits, [(q, scale, h bits) per group]) of the specification for 2-D a, b, c (any device; computed on the CPU)"""
    s = add_a2(a, b, c)
    return to_bits(s), layernorm_quantize_groups(s, groups)


def inputs(rows: int, cols: int, dtype, seed: int):
    """(a, b, c, w1, b1, w2, b2): CPU tensors of `dtype`; the addends have different magnitudes, as a residual stream and two branch outputs do"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(rows, cols, generator=g).to(dtype)
    b = (torch.randn(rows, cols, generator=g) * 3.0).to(dtype)
    c = (torch.randn(rows, cols, generator=g) * 0.5).to(dtype)
    w1 = (1.0 + 0.25 * torch.randn(cols, generator=g)).to(dtype)
    b1 = (0.25 * torch.randn(cols, generator=g)).to(dtype)
    w2 = (1.0 + 0.25 * torch.randn(cols, generator=g)).to(dtype)
    b2 = (0.25 * torch.randn(cols, generator=g)).to(dtype)
    return a, b, c, w1, b1, w2, b2
