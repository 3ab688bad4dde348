"""TEST INFRASTRUCTURE — the test-side statement of QSPEC S1 in numpy, composed with A1 (tests/addnorm_spec.py: torch on the CPU) and the existing
oracle's N1-N6 / Q1-Q6: the scaled residual add of the Granite decoders fused into RMSNorm + per-token quantisation (K1ma, K1mo).

S1:  p = round_storage(f32(x) * f32(m)) — the multiplier rounded ONCE to binary32, one binary32 product, one storage rounding (for f32 rows the binary32 product
itself); then A1 on p and the residual, then the oracle on the rows of the sum AS STORED.  oracle/qspec_oracle.c has no such form; this composition is the reference.
Half types travel as uint16 bit patterns with a dtype code, as in oracle.qspec_numpy.  MULTIPLIERS is the set every test of the form uses: Granite-3's 0.22, an exact
power of two, the identity, a negative one, one that is no binary fraction, and one under which the largest finite value of every storage dtype overflows to Inf."""
import numpy as np
import torch

from oracle import qspec_numpy as Q
from tests import addnorm_spec as A

MULTIPLIERS = (0.22, 0.0625, 1.0, -0.5, 1.0 / 3.0, 4.0)
OVERFLOWING = 4.0


def scale_s1(x_bits: np.ndarray, m: float, code: int) -> np.ndarray:
    """S1 on storage bits: the bits of p"""
    with np.errstate(over="ignore", invalid="ignore"):
        return Q.from_f32((Q.to_f32(x_bits, code) * np.float32(m)).astype(np.float32), code)


def fma_single_rounding(x: np.ndarray, m: float, r: np.ndarray) -> np.ndarray:
    """what S1 + A1 must NOT be for f32 rows: fma(x, m, r), one rounding.  Computed in float64 — the product is exact there (24 + 24 significand bits), the sum is
    rounded to 53 bits before the rounding to binary32, which can move the result only when the float64 sum lands exactly on a binary32 tie: a vanishing share of
    elements, and the tests only COUNT how often this form differs from the two-rounding chain"""
    return (x.astype(np.float64) * np.float64(np.float32(m)) + r.astype(np.float64)).astype(np.float32)


def scaled_add(x: torch.Tensor, r: torch.Tensor, m: float) -> torch.Tensor:
    """S1 then A1 on CPU tensors of the storage dtype: the sum as stored"""
    code = {v: k for k, v in A.TD.items()}[x.dtype]
    p = scale_s1(A.to_bits(x), m, code)
    pt = torch.from_numpy(p.copy()) if code == 2 else torch.from_numpy(p.view(np.int16).copy()).view(x.dtype)
    return A.add_a1(pt.reshape(x.shape), r)


def scaled_add_rmsnorm_quantize(x: torch.Tensor, r: torch.Tensor, m: float, w: torch.Tensor, eps: float):
    """(q int8 [rows, cols], scale f32 [rows], s bits, h bits) of the specification for 2-D x, r and 1-D w (any device; computed on the CPU)"""
    from oracle import c_oracle as C
    code = {v: k for k, v in A.TD.items()}[x.dtype]
    s = scaled_add(x.detach().cpu(), r.detach().cpu(), m)
    q, sc, h, _ = C.rmsnorm_quant_rowwise(A.to_bits(s), A.to_bits(w), float(eps), code)
    return q, sc, A.to_bits(s), h
