"""TEST INFRASTRUCTURE — numpy / torch-on-CPU restatement of the sandwich residual flow (QSPEC PN1, A1, NG1-NG6, Q1-Q6), composed from
tests/gemma_spec.gemma_h (NG1-NG5), tests/addnorm_spec.add_a1 (A1) and tests/gemma_spec.gemma_rmsnorm_quantize (NG1-NG6, Q1-Q6) and from nothing else:

    PN1  p = cast_rne((f32(x) * rs_p) * (1.0f + f32(post_weight)))     NG1-NG5 on x; ROUNDED to the storage dtype
    A1   s = cast_rne(f32(r) + f32(p))                                 the new residual stream, stored
    then NG1-NG6 and Q1-Q6 on the rows of s as stored, with weight / eps

`unrounded_sum` is NOT the specification: it is what a kernel that skips the storage rounding of p would store, kept here so that a test can show that its case
tells the two apart."""
import numpy as np
import torch

from oracle import qspec_numpy as Q
from tests import gemma_spec as G
from tests.addnorm_spec import add_a1, to_bits


def postnorm(x: torch.Tensor, post_weight: torch.Tensor, post_eps: float) -> torch.Tensor:
    """PN1 for 2-D x and 1-D post_weight (any device; computed on the CPU): p as a CPU tensor of x's dtype"""
    p = G.gemma_h(to_bits(x), to_bits(post_weight), float(post_eps), G.CODE[x.dtype])
    return G.as_tensor(p, x.dtype).reshape(x.shape)


def postnorm_add(x: torch.Tensor, post_weight: torch.Tensor, r: torch.Tensor, post_eps: float) -> torch.Tensor:
    """PN1 + A1: the stored sum as a CPU tensor (what K1pa stores, and K1pang's `summed`)"""
    return add_a1(postnorm(x, post_weight, post_eps), r)


def postnorm_add_rmsnorm_quantize(x: torch.Tensor, post_weight: torch.Tensor, r: torch.Tensor, w: torch.Tensor, eps: float, post_eps: float):
    """(q int8, scale f32, s bits, h bits) of PN1 + A1 + NG1-NG6 for 2-D x, r and 1-D post_weight, w"""
    s = postnorm_add(x, post_weight, r, post_eps)
    q, sc, h = G.gemma_rmsnorm_quantize(to_bits(s), to_bits(w), float(eps), G.CODE[x.dtype])
    return q, sc, to_bits(s), h


def unrounded_p(x: torch.Tensor, post_weight: torch.Tensor, post_eps: float) -> np.ndarray:
    """(f32(x) * rs_p) * (1 + f32(post_weight)) in binary32 BEFORE its storage rounding, with rs_p from the pinned sum of x's own dtype"""
    d = Q.dt(G.CODE[x.dtype])
    xf, wf = Q.to_f32(to_bits(x), d), Q.to_f32(to_bits(post_weight), d)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        ss = Q.rms_sumsq(xf, 4 if d == Q.DT_F32 else 8)
        var = (ss / np.float32(xf.shape[1])).astype(np.float32)
        rs = (np.float32(1) / np.sqrt((var + np.float32(post_eps)).astype(np.float32)).astype(np.float32)).astype(np.float32)
        return ((xf * rs[:, None]).astype(np.float32) * (np.float32(1) + wf).astype(np.float32)[None, :]).astype(np.float32)


def unrounded_sum(x: torch.Tensor, post_weight: torch.Tensor, r: torch.Tensor, post_eps: float) -> torch.Tensor:
    """cast_rne(f32(r) + p_unrounded): what a kernel that skips the rounding of p would store (NOT the specification)"""
    p = torch.from_numpy(unrounded_p(x, post_weight, post_eps))
    return (r.detach().cpu().float() + p).to(x.dtype)
