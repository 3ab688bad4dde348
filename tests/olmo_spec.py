"""TEST INFRASTRUCTURE — numpy / torch-on-CPU restatement of the OLMo-2 / OLMo-3 forms of QSPEC (NO1-NO5, PO1, A1, Q1-Q6), built on oracle.qspec_numpy
(rms_sumsq, to_f32, from_f32, quantize) and tests/addnorm_spec.add_a1 (A1) and on nothing else:

    NO1-NO4 = N1-N4    the pinned sum of squares, var = ss / cols, rs = 1 / sqrt(var + eps): IEEE division and square root
    NO5                h = cast_rne((f32(x) * rs) * f32(w)): binary32 throughout, ONE storage rounding, gain w (Llama's N5 rounds x * rs first; Gemma's NG5 has 1 + w)
    PO1                p = NO1-NO5 on the sublayer output with post_weight / post_eps; rounded to the storage dtype, never stored
    A1                 s = cast_rne(f32(r) + f32(p)), the new residual stream, stored
    Q1-Q6              on the rows of s as stored

`unrounded_sum` is NOT the specification: it is what a kernel that skips the storage rounding of p would store, kept here so that a test can show that its case
tells the two apart.  Half types travel as uint16 bit patterns with a dtype code (0 bf16, 1 fp16, 2 f32), as in oracle.qspec_numpy."""
import numpy as np
import torch

from oracle import qspec_numpy as Q
from tests.addnorm_spec import TD, add_a1, to_bits

CODE = {v: k for k, v in TD.items()}


def _rs(xf: np.ndarray, eps: float, d) -> np.ndarray:
    """NO1-NO4 on binary32 rows"""
    ss = Q.rms_sumsq(xf, 4 if d == Q.DT_F32 else 8)
    var = (ss / np.float32(xf.shape[1])).astype(np.float32)
    return (np.float32(1) / np.sqrt((var + np.float32(eps)).astype(np.float32)).astype(np.float32)).astype(np.float32)


def unrounded_h(x: np.ndarray, w: np.ndarray, eps: float, dtype) -> np.ndarray:
    """(f32(x) * rs) * f32(w) in binary32, BEFORE the storage rounding, for x [rows, cols] and w [cols] given as storage bits"""
    d = Q.dt(dtype)
    xf, wf = Q.to_f32(x, d), Q.to_f32(w, d)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        xn = (xf * _rs(xf, eps, d)[:, None]).astype(np.float32)
        return (xn * wf[None, :]).astype(np.float32)


def olmo_h(x: np.ndarray, w: np.ndarray, eps: float, dtype) -> np.ndarray:
    """NO1-NO5 on storage bits: the normalised activation in the storage dtype"""
    return Q.from_f32(unrounded_h(x, w, eps, dtype), Q.dt(dtype))


def as_tensor(b: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    """storage bits -> a CPU tensor of `dtype`"""
    t = torch.from_numpy(np.ascontiguousarray(b))
    return t if dtype == torch.float32 else t.view(torch.int16).view(dtype)


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    """NO1-NO5 for 2-D x and 1-D w (any device; computed on the CPU): a CPU tensor of x's dtype — what K1on stores, and PO1's p"""
    return as_tensor(olmo_h(to_bits(x), to_bits(w), float(eps), CODE[x.dtype]), x.dtype).reshape(x.shape)


def postnorm_add(x: torch.Tensor, post_weight: torch.Tensor, r: torch.Tensor, post_eps: float) -> torch.Tensor:
    """PO1 + A1: the stored sum as a CPU tensor (what K1oa stores, and K1oq's `summed`)"""
    return add_a1(rmsnorm(x, post_weight, post_eps), r)


def postnorm_add_quantize(x: torch.Tensor, post_weight: torch.Tensor, r: torch.Tensor, post_eps: float):
    """(q int8, scale f32, s bits) of PO1 + A1 + Q1-Q6 for 2-D x, r and 1-D post_weight"""
    s = to_bits(postnorm_add(x, post_weight, r, post_eps))
    q, sc = Q.quantize(s, Q.dt(CODE[x.dtype]), 1)
    return q, sc, s


def unrounded_p(x: torch.Tensor, post_weight: torch.Tensor, post_eps: float) -> np.ndarray:
    return unrounded_h(to_bits(x), to_bits(post_weight), float(post_eps), CODE[x.dtype])


def unrounded_sum(x: torch.Tensor, post_weight: torch.Tensor, r: torch.Tensor, post_eps: float) -> torch.Tensor:
    """cast_rne(f32(r) + p_unrounded): what a kernel that skips the rounding of p would store (NOT the specification)"""
    p = torch.from_numpy(unrounded_p(x, post_weight, post_eps))
    return (r.detach().cpu().float() + p).to(x.dtype)


# the three formulas in torch, as the recognisers evaluate them (eager order of the sum: close to NO, not bit-equal in general)
def olmo_formula(x, w, eps):
    xf = x.float()
    return (w * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps))).to(x.dtype)


def llama_formula(x, w, eps):
    xf = x.float()
    return w * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).to(x.dtype)


def gemma_formula(x, w, eps):
    xf = x.float()
    return ((xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)) * (1.0 + w.float())).type_as(x)
