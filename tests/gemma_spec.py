"""TEST INFRASTRUCTURE — numpy restatement of the Gemma forms of QSPEC, built on oracle.qspec_numpy (rms_sumsq, to_f32, from_f32, quantize), on
tests/addnorm_spec.add_a1 (A1) and on tests/act_spec.act (U2):

    gemma_rmsnorm_quantize      NG1-NG4 = N1-N4;  NG5 g = 1.0f + f32(w), h = cast_rne((f32(x) * rs) * g): binary32 throughout, ONE storage rounding;  NG6 Q1-Q6
    add_gemma_rmsnorm_quantize  A1 (the sum, stored), then NG1-NG6 on the rows of the sum as stored
    gelu_mul_quantize           GG1 a = cast_rne(gelu_tanh_U2(f32(g)));  GG2 h = cast_rne(f32(a) * f32(u));  GG3 Q1-Q6

Half types travel as uint16 bit patterns with a dtype code (0 bf16, 1 fp16, 2 f32), as in oracle.qspec_numpy."""
import numpy as np
import torch

from oracle import qspec_numpy as Q
from tests import act_spec as U
from tests.addnorm_spec import TD, add_a1, to_bits
from tests.gpu_util import bits

CODE = {v: k for k, v in TD.items()}


def gemma_h(x: np.ndarray, w: np.ndarray, eps: float, dtype) -> np.ndarray:
    """NG1-NG5: the normalised activation in the storage dtype, for x [rows, cols] and w [cols] given as storage bits"""
    d = Q.dt(dtype)
    xf, wf = Q.to_f32(x, d), Q.to_f32(w, d)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        ss = Q.rms_sumsq(xf, 4 if d == Q.DT_F32 else 8)                                                                        # NG1-NG3
        var = (ss / np.float32(xf.shape[1])).astype(np.float32)
        rs = (np.float32(1) / np.sqrt((var + np.float32(eps)).astype(np.float32)).astype(np.float32)).astype(np.float32)      # NG4
        g = (np.float32(1) + wf).astype(np.float32)                                                                            # NG5
        xn = (xf * rs[:, None]).astype(np.float32)
        return Q.from_f32((xn * g[None, :]).astype(np.float32), d)


def gemma_rmsnorm_quantize(x: np.ndarray, w: np.ndarray, eps: float, dtype):
    """QSPEC NG1-NG6 on storage bits.  Returns (q int8, scale f32, h stored dtype)."""
    h = gemma_h(x, w, eps, dtype)
    q, s = Q.quantize(h, Q.dt(dtype), 1)
    return q, s, h


def gemma_rmsnorm_quantize_t(x: torch.Tensor, w: torch.Tensor, eps: float):
    """the same for 2-D x and 1-D w tensors (any device; computed on the CPU)"""
    return gemma_rmsnorm_quantize(to_bits(x), to_bits(w), float(eps), CODE[x.dtype])


def add_gemma_rmsnorm_quantize(x: torch.Tensor, r: torch.Tensor, w: torch.Tensor, eps: float):
    """(q, scale, s bits, h bits) of A1 + NG1-NG6 for 2-D x, r and 1-D w tensors"""
    s = add_a1(x, r)
    q, sc, h = gemma_rmsnorm_quantize(to_bits(s), to_bits(w), float(eps), CODE[x.dtype])
    return q, sc, to_bits(s), h


def gelu_mul(g: np.ndarray, u: np.ndarray, dtype) -> np.ndarray:
    """GG1-GG2 on storage bits: h in the storage dtype"""
    d = Q.dt(dtype)
    a = U.act(g, d, U.GELU_TANH)                                                  # GG1: U2 and its storage rounding
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return Q.from_f32((Q.to_f32(a, d) * Q.to_f32(u, d)).astype(np.float32), d)          # GG2


def gelu_mul_quantize(g: np.ndarray, u: np.ndarray, dtype):
    """QSPEC GG1-GG3 on storage bits.  Returns (q int8, scale f32, h stored dtype)."""
    h = gelu_mul(g, u, dtype)
    q, s = Q.quantize(h, Q.dt(dtype), 1)
    return q, s, h


def gelu_mul_quantize_t(g: torch.Tensor, u: torch.Tensor):
    return gelu_mul_quantize(to_bits(g), to_bits(u), CODE[g.dtype])


def as_tensor(b: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    """storage bits -> a CPU tensor of `dtype`"""
    t = torch.from_numpy(np.ascontiguousarray(b))
    return t if dtype == torch.float32 else t.view(torch.int16).view(dtype)


def ulp_distance(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """distance in units of the last place between two 16-bit tensors of one dtype (finite values): the difference of their sign-magnitude bit patterns mapped to a
    monotone integer line"""
    def line(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (line(a) - line(b)).abs()


def nan_class_equal(got: torch.Tensor, want, what):
    """a float tensor against storage bits (or a tensor): NaN positions equal, every other element bit for bit"""
    want_t = want if isinstance(want, torch.Tensor) else as_tensor(np.asarray(want), got.dtype).reshape(got.shape)
    g, w = bits(got), bits(want_t)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    gn, wn = torch.isnan(got.detach().float().cpu()).numpy(), torch.isnan(want_t.detach().float().cpu()).numpy()
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ"
    bad = (g != w) & ~wn
    assert not bad.any(), f"{what}: {int(bad.sum())} of {g.size} elements differ (first at {np.argwhere(bad)[:3].tolist()})"
