"""TEST INFRASTRUCTURE — numpy restatement of QSPEC G1-G6: the clamped gates of GPT-OSS's and DeepSeek-V4's experts fused with the per-token
quantisation, built on oracle.qspec_numpy (exp_spec, to_f32, from_f32, quantize).  Half types travel as uint16 bit patterns with a dtype code, as there."""
import numpy as np

from oracle import qspec_numpy as Q

CLAMPED_SILU, ALPHA_SIGMOID = 0, 1
KIND_NAMES = {CLAMPED_SILU: "clamped_silu", ALPHA_SIGMOID: "alpha_sigmoid"}


def limit_in_dtype(limit: float, dtype) -> np.float32:
    """L of G1: the limit rounded to binary32, then to the storage dtype (round to nearest even) — what torch.clamp does with a Python scalar on a 16-bit tensor"""
    d = Q.dt(dtype)
    return Q.to_f32(Q.from_f32(np.array([limit], np.float32), d), d)[0]


def glu(g: np.ndarray, u: np.ndarray, dtype, kind: int, limit: float, alpha: float = 0.0) -> np.ndarray:
    """QSPEC G1-G5: h in the storage dtype"""
    d = Q.dt(dtype)
    cast = lambda t: Q.to_f32(Q.from_f32(np.asarray(t, np.float32), d), d)
    gf, uf = Q.to_f32(g, d), Q.to_f32(u, d)
    L = limit_in_dtype(limit, d)
    one = np.float32(1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        gc = np.where(gf > L, L, gf).astype(np.float32)                                   # G1 (a NaN fails both comparisons and stays; -0 stays -0)
        uc = np.where(uf > L, L, np.where(uf < -L, -L, uf)).astype(np.float32)
        if kind == CLAMPED_SILU:
            sg = cast((gc / (one + Q.exp_spec(-gc)).astype(np.float32)).astype(np.float32))                      # G2
            h = (sg * uc).astype(np.float32)                                                                      # G5
        elif kind == ALPHA_SIGMOID:
            a = cast((gc * np.float32(alpha)).astype(np.float32))                                                 # G2
            s = cast((one / (one + Q.exp_spec(-a)).astype(np.float32)).astype(np.float32))                       # G3
            glu_ = cast((gc * s).astype(np.float32))                                                              # G4
            v = cast((uc + one).astype(np.float32))
            h = (glu_ * v).astype(np.float32)                                                                     # G5
        else:
            raise ValueError(f"unknown kind {kind}")
        h = np.where(np.isnan(gf) | np.isnan(uf), np.float32(np.nan), h).astype(np.float32)                       # G1: a NaN in g or u propagates
    return Q.from_f32(h, d)


def glu_quantize(g, u, dtype, kind, limit, alpha=0.0):
    """QSPEC G6: per-token quantisation of glu(g, u).  Returns (q int8, scale f32, h stored dtype)."""
    h = glu(g, u, dtype, kind, limit, alpha)
    q, s = Q.quantize(h, Q.dt(dtype), 1)
    return q, s, h


def glu_f64(gate, up, kind: int, limit: float, alpha: float = 0.0) -> np.ndarray:
    """the same gate in float64 without any storage rounding (what a recogniser compares a module's own _apply_gate with)"""
    g, u = np.asarray(gate, np.float64), np.asarray(up, np.float64)
    gc, uc = np.minimum(g, limit), np.clip(u, -limit, limit)
    if kind == CLAMPED_SILU:
        return gc / (1 + np.exp(-gc)) * uc
    return (uc + 1) * (gc / (1 + np.exp(-alpha * gc)))
