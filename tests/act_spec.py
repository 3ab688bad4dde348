"""TEST INFRASTRUCTURE — numpy restatement of QSPEC U1-U4: a unary activation (relu, the tanh GELU, the erf GELU) fused with the per-token
quantisation, built on oracle.qspec_numpy (exp_spec, fma32, to_f32, from_f32, quantize).  Half types travel as uint16 bit patterns with a dtype code, as there.
Every operation is binary32, round to nearest even, no contraction; `fma` is the correctly rounded fused multiply-add."""
import numpy as np

from oracle import qspec_numpy as Q

RELU, GELU_TANH, GELU_ERF = 0, 1, 2
KIND_NAMES = {RELU: "relu", GELU_TANH: "gelu_tanh", GELU_ERF: "gelu_erf"}
KIND_CODES = {v: k for k, v in KIND_NAMES.items()}

f32 = np.float32


def _b(u: int) -> np.float32:
    return np.array([u], np.uint32).view(np.float32)[0]


# U2: a = 2 u = x (K0 + K1 x^2), K0 = 2 sqrt(2 / pi), K1 = 0.044715 K0, both rounded to binary32
TANH_K0, TANH_K1 = _b(0x3FCC422A), _b(0x3D922279)
# U3: Q(t) = 0.5 erfcx(t / sqrt 2) = Phi(-t) exp(t^2 / 2) on 0 <= t <= 12 as a degree-10 polynomial in v = (t - 4) / (t + 4), constant term first
ERF_K = f32(4.0)
ERF_CUT = f32(12.0)
ERF_C = tuple(_b(u) for u in (0x3DC15A5E, 0xBE2E7CBE, 0x3DFEBA8B, 0xBD92DB41, 0x3CFCD8BA, 0xBC0B29CD, 0x3A046D68, 0x3A29677D, 0xB93891BB, 0xB866CA2D, 0x370ACBB8))


def _full(like, v):
    return np.full(np.shape(like), v, np.float32)


def relu_f32(x):
    """U1: x < 0 -> +0, everything else (a NaN, -0, +0, positives) unchanged"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(x < f32(0), f32(0), x).astype(np.float32)


def gelu_tanh_f32(x):
    """U2: h = x / (1 + exp_spec(-a)), a = x * fma(x * x, K1, K0); -Inf -> -0"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        s = (x * x).astype(np.float32)
        w = Q.fma32(s, _full(x, TANH_K1), _full(x, TANH_K0))
        a = (x * w).astype(np.float32)
        d = (f32(1) + Q.exp_spec(-a)).astype(np.float32)
        h = (x / d).astype(np.float32)
        return np.where(x == f32(-np.inf), f32(-0.0), h).astype(np.float32)


def phi_neg_f32(t):
    """Phi(-t) for 0 <= t <= 12 (U3): exp(-t^2 / 2) * Q(t), the exponential as the fourth power of exp_spec(-t^2 / 8), the rounding error of t * t carried
    to first order (it is zero for a t of a 16-bit type)"""
    t = np.asarray(t, np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        v = ((t - ERF_K).astype(np.float32) / (t + ERF_K).astype(np.float32)).astype(np.float32)
        p = _full(t, ERF_C[10])
        for c in ERF_C[9::-1]:
            p = Q.fma32(p, v, _full(t, c))
        s = (t * t).astype(np.float32)
        e = Q.fma32(t, t, -s)
        ex = Q.exp_spec((s * f32(-0.125)).astype(np.float32))
        ex = (ex * ex).astype(np.float32)
        ex = (ex * ex).astype(np.float32)
        ex = Q.fma32(ex, (e * f32(-0.5)).astype(np.float32), ex)
        return (ex * p).astype(np.float32)


def gelu_erf_f32(x):
    """U3: h = x * Phi(x), Phi(x) = Phi(-|x|) for x < 0 and 1 - Phi(-|x|) otherwise, |x| clamped to 12; x < -12 (and -Inf) -> -0"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        ax = np.abs(x)
        t = np.where(ax < ERF_CUT, ax, ERF_CUT).astype(np.float32)          # a NaN becomes 12 here and comes back through x * Phi
        pn = phi_neg_f32(t)
        phi = np.where(x < f32(0), pn, (f32(1) - pn).astype(np.float32)).astype(np.float32)
        h = (x * phi).astype(np.float32)
        return np.where(x < -ERF_CUT, f32(-0.0), h).astype(np.float32)


_FN = {RELU: relu_f32, GELU_TANH: gelu_tanh_f32, GELU_ERF: gelu_erf_f32}


def kind_code(kind) -> int:
    return KIND_CODES[kind] if isinstance(kind, str) else int(kind)


def act(x: np.ndarray, dtype, kind) -> np.ndarray:
    """QSPEC U1-U3: h in the storage dtype (one storage rounding of the binary32 result)"""
    d = Q.dt(dtype)
    return Q.from_f32(_FN[kind_code(kind)](Q.to_f32(x, d)), d)


def act_quantize(x: np.ndarray, dtype, kind):
    """QSPEC U4: per-token quantisation of act(x).  Returns (q int8, scale f32, h stored dtype)."""
    h = act(x, dtype, kind)
    q, s = Q.quantize(h, Q.dt(dtype), 1)
    return q, s, h


def act_f64(x, kind) -> np.ndarray:
    """the same function in float64 (what a recogniser compares a model's activation with, and the reference of the accuracy bars)"""
    from math import erfc
    x = np.asarray(x, np.float64)
    k = kind_code(kind)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        if k == RELU:
            return np.where(x < 0, 0.0, x)
        if k == GELU_TANH:
            u = np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)
            return np.where(np.isinf(x), np.where(x > 0, x, -0.0), x / (1.0 + np.exp(-2.0 * u)))
        e = np.vectorize(erfc, otypes=[np.float64])(-x / np.sqrt(2.0))
        return np.where(np.isinf(x), np.where(x > 0, x, -0.0), 0.5 * x * e)
