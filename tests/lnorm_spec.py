"""TEST INFRASTRUCTURE — numpy restatement of QSPEC L1-L6: LayerNorm (weight, optional bias) fused with the per-token quantisation, built on
oracle.qspec_numpy (fma32, to_f32, from_f32, quantize).  Half types travel as uint16 bit patterns with a dtype code, as there.  The pinned order of the two sums
(L2, L3) is restated here from its definition — 16-byte vector v of a row belongs to lane v mod 256, a lane walks its vectors in increasing v and their elements in
order, an xor butterfly (offsets 32 .. 1) per 64 lanes, the four partial sums added left to right — and `slots` lets a test deal the same row differently."""
import numpy as np

from oracle import qspec_numpy as Q


def pinned_sum(vals: np.ndarray, epv: int, square: bool, lanes: int = 256) -> np.ndarray:
    """The pinned-order sum of each row of vals (float32 [rows, cols]); square=False: acc = acc + v (L2), square=True: acc = fma(v, v, acc) (L3).
    `lanes` = 256 is the specification.  A layout that holds the row on 64 physical lanes (one wave per row) must play the four 64-lane groups itself:
    pinned_sum_wave below restates that and must agree with this."""
    rows, cols = vals.shape
    nvec = (cols + epv - 1) // epv
    slots = max((nvec + lanes - 1) // lanes, 1)
    pad = np.zeros((rows, slots * lanes * epv), np.float32)          # +0 padding: acc + 0 = acc and fma(0, 0, acc) = acc (acc is never -0)
    pad[:, :cols] = vals
    v = pad.reshape(rows, slots, lanes, epv)                         # [row, i, lane, e]: vector i * lanes + lane
    acc = np.zeros((rows, lanes), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(slots):
            for e in range(epv):
                acc = Q.fma32(v[:, i, :, e], v[:, i, :, e], acc) if square else (acc + v[:, i, :, e]).astype(np.float32)
        s = acc.reshape(rows, 4, 64)
        idx = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            s = (s + s[:, :, idx ^ off]).astype(np.float32)
        g = s[:, :, 0]
        return (((g[:, 0] + g[:, 1]).astype(np.float32) + g[:, 2]).astype(np.float32) + g[:, 3]).astype(np.float32)


def pinned_sum_wave(vals: np.ndarray, epv: int, square: bool, vpl: int) -> np.ndarray:
    """The same sum as a one-wave-per-row layout computes it: 64 physical lanes, `vpl` vectors per lane (vector i * 64 + l on lane l), one accumulator per
    group i mod 4 — physical lane l plays the specification's lanes l, l + 64, l + 128, l + 192."""
    rows, cols = vals.shape
    nvec = (cols + epv - 1) // epv
    assert nvec <= 64 * vpl
    pad = np.zeros((rows, vpl * 64 * epv), np.float32)
    pad[:, :cols] = vals
    v = pad.reshape(rows, vpl, 64, epv)
    acc = np.zeros((rows, 4, 64), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(vpl):
            for e in range(epv):
                a = acc[:, i & 3, :]
                acc[:, i & 3, :] = Q.fma32(v[:, i, :, e], v[:, i, :, e], a) if square else (a + v[:, i, :, e]).astype(np.float32)
        idx = np.arange(64)
        s = acc
        for off in (32, 16, 8, 4, 2, 1):
            s = (s + s[:, :, idx ^ off]).astype(np.float32)
        g = s[:, :, 0]
        return (((g[:, 0] + g[:, 1]).astype(np.float32) + g[:, 2]).astype(np.float32) + g[:, 3]).astype(np.float32)


def layernorm(x: np.ndarray, weight: np.ndarray, bias, eps: float, dtype):
    """QSPEC L1-L5.  Returns (h stored dtype, mean f32, rs f32)."""
    d = Q.dt(dtype)
    epv = 4 if d == Q.DT_F32 else 8
    xf, wf = Q.to_f32(x, d), Q.to_f32(weight, d)                                                   # L1
    c = np.float32(xf.shape[1])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        mean = (pinned_sum(xf, epv, False) / c).astype(np.float32)                                 # L2
        dv = (xf - mean[:, None]).astype(np.float32)                                               # L3
        var = (pinned_sum(dv, epv, True) / c).astype(np.float32)
        rs = (np.float32(1) / np.sqrt((var + np.float32(eps)).astype(np.float32)).astype(np.float32)).astype(np.float32)      # L4
        h = ((dv * rs[:, None]).astype(np.float32) * wf[None, :]).astype(np.float32)               # L5
        if bias is not None:
            h = (h + Q.to_f32(bias, d)[None, :]).astype(np.float32)
    return Q.from_f32(h, d), mean, rs


def layernorm_quantize(x: np.ndarray, weight: np.ndarray, bias, eps: float, dtype):
    """QSPEC L1-L6.  Returns (q int8, scale f32, h stored dtype)."""
    h, _, _ = layernorm(x, weight, bias, eps, dtype)
    q, s = Q.quantize(h, Q.dt(dtype), 1)
    return q, s, h


def layernorm_f64(x: np.ndarray, weight: np.ndarray, bias, eps: float) -> np.ndarray:
    x = np.asarray(x, np.float64)
    m = x.mean(axis=1, keepdims=True)
    v = ((x - m) ** 2).mean(axis=1, keepdims=True)
    h = (x - m) / np.sqrt(v + eps) * np.asarray(weight, np.float64)[None, :]
    return h if bias is None else h + np.asarray(bias, np.float64)[None, :]
