"""TEST INFRASTRUCTURE — QSPEC W1-W4 in numpy: the int4 weight format "W4 v1", a second, integer quantisation level on top of the per-channel int8
weight.  The rule, the layout and the expansion; it is the specification, not a test.  Integers only: there is one result."""
import numpy as np

GROUP = 128


def round_k(K):
    return -(-K // GROUP) * GROUP


def group_mult(a):
    """W1: the multiplier of a group whose largest |code| is a"""
    return np.clip(-(-np.asarray(a, np.int64) // 7), 1, 18)


def code(w, g):
    """W2: clamp(sign(w) * ((2 |w| + g) div (2 g)), -7, 7) — round half away from zero"""
    w = np.asarray(w, np.int64)
    return np.sign(w) * np.minimum((2 * np.abs(w) + g) // (2 * g), 7)


def levels(wq):
    """int8 [N, K] -> (q int64 [N, Kp], g int64 [N, Kp / 128]); Kp = K rounded up to 128, tail codes 0"""
    N, K = wq.shape
    w = np.zeros((N, round_k(K)), np.int64)
    w[:, :K] = wq
    g = group_mult(np.abs(w).reshape(N, -1, GROUP).max(axis=2))
    return code(w, np.repeat(g, GROUP, axis=1)), g


def pack(wq):
    """W3-W4: (w4 u8[N, Kp / 2], gs u8[ceil(N / 4), Kp / 128, 4]) — byte 64 j + i of a row: q[128 j + i] low nibble, q[128 j + 64 + i] high; rows of gs past N hold 1"""
    q, g = levels(wq)
    N, G = g.shape
    q = q.reshape(N, G, 2, GROUP // 2) & 0xF
    w4 = (q[:, :, 0] | (q[:, :, 1] << 4)).astype(np.uint8).reshape(N, G * GROUP // 2)
    gs = np.ones((-(-N // 4) * 4, G), np.uint8)
    gs[:N] = g
    return w4, np.ascontiguousarray(gs.reshape(-1, 4, G).transpose(0, 2, 1))


def expand(w4, gs):
    """the int8 weight the pair stands for: W8[n, k] = q[n, k] * g[n, k / 128], s8 [N, Kp]"""
    N, G = w4.shape[0], w4.shape[1] // (GROUP // 2)
    b = w4.reshape(N, G, 1, GROUP // 2).astype(np.int64)
    q = (np.concatenate([b & 0xF, b >> 4], axis=2) ^ 8) - 8                      # two's-complement nibbles
    g = gs.transpose(0, 2, 1).reshape(-1, G)[:N].astype(np.int64)
    return (q * g[:, :, None, None]).reshape(N, G * GROUP).astype(np.int8)
