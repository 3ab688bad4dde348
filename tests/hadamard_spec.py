"""TEST INFRASTRUCTURE — QSPEC H1-H5 in numpy: the block Hadamard rotation of kernel K1h and the per-token quantisation of its stored result.  Half types
are uint16 bit patterns with the dtype codes of oracle/qspec_numpy.py (0 bf16, 1 fp16, 2 f32), whose conversions and quantiser this restatement uses."""
import numpy as np

from oracle import qspec_numpy as Q


def hadamard(x: np.ndarray, dtype, block: int) -> np.ndarray:
    """H1-H4 on a [rows, cols] tensor: every block of `block` consecutive elements of a row through log2(block) butterfly stages in ascending stride, one binary32
    operation per result; times the binary32 nearest to block^(-1/2); rounded to the storage dtype."""
    v = Q.to_f32(x, dtype).copy()                                        # H1
    rows, cols = v.shape
    assert block >= 2 and block & (block - 1) == 0 and cols % block == 0
    v = v.reshape(rows, cols // block, block)
    with np.errstate(invalid="ignore", over="ignore"):
        s = 1
        while s < block:                                                 # H2: stage log2(s); pairs (i, i + s) with that bit of i clear
            w = v.reshape(rows, cols // block, block // (2 * s), 2, s)
            a, b = w[..., 0, :].copy(), w[..., 1, :].copy()
            w[..., 0, :] = a + b
            w[..., 1, :] = a - b
            s *= 2
        y = v * np.float32(1.0 / np.sqrt(np.float64(block)))             # H3
    return Q.from_f32(y.reshape(rows, cols).astype(np.float32), dtype)   # H4


def hadamard_quantize(x: np.ndarray, dtype, block: int):
    """H1-H5: (codes, scales, h) — Q1-Q6 on the rows of h as stored"""
    h = hadamard(x, dtype, block)
    q, scale = Q.quantize(h, dtype, 1)
    return q, scale, h


def hadamard_matrix(block: int) -> np.ndarray:
    """the Sylvester matrix H_block in float64 (entries +-1): the transform above is x @ H / sqrt(block) in real arithmetic"""
    h = np.ones((1, 1))
    while h.shape[0] < block:
        h = np.block([[h, h], [h, -h]])
    return h
