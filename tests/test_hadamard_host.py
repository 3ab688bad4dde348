"""CPU: the host side of K1h (pq_hadamard_quant_rows / hadamard / hadamard_quantize): QSPEC H1-H4 in numpy (tests/hadamard_spec.py) against the float64 product within the
forward-error bound of its summation tree; the rotated quantisation beats the plain one on the designed outlier rows (a property of the specification alone); every bad
argument is refused and named before any HIP call; the Python entries check their block and have no CPU path."""
import numpy as np
import pytest
import torch

from oracle import qspec_numpy as Q
from tests import hadamard_spec as H

SYM = "pq_hadamard_quant_rows"


@pytest.mark.parametrize("code", [0, 1, 2], ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("cols,block", [(64, 2), (48, 16), (192, 64), (512, 512), (8192, 4096), (6144, 2048)])
def test_spec_is_the_float64_product_within_the_tree_bound(code, cols, block):
    """per element at most (log2 B + 2) 2^-24 sum|x_i| / sqrt(B) over its block — a balanced tree of depth log2 B, one scaling, one cast to binary32 — plus half an ulp
    of the storage dtype for 16-bit outputs"""
    g = np.random.default_rng(cols + block)
    xb = Q.from_f32((g.standard_normal((4, cols)) * g.choice([0.01, 1.0, 300.0], size=(4, 1))).astype(np.float32), code)
    x64 = Q.to_f32(xb, code).astype(np.float64).reshape(4, -1, block)
    exact = x64 @ H.hadamard_matrix(block) / np.sqrt(block)
    got = Q.to_f32(H.hadamard(xb, code, block), code).astype(np.float64).reshape(4, -1, block)
    bound = (np.log2(block) + 2) * 2.0 ** -24 * np.abs(x64).sum(axis=-1, keepdims=True) / np.sqrt(block)
    # half an ulp of a p-bit significand is at most 2^-p of the value (bf16: p = 8, fp16: p = 11; fp16 below 2^-14: half a subnormal step)
    half_ulp = {0: 2.0 ** -8, 1: 2.0 ** -11, 2: 0.0}[code] * np.maximum(np.abs(exact), np.abs(got)) + (2.0 ** -25 if code == 1 else 0.0)
    assert (np.abs(got - exact) <= bound + half_ulp).all()


@pytest.mark.parametrize("K,block,amp", [(256, 256, 50), (256, 64, 50), (192, 64, 50), (1024, 256, 100)])
def test_rotation_lowers_the_quantisation_error_on_the_designed_outlier_rows(K, block, amp):
    """M, N = 32, 64; x standard normal with column 5 times amp and column K / 2 + 3 times amp / 2; W normal / sqrt(K); default_rng(0); the symmetric / 127 quantiser
    on both operands (f32 storage), the relative L2 error of y against the exact product"""
    g = np.random.default_rng(0)
    x = g.standard_normal((32, K))
    x[:, 5] *= amp
    x[:, K // 2 + 3] *= amp / 2
    w = g.standard_normal((64, K)) / np.sqrt(K)
    x, w = x.astype(np.float32), w.astype(np.float32)
    exact = x.astype(np.float64) @ w.astype(np.float64).T

    def err(xq, xs, wq, ws):
        y = (xq.astype(np.float64) * xs[:, None]) @ (wq.astype(np.float64) * ws[:, None]).T
        return np.linalg.norm(y - exact) / np.linalg.norm(exact)
    plain = err(*Q.quantize(x, 2, 1), *Q.quantize(w, 2, 1))
    rotated = err(*H.hadamard_quantize(x, 2, block)[:2], *H.hadamard_quantize(w, 2, block)[:2])
    print(f"K={K} block={block} amp={amp}: plain {plain:.4f} rotated {rotated:.4f} ratio x{plain / rotated:.1f}")
    assert rotated < plain


def _call(L, **kw):
    """the entry with plausible (never dereferenced) operands, bf16 4 x 128 in blocks of 64, some arguments overridden"""
    a = dict(x=0x10000, dtype=0, rows=4, cols=128, ldx=128, block=64, q=0x50000, ldq=128, scale=0x60000, h=None, ldh=0)
    a.update(kw)
    return getattr(L, SYM)(a["x"], a["dtype"], a["rows"], a["cols"], a["ldx"], a["block"], a["q"], a["ldq"], a["scale"], a["h"], a["ldh"], None)


BAD = [(dict(block=48), b"power of two"), (dict(block=0), b"power of two"), (dict(block=1), b"power of two"), (dict(block=8192, cols=8192, ldx=8192, ldq=8192), b"power of two"),
       (dict(block=256), b"does not divide"), (dict(cols=96, block=64), b"does not divide"), (dict(dtype=3), b"dtype"), (dict(rows=-1), b"rows"), (dict(rows=1 << 31), b"rows"),
       (dict(x=None), b"x is null"), (dict(ldx=64), b"ld_x"), (dict(ldq=64), b"ld_q"), (dict(h=0x70000, ldh=64), b"ld_h"),
       (dict(q=None), b"q is null"), (dict(scale=None), b"scale is null"), (dict(q=None, scale=None, ldh=128), b"h_out is null"),
       (dict(q=0x10000), b"q overlaps x"), (dict(q=0x10000 + 4 * 256 - 1), b"q overlaps x"), (dict(scale=0x10000 + 8), b"scale overlaps x"),
       (dict(h=0x10000, ldh=128), b"h_out overlaps x"), (dict(h=0x10000 + 2, ldh=128), b"h_out overlaps x"), (dict(h=0x50000 + 64, ldh=128), b"q overlaps h_out"),
       (dict(q=None, scale=None, h=0x10000 + 256, ldh=128), b"h_out overlaps x")]


@pytest.mark.parametrize("kw,named", BAD)
def test_bad_arguments_are_named_without_a_gpu(kw, named):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _call(L, **kw) == 1, kw
    err = L.pq_last_error()
    assert SYM.encode() in err and named in err, (kw, err)
    assert _call(L, rows=0) == 0 and _call(L, cols=0, ldx=0, ldq=0) == 0          # empty problems are no-ops


def test_python_entries_check_the_block_and_have_no_cpu_path():
    import protoquant_amd as pq
    from protoquant_amd import _lib
    from protoquant_amd.hadamard import default_block
    x = torch.zeros(4, 96, dtype=torch.bfloat16)
    for f in (pq.hadamard, pq.hadamard_quantize):
        with pytest.raises(_lib.PQError):
            f(x)
    assert default_block(96) == 32 and default_block(11008) == 256 and default_block(14336) == 2048 and default_block(8192) == 4096
    orig = _lib.require_gpu
    _lib.require_gpu = lambda t, name: None
    try:
        for f in (pq.hadamard, pq.hadamard_quantize):
            for bad in (48, 64, 8, 8192):          # no power of two; does not divide 96; below 16; above 4096
                with pytest.raises(ValueError, match="block"):
                    f(x, bad)
            with pytest.raises(ValueError, match="block"):
                f(torch.zeros(4, 72, dtype=torch.bfloat16))          # the default for 72 columns is 8: below 16
        with pytest.raises(ValueError):
            pq.hadamard(x, 32, out=torch.zeros(4, 96, dtype=torch.float16))
    finally:
        _lib.require_gpu = orig
    for name in ("hadamard", "hadamard_quantize", "RotatedQLinear", "rotate_linears"):
        assert name in pq.__all__ and callable(getattr(pq, name))
    from protoquant_amd.qlinear import is_code_fed
    rot = pq.RotatedQLinear(64, 8)
    assert not is_code_fed(rot) and is_code_fed(pq.qlinear(64, 8)) and int(rot.rot_block) == 64 and "rot_block" in rot.state_dict()
    with pytest.raises(TypeError, match="QTensor"):
        rot(pq.QTensor(torch.zeros(2, 64, dtype=torch.int8), torch.ones(2), 1, torch.bfloat16, torch.Size((2, 64))))
