"""-m gpu: K1h, pq_hadamard_quant_rows / hadamard / hadamard_quantize — the block Hadamard rotation fused with the per-token int8 quantisation, bit for bit against
tests/hadamard_spec.py (QSPEC H1-H5; NaNs as a class).  Every case runs the C entry on x as a column block of a wider NaN-filled buffer with q, scale and h as windows
of sentinel-filled buffers whose margins are compared whole — with h_out, without it and in the transform-only form — and the Python entries for the composition
property hadamard_quantize(x) == quantize(hadamard(x))."""
import numpy as np
import pytest
import torch

from oracle import qspec_numpy as Q
from tests import hadamard_spec as H
from tests.gpu_util import TD, same, same_f, to_gpu

pytestmark = pytest.mark.gpu

PAD = 64                    # columns of margin: 16-byte multiples in every dtype, so the register layouts stay reachable
SENT_Q, SENT_S = 0x5B, 0x5A5B5A5B
# (rows, cols, block): the generic form (three blocks); sub-wave rows packed several to a wave; blocks of 256 / 512 (4 / 8 lanes transposed through LDS); the 64-lane
# transpose, smallest and largest row; several blocks per row and a real width; several waves per row and the cross-wave amax; a row too long for registers (the two-pass
# generic form)
CASES = [(1, 16, 16), (5, 48, 16), (5, 192, 64), (3, 128, 128), (5, 512, 512), (5, 256, 256), (5, 1024, 1024), (3, 4096, 4096), (3, 6144, 2048), (2, 11008, 256),
         (2, 12288, 4096), (2, 36864, 4096)]


@pytest.fixture(scope="module")
def lib():
    from protoquant_amd import _lib
    assert torch.cuda.is_available()
    return _lib.lib()


def _rows(code, rows, cols, seed):
    """seeded rows with two outlier channels, as stored bit patterns"""
    g = np.random.default_rng(seed)
    x = g.standard_normal((rows, cols)).astype(np.float32) * 3
    x[:, 5 % cols] *= 50
    x[:, (cols // 2 + 3) % cols] *= 25
    return Q.from_f32(x, code)


def _specials(code, cols, block):
    """all zero; a NaN in one block; +Inf and -Inf in one block; the largest finite value everywhere; the maximum of |h| in the last block"""
    x = Q.to_f32(_rows(code, 5, cols, 7), code)
    big = {0: 3.3895314e38, 1: 65504.0, 2: 3.4028235e38}[code]
    x[0] = 0
    x[1, min(block + 1, cols - 1)] = np.nan
    x[2, 1], x[2, block - 1] = np.inf, -np.inf
    x[3] = big
    x[4] = 0.25
    x[4, cols - block:] = 100.0          # a constant block: its h is 100 sqrt(block) at the block's first element, the row's maximum
    return Q.from_f32(x, code)


def _window(rows, cols, dtype, fill):
    raw = torch.full((rows + 2, cols + 2 * PAD), fill, dtype=dtype, device="cuda")
    return raw, raw[1:rows + 1, PAD:PAD + cols]


def _margins_clean(raw, win, fill):
    keep = win.clone()
    win.fill_(fill)
    ok = bool((raw == fill).all())
    win.copy_(keep)
    return ok


def _run(lib, xb, code, block):
    """the three forms of the C entry on guarded operands, each against the spec"""
    rows, cols = xb.shape
    it = torch.int32 if code == 2 else torch.int16
    want_q, want_s, want_h = H.hadamard_quantize(xb, code, block)
    xraw = torch.full((rows, cols + 2 * PAD), float("nan"), dtype=TD[code], device="cuda")
    x = xraw[:, PAD:PAD + cols]
    x.copy_(to_gpu(xb, code))
    st = torch.cuda.current_stream().cuda_stream
    for with_q, with_h in ((True, False), (True, True), (False, True)):
        qraw, q = _window(rows, cols, torch.int8, SENT_Q)
        fill_h = SENT_S if code == 2 else 0x5A5B          # finite in every dtype
        hraw, hw = _window(rows, cols, it, fill_h)
        sraw = torch.full((rows + 16,), SENT_S, dtype=torch.int32, device="cuda")
        sc = sraw[8:8 + rows]
        rc = lib.pq_hadamard_quant_rows(x.data_ptr(), code, rows, cols, x.stride(0), block, q.data_ptr() if with_q else None, q.stride(0),
                                        sc.data_ptr() if with_q else None, hw.data_ptr() if with_h else None, hw.stride(0), st)
        assert rc == 0, lib.pq_last_error()
        torch.cuda.synchronize()
        what = f"{rows}x{cols} block {block} dtype {code} q={with_q} h={with_h}"
        if with_q:
            same(q, want_q, what + ": codes")
            same(sc, want_s.view(np.uint32).view(np.int32), what + ": scales")
        else:
            assert bool((q == SENT_Q).all()) and bool((sc == SENT_S).all()), what + ": the transform-only form wrote codes or scales"
        if with_h:
            same_f(hw.view(TD[code]), want_h, code, what + ": h")
        else:
            assert bool((hw == fill_h).all()), what + ": h written without h_out"
        assert _margins_clean(qraw, q, SENT_Q) and _margins_clean(hraw, hw, fill_h), what + ": a margin of q or h was written"
        assert bool((sraw[:8] == SENT_S).all()) and bool((sraw[8 + rows:] == SENT_S).all()), what + ": a margin of scale was written"
    return x, want_q, want_s, want_h


@pytest.mark.parametrize("code", [0, 1, 2], ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("rows,cols,block", CASES)
def test_bits_against_the_spec_on_guarded_operands(lib, code, rows, cols, block):
    import protoquant_amd as pq
    x, want_q, want_s, want_h = _run(lib, _rows(code, rows, cols, cols + block), code, block)
    qt, h = pq.hadamard_quantize(x, block, return_h=True)
    h2 = pq.hadamard(x, block)
    two = pq.quantize(h2)
    assert torch.equal(bits_t(h), bits_t(h2)) and torch.equal(qt.int_data, two.int_data) and torch.equal(bits_t(qt.scale), bits_t(two.scale))
    same(qt.int_data, want_q, "hadamard_quantize: codes")
    same_f(h, want_h, code, "hadamard_quantize: h")


def bits_t(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("code", [0, 1, 2], ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("cols,block", [(48, 16), (768, 256), (12288, 4096)])
def test_special_rows(lib, code, cols, block):
    xb = _specials(code, cols, block)
    _, _, want_s, want_h = _run(lib, xb, code, block)
    hf = Q.to_f32(want_h, code)
    assert not hf[0].any() and want_s[0] == 1.0                                                    # all zero: scale 1
    nan_blocks = np.isnan(hf[1].reshape(-1, block)).all(axis=1)
    assert nan_blocks.sum() == 1 and not np.isnan(hf[1].reshape(-1, block)[~nan_blocks]).any() and np.isnan(want_s[1])      # only that block is NaN; the row's scale is
    assert np.isnan(hf[2, :block]).any() and not np.isnan(hf[2, block:]).any() and np.isnan(want_s[2])      # +Inf and -Inf in one block: Inf - Inf in that block alone
    assert np.argmax(np.abs(hf[4])) == cols - block                                                # the row maximum sits in the last block
