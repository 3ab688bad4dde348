"""-m gpu: K1gh, pq_gated_hadamard_quant_rows / gated_hadamard_quantize — the gated activation of an MLP, the block Hadamard rotation and the per-token int8
quantisation in one launch, bit for bit (NaNs as a class) against the numpy specification hadamard_spec.hadamard_quantize(silu_mul | gelu_mul) (QSPEC GH1).  Every case
runs the C entry on g and u as column blocks of NaN-filled wider buffers — separate ones, and the two halves of one — with q, scale and h as windows of sentinel-filled
buffers whose margins are compared whole, with and without h_out; and the Python entry against the library's own two-launch composition."""
import numpy as np
import pytest
import torch
from oracle import qspec_numpy as Q
from tests import gemma_spec as G
from tests import hadamard_spec as H
from tests.gpu_util import TD, same, same_f, to_gpu
from tests.test_gpu_hadamard import PAD, SENT_Q, SENT_S, _margins_clean, _window, bits_t, lib  # noqa: F401  (the window / margin helpers and the fixture)

pytestmark = pytest.mark.gpu

# (rows, cols, block): generic, three blocks; packed sub-wave rows, no transpose; the 8-lane and the 64-lane transpose; two waves per row and the cross-wave amax; a real
# width; a row too long for registers (the two-pass generic form)
CASES = [(5, 48, 16), (5, 192, 64), (5, 512, 512), (3, 4096, 4096), (3, 6144, 2048), (2, 11008, 256), (2, 36864, 4096)]
GELU_CASES = [(5, 48, 16), (3, 6144, 2048), (2, 36864, 4096)]          # one per form: generic, wave, two-pass generic
SPEC = {"silu": Q.silu_mul, "gelu_tanh": G.gelu_mul}


def _inputs(code, rows, cols, seed, slow):
    """set F: gates N(0, 3) with |g| in [2^-20, 86] and no zero, the outlier channels planted in u — every wave of the silu takes the division-free quotient; set S
    (slow): a zero, +100 and -100 planted into the gate of every row — every wave divides.  Stored bit patterns."""
    r = np.random.default_rng(seed)
    g = r.standard_normal((rows, cols)).astype(np.float32) * 3
    g = np.copysign(np.clip(np.abs(g), 2.0 ** -20, 86.0), g)
    u = r.standard_normal((rows, cols)).astype(np.float32) * 3
    u[:, 5 % cols] *= 50
    u[:, (cols // 2 + 3) % cols] *= 25
    if slow:
        g[:, 7], g[:, 11], g[:, 13] = 0.0, 100.0, -100.0
    gb = Q.from_f32(g, code)
    mag = np.abs(Q.to_f32(gb, code))
    assert (mag.min() == 0 and mag.max() == 100) if slow else (0 < mag.min() and mag.max() <= 86)          # on the stored patterns
    return gb, Q.from_f32(u, code)


def _run(lib, gb, ub, code, act, block):
    """the C entry on guarded operands — g and u apart and as the halves of one buffer, with and without h_out — each against the spec; returns g, u (halves) on the GPU"""
    rows, cols = gb.shape
    it = torch.int32 if code == 2 else torch.int16
    want_q, want_s, want_h = H.hadamard_quantize(SPEC[act](gb, ub, code), code, block)
    nan = lambda w: torch.full((rows, w), float("nan"), dtype=TD[code], device="cuda")          # noqa: E731
    ga, ua, both = nan(cols + 2 * PAD), nan(cols + 2 * PAD), nan(2 * cols + 2 * PAD)
    pairs = [(ga[:, PAD:PAD + cols], ua[:, PAD:PAD + cols]), (both[:, PAD:PAD + cols], both[:, PAD + cols:PAD + 2 * cols])]
    st = torch.cuda.current_stream().cuda_stream
    for halves, (g, u) in enumerate(pairs):
        g.copy_(to_gpu(gb, code))
        u.copy_(to_gpu(ub, code))
        for with_h in (False, True):
            qraw, q = _window(rows, cols, torch.int8, SENT_Q)
            fill_h = SENT_S if code == 2 else 0x5A5B          # finite in every dtype
            hraw, hw = _window(rows, cols, it, fill_h)
            sraw = torch.full((rows + 16,), SENT_S, dtype=torch.int32, device="cuda")
            sc = sraw[8:8 + rows]
            rc = lib.pq_gated_hadamard_quant_rows(g.data_ptr(), g.stride(0), u.data_ptr(), u.stride(0), code, rows, cols, {"silu": 0, "gelu_tanh": 1}[act], block, q.data_ptr(),
                                                  q.stride(0), sc.data_ptr(), hw.data_ptr() if with_h else None, hw.stride(0), st)
            assert rc == 0, lib.pq_last_error()
            torch.cuda.synchronize()
            what = f"{act} {rows}x{cols} block {block} dtype {code} halves={halves} h={with_h}"
            same(q, want_q, what + ": codes")
            same(sc, want_s.view(np.uint32).view(np.int32), what + ": scales")
            if with_h:
                same_f(hw.view(TD[code]), want_h, code, what + ": h")
            else:
                assert bool((hw == fill_h).all()), what + ": h written without h_out"
            assert _margins_clean(qraw, q, SENT_Q) and _margins_clean(hraw, hw, fill_h), what + ": a margin of q or h was written"
            assert bool((sraw[:8] == SENT_S).all()) and bool((sraw[8 + rows:] == SENT_S).all()), what + ": a margin of scale was written"
    return pairs[1]


@pytest.mark.parametrize("code", [0, 1, 2], ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("slow", [False, True], ids=["F", "S"])
@pytest.mark.parametrize("act,rows,cols,block", [("silu",) + c for c in CASES] + [("gelu_tanh",) + c for c in GELU_CASES])
def test_bits_against_the_spec_and_the_composition(lib, code, slow, act, rows, cols, block):
    import protoquant_amd as pq
    g, u = _run(lib, *_inputs(code, rows, cols, cols + block, slow), code, act, block)
    qt, h = pq.gated_hadamard_quantize(g, u, act, block, return_h=True)
    h0 = (pq.silu_mul_quantize if act == "silu" else pq.gelu_mul_quantize)(g, u, return_h=True)[1]
    two, h2 = pq.hadamard_quantize(h0, block, return_h=True)
    assert torch.equal(bits_t(h), bits_t(h2)) and torch.equal(qt.int_data, two.int_data) and torch.equal(bits_t(qt.scale), bits_t(two.scale))
    assert torch.equal(pq.gated_hadamard_quantize(g, u, act, block).int_data, qt.int_data)


@pytest.mark.parametrize("code", [0, 1, 2], ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("cols,block", [(48, 16), (768, 256), (12288, 4096)])
def test_special_rows(lib, code, cols, block):
    """all zero; a NaN in u in one block; u = +Inf and -Inf in one block (under positive gates); the largest finite u everywhere; the row maximum in the last block"""
    gb, ub = _inputs(code, 5, cols, 7, False)
    g, u = Q.to_f32(gb, code), Q.to_f32(ub, code)
    g[0], u[0] = 0, 0
    u[1, min(block + 1, cols - 1)] = np.nan
    g[2, 1], g[2, block - 1], u[2, 1], u[2, block - 1] = 1.0, 1.0, np.inf, -np.inf
    u[3] = {0: 3.3895314e38, 1: 65504.0, 2: 3.4028235e38}[code]
    g[4], u[4] = 1.0, 0.25
    u[4, cols - block:] = 100.0          # a constant block: its h is 100 silu(1) sqrt(block) at the block's first element, the row's maximum
    gb, ub = Q.from_f32(g, code), Q.from_f32(u, code)
    _, want_s, want_h = H.hadamard_quantize(Q.silu_mul(gb, ub, code), code, block)          # the properties on the specification first, then the kernel against it
    hf = Q.to_f32(want_h, code)
    assert not hf[0].any() and want_s[0] == 1.0                                                    # all zero: scale 1
    nan_blocks = np.isnan(hf[1].reshape(-1, block)).all(axis=1)
    assert nan_blocks.sum() == 1 and not np.isnan(hf[1].reshape(-1, block)[~nan_blocks]).any() and np.isnan(want_s[1])      # only that block is NaN; the row's scale is
    assert np.isnan(hf[2, :block]).any() and not np.isnan(hf[2, block:]).any() and np.isnan(want_s[2])      # +Inf and -Inf in one block: Inf - Inf in that block alone
    assert np.argmax(np.abs(hf[4])) == cols - block                                                # the row maximum sits in the last block
    _run(lib, gb, ub, code, "silu", block)
