"""-m gpu: what `fuse_gemma_layers` trades for its norms.  pq.gemma_rmsnorm_quantize is QSPEC-exact (NG1-NG6: tests/test_gpu_gemma_norm.py)
and eager-CLOSE: transformers' GemmaRMSNorm — torch eager on the CPU — sums the squares in torch's own order, so a small share of the stored bf16 activations and
of the int8 codes differ.  The rate is a TESTED number at Gemma's hidden sizes, on >= 10^7 elements each.  Bounds, from the CPU measurement of the specification
against GemmaRMSNorm (1.05e7 elements per case) with the margin tests/test_gpu_rmsnorm_vs_eager.py gives its own figures: stored activations <= 1e-5 (measured
4.0e-6 at H = 2304, 4.1e-6 at 3072), codes <= 2e-6 (2.9e-7 / 3.8e-7), no difference beyond 2 storage ulps, and the row scales IDENTICAL.
Measured by this test on an MI355X (1.05e7 elements each): H = 2304: stored activations 4.48e-6, codes 3.81e-7; H = 3072: 4.00e-6 and 2.86e-7; no scale differs, max 1 ulp."""
import numpy as np
import pytest
import torch

from oracle import torch_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("H", [2304, 3072])
def test_fused_gemma_rmsnorm_quantize_is_eager_close_at_a_bounded_rate(H):
    import protoquant_amd as pq
    g1 = pytest.importorskip("transformers.models.gemma.modeling_gemma")
    eps = 1e-6
    rows_total = -(-10_500_000 // H)
    g = torch.Generator().manual_seed(700 + H)
    w = (0.3 * torch.randn(H, generator=g)).to(torch.bfloat16)
    w_gpu = w.cuda()
    norm = g1.GemmaRMSNorm(H, eps=eps).to(torch.bfloat16)
    with torch.no_grad():
        norm.weight.copy_(w)
    n = dh = dq = ds = 0
    max_ulp = 0
    done = 0
    while done < rows_total:
        r = min(1024, rows_total - done)
        scale = torch.exp(torch.empty(r, 1).uniform_(float(np.log(0.05)), float(np.log(20.0)), generator=g))
        x = (torch.randn(r, H, generator=g) * scale).to(torch.bfloat16)
        # the eager chain on the CPU: transformers' GemmaRMSNorm, then QSPEC's per-token quantisation of what it stored
        with torch.no_grad():
            h_t = norm(x)
        q_t, s_t = R.quantize_ref(h_t, 1)
        # the fused kernel (K1ng) through the C-ABI
        qt, h = pq.gemma_rmsnorm_quantize(x.cuda(), w_gpu, eps, return_h=True)
        hb, hb_t = h.cpu().view(torch.int16).numpy(), h_t.view(torch.int16).numpy()
        diff = hb != hb_t
        dh += int(diff.sum())
        if diff.any():          # same-sign neighbours of a 16-bit float format differ by 1 in the bit pattern per ulp
            max_ulp = max(max_ulp, int(np.abs(hb[diff].astype(np.int32) - hb_t[diff].astype(np.int32)).max()))
        dq += int((qt.int_data.cpu() != q_t).sum())
        ds += int((qt.scale.cpu().view(torch.int32) != s_t.view(torch.int32)).sum())
        n += r * H
        done += r
    assert n >= 10_000_000
    print(f"H={H}: {n} elements, stored activations differing {dh} ({dh / n:.2e}), codes differing {dq} ({dq / n:.2e}), scales differing {ds}, max {max_ulp} ulp")
    assert dh / n <= 1e-5, (dh, n)
    assert dq / n <= 2e-6, (dq, n)
    assert ds == 0 and max_ulp <= 2
