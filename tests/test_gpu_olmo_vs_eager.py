"""-m gpu: what fuse_olmo_layers(fuse_residual=True) trades for its norms.  pq.olmo_rmsnorm (K1on) is QSPEC-exact (NO1-NO5:
tests/test_gpu_olmo_postnorm.py) and eager-CLOSE: transformers' Olmo2RMSNorm — torch eager on the GPU — sums the squares in torch's own order and takes rsqrt where the
specification divides by an IEEE square root, so a small share of the stored bf16 activations differ.  The rate is a TESTED number at H = 4096 on >= 10^7 elements,
held to the bounds tests/test_gpu_gemma_vs_eager.py holds for the same N1-N4 arithmetic: a differing share of stored elements <= 1e-5, and no difference beyond 2
storage ulps.
Measured by this test on an MI355X (1.05e7 elements): 56 stored activations differ (5.33e-6), max 1 ulp."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_k1on_is_eager_close_at_a_bounded_rate():
    import protoquant_amd as pq
    m2 = pytest.importorskip("transformers.models.olmo2.modeling_olmo2")
    H, eps = 4096, 1e-6
    rows_total = -(-10_500_000 // H)
    g = torch.Generator().manual_seed(700 + H)
    w = (1.0 + 0.3 * torch.randn(H, generator=g)).to(torch.bfloat16)
    norm = m2.Olmo2RMSNorm(H, eps=eps).to(torch.bfloat16).cuda()
    with torch.no_grad():
        norm.weight.copy_(w)
    w_gpu = norm.weight.detach()
    n = dh = 0
    max_ulp = 0
    done = 0
    while done < rows_total:
        r = min(1024, rows_total - done)
        scale = torch.exp(torch.empty(r, 1).uniform_(float(np.log(0.05)), float(np.log(20.0)), generator=g))
        x = (torch.randn(r, H, generator=g) * scale).to(torch.bfloat16).cuda()
        with torch.no_grad():
            h_t = norm(x)                                   # the eager chain on the GPU
        h = pq.olmo_rmsnorm(x, w_gpu, eps)                  # K1on through the C-ABI
        hb, hb_t = h.view(torch.int16).to(torch.int32), h_t.view(torch.int16).to(torch.int32)
        diff = hb != hb_t
        dh += int(diff.sum())
        if bool(diff.any()):          # same-sign neighbours of a 16-bit float format differ by 1 in the bit pattern per ulp
            max_ulp = max(max_ulp, int((hb[diff] - hb_t[diff]).abs().max()))
        n += r * H
        done += r
    assert n >= 10_000_000
    print(f"H={H}: {n} elements, stored activations differing {dh} ({dh / n:.2e}), max {max_ulp} ulp")
    assert dh / n <= 1e-5, (dh, n)
    assert max_ulp <= 2
