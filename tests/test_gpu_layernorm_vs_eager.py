"""-m gpu: what fuse_layernorm_layers trades.  pq.layernorm_quantize is QSPEC-exact (L1-L6: tests/test_gpu_layernorm_quant.py against the CPU
specification) and eager-CLOSE: torch's F.layer_norm — its eager CPU kernel here — sums in torch's own order and applies weight and bias in another association, so a
small share of the stored activations and of the int8 codes differ.  The rate is a TESTED number on >= 10^7 elements per 16-bit dtype at two hidden sizes; the
measured values are printed and written in DESIGN.md, the bounds sit a little above them.  The size of a difference is measured in CODE UNITS (|difference| / the row's
scale): where the bias cancels the normalised term a stored value near zero can differ by thousands of its own ulps and still be nothing against the row's range;
one ulp of the binade the row's amax lies in is between 127 / 256 = 0.50 and 127 / 128 = 0.99 code units for bf16 (0.06 .. 0.12 for fp16), depending on where in its binade
the amax sits: no difference is larger than that one ulp (measured: 0.55 / 0.45 and 0.080 / 0.064 code units)."""
import numpy as np
import pytest
import torch

from oracle import torch_ref as R

pytestmark = pytest.mark.gpu

# dtype -> (stored h, codes, row scales, largest difference in code units): bounds a little above what was measured
BOUNDS = {torch.bfloat16: (1e-4, 1e-5, 2e-4, 1.0), torch.float16: (6e-4, 3e-5, 2e-3, 0.125)}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("H", [768, 4096])
def test_fused_layernorm_quantize_is_eager_close_at_a_bounded_rate(dtype, H):
    import protoquant_amd as pq
    rows_total = -(-10_500_000 // H)
    g = torch.Generator().manual_seed(900 + H)
    w = (1 + 0.2 * torch.randn(H, generator=g)).to(dtype)
    b = (0.2 * torch.randn(H, generator=g)).to(dtype)
    w_gpu, b_gpu = w.cuda(), b.cuda()
    n = dh = dq = ds = nrows = 0
    max_units = 0.0
    done = 0
    while done < rows_total:
        r = min(2048, rows_total - done)
        scale = torch.exp(torch.empty(r, 1).uniform_(float(np.log(0.05)), float(np.log(20.0)), generator=g))
        x = ((torch.randn(r, H, generator=g) + 0.25) * scale).to(dtype)
        h_t = torch.nn.functional.layer_norm(x, (H,), w, b, 1e-5)          # torch's eager CPU kernel on the 16-bit tensor
        q_t, s_t = R.quantize_ref(h_t, 1)
        qt, h = pq.layernorm_quantize(x.cuda(), w_gpu, b_gpu, 1e-5, return_h=True)
        hb, hb_t = h.cpu().view(torch.int16).numpy(), h_t.view(torch.int16).numpy()
        diff = hb != hb_t
        dh += int(diff.sum())
        if diff.any():
            units = ((h.cpu().float() - h_t.float()).abs() / qt.scale.cpu()[:, None]).numpy()
            max_units = max(max_units, float(units[diff].max()))
        dq += int((qt.int_data.cpu() != q_t).sum())
        ds += int((qt.scale.cpu().view(torch.int32) != s_t.view(torch.int32)).sum())
        n += r * H
        nrows += r
        done += r
    assert n >= 10_000_000
    print(f"LNEAGER {dtype} H={H}: {n} elements, stored activations differing {dh} ({dh / n:.2e}), codes differing {dq} ({dq / n:.2e}), scales differing {ds} of {nrows} "
          f"({ds / nrows:.2e}), largest difference {max_units:.3f} code units")
    bh, bq, bs, bu = BOUNDS[dtype]
    assert dh / n <= bh and dq / n <= bq and ds / nrows <= bs and max_units <= bu, (dh / n, dq / n, ds / nrows, max_units)
