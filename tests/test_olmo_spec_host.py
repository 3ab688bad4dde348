"""CPU: the specification of the OLMo-2 / OLMo-3 forms (tests/olmo_spec.py: NO1-NO5, PO1, A1, Q1-Q6) — against transformers' Olmo2RMSNorm and Olmo3RMSNorm at the
rate tests/test_gemma_spec_host.py holds NG to (identical row scales, no stored value more than 2 ulp apart), against the Llama and Gemma forms it is not, on the
probe operands of the recognisers (where it IS the eager module, bit for bit), as the composition of its parts, on one hand-computed row, and on NaN, Inf and zero
rows."""
import numpy as np
import pytest
import torch

from oracle import qspec_numpy as Q
from tests import olmo_spec as O
from tests.addnorm_spec import to_bits
from tests.gemma_spec import ulp_distance

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
IDS = ["bf16", "fp16", "f32"]


def _inputs(rows, H, dtype, seed):
    """rows scaled log-uniformly over 0.05 .. 20, weight 0.3 randn (the operands of tests/test_gemma_spec_host.py)"""
    g = torch.Generator().manual_seed(seed)
    scale = torch.exp(torch.empty(rows, 1).uniform_(float(np.log(0.05)), float(np.log(20.0)), generator=g))
    x = (torch.randn(rows, H, generator=g) * scale).to(dtype)
    w = (0.3 * torch.randn(H, generator=g)).to(dtype)
    return x, w


def _olmo_norm_classes():
    m2 = pytest.importorskip("transformers.models.olmo2.modeling_olmo2")
    m3 = pytest.importorskip("transformers.models.olmo3.modeling_olmo3")
    return m2.Olmo2RMSNorm, m3.Olmo3RMSNorm


@pytest.mark.parametrize("which", [0, 1], ids=["Olmo2RMSNorm", "Olmo3RMSNorm"])
def test_no_spec_against_transformers_olmo_rmsnorm(which):
    """10^6 bf16 elements through the eager module and through NO1-NO5: they differ only by the pinned summation order — identical row scales of the quantised result,
    and no stored value more than 2 ulp apart"""
    cls = _olmo_norm_classes()[which]
    rows, H, eps = 435, 2304, 1e-6
    assert rows * H >= 10 ** 6
    x, w = _inputs(rows, H, torch.bfloat16, 11)
    norm = cls(H, eps=eps).to(torch.bfloat16)
    with torch.no_grad():
        norm.weight.copy_(w)
        want = norm(x)
    got = O.rmsnorm(x, w, eps)
    d = ulp_distance(got, want)
    q, sc = Q.quantize(to_bits(got), 0, 1)
    q_e, sc_e = Q.quantize(to_bits(want), 0, 1)
    print(f"NO vs {cls.__name__}, {rows} x {H} bf16: stored values differing {float((d > 0).float().mean()):.3g}, max {int(d.max())} ulp, "
          f"codes differing {float((q != q_e).mean()):.3g}, scales differing {int((sc != sc_e).sum())}")
    assert int(d.max()) <= 2
    assert np.array_equal(sc, sc_e)


def test_no_on_the_probe_operands_is_the_eager_module_and_not_the_llama_or_gemma_form():
    """the operands of is_gemma_rmsnorm / is_olmo_rmsnorm (seed 20240221, width 64): the NO formula in torch equals the eager Olmo2RMSNorm bit for bit in all three
    dtypes, and so does the specification (pinned order, IEEE division and square root) in the 16-bit dtypes — in f32 the two orders of a 64-term sum and rsqrt against 1 / sqrt show, within 2^-20 relative (each order of the sum
    is within 6 roundings of the exact one, rs takes half of that, the reciprocal square roots are within 2 ulp of each other and two products follow); the
    Llama formula differs in 246 of 960 bf16 and 244 of 960 fp16 elements and in no f32 element; the Gemma formula differs in every dtype"""
    cls = _olmo_norm_classes()[0]
    g = torch.Generator().manual_seed(20240221)
    xs = torch.randn(3, 5, 64, generator=g) * torch.tensor([0.05, 1.0, 20.0]).reshape(3, 1, 1)
    ws = 0.3 * torch.randn(64, generator=g)
    eps = 1e-6
    counts = {}
    for dt in DTYPES:
        x, w = xs.to(dt).reshape(15, 64), ws.to(dt)
        norm = cls(64, eps=eps).to(dt)
        with torch.no_grad():
            norm.weight.copy_(w)
            eager = norm(x)
        spec = O.rmsnorm(x, w, eps)
        assert torch.equal(O.olmo_formula(x, w, eps), eager), dt
        if dt != torch.float32:
            assert torch.equal(spec, eager), dt
        else:
            assert bool(((spec - eager).abs() <= eager.abs() * 2.0 ** -20).all())
        counts[dt] = int((O.llama_formula(x, w, eps) != eager).sum())
        assert not torch.equal(O.gemma_formula(x, w, eps), eager), dt
    assert counts == {torch.bfloat16: 246, torch.float16: 244, torch.float32: 0}, counts


def test_no_is_not_the_llama_spec():
    """why K1n cannot serve: N5 rounds x * rs to the storage dtype before the gain, NO5 does not — other stored values in the 16-bit dtypes"""
    x, w = _inputs(64, 512, torch.bfloat16, 5)
    h_n = Q.rmsnorm_quantize(to_bits(x), to_bits(w), 1e-6, 0)[2]
    h_o = O.olmo_h(to_bits(x), to_bits(w), 1e-6, 0)
    assert (h_n != h_o).mean() > 0.01
    xf, wf = x.float(), w.float()
    assert np.array_equal(Q.rmsnorm_quantize(to_bits(xf), to_bits(wf), 1e-6, 2)[2], O.olmo_h(to_bits(xf), to_bits(wf), 1e-6, 2))          # f32: the same bits


def test_spec_on_one_hand_computed_row():
    """x = 2 2 2 2, post_eps = 0: mean(x^2) = 4, rs = 1/2;  post_weight = 0 1 -.5 4  ->  p = 0 1 -.5 4;  residual = 1 0 1.5 0  ->  s = 1 1 1 4;  amax 4, scale = 4/127,
    codes = rne(s * 127/4) = rne(31.75 31.75 31.75 127) = 32 32 32 127"""
    for dt in DTYPES:
        x = torch.tensor([[2.0, 2.0, 2.0, 2.0]], dtype=dt)
        pw = torch.tensor([0.0, 1.0, -0.5, 4.0], dtype=dt)
        r = torch.tensor([[1.0, 0.0, 1.5, 0.0]], dtype=dt)
        assert O.rmsnorm(x, pw, 0.0).float().tolist() == [[0.0, 1.0, -0.5, 4.0]]
        assert O.postnorm_add(x, pw, r, 0.0).float().tolist() == [[1.0, 1.0, 1.0, 4.0]]
        q, sc, s = O.postnorm_add_quantize(x, pw, r, 0.0)
        assert O.as_tensor(s, dt).float().tolist() == [[1.0, 1.0, 1.0, 4.0]]
        assert q.tolist() == [[32, 32, 32, 127]] and sc.dtype == np.float32 and sc.tolist() == [float(np.float32(4.0) / np.float32(127.0))]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_k1oq_spec_is_norm_then_add_then_q(dt):
    """the composition identity: K1oq's outputs are NO1-NO5, then A1, then Q1-Q6 — part by part; the storage rounding of p changes stored sums in the 16-bit dtypes and
    nothing in f32; the eps is felt on small rows"""
    g = torch.Generator().manual_seed(19)
    x = (torch.randn(5, 520, generator=g) * torch.tensor([[0.05], [1.0], [20.0], [3.0], [0.3]])).to(dt)
    r = (torch.randn(5, 520, generator=g) * 2).to(dt)
    pw = (0.3 * torch.randn(520, generator=g)).to(dt)
    post_eps = 1e-5
    q, sc, s = O.postnorm_add_quantize(x, pw, r, post_eps)
    p = O.rmsnorm(x, pw, post_eps)
    summed = (r.float() + p.float()).to(dt)
    assert np.array_equal(s, to_bits(summed)) and torch.equal(O.postnorm_add(x, pw, r, post_eps), summed)
    q2, sc2 = Q.quantize(to_bits(summed), Q.dt(O.CODE[dt]), 1)
    assert np.array_equal(q, q2) and np.array_equal(sc, sc2)
    pu = torch.from_numpy(O.unrounded_p(x, pw, post_eps))
    assert torch.equal(pu.to(dt), p)                                                                             # p IS the rounding of that binary32 value
    assert torch.equal(O.unrounded_sum(x, pw, r, post_eps), summed) == (dt == torch.float32)
    x_small = (x.float() * 1e-3).to(dt)
    assert not torch.equal(O.rmsnorm(x_small, pw, 1e-5), O.rmsnorm(x_small, pw, 1e-6))
    if dt != torch.float32:          # on these operands the specified norm is the eager formula in the 16-bit dtypes (the sums differ only below the rounding)
        assert torch.equal(O.olmo_formula(x, pw, post_eps), p)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_nan_inf_and_zero_rows(dt):
    """a NaN in x: the whole row of p and of the sum is NaN, the scale NaN and the codes 0 (QSPEC Q: a NaN propagates); an Inf in x: rs = 0, so p is 0 where x is finite
    and NaN (Inf * 0) where it is not; a zero row with eps > 0: p = 0 and the sum is the residual; a zero row with eps = 0: rs = Inf and p = 0 * Inf = NaN"""
    g = torch.Generator().manual_seed(23)
    x = torch.randn(4, 40, generator=g).to(dt)
    r = torch.randn(4, 40, generator=g).to(dt)
    pw = (0.3 * torch.randn(40, generator=g) + 1.0).to(dt)
    x[0, 7] = float("nan")
    x[1, 9] = float("inf")
    x[2] = 0.0
    q, sc, s = O.postnorm_add_quantize(x, pw, r, 1e-6)
    st = O.as_tensor(s, dt).float()
    assert bool(torch.isnan(st[0]).all()) and np.isnan(sc[0]) and not q[0].any()
    nan1 = torch.isnan(st[1])
    assert nan1.tolist() == [c == 9 for c in range(40)] and torch.equal(st[1][~nan1], r[1].float()[~nan1]) and np.isnan(sc[1])
    assert torch.equal(O.as_tensor(s, dt)[2], r[2]) and np.isfinite(sc[2])
    assert bool(torch.isfinite(st[3]).all()) and np.isfinite(sc[3]) and int(np.abs(q[3].astype(np.int32)).max()) == 127
    assert bool(torch.isnan(O.rmsnorm(x[2:3], pw, 0.0)).all())
