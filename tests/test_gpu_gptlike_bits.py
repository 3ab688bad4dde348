"""-m gpu: whole LayerNorm-family decoders after fuse_layernorm_layers, held to bits.  A tiny random-init GPT-2 / StarCoder2 / GPT-NeoX (both residual settings) is swapped
(swap_linears) and fused; its TWIN is the same swapped model whose LayerNorms and activations — exactly the ones the fused model replaced — are the CPU SPECIFICATION
(tests/lnorm_spec.py, tests/act_spec.py) storing h in the model dtype, followed by the projections' own quantize().  QSPEC L6 / U4 say the fused kernels' codes are Q1-Q6
on those stored rows, so logits, every hidden state and greedy generation with the KV cache must be torch.equal — in bf16 and fp16, at a hidden size that is a multiple of
128 and one that is not.  The library calls of one forward are counted (every fused norm and activation is one call that replaces a torch op AND the K1 launch inside the
projection it feeds), and the cosine of the logits to the unquantised model is recorded."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from tests import act_spec as AS
from tests import gptlike_models as G
from tests import lnorm_spec as LS

pytestmark = pytest.mark.gpu

CODE = {torch.bfloat16: 0, torch.float16: 1}


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    from protoquant_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return protoquant_amd


def _store(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16).copy()


def _load(a, like):
    return torch.from_numpy(a.view(np.int16)).view(like.dtype).reshape(like.shape).to(like.device)


class SpecLayerNorm(nn.Module):
    def __init__(self, ln):
        super().__init__()
        self.weight, self.bias, self.eps = ln.weight, ln.bias, ln.eps

    def forward(self, x):
        h, _, _ = LS.layernorm(_store(x.reshape(-1, x.shape[-1])), _store(self.weight), None if self.bias is None else _store(self.bias), self.eps, CODE[x.dtype])
        return _load(h, x)


class SpecAct(nn.Module):
    def __init__(self, kind):
        super().__init__()
        self.kind = kind

    def forward(self, x):
        return _load(AS.act(_store(x.reshape(-1, x.shape[-1])), CODE[x.dtype], self.kind), x)


def _pair(pq, family, dtype, hidden, with_llama=None):
    base = G.build(family, hidden=hidden).to(dtype).cuda()
    with torch.no_grad():
        for m in base.modules():
            if isinstance(m, nn.LayerNorm):
                m.weight.copy_((1 + 0.2 * torch.randn(m.weight.shape)).to(dtype))
                m.bias.copy_((0.2 * torch.randn(m.bias.shape)).to(dtype))
    swapped = pq.swap_linears(copy.deepcopy(base))
    fused = copy.deepcopy(swapped)
    if with_llama == "first":
        pq.fuse_llama_layers(fused)
    n = pq.fuse_layernorm_layers(fused)
    if with_llama == "after":
        pq.fuse_llama_layers(fused)
    assert n == 2
    twin = copy.deepcopy(swapped)
    fm, tm = dict(fused.named_modules()), dict(twin.named_modules())
    nrepl = 0
    for name, m in fm.items():
        if isinstance(m, (pq.LayerNormQuant, pq.ActQuant)):
            parent, attr = name.rsplit(".", 1)
            setattr(tm[parent], attr, SpecLayerNorm(m) if isinstance(m, pq.LayerNormQuant) else SpecAct(m.kind))
            nrepl += 1
    assert nrepl == 2 * 3
    return base, swapped, fused, twin


CASES = [("gpt2", None), ("starcoder2", None), ("starcoder2", "first"), ("starcoder2", "after"), ("gpt_neox", None), ("gpt_neox_seq", None)]


@pytest.mark.parametrize("family,with_llama", CASES, ids=[f"{a}-{b}" for a, b in CASES])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("hidden", [128, 96])
def test_fused_models_equal_the_spec_twin_bit_for_bit(pq, family, with_llama, dtype, hidden):
    base, swapped, fused, twin = _pair(pq, family, dtype, hidden, with_llama)
    g = torch.Generator().manual_seed(hidden)
    ids = torch.randint(3, 128, (2, 11), generator=g).cuda()
    with torch.no_grad():
        of = fused(input_ids=ids, output_hidden_states=True, use_cache=False)
        ot = twin(input_ids=ids, output_hidden_states=True, use_cache=False)
        assert torch.equal(of.logits, ot.logits), f"logits differ in {int((of.logits != ot.logits).sum())} places"
        assert len(of.hidden_states) == len(ot.hidden_states) == 3
        for i, (a, b) in enumerate(zip(of.hidden_states, ot.hidden_states)):
            assert torch.equal(a, b), f"hidden state {i} differs"
        gf = fused.generate(ids[:1, :5], max_new_tokens=6, do_sample=False, use_cache=True, pad_token_id=0)
        gt = twin.generate(ids[:1, :5], max_new_tokens=6, do_sample=False, use_cache=True, pad_token_id=0)
        assert torch.equal(gf, gt)
        ob = base(input_ids=ids, use_cache=False)
    cos = torch.nn.functional.cosine_similarity(of.logits.float().flatten(), ob.logits.float().flatten(), dim=0).item()
    print(f"COSINE {family} {with_llama} {dtype} hidden={hidden}: fused vs unquantised logits {cos:.5f}")
    assert cos >= 0.99, cos


@pytest.mark.parametrize("family", ["gpt2", "gpt_neox"])
def test_library_calls_of_one_forward(pq, family):
    """per layer, unfused: four qlinear_dyn calls (K1 + GEMM each).  Fused: two layernorm_quant calls, one act_quant call, three GEMM-only qlinear_s8 calls (the
    projections that now receive a QTensor) and ONE qlinear_dyn (the attention's output projection): the two torch LayerNorms and the torch activation are gone and
    three K1 launches with them."""
    from protoquant_amd import _lib
    _, swapped, fused, _ = _pair(pq, family, torch.bfloat16, 128)
    L = _lib.lib()
    names = ("pq_qlinear_dyn", "pq_qlinear_s8", "pq_layernorm_quant_rowwise", "pq_act_quant_rowwise", "pq_quant_rowwise")
    ids = torch.randint(3, 128, (1, 9)).cuda()

    def count(model):
        calls = dict.fromkeys(names, 0)
        orig = {n: getattr(L, n) for n in names}

        def wrap(n):
            def f(*a):
                calls[n] += 1
                return orig[n](*a)
            return f
        try:
            for n in names:
                setattr(L, n, wrap(n))
            with torch.no_grad():
                model(input_ids=ids, use_cache=False)
        finally:
            for n in names:
                setattr(L, n, orig[n])
        return calls
    cu, cf = count(swapped), count(fused)
    layers = 2
    assert cu["pq_layernorm_quant_rowwise"] == 0 and cu["pq_act_quant_rowwise"] == 0
    assert cf["pq_layernorm_quant_rowwise"] == 2 * layers and cf["pq_act_quant_rowwise"] == layers
    dyn = lambda c: c["pq_qlinear_dyn"] + c["pq_quant_rowwise"]          # noqa: E731  (activations quantised by K1)
    assert dyn(cu) - dyn(cf) == 3 * layers, (cu, cf)
    assert cf["pq_qlinear_s8"] - cu["pq_qlinear_s8"] == 3 * layers, (cu, cf)
