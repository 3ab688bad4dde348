"""-m gpu: fuse_qk_norms on whole Qwen3, Qwen3-MoE and Gemma-3 (text) decoders, held to BITS.  tests/llama_twin.py, tests/gemma_twin.py and tests/moe_models.py build the
tiny models in code.

a. a model after fuse_qk_norms equals a TWIN — a deep copy taken before the call whose q_norm / k_norm are a test-local module that computes the specified norm with the
   library's EXISTING row kernel (rmsnorm_quantize / gemma_rmsnorm_quantize, return_h) on x.reshape(-1, D).contiguous() — bit for bit: logits, every hidden state,
   greedy generation with the KV cache.  Qwen3 at head_dim 64 and 80 (GQA 4 / 2), plain bf16 with nothing else swapped and after swap_linears +
   fuse_llama_layers(fuse_residual=True); Gemma-3 at head_dim 64 after fuse_gemma_layers + fuse_gemma_postnorm_residual; Qwen3-MoE after swap_moe_experts; fp16 and
   f32 once each;
b. the launches of a forward: no eager norm class is called under self_attn, exactly 2L HeadRMSNorm calls are made, and none of them copies its input;
c. the cosine of all logits to the unquantised bf16 model over seeds 0-7, with and without the switch: printed (README carries it), nothing asserted beyond (a)."""
import copy
import importlib

import pytest
import torch
from torch import nn

from tests import gemma_twin as GT
from tests import llama_twin as T
from tests import moe_models as M

pytestmark = pytest.mark.gpu
tr = pytest.importorskip("transformers")

DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    from protoquant_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return protoquant_amd


class TwinHeadNorm(nn.Module):
    """the specified per-head norm by the library's existing one-wave-per-row kernel on the rows copied contiguous, laid out as eager's chain lays its result out"""

    def __init__(self, weight, eps, kind):
        super().__init__()
        self.weight, self.eps, self.kind = nn.Parameter(weight.detach().clone(), requires_grad=False), float(eps), kind

    def forward(self, x):
        from protoquant_amd.qtensor import gemma_rmsnorm_quantize, rmsnorm_quantize
        fn = rmsnorm_quantize if self.kind == "llama" else gemma_rmsnorm_quantize
        h = fn(x.reshape(-1, x.shape[-1]).contiguous(), self.weight, self.eps, return_h=True)[1]
        out = torch.empty_like(x)          # dense, in x's stride order
        out.copy_(h.reshape(x.shape))
        return out


def _attentions(model):
    return [m for m in model.modules() if isinstance(getattr(m, "q_norm", None), nn.Module) and isinstance(getattr(m, "k_norm", None), nn.Module)]


def _twin_and_fused(pq, model, kind, layers):
    """(twin, fused): the twin is a deep copy taken BEFORE fuse_qk_norms; `model` itself is fused in place"""
    from protoquant_amd.olmo import _norm_eps
    tw = copy.deepcopy(model)
    for a in _attentions(tw):
        for n in ("q_norm", "k_norm"):
            old = getattr(a, n)
            assert old.weight.shape == (a.head_dim,)
            setattr(a, n, TwinHeadNorm(old.weight, _norm_eps(old)[1], kind))
    keys = list(model.state_dict())
    assert pq.fuse_qk_norms(model) == 2 * layers and list(model.state_dict()) == keys
    assert all(isinstance(a.q_norm, pq.HeadRMSNorm) and isinstance(a.k_norm, pq.HeadRMSNorm) and a.q_norm.kind == kind for a in _attentions(model))
    return tw, model


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ, max |d| {float((a.float() - b.float()).abs().max())}"


def _equal_to_the_twin(tw, fused, vocab):
    g = torch.Generator().manual_seed(11)
    batches = [torch.randint(3, vocab, s, generator=g).cuda() for s in ((2, 48), (1, 1), (3, 7))]          # 96, 1 and 21 tokens
    for ids in batches:
        with torch.no_grad():
            a, b = tw(ids, output_hidden_states=True), fused(ids, output_hidden_states=True)
        _same_bits(b.logits, a.logits, f"ids {tuple(ids.shape)}: logits")
        assert bool(torch.isfinite(a.logits.float()).all()) and len(a.hidden_states) == len(b.hidden_states)
        for i, (h, hw) in enumerate(zip(b.hidden_states, a.hidden_states)):
            _same_bits(h, hw, f"ids {tuple(ids.shape)}: hidden state {i}")
    with torch.no_grad():          # a prefill and four decode steps against the KV cache
        gen = [m.generate(batches[0][:, :16], max_new_tokens=4, min_new_tokens=4, do_sample=False, use_cache=True, pad_token_id=0) for m in (tw, fused)]
    assert gen[0].shape == (2, 20) and torch.equal(gen[1], gen[0]), "greedy generation differs from the twin's"


def _qwen3(pq, dt, head_dim, fused, layers=2, seed=0):
    b = T.build("qwen3", DT[dt], "aligned", layers=layers, seed=seed, head_dim=head_dim)
    model = b.model
    with torch.no_grad():          # transformers initialises q_norm / k_norm to ones: a gain that matters
        for a in _attentions(model):
            for n in ("q_norm", "k_norm"):
                getattr(a, n).weight.copy_((1 + 0.3 * torch.randn(head_dim)).to(DT[dt]))
    if fused:
        model = pq.swap_linears(model, fuse_gated_mlp=True)
        assert pq.fuse_llama_layers(model, fuse_residual=True) == layers
    return model


def _gemma3(pq, dt, layers=2, seed=0):
    from protoquant_amd.llama import residual_fused_layers
    b = GT.build("gemma3", DT[dt], "aligned", layers=layers, seed=seed)
    model = pq.swap_linears(b.model)
    assert pq.fuse_gemma_layers(model) == layers and pq.fuse_gemma_postnorm_residual(model) == layers and residual_fused_layers(model) == layers
    return model


# ---------------------------------------------------------------------------------------------------------------- a. the twin
CASES_QWEN3 = [("bf16", 64, False), ("bf16", 80, False), ("bf16", 64, True), ("bf16", 80, True), ("fp16", 64, True), ("f32", 80, False)]


@pytest.mark.parametrize("dt,head_dim,fused", CASES_QWEN3, ids=[f"{d}-hd{h}-{'int8-residual-fused' if f else 'plain'}" for d, h, f in CASES_QWEN3])
def test_qwen3_equals_the_twin_bit_for_bit(pq, dt, head_dim, fused):
    layers = 3 if head_dim == 80 else 2
    model = _qwen3(pq, dt, head_dim, fused, layers=layers)
    tw, fz = _twin_and_fused(pq, model, "llama", layers)
    _equal_to_the_twin(tw, fz, T.VOCAB)


def test_gemma3_sandwich_fused_equals_the_twin_bit_for_bit(pq):
    model = _gemma3(pq, "bf16", layers=3)
    tw, fz = _twin_and_fused(pq, model, "gemma", 3)
    _equal_to_the_twin(tw, fz, GT.VOCAB)


def test_qwen3_moe_after_swap_moe_experts_equals_the_twin_bit_for_bit(pq):
    if not hasattr(tr, "Qwen3MoeConfig"):
        pytest.skip("the installed transformers has no Qwen3-MoE")
    model = M.build("qwen3_moe", seed=0, H=256, I=384, E=8, k=2)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for _, blk in M.sparse_blocks(model):
            blk.experts.gate_up_proj.normal_(0, 0.05, generator=g); blk.experts.down_proj.normal_(0, 0.05, generator=g)
        for a in _attentions(model):
            for n in ("q_norm", "k_norm"):
                getattr(a, n).weight.copy_(1 + 0.3 * torch.randn(a.head_dim, generator=g))
    model = model.to(torch.bfloat16).cuda().eval()
    assert pq.swap_moe_experts(model) == 2
    tw, fz = _twin_and_fused(pq, model, "llama", 2)
    _equal_to_the_twin(tw, fz, M.VOCAB)


# ---------------------------------------------------------------------------------------------------------------- b. the launches of a forward
def _count(monkeypatch, model):
    """per forward: calls of stock *RMSNorm modules under self_attn (the eager chains), calls of HeadRMSNorm, and what the stride collapse of every head_rmsnorm gave"""
    import protoquant_amd as pq
    QT = importlib.import_module("protoquant_amd.qtensor")
    counts = {"eager": 0, "head": 0, "plans": []}
    real = QT._collapse_heads

    def collapse(shape, strides):
        plan = real(shape, strides)
        counts["plans"].append(plan)
        return plan
    monkeypatch.setattr(QT, "_collapse_heads", collapse)
    for a in _attentions(model):
        for n, mod in a.named_modules():
            if isinstance(mod, pq.HeadRMSNorm):
                mod.register_forward_hook(lambda m, i, o: counts.__setitem__("head", counts["head"] + 1))
            elif "norm" in type(mod).__name__.lower():
                mod.register_forward_hook(lambda m, i, o: counts.__setitem__("eager", counts["eager"] + 1))
    return counts


@pytest.mark.parametrize("family", ["qwen3-plain", "qwen3-fused", "gemma3"])
def test_launch_counts(pq, monkeypatch, family):
    L = 4
    model = _gemma3(pq, "bf16", layers=L, seed=1) if family == "gemma3" else _qwen3(pq, "bf16", 64, family == "qwen3-fused", layers=L, seed=1)
    assert pq.fuse_qk_norms(model) == 2 * L
    counts = _count(monkeypatch, model)
    for shape in ((1, 40), (2, 1)):          # a prefill and a decode-sized batch
        counts.update(eager=0, head=0, plans=[])
        with torch.no_grad():
            model(torch.randint(3, T.VOCAB, shape, device="cuda"))
        assert counts["eager"] == 0 and counts["head"] == 2 * L, counts
        assert len(counts["plans"]) == 2 * L and all(p is not None for p in counts["plans"]), f"a head_rmsnorm copied its input: {counts['plans']}"
        if family != "qwen3-plain":          # column slices of the fused q/k/v output: (tokens, its leading dimension) x (heads, D)
            tokens = shape[0] * shape[1]
            assert all(p[0] * p[2] in (tokens * 4, tokens * 2) and p[3] == 64 for p in counts["plans"]), counts["plans"]
            if tokens > 1:
                assert all(p[1] == (4 + 2 + 2) * 64 for p in counts["plans"]), counts["plans"]


# ---------------------------------------------------------------------------------------------------------------- c. against the unquantised model
SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)


@pytest.mark.parametrize("family", ["qwen3", "gemma3"])
def test_cosine_of_all_logits_to_the_unquantised_model(pq, family):
    """Per seed (2 layers, `aligned`, bf16, ids [2, 96]): the cosine of all logits of the unquantised bf16 model to the int8 model without fuse_qk_norms (eager q / k
    norms) and with it (QSPEC HN1).  The switch replaces the eager chain by the specified norm, which differs from it only by the pinned summation order and the IEEE
    square root.  Printed for the README; nothing is asserted about it beyond finiteness — the bits are held by the twin tests above."""
    rows = []
    for seed in SEEDS:
        if family == "qwen3":
            b = T.build("qwen3", torch.bfloat16, "aligned", layers=2, seed=seed)
            ref = copy.deepcopy(b.model)
            without = pq.swap_linears(b.model, fuse_gated_mlp=True)
            assert pq.fuse_llama_layers(without, fuse_residual=True) == 2
        else:
            b = GT.build("gemma3", torch.bfloat16, "aligned", layers=2, seed=seed)
            ref = copy.deepcopy(b.model)
            without = pq.swap_linears(b.model)
            assert pq.fuse_gemma_layers(without) == 2 and pq.fuse_gemma_postnorm_residual(without) == 2
        with_ = copy.deepcopy(without)
        assert pq.fuse_qk_norms(with_) == 4
        ids = torch.randint(0, T.VOCAB, (2, 96), generator=torch.Generator().manual_seed(5)).cuda()
        with torch.no_grad():
            a, u, f = (m(ids).logits.float().flatten() for m in (ref, without, with_))
        cos = lambda p, q: float(torch.dot(p, q) / (p.norm() * q.norm()))          # noqa: E731
        rows.append((seed, cos(a, u), cos(a, f)))
    for seed, cu, cf in rows:
        print(f"{family} seed {seed}: cosine of all logits to the unquantised bf16 model: without fuse_qk_norms {cu:.6f}, with {cf:.6f}")
    assert all(cu == cu and cf == cf for _, cu, cf in rows)
