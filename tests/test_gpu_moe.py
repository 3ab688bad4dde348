"""-m gpu: the mixture-of-experts modules (protoquant_amd.moe) against the eager per-expert loop over GatedMLP modules with the index_add_ combine — bit for bit."""
import copy
import os
import tempfile

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu


def _same(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{what}: {int((a.view(torch.int16) != b.view(torch.int16)).sum())} of {a.numel()} elements differ"


def _expert_linears(E, H, I, seed, dtype=torch.bfloat16):
    torch.manual_seed(seed)
    return [tuple(nn.Linear(i, o, bias=False, dtype=dtype, device="cuda") for (i, o) in ((H, I), (H, I), (I, H))) for _ in range(E)]


def _eager_loop(mlps, x, ids, w):
    """the reference: Mixtral's loop over the experts, each a per-expert GatedMLP (which quantises the rows it is handed), index_add_ into zeros"""
    final = torch.zeros_like(x)
    mask = torch.nn.functional.one_hot(ids, num_classes=len(mlps)).permute(2, 1, 0)
    for e, mlp in enumerate(mlps):
        slot, tok = torch.where(mask[e])
        if tok.numel() == 0:
            continue
        out = mlp(x[tok]) * w[tok, slot, None]
        final.index_add_(0, tok, out.to(x.dtype))
    return final


def _routing(T, E, k, kind, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    logits = torch.randn(T, E, generator=g, device="cuda")
    if kind == "skewed":
        logits = logits + torch.linspace(3, -3, E, device="cuda")[None, :]
    wts, ids = torch.topk(torch.softmax(logits, dim=1), k, dim=-1)
    return ids, (wts / wts.sum(dim=-1, keepdim=True)).to(torch.bfloat16)


@pytest.mark.parametrize("kind", ("balanced", "skewed"))
@pytest.mark.parametrize("k", (1, 2, 8))
def test_moe_gated_mlp_equals_eager_per_expert_loop(k, kind):
    import protoquant_amd as pq
    E, H, I, T = 16, 256, 384, 200
    lins = _expert_linears(E, H, I, 1)
    mlps = [pq.GatedMLP.from_linears(*l) for l in lins]
    moe = pq.MoEGatedMLP.from_experts(mlps)
    x = (torch.randn(T, H, device="cuda") * 1.5).to(torch.bfloat16)
    ids, w = _routing(T, E, k, kind, 10 * k)
    w[3] = 0                                                   # a token routed nowhere useful
    _same(moe(x, ids, w), _eager_loop(mlps, x, ids, w), f"k={k} {kind}")
    x3 = x.reshape(4, 50, H)                                   # 3-D hidden input
    _same(moe(x3, ids.reshape(4, 50, k), w.reshape(4, 50, k)).reshape(T, H), _eager_loop(mlps, x, ids, w), "3-D")


def test_padded_k_experts():
    """hidden and intermediate sizes that are not multiples of 128: zero-padded weights and codes, same bits"""
    import protoquant_amd as pq
    E, H, I, T, k = 4, 200, 72, 90, 2
    mlps = [pq.GatedMLP.from_linears(*l) for l in _expert_linears(E, H, I, 2)]
    x = torch.randn(T, H, device="cuda").to(torch.bfloat16)
    ids, w = _routing(T, E, k, "balanced", 3)
    _same(pq.MoEGatedMLP.from_experts(mlps)(x, ids, w), _eager_loop(mlps, x, ids, w), "padded K")


def test_grouped_qlinear_constructors_agree():
    import protoquant_amd as pq
    torch.manual_seed(4)
    lins = [nn.Linear(256, 96, bias=True, dtype=torch.bfloat16, device="cuda") for _ in range(5)]
    a = pq.GroupedQLinear.from_linears(lins)
    b = pq.GroupedQLinear.from_weight(torch.stack([l.weight for l in lins]), torch.stack([l.bias for l in lins]))
    c = pq.GroupedQLinear.from_linears([pq.qlinear.from_linear(l) for l in lins])
    for other in (b, c):
        assert torch.equal(a.wq, other.wq) and torch.equal(a.ws, other.ws) and torch.equal(a.bias, other.bias)
    assert a.wq.shape == (5, 96, 256) and a.ws.shape == (5, 96)


class _MixtralExpert(nn.Module):
    def __init__(self, H, I):
        super().__init__()
        self.w1, self.w3, self.w2 = nn.Linear(H, I, bias=False), nn.Linear(H, I, bias=False), nn.Linear(I, H, bias=False)
        self.act_fn = nn.SiLU()

    def forward(self, x):
        return self.w2(self.act_fn(self.w1(x)) * self.w3(x))


class _LlamaExpert(nn.Module):
    def __init__(self, H, I):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj = nn.Linear(H, I, bias=False), nn.Linear(H, I, bias=False), nn.Linear(I, H, bias=False)
        self.act_fn = nn.SiLU()

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


class _SparseMoeBlock(nn.Module):
    """Mixtral's block, as its model code writes it"""

    def __init__(self, expert_cls, E, H, I, top_k):
        super().__init__()
        self.top_k = top_k
        self.gate = nn.Linear(H, E, bias=False)
        self.experts = nn.ModuleList([expert_cls(H, I) for _ in range(E)])

    def forward(self, hidden_states):
        b, s, h = hidden_states.shape
        x = hidden_states.view(-1, h)
        router_logits = self.gate(x)
        w = torch.softmax(router_logits, dim=1, dtype=torch.float)
        w, sel = torch.topk(w, self.top_k, dim=-1)
        w = (w / w.sum(dim=-1, keepdim=True)).to(x.dtype)
        final = torch.zeros_like(x)
        mask = torch.nn.functional.one_hot(sel, num_classes=len(self.experts)).permute(2, 1, 0)
        for e, expert in enumerate(self.experts):
            slot, tok = torch.where(mask[e])
            if tok.numel():
                final.index_add_(0, tok, (expert(x[tok]) * w[tok, slot, None]).to(x.dtype))
        return final.reshape(b, s, h), router_logits


class _Model(nn.Module):
    def __init__(self, expert_cls):
        super().__init__()
        self.block = _SparseMoeBlock(expert_cls, 8, 256, 128, 2)


def _per_expert_swapped(model):
    """every expert replaced by a per-expert GatedMLP, the block's own loop kept"""
    import protoquant_amd as pq
    m = copy.deepcopy(model)
    for i, ex in enumerate(m.block.experts):
        names = ("w1", "w3", "w2") if hasattr(ex, "w1") else ("gate_proj", "up_proj", "down_proj")
        m.block.experts[i] = pq.GatedMLP.from_linears(*(getattr(ex, n) for n in names))
    return m


@pytest.mark.parametrize("expert_cls", (_MixtralExpert, _LlamaExpert))
def test_swap_moe_experts_equals_per_expert_swapped_block(expert_cls):
    import protoquant_amd as pq
    torch.manual_seed(6)
    model = _Model(expert_cls).to(device="cuda", dtype=torch.bfloat16)
    ref = _per_expert_swapped(model)
    assert pq.swap_moe_experts(model) == 1 and isinstance(model.block, pq.MoEBlock)
    x = torch.randn(2, 75, 256, device="cuda").to(torch.bfloat16)
    (got, got_logits), (want, want_logits) = model.block(x), ref.block(x)
    _same(got_logits, want_logits, "router logits")
    _same(got, want, "block output")


def test_swap_moe_experts_leaves_a_dense_model_alone():
    import protoquant_amd as pq
    dense = nn.Sequential(nn.Linear(64, 64), nn.SiLU(), nn.Linear(64, 64)).cuda()
    before = [type(m) for m in dense.modules()]
    assert pq.swap_moe_experts(dense) == 0
    assert [type(m) for m in dense.modules()] == before


def test_serialisation_round_trip():
    """state_dict of a swapped model -> save_quantized -> a fresh float model prepared WITHOUT its weights -> same outputs"""
    import protoquant_amd as pq
    from protoquant_amd import serialize as S
    torch.manual_seed(8)
    model = _Model(_MixtralExpert).to(device="cuda", dtype=torch.bfloat16)
    pq.swap_moe_experts(model)
    x = torch.randn(1, 40, 256, device="cuda").to(torch.bfloat16)
    want, _ = model.block(x)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "moe.safetensors")
        S.save_quantized({k: v.cpu() for k, v in model.state_dict().items()}, path)
        sd = S.load_quantized(path)
    with torch.device("meta"):
        fresh = _Model(_MixtralExpert).to(torch.bfloat16)
    fresh.block.gate = nn.Linear(256, 8, bias=False, dtype=torch.bfloat16)      # (the router stays a float layer and comes with the checkpoint)
    fresh = S.prepare_for_int8(fresh, predicate=lambda name, mod: not isinstance(mod, nn.Linear))
    assert isinstance(fresh.block, pq.MoEBlock)
    fresh.load_state_dict(sd)
    got, _ = fresh.cuda().block(x)
    _same(got, want, "round trip")
