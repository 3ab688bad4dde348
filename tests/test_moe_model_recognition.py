"""Which mixture-of-experts layouts of real model code the library recognises (protoquant_amd.moe.fused_experts_parts / moe_block_parts) and which it refuses: no GPU,
no library call — tiny transformers models built from a config on the CPU, and the table of tests/moe_models.py.  "Refused" means the recognisers return None,
swap_moe_experts returns 0 and every module object is the very same object afterwards."""
import pytest
import torch
from torch import nn

tr = pytest.importorskip("transformers")

from protoquant_amd import moe                       # noqa: E402
from protoquant_amd import serialize as S            # noqa: E402
from protoquant_amd.qlinear import is_plain_linear   # noqa: E402
from tests import moe_models as M                    # noqa: E402


def _recognised(model):
    return {n: moe.fused_experts_parts(m) for n, m in model.named_modules() if moe.fused_experts_parts(m) is not None}


def _untouched_by_swap(model):
    before = [(n, id(m)) for n, m in model.named_modules()]
    assert moe.swap_moe_experts(model) == 0
    S.prepare_for_int8(model, predicate=lambda name, mod: not isinstance(mod, nn.Linear))      # (the MoE half of prepare_for_int8 alone)
    assert [(n, id(m)) for n, m in model.named_modules()] == before


# H = 2 I is the trap shape: a transposed [E, H, 2 I] gate_up_proj has the shape of [E, 2 I, H]
SHAPES = ((64, 128, 4, 2), (64, 32, 4, 2), (64, 128, 1, 1), (64, 128, 4, 4))


# (DeepSeek-V3's grouped router takes the top 2 of every group: it has no one-expert model)
@pytest.mark.parametrize("family,H,I,E,k", [(f, *s) for f in M.SWAPPED for s in SHAPES if not (f == "deepseek_v3" and s[2] == 1)])
def test_fused_experts_of_every_sparse_layer_are_recognised(family, H, I, E, k):
    model = M.build(family, H=H, I=I, E=E, k=k)
    blocks = M.sparse_blocks(model)
    assert len(blocks) == (1 if family == "deepseek_v3" else 2)            # (first_k_dense_replace = 1: DeepSeek's first layer is dense)
    found = _recognised(model)
    assert set(found) == {n + ".experts" for n, _ in blocks}
    for parts in found.values():
        assert parts == moe.FusedExperts(num_experts=E, hidden=H, intermediate=I, gate_up_bias=False, down_bias=False, gate_first=True)
    assert all(moe.moe_block_parts(m) is None for m in model.modules())     # and nothing is taken for the ModuleList layout


@pytest.mark.parametrize("family", M.SWAPPED)
def test_reported_gate_before_up_order_is_the_models_arithmetic(family):
    """what FusedExperts says — gate rows first, y = x @ W[e].T — restated in float64 from the two parameters alone, against the module's own forward"""
    torch.manual_seed(3)
    model = M.build(family, H=64, I=32, E=4, k=2).double()                    # H = 2 I: a transposed or interleaved reading has the same shapes
    name, block = M.sparse_blocks(model)[-1]
    ex, parts = block.experts, moe.fused_experts_parts(block.experts)
    with torch.no_grad():
        ex.gate_up_proj.normal_(0, 0.2); ex.down_proj.normal_(0, 0.2)
        x = torch.randn(10, parts.hidden, dtype=torch.float64)
        ids = torch.stack([torch.randperm(parts.num_experts)[:2] for _ in range(10)])
        w = torch.rand(10, 2, dtype=torch.float64)
        want = torch.zeros_like(x)
        I = parts.intermediate
        for t in range(10):
            for j in range(2):
                gu = ex.gate_up_proj[ids[t, j]] @ x[t]
                gate, up = (gu[:I], gu[I:]) if parts.gate_first else (gu[I:], gu[:I])
                want[t] += w[t, j] * (ex.down_proj[ids[t, j]] @ (torch.nn.functional.silu(gate) * up))
        got = ex(x, ids, w)
    assert torch.allclose(got, want, rtol=1e-9, atol=1e-9), float((got - want).abs().max())


def test_qwen2_moe_keeps_its_shared_expert():
    """only `experts` is recognised in a Qwen2-MoE block: with a stand-in of MoEGatedMLP's signature in its place, the block still adds its gated shared expert"""
    model = M.build("qwen2_moe", decoder_sparse_step=2, layers=4, mlp_only_layers=[3])
    blocks = M.sparse_blocks(model)
    assert [n for n, _ in blocks] == ["model.layers.1.mlp"]                   # layers 0 and 2 are dense by the step, layer 3 by mlp_only_layers
    assert set(_recognised(model)) == {"model.layers.1.mlp.experts"}
    block = blocks[0][1]
    shared, shared_gate = block.shared_expert, block.shared_expert_gate
    seen = []

    class Stand(nn.Module):
        def forward(self, hidden, top_k_index, top_k_weights):
            seen.append((tuple(hidden.shape), tuple(top_k_index.shape), tuple(top_k_weights.shape)))
            return torch.zeros_like(hidden)

    block.experts = Stand()
    x = torch.randn(2, 5, 64)
    with torch.no_grad():
        out = block(x)
        want = torch.sigmoid(shared_gate(x)) * shared(x)
    assert seen == [((10, 64), (10, 2), (10, 2))]
    assert block.shared_expert is shared and block.shared_expert_gate is shared_gate and torch.allclose(out, want, atol=1e-6)
    assert isinstance(out, torch.Tensor)


def test_deepseek_v3_is_recognised_at_the_experts_module_only():
    model = M.build("deepseek_v3")
    (name, block), = M.sparse_blocks(model)
    assert set(_recognised(model)) == {name + ".experts"}
    assert moe.fused_experts_parts(block) is None and moe.fused_experts_parts(block.gate) is None and moe.fused_experts_parts(block.shared_experts) is None
    S.prepare_for_int8(model, predicate=lambda n, m: not isinstance(m, nn.Linear))
    assert isinstance(block.experts, moe.MoEGatedMLP) and type(block.gate).__name__ == "DeepseekV3TopkRouter" and type(block.shared_experts).__name__ == "DeepseekV3MLP"


@pytest.mark.parametrize("H,I", ((64, 128), (64, 32)))
def test_gpt_oss_is_refused(H, I):
    model = M.build("gpt_oss", H=H, I=I)
    ex = model.model.layers[0].mlp.experts
    assert tuple(ex.gate_up_proj.shape) == (4, H, 2 * I) and ex.gate_up_proj_bias is not None
    assert not _recognised(model)
    _untouched_by_swap(model)


@pytest.mark.parametrize("H,I", ((64, 128), (64, 32)))
def test_deepseek_v4_is_refused_for_the_clamp_in_its_own_gate(H, I):
    """DeepseekV4Experts is MixtralExperts to every shape, flag and name; only its class-level _apply_gate says that gate and up are clamped to +-swiglu_limit"""
    model = M.build("deepseek_v4", H=H, I=I)
    blocks = M.sparse_blocks(model)
    assert len(blocks) == 2
    ex = blocks[0][1].experts
    assert type(ex).__name__ == "DeepseekV4Experts" and tuple(ex.gate_up_proj.shape) == (4, 2 * I, H) and tuple(ex.down_proj.shape) == (4, H, I)
    assert type(ex)._apply_gate.__name__ == "_apply_gate" and type(M.build("mixtral").model.layers[0].mlp.experts)._apply_gate.__name__ == "_default_apply_gate"
    # the clamp is live arithmetic: beyond the limit the module's output is not that of silu(gate) * up
    with torch.no_grad():
        ex.gate_up_proj.fill_(1.0); ex.down_proj.fill_(1.0)
        x, ids, w = torch.full((1, H), 4.0), torch.tensor([[0, 1]]), torch.ones(1, 2)
        clamped = ex(x, ids, w)
        ex.limit = 1e30
        assert not torch.allclose(ex(x, ids, w), clamped)
    assert not _recognised(model)
    _untouched_by_swap(model)


@pytest.mark.parametrize("family", ("mixtral", "phimoe", "granitemoe", "qwen3_moe"))
def test_an_activation_that_is_not_silu_is_refused(family):
    model = M.build(family, act="gelu")
    assert M.sparse_blocks(model) and not _recognised(model)
    _untouched_by_swap(model)


class _Experts(nn.Module):
    """a fused-parameter experts module written out here, to vary one property at a time"""

    def __init__(self, gu_shape, dn_shape, act=nn.SiLU, **flags):
        super().__init__()
        self.gate_up_proj, self.down_proj = nn.Parameter(torch.zeros(gu_shape)), nn.Parameter(torch.zeros(dn_shape))
        if act is not None:
            self.act_fn = act()
        for k, v in flags.items():
            setattr(self, k, v)

    def forward(self, hidden_states, top_k_index, top_k_weights):
        raise NotImplementedError


class _WeightsFirst(_Experts):
    def forward(self, hidden_states, top_k_weights, top_k_index):
        raise NotImplementedError


class _HiddenOnly(_Experts):
    def forward(self, hidden_states):
        raise NotImplementedError


class _OwnGate(_Experts):
    def _apply_gate(self, gate_up):
        gate, up = gate_up.chunk(2, dim=-1)
        return self.act_fn(gate.clamp(max=7.0)) * up


def _default_apply_gate(self, gate_up):
    gate, up = gate_up.chunk(2, dim=-1)
    return self.act_fn(gate) * up


class _DefaultGate(_Experts):
    """what transformers' decorator leaves on a class that has no gate of its own"""
    _apply_gate = _default_apply_gate


def test_look_alike_experts_one_property_at_a_time():
    E, H, I = 4, 64, 32                                                   # H = 2 I throughout
    ok = _Experts((E, 2 * I, H), (E, H, I))
    assert moe.fused_experts_parts(ok) == moe.FusedExperts(E, H, I, False, False, True)
    assert moe.fused_experts_parts(_Experts((E, 2 * I, H), (E, H, I), is_transposed=False, is_concatenated=True, has_bias=False, has_gate=True, num_experts=E)) is not None
    assert moe.fused_experts_parts(_DefaultGate((E, 2 * I, H), (E, H, I))) is not None
    refused = {
        "transposed storage, told by down_proj alone": _Experts((E, H, 2 * I), (E, I, H)),
        "transposed storage, told by the flag alone": _Experts((E, 2 * I, H), (E, H, I), is_transposed=True),
        "interleaved gate / up columns": _Experts((E, 2 * I, H), (E, H, I), is_concatenated=False),
        "biases announced": _Experts((E, 2 * I, H), (E, H, I), has_bias=True),
        "no gate": _Experts((E, 2 * I, H), (E, H, I), has_gate=False),
        "no activation": _Experts((E, 2 * I, H), (E, H, I), act=None),
        "gelu": _Experts((E, 2 * I, H), (E, H, I), act=nn.GELU),
        "2-D parameters": _Experts((2 * I, H), (H, I)),
        "gate_up is not twice down's width": _Experts((E, 3 * I, H), (E, H, I)),
        "experts counts differ": _Experts((E, 2 * I, H), (E + 1, H, I)),
        "another number of experts announced": _Experts((E, 2 * I, H), (E, H, I), num_experts=E + 1),
        "weights before indices": _WeightsFirst((E, 2 * I, H), (E, H, I)),
        "forward takes the hidden states only": _HiddenOnly((E, 2 * I, H), (E, H, I)),
        "its own _apply_gate": _OwnGate((E, 2 * I, H), (E, H, I)),
    }
    extra = _Experts((E, 2 * I, H), (E, H, I))
    extra.gate_up_proj_bias = nn.Parameter(torch.zeros(E, 2 * I))
    refused["a third parameter"] = extra
    buf = _Experts((E, 2 * I, H), (E, H, I))
    buf.register_buffer("scale", torch.ones(E))
    refused["a buffer"] = buf
    child = _Experts((E, 2 * I, H), (E, H, I))
    child.norm = nn.LayerNorm(H)
    refused["a child module besides the activation"] = child
    for why, mod in refused.items():
        assert moe.fused_experts_parts(mod) is None, why
        holder = nn.ModuleDict({"experts": mod})
        assert moe.swap_moe_experts(holder) == 0 and holder["experts"] is mod, why


@pytest.mark.parametrize("names", (("gate_proj", "up_proj", "down_proj"), ("w1", "w3", "w2")))
def test_the_module_list_layout_is_recognised_as_before(names):
    blk = M.ListMoeBlock(4, 64, 128, 2, names=names)
    parts = moe.moe_block_parts(blk)
    assert parts is not None
    lins, top_k, renorm, returns_logits = parts
    assert len(lins) == 4 and top_k == 2 and renorm is True and returns_logits is False
    assert all(g is getattr(ex, names[0]) and u is getattr(ex, names[1]) and d is getattr(ex, names[2]) for (g, u, d), ex in zip(lins, blk.experts))
    assert moe.fused_experts_parts(blk) is None and moe.fused_experts_parts(blk.experts) is None
    assert moe.moe_block_parts(M.ListMoeBlock(4, 64, 128, 2, norm_topk_prob=False))[2] is False
    fresh = S.prepare_for_int8(nn.ModuleDict({"mlp": blk}), predicate=lambda n, m: not isinstance(m, nn.Linear))
    assert isinstance(fresh["mlp"], moe.MoEBlock) and fresh["mlp"].gate is blk.gate and tuple(fresh["mlp"].experts.gate_up.wq.shape) == (4, 256, 64)


def test_a_router_that_overrides_linear_forward_is_no_router_of_the_module_list_layout():
    class Router(nn.Linear):
        def forward(self, x):
            logits = super().forward(x)
            return logits, logits, logits

    blk = M.ListMoeBlock(4, 64, 128, 2)
    blk.gate = Router(64, 4, bias=False)
    assert moe.moe_block_parts(blk) is None


def test_a_dense_llama_has_nothing_to_swap():
    model = M.build("llama")
    assert not _recognised(model) and not M.sparse_blocks(model)
    _untouched_by_swap(model)


def test_phimoe_router_is_not_a_linear_layer():
    """PhimoeTopKRouter subclasses nn.Linear and returns (logits, weights, indices): qlinear in its place would return one tensor"""
    model = M.build("phimoe")
    router = model.model.layers[0].mlp.router
    assert isinstance(router, nn.Linear) and not is_plain_linear(router)
    assert is_plain_linear(model.model.layers[0].self_attn.q_proj) and is_plain_linear(model.lm_head)
    S.prepare_for_int8(model)
    from protoquant_amd import qlinear
    assert model.model.layers[0].mlp.router is router and isinstance(model.model.layers[0].self_attn.q_proj, qlinear)
    assert isinstance(model.model.layers[0].mlp.experts, moe.MoEGatedMLP)


def test_prepare_for_int8_on_a_meta_mixtral_names_the_serialised_tensors():
    with torch.device("meta"):
        model = tr.AutoModelForCausalLM.from_config(M.config("mixtral", H=64, I=128, E=4, k=2)).to(torch.bfloat16)
    S.prepare_for_int8(model)
    sd = model.state_dict()
    p = "model.layers.1.mlp."
    assert not any(k.endswith("gate_up_proj") or k.endswith("down_proj") for k in sd)
    assert sd[p + "experts.gate_up.wq"].shape == (4, 256, 64) and sd[p + "experts.gate_up.wq"].dtype == torch.int8 and sd[p + "experts.gate_up.ws"].shape == (4, 256)
    assert sd[p + "experts.down.wq"].shape == (4, 64, 128) and sd[p + "experts.down.ws"].dtype == torch.float32 and sd[p + "experts.down.wq"].device.type == "cpu"
    assert sd[p + "gate.weight"].shape == (4, 64) and type(model.model.layers[1].mlp.gate).__name__ == "MixtralTopKRouter"      # the router: the model's own, a float tensor
    assert type(model.model.layers[1].mlp).__name__ == "MixtralSparseMoeBlock"


def test_convert_checkpoint_names_a_fused_experts_tensor_of_the_wrong_shape():
    """the experts' tensors are looked at before anything is quantised: a checkpoint that does not fit the model fails there, by name (no GPU is reached)"""
    model = M.build("mixtral")
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    key = "model.layers.1.mlp.experts.gate_up_proj"
    for wrong in (sd[key].transpose(1, 2), sd[key][0], sd[key][:3], sd[key][None]):
        with pytest.raises(ValueError, match=r"model\.layers\.1\.mlp\.experts\.gate_up_proj.*\[4, 256, 64\]"):
            S.convert_checkpoint(dict(sd, **{key: wrong}), model=model)
    with pytest.raises(KeyError, match="experts.down_proj"):
        S.convert_checkpoint({k: v for k, v in sd.items() if not k.endswith("layers.0.mlp.experts.down_proj")}, model=model)
