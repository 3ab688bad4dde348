"""CPU: what protoquant_amd/olmo.py recognises, on real transformers classes and on hand-made counter-examples, and what fuse_olmo_layers does to tiny random-init
Olmo2 and Olmo3 models whose linears were replaced by empty int8 modules (serialize.prepare_for_int8: no GPU, no quantisation): the norm probe (is_olmo_rmsnorm), the
data-flow probe (residual_flow_is_postnorm), which objects the switch replaces and which it leaves alone object for object, the chain it links, a hooked post-norm, a
second call, and that Llama, Gemma-2 and Mixtral models — and the other families' entry points on an OLMo model — are untouched."""
import copy

import pytest
import torch
from torch import nn

tr = pytest.importorskip("transformers")

L = 3
FAMILIES = {"olmo2": ("Olmo2Config", "Olmo2ForCausalLM"), "olmo3": ("Olmo3Config", "Olmo3ForCausalLM")}
POSTS = ("post_attention_layernorm", "post_feedforward_layernorm")


def _model(family, swapped=True, layers=L):
    from protoquant_amd.serialize import prepare_for_int8
    cname, mname = FAMILIES[family]
    if not (hasattr(tr, cname) and hasattr(tr, mname)):
        pytest.skip(f"the installed transformers has no {mname}")
    torch.manual_seed(0)
    extra = dict(sliding_window=8, layer_types=["sliding_attention", "full_attention", "sliding_attention", "full_attention"][:layers]) if family == "olmo3" else {}
    cfg = getattr(tr, cname)(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=layers, num_attention_heads=4, num_key_value_heads=2,
                             max_position_embeddings=64, **extra)
    model = getattr(tr, mname)(cfg).to(torch.bfloat16).eval()
    with torch.no_grad():
        for m in model.modules():
            if type(m).__name__.endswith("RMSNorm"):
                m.weight.copy_((1.0 + 0.3 * torch.randn(m.weight.shape)).to(m.weight.dtype))
    if swapped:
        prepare_for_int8(model, fuse_gated_mlp=True)
    return model


def _other(kind):
    from protoquant_amd.serialize import prepare_for_int8
    torch.manual_seed(0)
    common = dict(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=64)
    if kind == "llama":
        model = tr.LlamaForCausalLM(tr.LlamaConfig(**common))
    elif kind == "gemma2":
        model = tr.Gemma2ForCausalLM(tr.Gemma2Config(head_dim=16, **common))
    elif kind == "granite":
        model = tr.GraniteForCausalLM(tr.GraniteConfig(residual_multiplier=0.5, **common))
    else:
        model = tr.MixtralForCausalLM(tr.MixtralConfig(num_local_experts=4, num_experts_per_tok=2, **common))
    model = model.to(torch.bfloat16).eval()
    prepare_for_int8(model, fuse_gated_mlp=True)
    return model


def _layers(model):
    return list(model.model.layers)


# ---------------------------------------------------------------------------------------------------------------- the norm probe
def test_is_olmo_rmsnorm_accepts_the_olmo_norms_and_refuses_the_others():
    from transformers.models.gemma.modeling_gemma import GemmaRMSNorm
    from transformers.models.llama.modeling_llama import LlamaRMSNorm
    from transformers.models.olmo2.modeling_olmo2 import Olmo2RMSNorm
    from transformers.models.olmo3.modeling_olmo3 import Olmo3RMSNorm
    from transformers.models.t5.modeling_t5 import T5LayerNorm

    from protoquant_amd import OlmoRMSNorm, is_olmo_rmsnorm
    from protoquant_amd.gemma import is_gemma_rmsnorm
    for cls in (Olmo2RMSNorm, Olmo3RMSNorm):
        for dt in (torch.bfloat16, torch.float32):
            assert is_olmo_rmsnorm(cls(64, eps=1e-6).to(dt)), (cls.__name__, dt)
        assert is_olmo_rmsnorm(cls(8, eps=1e-5)) and is_olmo_rmsnorm(cls(16, eps=0.0))
        assert not is_gemma_rmsnorm(cls(64, eps=1e-6))
    for m in (LlamaRMSNorm(64, eps=1e-6), T5LayerNorm(64, eps=1e-6).to(torch.bfloat16), T5LayerNorm(64, eps=1e-6), GemmaRMSNorm(64, eps=1e-6), nn.LayerNorm(64),
              nn.LayerNorm(64, bias=False), nn.Identity(), nn.Linear(64, 64), OlmoRMSNorm(torch.ones(64), 1e-6), None, "Olmo2RMSNorm"):
        assert not is_olmo_rmsnorm(m), type(m).__name__

    class TwoRoundings(Olmo2RMSNorm):          # the Llama order under the OLMo class
        def forward(self, hidden_states):
            dt = hidden_states.dtype
            h = hidden_states.to(torch.float32)
            h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + self.variance_epsilon)
            return self.weight * h.to(dt)

    class Doubled(Olmo2RMSNorm):
        def forward(self, hidden_states):
            return super().forward(hidden_states) * 2.0

    class OnePlusW(Olmo2RMSNorm):
        def forward(self, hidden_states):
            dt = hidden_states.dtype
            h = hidden_states.to(torch.float32)
            h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + self.variance_epsilon)
            return (h * (1.0 + self.weight.float())).to(dt)

    class NoEps(Olmo2RMSNorm):
        def forward(self, hidden_states):
            dt = hidden_states.dtype
            h = hidden_states.to(torch.float32)
            return (self.weight * (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True)))).to(dt)

    class Raises(Olmo2RMSNorm):
        def forward(self, hidden_states):
            raise RuntimeError("no")

    class SameNormRewritten(Olmo2RMSNorm):
        def forward(self, x):
            xf = x.float()
            return (self.weight * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + self.variance_epsilon))).to(x.dtype)

    class UnderTheNameEps(nn.Module):
        def __init__(self, n, eps):
            super().__init__()
            self.weight, self.eps = nn.Parameter(torch.ones(n)), eps

        def forward(self, x):
            xf = x.float()
            return (self.weight * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + self.eps))).to(x.dtype)

    for cls in (TwoRoundings, Doubled, OnePlusW, NoEps, Raises):
        assert not is_olmo_rmsnorm(cls(64, eps=1e-6)), cls.__name__
    assert is_olmo_rmsnorm(SameNormRewritten(64, eps=1e-6)) and is_olmo_rmsnorm(UnderTheNameEps(64, 1e-6))          # probed, not recognised by name
    with_buffer = Olmo2RMSNorm(64, eps=1e-6)
    with_buffer.register_buffer("extra", torch.zeros(1))
    with_child = Olmo2RMSNorm(64, eps=1e-6)
    with_child.child = nn.Identity()
    int_eps = Olmo2RMSNorm(64, eps=1e-6)
    int_eps.variance_epsilon = 1
    two_d = Olmo2RMSNorm(64, eps=1e-6)
    two_d.weight = nn.Parameter(torch.ones(2, 64))
    for m in (with_buffer, with_child, int_eps, two_d):
        assert not is_olmo_rmsnorm(m)


# ---------------------------------------------------------------------------------------------------------------- the data-flow probe
@pytest.mark.parametrize("family", list(FAMILIES))
def test_probe_accepts_olmo2_and_olmo3(family):
    from protoquant_amd import residual_flow_is_postnorm, residual_flow_is_sandwich
    from protoquant_amd.llama import residual_flow_is_llama
    for swapped in (False, True):
        layer = _layers(_model(family, swapped=swapped))[0]
        assert residual_flow_is_postnorm(layer) and residual_flow_is_postnorm(layer, type(layer))
        assert not residual_flow_is_llama(layer) and not residual_flow_is_sandwich(layer)


@pytest.mark.parametrize("kind", ["llama", "gemma2", "granite"])
def test_probe_refuses_the_other_families(kind):
    from protoquant_amd import residual_flow_is_postnorm
    assert not residual_flow_is_postnorm(_layers(_other(kind))[0])


def test_probe_refuses_other_flows():
    from transformers.models.olmo2.modeling_olmo2 import Olmo2DecoderLayer

    from protoquant_amd import residual_flow_is_postnorm
    layer = _layers(_model("olmo2", swapped=False))[0]

    class ScaledSum(Olmo2DecoderLayer):
        def forward(self, hidden_states, **kwargs):
            residual = hidden_states
            h = self.post_attention_layernorm(self.self_attn(hidden_states=hidden_states, **kwargs)[0])
            r1 = residual * 0.5 + h
            return r1 + self.post_feedforward_layernorm(self.mlp(r1))

    class CallsADropout(Olmo2DecoderLayer):
        def forward(self, hidden_states, **kwargs):
            h = self.post_attention_layernorm(self.self_attn(hidden_states=hidden_states, **kwargs)[0])
            r1 = hidden_states + self.dropout(h)
            return r1 + self.post_feedforward_layernorm(self.mlp(r1))

    class DropsAPostNorm(Olmo2DecoderLayer):
        def forward(self, hidden_states, **kwargs):
            r1 = hidden_states + self.post_attention_layernorm(self.self_attn(hidden_states=hidden_states, **kwargs)[0])
            return r1 + self.mlp(r1)

    class NormsTheInput(Olmo2DecoderLayer):          # the Llama placement of the same two norms
        def forward(self, hidden_states, **kwargs):
            r1 = hidden_states + self.self_attn(hidden_states=self.post_attention_layernorm(hidden_states), **kwargs)[0]
            return r1 + self.mlp(self.post_feedforward_layernorm(r1))

    class CallsAChildTwice(Olmo2DecoderLayer):
        def forward(self, hidden_states, **kwargs):
            r1 = hidden_states + self.post_attention_layernorm(self.self_attn(hidden_states=hidden_states, **kwargs)[0])
            self.mlp(r1)
            return r1 + self.post_feedforward_layernorm(self.mlp(r1))

    class WithholdsAKeyword(Olmo2DecoderLayer):
        def forward(self, hidden_states, attention_mask=None, **kwargs):
            r1 = hidden_states + self.post_attention_layernorm(self.self_attn(hidden_states=hidden_states, **kwargs)[0])
            return r1 + self.post_feedforward_layernorm(self.mlp(r1))

    class PositionalHiddenState(Olmo2DecoderLayer):          # the fused layer calls self_attn(hidden_states=...): another calling form is not replayed
        def forward(self, hidden_states, **kwargs):
            r1 = hidden_states + self.post_attention_layernorm(self.self_attn(hidden_states, **kwargs)[0])
            return r1 + self.post_feedforward_layernorm(self.mlp(r1))

    class Raises(Olmo2DecoderLayer):
        def forward(self, hidden_states, **kwargs):
            raise RuntimeError("no")

    class SameFlowRewritten(Olmo2DecoderLayer):
        def forward(self, hidden_states, **kwargs):
            a = self.post_attention_layernorm(self.self_attn(hidden_states=hidden_states, **kwargs)[0])
            r1 = hidden_states + a
            m = self.post_feedforward_layernorm(self.mlp(r1))
            return r1 + m

    layer.dropout = nn.Dropout(0.0)
    for cls in (ScaledSum, CallsADropout, DropsAPostNorm, NormsTheInput, CallsAChildTwice, WithholdsAKeyword, PositionalHiddenState, Raises):
        assert not residual_flow_is_postnorm(layer, cls), cls.__name__
    assert residual_flow_is_postnorm(layer, SameFlowRewritten) and residual_flow_is_postnorm(layer, Olmo2DecoderLayer)          # probed, not pattern-matched


# ---------------------------------------------------------------------------------------------------------------- the switch
def _snapshot(model):
    return {n: (m, type(m)) for n, m in model.named_modules()}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_without_fuse_residual_only_qkv_changes(family):
    from protoquant_amd import FusedQLinear, GatedMLP, fuse_olmo_layers, qlinear
    from protoquant_amd.llama import _FusedSlice, _SharedFused, residual_fused_layers
    model = _model(family)
    layers = _layers(model)
    before = _snapshot(model)
    classes = [type(l) for l in layers]
    assert all(isinstance(l.mlp, GatedMLP) and isinstance(l.self_attn.q_proj, qlinear) for l in layers)
    assert fuse_olmo_layers(model) == L
    after = _snapshot(model)
    changed = {n for n in after if n not in before or after[n] != before[n]}
    gone = {n for n in before if n not in after}
    assert gone == set() and [type(l) for l in layers] == classes and residual_fused_layers(model) == 0 and not hasattr(model.model, "_rf_layers")
    want = set()
    for i in range(L):
        a = f"model.layers.{i}.self_attn"
        want |= {f"{a}.q_proj", f"{a}.k_proj", f"{a}.v_proj", f"{a}.qkv_fused", f"{a}.qkv_fused.fused"}
    assert changed == want, sorted(changed ^ want)
    for l in layers:
        a = l.self_attn
        assert isinstance(a.qkv_fused, _SharedFused) and isinstance(a.qkv_fused.fused, FusedQLinear) and a.qkv_fused.fused.splits == [64, 32, 32]
        assert all(isinstance(getattr(a, p), _FusedSlice) for p in ("q_proj", "k_proj", "v_proj")) and isinstance(a.o_proj, qlinear)
        assert type(a.q_norm).__name__.endswith("RMSNorm") and type(a.k_norm).__name__.endswith("RMSNorm")          # the model's modules
    assert fuse_olmo_layers(model) == 0 and _snapshot(model) == after                                             # a second call finds nothing to do
    assert fuse_olmo_layers(model, fuse_qkv=False) == 0 and _snapshot(model) == after


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("qkv_first", [False, True])
def test_fuse_residual_replaces_what_it_says_and_keeps_the_objects(family, qkv_first):
    from protoquant_amd import OlmoRMSNorm, PostNormFusedLayer, fuse_gemma_layers, fuse_gemma_postnorm_residual, fuse_llama_layers, fuse_olmo_layers
    from protoquant_amd.llama import ResidualFusedLayer, _FusedSlice, residual_fused_layers
    model = _model(family)
    if qkv_first:
        assert fuse_olmo_layers(model) == L          # the default call first, the switch in a second call
    layers = _layers(model)
    keys = list(model.state_dict()) if qkv_first else None
    classes = [type(l) for l in layers]
    posts = [{n: getattr(l, n) for n in POSTS} for l in layers]
    others = [(l.self_attn, l.mlp, l.self_attn.o_proj) for l in layers]
    qk_weights = [(l.self_attn.q_norm.weight, l.self_attn.k_norm.weight) for l in layers]
    norm_keys = [k for k in model.state_dict() if "norm" in k]
    final, head = model.model.norm, model.lm_head
    assert fuse_olmo_layers(model, fuse_residual=True) == L
    assert _layers(model) == layers and residual_fused_layers(model) == L
    for layer, cls, post, (attn, mlp, o), (qw, kw) in zip(layers, classes, posts, others, qk_weights):
        assert isinstance(layer, PostNormFusedLayer) and isinstance(layer, cls) and not isinstance(layer, ResidualFusedLayer)
        assert type(layer).forward is PostNormFusedLayer.forward and type(layer).__bases__ == (PostNormFusedLayer, cls)
        assert all(getattr(layer, n) is post[n] and type(post[n]).__name__.endswith("RMSNorm") and type(post[n]) is not OlmoRMSNorm for n in POSTS)
        assert layer.self_attn is attn and layer.mlp is mlp and attn.o_proj is o and isinstance(attn.q_proj, _FusedSlice)
        assert type(attn.q_norm) is OlmoRMSNorm and type(attn.k_norm) is OlmoRMSNorm
        assert attn.q_norm.weight is qw and attn.k_norm.weight is kw and attn.q_norm.variance_epsilon == post[POSTS[0]].variance_epsilon
        assert not layer._rf_inbox.pending
    assert [l._rf_next[0] for l in layers] == layers[1:] + [None]
    assert model.model.norm is final and model.lm_head is head and model.model._rf_layers == layers
    assert [k for k in model.state_dict() if "norm" in k] == norm_keys
    if keys is not None:
        assert list(model.state_dict()) == keys
    # a second call returns 0; the other families' entry points find nothing of theirs
    hooks = len(model.model._forward_hooks)
    snap = _snapshot(model)
    assert fuse_olmo_layers(model, fuse_residual=True) == 0 and fuse_olmo_layers(model) == 0
    assert fuse_llama_layers(model) == 0 and fuse_llama_layers(model, fuse_residual=True) == 0 and fuse_gemma_layers(model, fuse_residual=True) == 0
    assert fuse_gemma_postnorm_residual(model) == 0
    assert _snapshot(model) == snap and residual_fused_layers(model) == L and len(model.model._forward_hooks) == hooks
    # a deep copy is a model of its own: fused layers of the same classes, linked among themselves, with empty hand-overs
    twin = copy.deepcopy(model)
    tl = _layers(twin)
    assert [type(a) is type(b) and a is not b for a, b in zip(tl, layers)] == [True] * L
    assert [l._rf_next[0] for l in tl] == tl[1:] + [None] and twin.model._rf_layers == tl and not any(l._rf_inbox.pending for l in tl)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_other_entry_points_return_zero_on_an_olmo_model(family):
    from protoquant_amd import fuse_gemma_layers, fuse_gemma_postnorm_residual, fuse_llama_layers
    for swapped in (False, True):
        model = _model(family, swapped=swapped)
        before = _snapshot(model)
        assert fuse_llama_layers(model) == 0 and fuse_llama_layers(model, fuse_residual=True) == 0
        assert fuse_gemma_layers(model) == 0 and fuse_gemma_layers(model, fuse_residual=True) == 0 and fuse_gemma_postnorm_residual(model) == 0
        assert _snapshot(model) == before


@pytest.mark.parametrize("kind", ["llama", "gemma2", "mixtral"])
def test_other_models_are_untouched(kind):
    from protoquant_amd import fuse_olmo_layers
    from protoquant_amd.llama import residual_fused_layers
    model = _other(kind)
    before, hooks = _snapshot(model), len(model.model._forward_hooks)
    assert fuse_olmo_layers(model) == 0 and fuse_olmo_layers(model, fuse_residual=True) == 0
    assert _snapshot(model) == before and residual_fused_layers(model) == 0 and len(model.model._forward_hooks) == hooks
    unswapped = _model("olmo2", swapped=False)          # nn.Linear projections: swap_linears has not run
    before = _snapshot(unswapped)
    assert fuse_olmo_layers(unswapped, fuse_residual=True) == 0 and _snapshot(unswapped) == before


@pytest.mark.parametrize("which", POSTS)
@pytest.mark.parametrize("kind", ["forward_hook", "forward_pre_hook"])
def test_a_layer_with_a_hooked_post_norm_is_refused_and_breaks_the_chain(which, kind):
    from protoquant_amd import OlmoRMSNorm, PostNormFusedLayer, fuse_olmo_layers
    from protoquant_amd.llama import _FusedSlice, residual_fused_layers
    model = _model("olmo2")
    layers = _layers(model)
    post = getattr(layers[1], which)
    handle = post.register_forward_hook(lambda m, a, o: None) if kind == "forward_hook" else post.register_forward_pre_hook(lambda m, a: None)
    cls = type(layers[1])
    assert fuse_olmo_layers(model, fuse_residual=True) == L and residual_fused_layers(model) == L - 1          # (the refused layer still got its q / k / v fused)
    assert type(layers[1]) is cls and not hasattr(layers[1], "_rf_inbox") and isinstance(layers[1].self_attn.q_proj, _FusedSlice)
    assert type(layers[1].self_attn.q_norm) is not OlmoRMSNorm and type(layers[1].self_attn.k_norm) is not OlmoRMSNorm          # the refused layer keeps its norms
    assert isinstance(layers[0], PostNormFusedLayer) and layers[0]._rf_next == [None]     # the predecessor ends its chain (K1oa)
    assert isinstance(layers[2], PostNormFusedLayer) and layers[2]._rf_next == [None]
    assert fuse_olmo_layers(model, fuse_residual=True) == 0
    # the hook gone, a further call takes the layer and links the chain again
    handle.remove()
    assert fuse_olmo_layers(model, fuse_residual=True) == 1 and residual_fused_layers(model) == L
    assert [l._rf_next[0] for l in layers] == layers[1:] + [None]


def test_other_refusals():
    from protoquant_amd import OlmoRMSNorm, PostNormFusedLayer, fuse_olmo_layers
    from protoquant_amd.llama import residual_fused_layers
    model = _model("olmo2")
    layers = _layers(model)

    class Doubled(type(layers[0].post_attention_layernorm)):          # a post-norm that is not the OLMo norm
        def forward(self, x):
            return super().forward(x) * 2.0
    layers[0].post_attention_layernorm.__class__ = Doubled
    layers[1].post_feedforward_layernorm = type(layers[1].post_feedforward_layernorm)(32)          # not as wide as the hidden size
    hooked = layers[2].self_attn.k_norm
    hooked.register_forward_hook(lambda m, a, o: None)                                            # a hooked k_norm stays the model's module; the layer is taken
    assert fuse_olmo_layers(model, fuse_residual=True) == L and residual_fused_layers(model) == 1
    assert [isinstance(l, PostNormFusedLayer) for l in layers] == [False, False, True]
    assert layers[2].self_attn.k_norm is hooked and type(layers[2].self_attn.q_norm) is OlmoRMSNorm
    # a layer class whose forward is not the post-norm flow: nothing of it is touched, q / k / v included; a fifth child likewise
    model = _model("olmo3")
    layers = _layers(model)

    class OtherFlow(type(layers[0])):
        def forward(self, hidden_states, **kwargs):
            return hidden_states
    layers[L - 1].__class__ = OtherFlow
    layers[0].dropout = nn.Dropout(0.0)
    before = {n: (m, type(m)) for n, m in list(layers[L - 1].named_modules()) + list(layers[0].named_modules())}
    assert fuse_olmo_layers(model, fuse_residual=True) == L - 2 and type(layers[L - 1]) is OtherFlow
    assert {n: (m, type(m)) for n, m in list(layers[L - 1].named_modules()) + list(layers[0].named_modules())} == before
    assert isinstance(layers[1], PostNormFusedLayer) and layers[1]._rf_next == [None]
    # an MLP that swap_linears did not turn into a GatedMLP: q / k / v are fused, the residual flow is not
    model = _model("olmo2")
    from protoquant_amd.serialize import prepare_for_int8
    plain = _model("olmo2", swapped=False)
    prepare_for_int8(plain)          # (without fuse_gated_mlp)
    assert fuse_olmo_layers(plain, fuse_residual=True) == L and residual_fused_layers(plain) == 0
