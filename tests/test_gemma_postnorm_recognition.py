"""CPU: what the sandwich residual fusion of protoquant_amd/gemma.py recognises, on tiny random-init Gemma, Gemma-2, Gemma-3 (text) and Llama models whose linears
were replaced by empty int8 modules (serialize.prepare_for_int8: no GPU, no quantisation): the data-flow probe (residual_flow_is_sandwich) on the stock classes and on
subclasses that break the flow, and fuse_gemma_postnorm_residual — which layers it takes, what it leaves alone object for object, the chain it links, and that
fuse_gemma_layers keeps its own behaviour."""
import copy

import pytest
import torch
from torch import nn

tr = pytest.importorskip("transformers")

from tests.test_gemma_recognition import ALL_NORMS, FAMILIES, L, _layers, _model, _norm_objects  # noqa: E402  (the tiny models of the Gemma recognition tests)

SANDWICH = ("gemma2", "gemma3")
POSTS = ("post_attention_layernorm", "post_feedforward_layernorm")
PRES = ("input_layernorm", "pre_feedforward_layernorm")


def _llama_model():
    from protoquant_amd.serialize import prepare_for_int8
    cfg = tr.LlamaConfig(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2)
    model = tr.LlamaForCausalLM(cfg).to(torch.bfloat16).eval()
    prepare_for_int8(model, fuse_gated_mlp=True)
    return model


# ---------------------------------------------------------------------------------------------------------------- the probe
@pytest.mark.parametrize("family", list(FAMILIES))
def test_probe_accepts_gemma2_and_gemma3_and_refuses_gemma(family):
    from protoquant_amd import residual_flow_is_sandwich
    from protoquant_amd.llama import residual_flow_is_llama
    for swapped in (False, True):
        layer = _layers(_model(family, swapped=swapped))[0]
        assert residual_flow_is_sandwich(layer) == (family in SANDWICH)
        assert residual_flow_is_sandwich(layer, type(layer)) == (family in SANDWICH)
        assert not (residual_flow_is_sandwich(layer) and residual_flow_is_llama(layer))


def test_probe_refuses_llama_and_other_flows():
    from transformers.models.gemma2.modeling_gemma2 import Gemma2DecoderLayer

    from protoquant_amd import residual_flow_is_sandwich
    assert not residual_flow_is_sandwich(_llama_model().model.layers[0])
    layer = _layers(_model("gemma2", swapped=False))[0]

    class DropsAPostNorm(Gemma2DecoderLayer):
        def forward(self, hidden_states, **kwargs):
            r = hidden_states
            h = self.self_attn(hidden_states=self.input_layernorm(hidden_states), **kwargs)[0]
            r1 = r + self.post_attention_layernorm(h)
            return r1 + self.mlp(self.pre_feedforward_layernorm(r1))          # post_feedforward_layernorm is never called

    class CallsAChildTwice(Gemma2DecoderLayer):
        def forward(self, hidden_states, **kwargs):
            r = hidden_states
            h = self.self_attn(hidden_states=self.input_layernorm(hidden_states), **kwargs)[0]
            r1 = r + self.post_attention_layernorm(h)
            self.pre_feedforward_layernorm(r1)
            return r1 + self.post_feedforward_layernorm(self.mlp(self.pre_feedforward_layernorm(r1)))

    class ScalesTheResidual(Gemma2DecoderLayer):
        def forward(self, hidden_states, **kwargs):
            r = hidden_states
            h = self.self_attn(hidden_states=self.input_layernorm(hidden_states), **kwargs)[0]
            r1 = r + 0.5 * self.post_attention_layernorm(h)
            return r1 + self.post_feedforward_layernorm(self.mlp(self.pre_feedforward_layernorm(r1)))

    class WithholdsAKeyword(Gemma2DecoderLayer):
        def forward(self, hidden_states, attention_mask=None, **kwargs):
            r = hidden_states
            h = self.self_attn(hidden_states=self.input_layernorm(hidden_states), **kwargs)[0]
            r1 = r + self.post_attention_layernorm(h)
            return r1 + self.post_feedforward_layernorm(self.mlp(self.pre_feedforward_layernorm(r1)))

    class TouchesAnotherSubmodule(Gemma2DecoderLayer):
        def forward(self, hidden_states, **kwargs):
            return self.extra(Gemma2DecoderLayer.forward(self, hidden_states, **kwargs))

    class PositionalHiddenState(Gemma2DecoderLayer):          # the fused layer calls self_attn(hidden_states=...): another calling form is not replayed, so it is refused
        def forward(self, hidden_states, **kwargs):
            r = hidden_states
            h = self.self_attn(self.input_layernorm(hidden_states), **kwargs)[0]
            r1 = r + self.post_attention_layernorm(h)
            return r1 + self.post_feedforward_layernorm(self.mlp(self.pre_feedforward_layernorm(r1)))

    class Raises(Gemma2DecoderLayer):
        def forward(self, hidden_states, **kwargs):
            raise RuntimeError("no")

    class SameFlowRewritten(Gemma2DecoderLayer):
        def forward(self, hidden_states, **kwargs):
            a = self.post_attention_layernorm(self.self_attn(hidden_states=self.input_layernorm(hidden_states), **kwargs)[0])
            r1 = hidden_states + a
            return r1 + self.post_feedforward_layernorm(self.mlp(self.pre_feedforward_layernorm(r1)))

    layer.extra = nn.Identity()
    for cls in (DropsAPostNorm, CallsAChildTwice, ScalesTheResidual, WithholdsAKeyword, TouchesAnotherSubmodule, PositionalHiddenState, Raises):
        assert not residual_flow_is_sandwich(layer, cls), cls.__name__
    assert residual_flow_is_sandwich(layer, SameFlowRewritten) and residual_flow_is_sandwich(layer, Gemma2DecoderLayer)          # probed, not pattern-matched


# ---------------------------------------------------------------------------------------------------------------- the switch
@pytest.mark.parametrize("family", SANDWICH)
def test_fuses_every_gemma2_and_gemma3_layer_and_keeps_the_objects(family):
    from protoquant_amd import GemmaRMSNormQuant, GemmaSandwichNormQuant, SandwichFusedLayer, fuse_gemma_layers, fuse_gemma_postnorm_residual
    from protoquant_amd.llama import ResidualFusedLayer, residual_fused_layers
    model = _model(family)
    assert fuse_gemma_layers(model) == L
    keys = list(model.state_dict())
    norms, classes, layers = _norm_objects(model), [type(l) for l in _layers(model)], _layers(model)
    others = [(l.self_attn, l.mlp) for l in layers]
    final = model.model.norm
    assert residual_fused_layers(model) == 0
    assert fuse_gemma_postnorm_residual(model) == L
    assert _layers(model) == layers and residual_fused_layers(model) == L
    for layer, cls, old, (attn, mlp) in zip(layers, classes, norms, others):
        assert isinstance(layer, SandwichFusedLayer) and isinstance(layer, cls) and not isinstance(layer, ResidualFusedLayer)
        assert type(layer).forward is SandwichFusedLayer.forward
        assert all(getattr(layer, n) is old[n] for n in ALL_NORMS)                        # the four norms: the same objects
        assert all(type(old[n]) is GemmaSandwichNormQuant and isinstance(old[n], GemmaRMSNormQuant) for n in PRES)
        assert all(type(old[n]).__name__.endswith("RMSNorm") for n in POSTS)              # the post-norms stay the model's modules
        assert layer.self_attn is attn and layer.mlp is mlp
        assert not layer._rf_inbox.pending
    assert [l._rf_next[0] for l in layers] == layers[1:] + [None]
    assert model.model.norm is final and list(model.state_dict()) == keys
    assert model.model._rf_layers == layers
    # idempotent; and fuse_gemma_layers finds nothing left to change either
    hooks = len(model.model._forward_hooks)
    assert fuse_gemma_postnorm_residual(model) == 0 and residual_fused_layers(model) == L and len(model.model._forward_hooks) == hooks
    assert fuse_gemma_layers(model) == 0 and fuse_gemma_layers(model, fuse_residual=True) == 0 and residual_fused_layers(model) == L
    # a deep copy is a model of its own: fused layers of the same classes, linked among themselves, with empty hand-overs
    twin = copy.deepcopy(model)
    tl = _layers(twin)
    assert [type(a) is type(b) and a is not b for a, b in zip(tl, layers)] == [True] * L
    assert [l._rf_next[0] for l in tl] == tl[1:] + [None] and twin.model._rf_layers == tl and not any(l._rf_inbox.pending for l in tl)


@pytest.mark.parametrize("family", SANDWICH)
def test_fuse_gemma_layers_keeps_refusing_the_sandwich_flow(family):
    from protoquant_amd import fuse_gemma_layers
    from protoquant_amd.llama import residual_fused_layers
    model = _model(family)
    classes = [type(l) for l in _layers(model)]
    assert fuse_gemma_layers(model, fuse_residual=True) == L
    assert residual_fused_layers(model) == 0 and [type(l) for l in _layers(model)] == classes and not hasattr(model.model, "_rf_layers")


def test_returns_zero_on_gemma_and_on_llama_and_touches_nothing():
    from protoquant_amd import fuse_gemma_layers, fuse_gemma_postnorm_residual, fuse_llama_layers
    from protoquant_amd.llama import residual_fused_layers
    for make, prepare in ((lambda: _model("gemma"), lambda m: fuse_gemma_layers(m)), (lambda: _model("gemma"), lambda m: fuse_gemma_layers(m, fuse_residual=True)),
                          (_llama_model, lambda m: fuse_llama_layers(m)), (_llama_model, lambda m: fuse_llama_layers(m, fuse_residual=True)),
                          (lambda: _model("gemma2", swapped=False), lambda m: None), (lambda: _model("gemma2"), lambda m: None)):
        model = make()
        prepare(model)
        before = {n: (m, type(m)) for n, m in model.named_modules()}
        fused, hooks = residual_fused_layers(model), len(model.model._forward_hooks)
        assert fuse_gemma_postnorm_residual(model) == 0
        assert {n: (m, type(m)) for n, m in model.named_modules()} == before
        assert residual_fused_layers(model) == fused and len(model.model._forward_hooks) == hooks


@pytest.mark.parametrize("which", POSTS)
@pytest.mark.parametrize("kind", ["forward_hook", "forward_pre_hook"])
def test_a_layer_with_a_hooked_post_norm_is_refused_and_breaks_the_chain(which, kind):
    from protoquant_amd import GemmaRMSNormQuant, GemmaSandwichNormQuant, SandwichFusedLayer, fuse_gemma_layers, fuse_gemma_postnorm_residual
    from protoquant_amd.llama import residual_fused_layers
    model = _model("gemma2")
    assert fuse_gemma_layers(model) == L
    layers = _layers(model)
    post = getattr(layers[1], which)
    handle = post.register_forward_hook(lambda m, a, o: None) if kind == "forward_hook" else post.register_forward_pre_hook(lambda m, a: None)
    cls = type(layers[1])
    assert fuse_gemma_postnorm_residual(model) == L - 1 and residual_fused_layers(model) == L - 1
    assert type(layers[1]) is cls and not hasattr(layers[1], "_rf_inbox")
    assert all(type(getattr(layers[1], n)) is GemmaRMSNormQuant for n in PRES)            # the refused layer keeps everything it had
    assert all(type(getattr(l, n)) is GemmaSandwichNormQuant for l in (layers[0], layers[2]) for n in PRES)
    assert isinstance(layers[0], SandwichFusedLayer) and layers[0]._rf_next == [None]     # the predecessor ends its chain (K1pa)
    assert isinstance(layers[2], SandwichFusedLayer) and layers[2]._rf_next == [None]
    # the hook gone, a second call takes the layer and links the chain again
    handle.remove()
    assert fuse_gemma_postnorm_residual(model) == 1 and residual_fused_layers(model) == L
    assert [l._rf_next[0] for l in layers] == layers[1:] + [None]


def test_other_refusals():
    from protoquant_amd import fuse_gemma_layers, fuse_gemma_postnorm_residual
    # a post-norm that is not the Gemma norm
    model = _model("gemma2")
    fuse_gemma_layers(model)
    layers = _layers(model)

    class Doubled(type(layers[0].post_attention_layernorm)):
        def forward(self, x):
            return super().forward(x) * 2.0
    layers[0].post_attention_layernorm.__class__ = Doubled
    # a pre-norm that fuse_gemma_layers did not replace
    stock = type(layers[2].post_feedforward_layernorm)(64)
    layers[2].pre_feedforward_layernorm = stock
    assert fuse_gemma_postnorm_residual(model) == L - 2
    assert [hasattr(l, "_rf_inbox") for l in layers] == [False, True, False] and layers[1]._rf_next == [None] and layers[2].pre_feedforward_layernorm is stock
    # a layer class whose forward is not the sandwich flow
    model = _model("gemma3")
    fuse_gemma_layers(model)
    layers = _layers(model)

    class OtherFlow(type(layers[0])):
        def forward(self, hidden_states, **kwargs):
            return hidden_states
    layers[L - 1].__class__ = OtherFlow
    assert fuse_gemma_postnorm_residual(model) == L - 1 and type(layers[L - 1]) is OtherFlow and layers[L - 2]._rf_next == [None]
