"""CPU: what the scaled-residual fusion of protoquant_amd/granite.py recognises, on tiny random-init transformers models whose linears were replaced by empty int8
modules (serialize.prepare_for_int8: no GPU, no quantisation): the data-flow probe (residual_flow_is_scaled) on the stock classes and on hand-written forwards that
break the flow, and fuse_granite_residual — which layers it takes, what it leaves alone object for object, the chain it links, the kernel sequence of the fused forward
(played with recording stand-ins for the two ops) and its copies.

Decision held here: a layer WITHOUT a residual_multiplier (Llama, Mistral, Qwen) is refused by this switch and returns 0 — fuse_llama_layers(fuse_residual=True) is its
switch; a Granite layer at residual_multiplier = 1.0 is accepted (its class reads the attribute)."""
import copy
import importlib
import pickle
import types

import pytest
import torch
from torch import nn

tr = pytest.importorskip("transformers")

from protoquant_amd import granite  # noqa: E402,F401  (the module this file is about)

L = 3
SMALL = dict(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=L, num_attention_heads=4, num_key_value_heads=2, pad_token_id=0, eos_token_id=1, bos_token_id=2)


def _model(mod, cfgname, clsname, swapped=True, **kw):
    pytest.importorskip(f"transformers.models.{mod}.modeling_{mod}")
    from protoquant_amd.serialize import prepare_for_int8
    cfg = getattr(importlib.import_module(f"transformers.models.{mod}.configuration_{mod}"), cfgname)(**{**SMALL, **kw})
    model = getattr(importlib.import_module(f"transformers.models.{mod}.modeling_{mod}"), clsname)(cfg).to(torch.bfloat16).eval()
    if swapped:
        prepare_for_int8(model, fuse_gated_mlp=True)
    return model


def _granite(m=0.22, **kw):
    return _model("granite", "GraniteConfig", "GraniteForCausalLM", residual_multiplier=m, **kw)


def _layers(model):
    return list(model.model.layers)


# ---------------------------------------------------------------------------------------------------------------- the probe
@pytest.mark.parametrize("m", [0.22, 1.0, 2, -0.5])
def test_probe_accepts_granite_at_any_finite_python_multiplier(m):
    from protoquant_amd import residual_flow_is_scaled
    from protoquant_amd.llama import residual_flow_is_llama
    for swapped in (False, True):
        layer = _layers(_granite(m, swapped=swapped))[0]
        before = {k: v.clone() for k, v in layer.state_dict().items()}
        assert residual_flow_is_scaled(layer) and residual_flow_is_scaled(layer, type(layer))
        assert layer.residual_multiplier == m and all(torch.equal(v, layer.state_dict()[k]) for k, v in before.items())          # probing changes nothing
        assert residual_flow_is_llama(layer) == (m == 1)          # (the Llama probe reads the real attribute: at 1 the two flows coincide)


OTHERS = [("llama", "LlamaConfig", "LlamaForCausalLM", {}), ("mistral", "MistralConfig", "MistralForCausalLM", {}), ("qwen2", "Qwen2Config", "Qwen2ForCausalLM", {}),
          ("granitemoe", "GraniteMoeConfig", "GraniteMoeForCausalLM", {"num_local_experts": 4, "num_experts_per_tok": 2}),
          ("gemma2", "Gemma2Config", "Gemma2ForCausalLM", {"head_dim": 16}), ("olmo2", "Olmo2Config", "Olmo2ForCausalLM", {}), ("phi3", "Phi3Config", "Phi3ForCausalLM", {})]


@pytest.mark.parametrize("mod,cfgname,clsname,kw", OTHERS, ids=[o[0] for o in OTHERS])
def test_other_families_return_zero_and_are_left_untouched(mod, cfgname, clsname, kw):
    from protoquant_amd import fuse_granite_residual, fuse_llama_layers, residual_flow_is_scaled
    from protoquant_amd.llama import residual_fused_layers
    for prepare in (lambda m: None, lambda m: fuse_llama_layers(m)):
        model = _model(mod, cfgname, clsname, **kw)
        prepare(model)
        assert not any(residual_flow_is_scaled(l) for l in _layers(model))
        before = {n: (m, type(m)) for n, m in model.named_modules()}
        keys, hooks = list(model.state_dict()), len(model.model._forward_hooks)
        assert fuse_granite_residual(model) == 0
        assert {n: (m, type(m)) for n, m in model.named_modules()} == before and list(model.state_dict()) == keys
        assert residual_fused_layers(model) == 0 and len(model.model._forward_hooks) == hooks and not hasattr(model.model, "_rf_layers")


def test_probe_refuses_hand_written_variants_and_bad_multipliers():
    from protoquant_amd import residual_flow_is_scaled

    class Base(nn.Module):
        def __init__(self, m=0.22):
            super().__init__()
            self.input_layernorm, self.post_attention_layernorm, self.self_attn, self.mlp = nn.Identity(), nn.Identity(), nn.Identity(), nn.Identity()
            self.residual_multiplier = m

    class Granite(Base):
        def forward(self, hidden_states, attention_mask=None, **kwargs):
            r1 = hidden_states + self.self_attn(hidden_states=self.input_layernorm(hidden_states), attention_mask=attention_mask, **kwargs)[0] * self.residual_multiplier
            return r1 + self.mlp(self.post_attention_layernorm(r1)) * self.residual_multiplier

    class MultiplierFirst(Base):                     # m * h: the same product
        def forward(self, hidden_states, **kwargs):
            r1 = hidden_states + self.residual_multiplier * self.self_attn(hidden_states=self.input_layernorm(hidden_states), **kwargs)[0]
            return self.residual_multiplier * self.mlp(self.post_attention_layernorm(r1)) + r1

    class IgnoresTheAttribute(Base):                 # the Llama flow
        def forward(self, hidden_states, **kwargs):
            r1 = hidden_states + self.self_attn(hidden_states=self.input_layernorm(hidden_states), **kwargs)[0]
            return r1 + self.mlp(self.post_attention_layernorm(r1))

    class ScalesTheResidual(Base):
        def forward(self, hidden_states, **kwargs):
            r1 = hidden_states * self.residual_multiplier + self.self_attn(hidden_states=self.input_layernorm(hidden_states), **kwargs)[0]
            return r1 * self.residual_multiplier + self.mlp(self.post_attention_layernorm(r1))

    class ScalesTheFirstAddOnly(Base):
        def forward(self, hidden_states, **kwargs):
            r1 = hidden_states + self.self_attn(hidden_states=self.input_layernorm(hidden_states), **kwargs)[0] * self.residual_multiplier
            return r1 + self.mlp(self.post_attention_layernorm(r1))

    class ScalesTheSecondAddOnly(Base):
        def forward(self, hidden_states, **kwargs):
            r1 = hidden_states + self.self_attn(hidden_states=self.input_layernorm(hidden_states), **kwargs)[0]
            return r1 + self.mlp(self.post_attention_layernorm(r1)) * self.residual_multiplier

    class ScalesTheSum(Base):
        def forward(self, hidden_states, **kwargs):
            r1 = (hidden_states + self.self_attn(hidden_states=self.input_layernorm(hidden_states), **kwargs)[0]) * self.residual_multiplier
            return (r1 + self.mlp(self.post_attention_layernorm(r1))) * self.residual_multiplier

    class ConstantMultiplier(Base):                  # right at one multiplier only: the second stand-in tells
        def forward(self, hidden_states, **kwargs):
            r1 = hidden_states + self.self_attn(hidden_states=self.input_layernorm(hidden_states), **kwargs)[0] * 0.5
            return r1 + self.mlp(self.post_attention_layernorm(r1)) * 0.5

    class DropsKwargs(Base):
        def forward(self, hidden_states, attention_mask=None, **kwargs):
            r1 = hidden_states + self.self_attn(hidden_states=self.input_layernorm(hidden_states))[0] * self.residual_multiplier
            return r1 + self.mlp(self.post_attention_layernorm(r1)) * self.residual_multiplier

    class Tuple(Granite):
        def forward(self, hidden_states, attention_mask=None, **kwargs):
            return (super().forward(hidden_states, attention_mask, **kwargs),)

    class Raises(Base):
        def forward(self, hidden_states, **kwargs):
            raise RuntimeError("no")

    assert residual_flow_is_scaled(Granite()) and residual_flow_is_scaled(MultiplierFirst()) and residual_flow_is_scaled(Granite(1.0)) and residual_flow_is_scaled(Granite(3))
    for cls in (IgnoresTheAttribute, ScalesTheResidual, ScalesTheFirstAddOnly, ScalesTheSecondAddOnly, ScalesTheSum, ConstantMultiplier, DropsKwargs, Tuple, Raises):
        assert not residual_flow_is_scaled(cls()), cls.__name__
    for bad in (torch.tensor(0.22), nn.Parameter(torch.tensor(0.22)), None, "0.22", True, float("nan"), float("inf"), [0.22]):
        assert not residual_flow_is_scaled(Granite(bad)), repr(bad)
    layer = Granite()
    del layer.residual_multiplier
    assert not residual_flow_is_scaled(layer)


# ---------------------------------------------------------------------------------------------------------------- the switch
@pytest.mark.parametrize("m", [0.22, 1.0])
def test_fuses_every_granite_layer_and_keeps_the_objects(m):
    from protoquant_amd import RMSNormQuant, ScaledResidualFusedLayer, fuse_granite_residual, fuse_llama_layers
    from protoquant_amd.llama import ResidualFusedLayer, residual_fused_layers
    model = _granite(m)
    assert fuse_granite_residual(model) == 0 and not hasattr(model.model, "_rf_layers")          # the norms are not RMSNormQuant yet: nothing to fuse
    assert fuse_llama_layers(model, fuse_residual=(m != 1.0)) == L                                # the Llama switch keeps refusing Granite (at 1.0 the flows coincide)
    assert residual_fused_layers(model) == 0
    keys, layers, classes = list(model.state_dict()), _layers(model), [type(l) for l in _layers(model)]
    children = [dict(l.named_children()) for l in layers]
    assert fuse_granite_residual(model) == L
    assert _layers(model) == layers and residual_fused_layers(model) == L and list(model.state_dict()) == keys
    for layer, cls, old in zip(layers, classes, children):
        assert isinstance(layer, ScaledResidualFusedLayer) and isinstance(layer, cls) and not isinstance(layer, ResidualFusedLayer)
        assert type(layer).forward is ScaledResidualFusedLayer.forward and type(layer).__name__ == "ScaledResidualFused" + cls.__name__
        assert dict(layer.named_children()) == old and all(dict(layer.named_children())[n] is c for n, c in old.items())
        assert isinstance(layer.input_layernorm, RMSNormQuant) and isinstance(layer.post_attention_layernorm, RMSNormQuant)
        assert layer.residual_multiplier == m and not layer._rf_inbox.pending
    assert [l._rf_next[0] for l in layers] == layers[1:] + [None] and model.model._rf_layers == layers
    hooks = len(model.model._forward_hooks)
    assert fuse_granite_residual(model) == 0 and residual_fused_layers(model) == L and len(model.model._forward_hooks) == hooks          # idempotent
    fuse_llama_layers(model, fuse_residual=True)                                                  # the Llama switch finds nothing to take from a fused layer
    assert residual_fused_layers(model) == L and all(type(l).forward is ScaledResidualFusedLayer.forward for l in layers)
    # a deep copy and a pickled copy are models of their own: fused layers of the same classes, linked among themselves, with empty hand-overs
    layers[1]._rf_inbox.put(torch.zeros(2), "q")
    for twin in (copy.deepcopy(model), pickle.loads(pickle.dumps(model))):
        tl = _layers(twin)
        assert [type(a) is type(b) and a is not b for a, b in zip(tl, layers)] == [True] * L
        assert [l._rf_next[0] for l in tl] == tl[1:] + [None] and twin.model._rf_layers == tl and not any(l._rf_inbox.pending for l in tl)
    assert layers[1]._rf_inbox.pending


@pytest.mark.parametrize("which", ["input_layernorm", "post_attention_layernorm"])
@pytest.mark.parametrize("kind", ["forward_hook", "forward_pre_hook"])
def test_a_layer_with_a_hooked_norm_is_refused_and_breaks_the_chain(which, kind):
    from protoquant_amd import ScaledResidualFusedLayer, fuse_granite_residual, fuse_llama_layers
    from protoquant_amd.llama import residual_fused_layers
    model = _granite()
    fuse_llama_layers(model)
    layers = _layers(model)
    norm = getattr(layers[1], which)
    handle = norm.register_forward_hook(lambda m, a, o: None) if kind == "forward_hook" else norm.register_forward_pre_hook(lambda m, a: None)
    cls = type(layers[1])
    assert fuse_granite_residual(model) == L - 1 and residual_fused_layers(model) == L - 1
    assert type(layers[1]) is cls and not hasattr(layers[1], "_rf_inbox")
    assert isinstance(layers[0], ScaledResidualFusedLayer) and layers[0]._rf_next == [None]          # the predecessor ends its chain (K1mo)
    assert isinstance(layers[2], ScaledResidualFusedLayer) and layers[2]._rf_next == [None]
    handle.remove()
    assert fuse_granite_residual(model) == 1 and residual_fused_layers(model) == L
    assert [l._rf_next[0] for l in layers] == layers[1:] + [None]


def test_other_refusals_keep_what_the_layer_had():
    from protoquant_amd import fuse_granite_residual, fuse_llama_layers
    model = _granite()
    fuse_llama_layers(model)
    layers = _layers(model)
    layers[0].residual_multiplier = torch.tensor(0.22)                          # a tensor multiplier
    stock = type(model.model.norm)(64)
    layers[2].post_attention_layernorm = stock                                  # a norm that is no RMSNormQuant
    classes = [type(l) for l in layers]
    assert fuse_granite_residual(model) == 1
    assert [type(l) is c for l, c in zip(layers, classes)] == [True, False, True] and layers[1]._rf_next == [None] and layers[2].post_attention_layernorm is stock

    model = _granite()
    fuse_llama_layers(model)
    layers = _layers(model)

    class ScalesTheResidual(type(layers[1])):
        def forward(self, hidden_states, **kwargs):
            r1 = hidden_states * self.residual_multiplier + self.self_attn(hidden_states=self.input_layernorm(hidden_states), **kwargs)[0]
            return r1 * self.residual_multiplier + self.mlp(self.post_attention_layernorm(r1))
    layers[1].__class__ = ScalesTheResidual
    assert fuse_granite_residual(model) == 2 and type(layers[1]) is ScalesTheResidual
    assert layers[0]._rf_next == [None] and layers[2]._rf_next == [None]


# ---------------------------------------------------------------------------------------------------------------- the kernel sequence of the fused forward
def test_fused_forward_runs_k1ma_with_each_layers_own_multiplier_and_ends_a_chain_with_k1mo(monkeypatch):
    """ScaledResidualFusedLayer.forward on stand-in layers, with recording CPU stand-ins for the two ops: the sequence of a chain of two layers and of its end, the
    multiplier read at call time from the layer whose add it is, the hand-over, and the tensor values of the eager flow"""
    from protoquant_amd import granite
    calls = []

    def fake_k1ma(x, residual, multiplier, weight, eps):
        calls.append(("K1ma", multiplier, weight, eps))
        s = residual + x * multiplier
        return ("q", s), s

    def fake_k1mo(x, residual, multiplier):
        calls.append(("K1mo", multiplier))
        return residual + x * multiplier

    monkeypatch.setattr(granite, "scaled_add_rmsnorm_quantize", fake_k1ma)
    monkeypatch.setattr(granite, "scaled_add", fake_k1mo)
    from protoquant_amd.residual_flow import _HandOver

    def standin(m, tag):
        norm_in = types.SimpleNamespace(weight=tag + ".in", variance_epsilon=1e-5)
        ns = types.SimpleNamespace(residual_multiplier=m, _rf_inbox=_HandOver(), _rf_next=[None], _rf_argnames=(), post_attention_layernorm=types.SimpleNamespace(weight=tag + ".post", variance_epsilon=1e-6))
        ns.input_layernorm = lambda t: (calls.append(("K1n", tag)), ("q", t))[1]
        ns.input_layernorm.weight, ns.input_layernorm.variance_epsilon = norm_in.weight, norm_in.variance_epsilon
        ns.self_attn = lambda hidden_states, **kw: (hidden_states[1] * 2.0 + 1.0, None)
        ns.mlp = lambda hq: hq[1] * 0.5 - 3.0
        return ns

    a, b = standin(0.5, "a"), standin(4.0, "b")
    a._rf_next = [b]
    fwd = granite.ScaledResidualFusedLayer.forward
    x = torch.arange(-6, 6, dtype=torch.float32).reshape(1, 3, 4)

    def eager(x, m):
        r1 = x + (x * 2.0 + 1.0) * m
        return r1 + (r1 * 0.5 - 3.0) * m

    out_a = fwd(a, x)
    assert torch.equal(out_a, eager(x, 0.5)) and b._rf_inbox.pending
    out_b = fwd(b, out_a)
    assert torch.equal(out_b, eager(out_a, 4.0)) and not b._rf_inbox.pending
    assert calls == [("K1n", "a"), ("K1ma", 0.5, "a.post", 1e-6), ("K1ma", 0.5, "b.in", 1e-5),          # the add into b's input norm is a's add: a's multiplier
                     ("K1ma", 4.0, "b.post", 1e-6), ("K1mo", 4.0)]
    # the multiplier is read at every call; a hidden state that is not the one handed over runs the layer's own input norm
    del calls[:]
    a.residual_multiplier = 0.25
    fwd(a, x)
    fwd(b, out_a.clone())
    assert [c[:2] for c in calls] == [("K1n", "a"), ("K1ma", 0.25), ("K1ma", 0.25), ("K1n", "b"), ("K1ma", 4.0), ("K1mo", 4.0)]
