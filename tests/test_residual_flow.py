"""CPU: what protoquant_amd/residual_flow.py gives every fused kind alike, on the tiny models of the five recognition test files: a copy of a fused model — deep or
pickled — is a fused model of its own, every public entry point finds nothing left to change in a second call, and the one rule in which the name-based probes differ
(probe_named_flow's attn_positional) is what it was per family."""
import copy
import pickle

import pytest
import torch
from torch import nn

tr = pytest.importorskip("transformers")

from tests import test_addlnorm_recognition as seq  # noqa: E402  (the tiny models of the recognition tests)
from tests import test_olmo_recognition as olmo  # noqa: E402
from tests import test_parallel_recognition as par  # noqa: E402
from tests.test_gemma_postnorm_recognition import _llama_model  # noqa: E402
from tests.test_gemma_recognition import _model as _gemma_model  # noqa: E402


def _llama():
    from protoquant_amd.llama import ResidualFusedLayer, fuse_llama_layers
    m = _llama_model()
    return m, ResidualFusedLayer, lambda: fuse_llama_layers(m, fuse_residual=True)


def _sandwich():
    from protoquant_amd import SandwichFusedLayer, fuse_gemma_layers, fuse_gemma_postnorm_residual
    m = _gemma_model("gemma2")
    fuse_gemma_layers(m)
    return m, SandwichFusedLayer, lambda: fuse_gemma_postnorm_residual(m)


def _postnorm():
    from protoquant_amd import PostNormFusedLayer, fuse_olmo_layers
    m = olmo._model("olmo2")
    return m, PostNormFusedLayer, lambda: fuse_olmo_layers(m, fuse_residual=True)


def _sequential():
    from protoquant_amd.gptlike import ResidualFusedBlock, fuse_layernorm_residual
    m = seq._fused("gpt2")[0]
    return m, ResidualFusedBlock, lambda: fuse_layernorm_residual(m)


def _parallel():
    from protoquant_amd.gptlike import ParallelFusedBlock, fuse_parallel_residual
    m = par._fused("gpt_neox")[0]
    return m, ParallelFusedBlock, lambda: fuse_parallel_residual(m)


# kind -> (model before its residual entry ran, the fused kind, the entry point), the number of layers of the model
KINDS = {"llama": (_llama, 2), "sandwich": (_sandwich, 3), "postnorm": (_postnorm, 3), "sequential": (_sequential, 2), "parallel": (_parallel, 2)}


def _fused_layers(model, kind):
    return [m for m in model.modules() if isinstance(m, kind)]


@pytest.mark.parametrize("name", list(KINDS))
def test_every_entry_point_returns_zero_the_second_time(name):
    build, n = KINDS[name]
    model, kind, entry = build()
    assert entry() == n and len(_fused_layers(model, kind)) == n
    types = {k: type(m) for k, m in model.named_modules()}
    assert entry() == 0 and {k: type(m) for k, m in model.named_modules()} == types


@pytest.mark.parametrize("how", ["deepcopy", "pickle"])
@pytest.mark.parametrize("name", list(KINDS))
def test_a_copy_is_a_fused_model_of_its_own(name, how):
    build, n = KINDS[name]
    model, kind, entry = build()
    assert entry() == n
    layers = _fused_layers(model, kind)
    key = torch.zeros(2)
    for l in layers:
        l._rf_inbox.put(key, "q")
    twin = copy.deepcopy(model) if how == "deepcopy" else pickle.loads(pickle.dumps(model))
    copies = _fused_layers(twin, kind)
    assert len(copies) == n and not any(c is l for c in copies for l in layers)
    for c, l in zip(copies, layers):          # the same run-time class, made again from the original class
        original = type(l).__bases__[1]
        assert type(c) is type(l) and type(c).__bases__ == (kind, original) and isinstance(c, original) and type(c).__name__ == kind._pq_prefix + original.__name__
    assert not any(c._rf_inbox.pending for c in copies) and all(l._rf_inbox.pending for l in layers)          # a copy starts empty; the original keeps what it held
    assert [c._rf_next[0] for c in copies] == copies[1:] + [None]                                              # linked among themselves
    assert list(twin.state_dict()) == list(model.state_dict())
    # the owner's clearing hook clears the copy's layers, and no others
    owners = [o for o in twin.modules() if hasattr(o, "_rf_layers")]
    assert len(owners) == 1 and owners[0]._rf_layers == copies
    for c in copies:
        c._rf_inbox.put(key, "q")
    for hook in owners[0]._forward_hooks.values():
        hook(owners[0], (), None)
    assert not any(c._rf_inbox.pending for c in copies) and all(l._rf_inbox.pending for l in layers)


def test_probe_named_flow_accepts_a_positional_hidden_state_only_where_asked_to():
    """With Llama's table a forward that calls self_attn(h, **kwargs) is refused unless attn_positional=True, which residual_flow_is_llama sets; the sandwich and the
    post-norm flow refuse that forward through probe_named_flow on their tables and through their public probes, which never set the switch; every table accepts the
    keyword form under either setting."""
    from protoquant_amd import gemma, llama
    from protoquant_amd import olmo as pq_olmo
    from protoquant_amd.residual_flow import probe_named_flow

    def flows(call):
        class Llama(nn.Module):
            def forward(self, hidden_states, position_ids=None, **kwargs):
                r1 = hidden_states + call(self.self_attn, self.input_layernorm(hidden_states), position_ids=position_ids, **kwargs)[0]
                return r1 + self.mlp(self.post_attention_layernorm(r1))

        class Sandwich(nn.Module):
            def forward(self, hidden_states, **kwargs):
                r1 = hidden_states + self.post_attention_layernorm(call(self.self_attn, self.input_layernorm(hidden_states), **kwargs)[0])
                return r1 + self.post_feedforward_layernorm(self.mlp(self.pre_feedforward_layernorm(r1)))

        class PostNorm(nn.Module):
            def forward(self, hidden_states, **kwargs):
                r1 = hidden_states + self.post_attention_layernorm(call(self.self_attn, hidden_states, **kwargs)[0])
                return r1 + self.post_feedforward_layernorm(self.mlp(r1))
        return Llama, Sandwich, PostNorm

    by_keyword = flows(lambda attn, h, **kw: attn(hidden_states=h, **kw))
    positional = flows(lambda attn, h, **kw: attn(h, **kw))
    layers = (_llama_model().model.layers[0], _gemma_model("gemma2").model.layers[0], olmo._model("olmo2").model.layers[0])
    tables = ((llama._CHILDREN, llama._llama_flow), (gemma._SANDWICH, gemma._sandwich_flow), (pq_olmo._POSTNORM, pq_olmo._postnorm_flow))
    for i, (layer, (children, want)) in enumerate(zip(layers, tables)):
        for switch in (False, True):
            assert probe_named_flow(layer, by_keyword[i], children, want, attn_positional=switch), (i, switch)
        assert not probe_named_flow(layer, positional[i], children, want), i
        # a table is its own flow's and no other's
        assert not any(probe_named_flow(layer, by_keyword[j], children, want, attn_positional=True) for j in range(3) if j != i), i
    assert probe_named_flow(layers[0], positional[0], *tables[0], attn_positional=True)
    # the public probes: the switch is Llama's alone, so the other two refuse the positional form either way — through the table and through their entry
    assert llama.residual_flow_is_llama(layers[0], positional[0]) and llama.residual_flow_is_llama(layers[0], by_keyword[0])
    assert not gemma.residual_flow_is_sandwich(layers[1], positional[1]) and gemma.residual_flow_is_sandwich(layers[1], by_keyword[1])
    assert not pq_olmo.residual_flow_is_postnorm(layers[2], positional[2]) and pq_olmo.residual_flow_is_postnorm(layers[2], by_keyword[2])
