"""CPU: fuse_layernorm_residual(model), run after fuse_layernorm_layers(model), on models whose linears are empty qlinears (tests/gptlike_models.fake_swap_linears): which blocks become
residual-fused and which are refused and left untouched, that fuse_layernorm_layers itself is what it was at the parent, that the probe recorded the attention call of each family, that copies
start with an empty hand-over, and that hand-written variants of the data flow are refused."""
import copy
import inspect
import pickle

import pytest
import torch
from torch import nn

from tests import gptlike_models as G

ACCEPTED = ["gpt2", "starcoder2", "gpt_neox_seq"]
REFUSED = ["gpt_neox", "opt", "phi", "falcon"]


def _fused(family, residual=False):
    """(model, what fuse_layernorm_layers returned, what fuse_layernorm_residual returned or None)"""
    from protoquant_amd import gptlike
    m = G.fake_swap_linears(G.build(family))
    n = gptlike.fuse_layernorm_layers(m)
    return m, n, (gptlike.fuse_layernorm_residual(m) if residual else None)


def _blocks(m):
    from protoquant_amd.gptlike import ResidualFusedBlock
    return [b for b in m.modules() if isinstance(b, ResidualFusedBlock)]


@pytest.mark.parametrize("family", ACCEPTED)
def test_accepted_families_become_residual_fused(family):
    from protoquant_amd import gptlike, llama
    plain, n0, _ = _fused(family)
    m, n1, nres = _fused(family, residual=True)
    assert n0 == n1 == 2 and nres == 2
    t0, t1 = G.module_types(plain), G.module_types(m)
    assert list(t0) == list(t1) and list(plain.state_dict()) == list(m.state_dict())
    changed = [n for n in t0 if t0[n] is not t1[n]]
    assert len(changed) == 2 and gptlike.residual_fused_blocks(m) == 2 and llama.residual_fused_layers(m) == 2 and gptlike.residual_fused_blocks(plain) == 0
    for n in changed:                                                   # a class derived from the fused class AND the original class, under a telling name
        assert issubclass(t1[n], gptlike.ResidualFusedBlock) and issubclass(t1[n], t0[n]) and t1[n].__name__ == "ResidualFused" + t0[n].__name__
    b0, b1 = _blocks(m)
    assert b0._rf_next[0] is b1 and b1._rf_next[0] is None              # the chain: the last block ends with a torch add
    owners = [o for o in m.modules() if hasattr(o, "_rf_layers")]
    assert len(owners) == 1 and owners[0]._rf_layers == [b0, b1]
    final = [mod for n, mod in m.named_modules() if n.split(".")[-1] in ("ln_f", "final_layer_norm", "norm")]
    assert len(final) == 1 and isinstance(final[0], nn.LayerNorm)       # the model's final norm is untouched
    # calling again changes nothing more
    before = G.module_types(m)
    hooks = len(owners[0]._forward_hooks)
    assert gptlike.fuse_layernorm_layers(m) == 0 and gptlike.fuse_layernorm_residual(m) == 0 and G.module_types(m) == before and len(owners[0]._forward_hooks) == hooks
    assert owners[0]._rf_layers == [b0, b1] and b0._rf_next[0] is b1


@pytest.mark.parametrize("family", REFUSED)
def test_refused_families_keep_every_module_object(family):
    from protoquant_amd import gptlike
    m = G.fake_swap_linears(G.build(family))
    gptlike.fuse_layernorm_layers(m)
    ids = {n: id(mod) for n, mod in m.named_modules()}
    types = G.module_types(m)
    hooks = {n: len(mod._forward_hooks) for n, mod in m.named_modules()}
    assert gptlike.fuse_layernorm_residual(m) == 0
    assert {n: id(mod) for n, mod in m.named_modules()} == ids and G.module_types(m) == types
    assert {n: len(mod._forward_hooks) for n, mod in m.named_modules()} == hooks
    assert gptlike.residual_fused_blocks(m) == 0 and not any(hasattr(mod, "_rf_layers") for mod in m.modules())


@pytest.mark.parametrize("family", ACCEPTED + REFUSED)
def test_fuse_layernorm_layers_alone_is_the_parent_behaviour(family):
    """the residual step is an entry of its own: fuse_layernorm_layers keeps its parameters and makes no residual-fused block, installs no hook, leaves no plan"""
    import protoquant_amd as pq
    from protoquant_amd import gptlike
    assert list(inspect.signature(gptlike.fuse_layernorm_layers).parameters) == ["model", "fuse_norms", "fuse_act"]
    assert list(inspect.signature(gptlike.fuse_layernorm_residual).parameters) == ["model"]
    assert pq.fuse_layernorm_residual is gptlike.fuse_layernorm_residual and "fuse_layernorm_residual" in pq.__all__ and "residual_fused_blocks" in pq.__all__
    b, nb, _ = _fused(family)
    assert nb == (0 if family == "falcon" else 2) and gptlike.residual_fused_blocks(b) == 0
    assert not any(hasattr(mod, "_rf_layers") or hasattr(mod, "_rfb_plan") or hasattr(mod, "_rf_inbox") for mod in b.modules())
    assert not any(isinstance(mod, gptlike.ResidualFusedBlock) for mod in b.modules())
    # before fuse_layernorm_layers there is no LayerNormQuant, hence nothing to fuse
    raw = G.fake_swap_linears(G.build(family))
    types = G.module_types(raw)
    assert gptlike.fuse_layernorm_residual(raw) == 0 and G.module_types(raw) == types


@pytest.mark.parametrize("order", ["first", "after"])
def test_starcoder2_with_fuse_llama_layers_in_either_order(order):
    from protoquant_amd import gptlike, llama
    m = G.fake_swap_linears(G.build("starcoder2"))
    if order == "first":
        assert llama.fuse_llama_layers(m, fuse_residual=True) == 2 and llama.residual_fused_layers(m) == 0          # that switch ignores LayerNorm layers
    gptlike.fuse_layernorm_layers(m)
    assert gptlike.fuse_layernorm_residual(m) == 2
    if order == "after":
        assert llama.fuse_llama_layers(m, fuse_residual=True) == 2
    assert gptlike.residual_fused_blocks(m) == 2 and llama.residual_fused_layers(m) == 2
    assert not any(isinstance(b, llama.ResidualFusedLayer) for b in m.modules())
    assert all(isinstance(b.self_attn.q_proj, llama._FusedSlice) for b in _blocks(m))


def test_the_recorded_attention_call():
    from protoquant_amd.gptlike import _H
    p = _blocks(_fused("gpt2", residual=True)[0])[0]._rfb_plan
    assert (p.n1, p.attn, p.n2, p.mlp) == ("ln_1", "attn", "ln_2", "mlp")
    assert p.args == (_H,) and p.kwargs == {k: ("param", k) for k in ("past_key_values", "attention_mask", "use_cache")} and p.var_kw
    assert set(p.withheld) == {"encoder_hidden_states", "encoder_attention_mask"} and p.stateless == ()
    p = _blocks(_fused("gpt_neox_seq", residual=True)[0])[0]._rfb_plan
    assert (p.n1, p.attn, p.n2, p.mlp) == ("input_layernorm", "attention", "post_attention_layernorm", "mlp")
    assert p.args == (_H,) and p.kwargs == {k: ("param", k) for k in ("attention_mask", "position_ids", "layer_past", "use_cache", "position_embeddings")} and p.var_kw
    assert p.withheld == () and set(p.stateless) == {"post_attention_dropout", "post_mlp_dropout"}
    p = _blocks(_fused("starcoder2", residual=True)[0])[0]._rfb_plan
    assert (p.n1, p.attn, p.n2, p.mlp) == ("input_layernorm", "self_attn", "post_attention_layernorm", "mlp")
    assert p.args == () and p.kwargs["hidden_states"] == _H and p.var_kw and p.withheld == ()
    assert {k for k, e in p.kwargs.items() if e != _H} == {"attention_mask", "position_ids", "past_key_values", "use_cache", "position_embeddings"}


@pytest.mark.parametrize("family", ACCEPTED)
def test_copies_start_with_an_empty_hand_over(family):
    from protoquant_amd import gptlike
    m, _, _ = _fused(family, residual=True)
    b0, b1 = _blocks(m)
    t = torch.zeros(2)
    b1._rf_inbox.put(t, "q")
    for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        c0, c1 = _blocks(c)
        assert type(c0).__name__ == type(b0).__name__ and issubclass(type(c0), b0._rfb_plan.cls)
        assert not c0._rf_inbox.pending and not c1._rf_inbox.pending and c0._rf_next[0] is c1 and c1 is not b1
        owner = [o for o in c.modules() if hasattr(o, "_rf_layers")][0]
        assert owner._rf_layers == [c0, c1] and list(c.state_dict()) == list(m.state_dict())
    assert b1._rf_inbox.pending and b1._rf_inbox.take(t) == "q"


# ---------------------------------------------------------------------------------------------------------------- hand-written variants
def _lnq():
    from protoquant_amd.gptlike import LayerNormQuant
    return LayerNormQuant(torch.ones(4), torch.zeros(4), 1e-5)


class _Attn(nn.Module):
    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(1))


class Base(nn.Module):
    def __init__(self):
        super().__init__()
        self.n_a, self.att, self.n_b, self.ff = _lnq(), _Attn(), _lnq(), _Attn()
        self.drop = nn.Dropout(0.1)
        self.third = nn.LayerNorm(4)


class Seq(Base):
    def forward(self, x, mask=None, cache=None, **kw):
        r1 = self.att(self.n_a(x), mask, cache=cache, flag=True, **kw)[0] + x
        return self.drop(self.ff(self.n_b(r1))) + r1


class ScaledResidual(Base):
    def forward(self, x, mask=None, **kw):
        r1 = x * 0.5 + self.att(self.n_a(x), mask, **kw)[0]
        return r1 + self.ff(self.n_b(r1))


class PostNorm(Base):
    def forward(self, x, mask=None, **kw):
        r1 = self.n_a(x + self.att(x, mask, **kw)[0])
        return self.n_b(r1 + self.ff(r1))


class ThirdNorm(Base):
    def forward(self, x, mask=None, **kw):
        r1 = x + self.att(self.n_a(x), mask, **kw)[0]
        return self.third(r1 + self.ff(self.n_b(r1)))


class AttnTwice(Base):
    def forward(self, x, mask=None, **kw):
        a = self.att(self.n_a(x), mask, **kw)[0]
        r1 = x + a
        return r1 + self.ff(self.n_b(r1)) + a * 0.0


class AttnAddedTwice(Base):
    def forward(self, x, mask=None, **kw):
        a = self.att(self.n_a(x), mask, **kw)[0]
        r1 = x + a + a
        return r1 + self.ff(self.n_b(r1))


class WritesInput(Base):
    def forward(self, x, mask=None, **kw):
        x += self.att(self.n_a(x), mask, **kw)[0]
        return x + self.ff(self.n_b(x))


class Parallel(Base):
    def forward(self, x, mask=None, **kw):
        return x + self.att(self.n_a(x), mask, **kw)[0] + self.ff(self.n_b(x))


class ReturnsTuple(Base):
    def forward(self, x, mask=None, **kw):
        r1 = x + self.att(self.n_a(x), mask, **kw)[0]
        return (r1 + self.ff(self.n_b(r1)),)


class Raises(Base):
    def forward(self, x, mask=None, **kw):
        raise RuntimeError("no")


class FlagTested(Base):
    def forward(self, x, mask=None, **kw):
        r1 = x + self.att(self.n_a(x), mask, **kw)[0]
        return r1 + self.ff(self.n_b(r1)) * (1.0 if mask is not None else 2.0)


class OneQuantNorm(Base):
    def __init__(self):
        super().__init__()
        self.n_b = nn.LayerNorm(4)

    forward = Seq.forward


def test_hand_written_variants():
    from protoquant_amd.gptlike import _H, residual_flow_plan
    p = residual_flow_plan(Seq())
    assert p is not None and (p.n1, p.attn, p.n2, p.mlp) == ("n_a", "att", "n_b", "ff")
    assert p.args == (_H, ("param", "mask")) and p.kwargs == {"cache": ("param", "cache"), "flag": ("const", True)} and p.var_kw and p.stateless == ("drop",)
    for cls in (ScaledResidual, PostNorm, ThirdNorm, AttnTwice, AttnAddedTwice, WritesInput, Parallel, ReturnsTuple, Raises, FlagTested, OneQuantNorm):
        assert residual_flow_plan(cls()) is None, cls.__name__


def test_a_stack_of_hand_written_blocks_links_only_what_it_accepts():
    from protoquant_amd import gptlike

    class Model(nn.Module):
        def __init__(self):
            super().__init__()
            self.h = nn.ModuleList([Seq(), Seq(), ScaledResidual(), Seq()])

    m = Model()
    refused = m.h[2]
    assert gptlike.fuse_layernorm_residual(m) == 3 and gptlike.residual_fused_blocks(m) == 3
    assert m.h[0]._rf_next[0] is m.h[1] and m.h[1]._rf_next[0] is None and m.h[3]._rf_next[0] is None          # the refused block breaks the chain
    assert m.h[2] is refused and type(refused) is ScaledResidual and isinstance(m.h[0], Seq)
