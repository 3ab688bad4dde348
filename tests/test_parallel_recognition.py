"""CPU: fuse_parallel_residual(model), run after fuse_layernorm_layers(model), on models whose linears are empty qlinears (tests/gptlike_models.fake_swap_linears):
GPT-NeoX with a parallel residual and Phi become parallel-fused with the association of their three-way sum recorded; every other family is refused with every
module object untouched; fuse_layernorm_layers and fuse_layernorm_residual give on these models what they gave before; copies start with an empty hand-over; and
hand-written variants of the data flow are accepted with the association they have, or refused."""
import copy
import inspect
import pickle

import pytest
import torch
from torch import nn

from tests import gptlike_models as G

ACCEPTED = ["gpt_neox", "phi"]
REFUSED = ["gpt_neox_seq", "gpt2", "starcoder2", "opt", "falcon", "gptj", "cohere"]


def _build(family):
    """the families of tests/gptlike_models, and GPT-J and Cohere (parallel residuals whose norms fuse_layernorm_layers does not fuse today), built here"""
    if family not in ("gptj", "cohere"):
        return G.build(family)
    tf = pytest.importorskip("transformers")
    torch.manual_seed(0)
    if family == "gptj":
        return tf.GPTJForCausalLM(tf.GPTJConfig(n_embd=64, n_layer=2, n_head=4, n_positions=64, rotary_dim=8, **G.COMMON)).eval()
    return tf.CohereForCausalLM(tf.CohereConfig(hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                                                max_position_embeddings=64, **G.COMMON)).eval()


def _fused(family, parallel=False):
    """(model, what fuse_layernorm_layers returned, what fuse_parallel_residual returned or None)"""
    from protoquant_amd import gptlike
    m = G.fake_swap_linears(_build(family))
    n = gptlike.fuse_layernorm_layers(m)
    return m, n, (gptlike.fuse_parallel_residual(m) if parallel else None)


def _blocks(m):
    from protoquant_amd.gptlike import ParallelFusedBlock
    return [b for b in m.modules() if isinstance(b, ParallelFusedBlock)]


@pytest.mark.parametrize("family", ACCEPTED)
def test_accepted_families_become_parallel_fused(family):
    from protoquant_amd import gptlike
    plain, n0, _ = _fused(family)
    m, n1, npar = _fused(family, parallel=True)
    assert n0 == n1 == 2 and npar == 2
    t0, t1 = G.module_types(plain), G.module_types(m)
    assert list(t0) == list(t1) and list(plain.state_dict()) == list(m.state_dict())          # the same modules under the same names, the same state-dict keys
    changed = [n for n in t0 if t0[n] is not t1[n]]
    assert len(changed) == 2 and gptlike.parallel_fused_blocks(m) == 2 and gptlike.parallel_fused_blocks(plain) == 0 and gptlike.residual_fused_blocks(m) == 0
    for n in changed:                                                   # a class derived from the fused class AND the original class, under a telling name
        assert issubclass(t1[n], gptlike.ParallelFusedBlock) and issubclass(t1[n], t0[n]) and t1[n].__name__ == "ParallelFused" + t0[n].__name__
    b0, b1 = _blocks(m)
    assert b0._rf_next[0] is b1 and b1._rf_next[0] is None              # the chain: the last block ends with the two torch adds
    owners = [o for o in m.modules() if hasattr(o, "_rf_layers")]
    assert len(owners) == 1 and owners[0]._rf_layers == [b0, b1]
    final = [mod for n, mod in m.named_modules() if n.split(".")[-1] in ("final_layer_norm", "final_layernorm")]
    assert len(final) == 1 and isinstance(final[0], nn.LayerNorm)       # the model's final norm is untouched
    # the norm modules stay the model's, object for object
    assert all(isinstance(getattr(b, n), gptlike.LayerNormQuant) for b in (b0, b1) for n in b._pfb_plan.norms)
    # calling again changes nothing more, and the sequential entry finds nothing to take
    before = G.module_types(m)
    hooks = len(owners[0]._forward_hooks)
    assert gptlike.fuse_parallel_residual(m) == 0 and gptlike.fuse_layernorm_layers(m) == 0 and gptlike.fuse_layernorm_residual(m) == 0
    assert G.module_types(m) == before and len(owners[0]._forward_hooks) == hooks and owners[0]._rf_layers == [b0, b1] and b0._rf_next[0] is b1


def test_the_recorded_flow_per_family():
    """the pair that is added first is the two branch outputs in both families (GPT-NeoX: mlp + attn, Phi: attn + mlp; an add commutes), the input comes last"""
    from protoquant_amd.gptlike import _H
    p = _blocks(_fused("gpt_neox", parallel=True)[0])[0]._pfb_plan
    assert (p.attn, p.mlp, p.attn_norm, p.mlp_norm, p.norms) == ("attention", "mlp", "input_layernorm", "post_attention_layernorm", ("input_layernorm", "post_attention_layernorm"))
    assert set(p.order[:2]) == {"m", "a"} and p.order[2] == "x"
    assert p.args == (_H,) and p.kwargs == {k: ("param", k) for k in ("attention_mask", "position_ids", "layer_past", "use_cache", "position_embeddings")} and p.var_kw
    assert p.withheld == () and set(p.stateless) == {"post_attention_dropout", "post_mlp_dropout"}
    p = _blocks(_fused("phi", parallel=True)[0])[0]._pfb_plan
    assert (p.attn, p.mlp, p.attn_norm, p.mlp_norm, p.norms) == ("self_attn", "mlp", "input_layernorm", "input_layernorm", ("input_layernorm",))
    assert set(p.order[:2]) == {"a", "m"} and p.order[2] == "x"
    assert p.args == () and p.kwargs["hidden_states"] == _H and p.var_kw and p.withheld == () and p.stateless == ("resid_dropout",)
    assert {k for k, e in p.kwargs.items() if e != _H} == {"attention_mask", "position_ids", "past_key_values", "use_cache", "position_embeddings"}


@pytest.mark.parametrize("family", REFUSED)
def test_refused_families_keep_every_module_object(family):
    from protoquant_amd import gptlike
    m = G.fake_swap_linears(_build(family))
    gptlike.fuse_layernorm_layers(m)
    ids = {n: id(mod) for n, mod in m.named_modules()}
    types = G.module_types(m)
    hooks = {n: len(mod._forward_hooks) for n, mod in m.named_modules()}
    assert gptlike.fuse_parallel_residual(m) == 0
    assert {n: id(mod) for n, mod in m.named_modules()} == ids and G.module_types(m) == types
    assert {n: len(mod._forward_hooks) for n, mod in m.named_modules()} == hooks
    assert gptlike.parallel_fused_blocks(m) == 0 and not any(hasattr(mod, "_rf_layers") or hasattr(mod, "_pfb_plan") for mod in m.modules())


@pytest.mark.parametrize("family", ACCEPTED + REFUSED)
def test_the_other_entries_are_what_they_were(family):
    """fuse_parallel_residual is an entry of its own: fuse_layernorm_layers and fuse_layernorm_residual keep their parameters and their answers — in particular the
    sequential entry still refuses the parallel blocks, and neither leaves a parallel plan, an inbox or a hook behind"""
    import protoquant_amd as pq
    from protoquant_amd import gptlike
    assert list(inspect.signature(gptlike.fuse_layernorm_layers).parameters) == ["model", "fuse_norms", "fuse_act"]
    assert list(inspect.signature(gptlike.fuse_layernorm_residual).parameters) == ["model"] and list(inspect.signature(gptlike.fuse_parallel_residual).parameters) == ["model"]
    assert pq.fuse_parallel_residual is gptlike.fuse_parallel_residual
    fused_blocks = {"falcon": 0, "cohere": 0}.get(family, 2)          # (what fuse_layernorm_layers changes in these models; GPT-J: the activation of its MLP, and no norm)
    b, nb, _ = _fused(family)
    assert nb == fused_blocks and gptlike.parallel_fused_blocks(b) == 0
    if family in ("falcon", "gptj", "cohere"):          # the out-of-scope families: none of their norms is a LayerNormQuant, so there is nothing to probe
        assert not any(isinstance(mod, gptlike.LayerNormQuant) for mod in b.modules())
    assert not any(hasattr(mod, "_rf_layers") or hasattr(mod, "_pfb_plan") or hasattr(mod, "_rf_inbox") for mod in b.modules())
    types = G.module_types(b)
    nres = gptlike.fuse_layernorm_residual(b)
    assert nres == (2 if family in ("gpt_neox_seq", "gpt2", "starcoder2") else 0) and gptlike.residual_fused_blocks(b) == nres
    if nres == 0:
        assert G.module_types(b) == types and not any(hasattr(mod, "_rf_layers") for mod in b.modules())
    assert gptlike.fuse_parallel_residual(b) == (2 if family in ACCEPTED else 0)          # after the sequential entry as well: the two do not take each other's blocks
    # before fuse_layernorm_layers there is no LayerNormQuant, hence nothing to fuse
    raw = G.fake_swap_linears(_build(family))
    types = G.module_types(raw)
    assert gptlike.fuse_parallel_residual(raw) == 0 and G.module_types(raw) == types
    for blk in raw.modules():
        assert gptlike.parallel_flow_plan(blk) is None and gptlike.residual_flow_plan(blk) is None


@pytest.mark.parametrize("family", ACCEPTED)
def test_copies_start_with_an_empty_hand_over(family):
    m, _, _ = _fused(family, parallel=True)
    b0, b1 = _blocks(m)
    t = torch.zeros(2)
    b1._rf_inbox.put(t, ("q1", "q2"))
    for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        c0, c1 = _blocks(c)
        assert type(c0).__name__ == type(b0).__name__ and issubclass(type(c0), b0._pfb_plan.cls)
        assert not c0._rf_inbox.pending and not c1._rf_inbox.pending and c0._rf_next[0] is c1 and c1 is not b1
        owner = [o for o in c.modules() if hasattr(o, "_rf_layers")][0]
        assert owner._rf_layers == [c0, c1] and list(c.state_dict()) == list(m.state_dict())
    assert b1._rf_inbox.pending and b1._rf_inbox.take(t) == ("q1", "q2")


# ---------------------------------------------------------------------------------------------------------------- hand-written variants
def _lnq():
    from protoquant_amd.gptlike import LayerNormQuant
    return LayerNormQuant(torch.ones(4), torch.zeros(4), 1e-5)


class _Child(nn.Module):
    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(1))


class Base(nn.Module):
    def __init__(self):
        super().__init__()
        self.n_a, self.att, self.n_b, self.ff = _lnq(), _Child(), _lnq(), _Child()
        self.drop = nn.Dropout(0.1)
        self.third = nn.LayerNorm(4)


class BranchesFirst(Base):          # GPT-NeoX's grouping
    def forward(self, x, mask=None, cache=None, **kw):
        a = self.att(self.n_a(x), mask, cache=cache, flag=True, **kw)[0]
        return self.drop(self.ff(self.n_b(x))) + a + x


class InputAndAttnFirst(Base):
    def forward(self, x, mask=None, **kw):
        return (x + self.att(self.n_a(x), mask, **kw)[0]) + self.ff(self.n_b(x))


class InputAndMlpFirst(Base):
    def forward(self, x, mask=None, **kw):
        a = self.att(self.n_a(x), mask, **kw)[0]
        return (self.ff(self.n_b(x)) + x) + a


class OneNorm(Base):                # Phi's shape: both branches read the same norm
    def __init__(self):
        super().__init__()
        self.n_b = nn.LayerNorm(4)

    def forward(self, x, mask=None, **kw):
        h = self.n_a(x)
        return self.att(hidden=h, mask=mask, **kw)[0] + self.ff(h) + x


class ScaledSum(Base):
    def forward(self, x, mask=None, **kw):
        return x + self.att(self.n_a(x), mask, **kw)[0] * 0.5 + self.ff(self.n_b(x))


class ScaledInput(Base):
    def forward(self, x, mask=None, **kw):
        return x * 0.5 + self.att(self.n_a(x), mask, **kw)[0] + self.ff(self.n_b(x))


class NormOfAttnOut(Base):          # a sequential residual in disguise: the second norm does not read the input
    def forward(self, x, mask=None, **kw):
        a = self.att(self.n_a(x), mask, **kw)[0]
        return x + a + self.ff(self.n_b(a))


class Sequential(Base):
    def forward(self, x, mask=None, **kw):
        r1 = x + self.att(self.n_a(x), mask, **kw)[0]
        return r1 + self.ff(self.n_b(r1))


class FourWay(Base):                # a sum that is none of the three groupings of x + a + m
    def forward(self, x, mask=None, **kw):
        a = self.att(self.n_a(x), mask, **kw)[0]
        m = self.ff(self.n_b(x))
        return (x * 0.5 + a) + (m + x * 0.5)


class ThirdNorm(Base):
    def forward(self, x, mask=None, **kw):
        return self.third(x + self.att(self.n_a(x), mask, **kw)[0] + self.ff(self.n_b(x)))


class ReturnsTuple(Base):
    def forward(self, x, mask=None, **kw):
        a, w = self.att(self.n_a(x), mask, **kw)
        return x + a + self.ff(self.n_b(x)), w


class AttnUsedTwice(Base):
    def forward(self, x, mask=None, **kw):
        a = self.att(self.n_a(x), mask, **kw)[0]
        return x + a + self.ff(self.n_b(x)) + a * 0.0


class WritesInput(Base):
    def forward(self, x, mask=None, **kw):
        x += self.att(self.n_a(x), mask, **kw)[0]
        return x + self.ff(self.n_b(x))


class FlagTested(Base):
    def forward(self, x, mask=None, **kw):
        return x + self.att(self.n_a(x), mask, **kw)[0] + self.ff(self.n_b(x)) * (1.0 if mask is not None else 2.0)


class Raises(Base):
    def forward(self, x, mask=None, **kw):
        raise RuntimeError("no")


def test_hand_written_variants():
    from protoquant_amd.gptlike import _H, parallel_flow_plan
    p = parallel_flow_plan(BranchesFirst())
    assert p is not None and (p.attn, p.mlp, p.attn_norm, p.mlp_norm) == ("att", "ff", "n_a", "n_b") and set(p.order[:2]) == {"a", "m"} and p.order[2] == "x"
    assert p.args == (_H, ("param", "mask")) and p.kwargs == {"cache": ("param", "cache"), "flag": ("const", True)} and p.var_kw and p.stateless == ("drop",)
    p = parallel_flow_plan(InputAndAttnFirst())          # the association (x + attn) + mlp is accepted and recorded as such
    assert p is not None and set(p.order[:2]) == {"x", "a"} and p.order[2] == "m"
    p = parallel_flow_plan(InputAndMlpFirst())
    assert p is not None and set(p.order[:2]) == {"x", "m"} and p.order[2] == "a"
    p = parallel_flow_plan(OneNorm())
    assert p is not None and p.norms == ("n_a",) and p.attn_norm == p.mlp_norm == "n_a" and p.args == () and p.kwargs == {"hidden": _H, "mask": ("param", "mask")}
    for cls in (ScaledSum, ScaledInput, NormOfAttnOut, Sequential, FourWay, ThirdNorm, ReturnsTuple, AttnUsedTwice, WritesInput, FlagTested, Raises):
        assert parallel_flow_plan(cls()) is None, cls.__name__
    hooked = BranchesFirst()
    hooked.n_b.register_forward_hook(lambda mod, args, out: None)
    assert parallel_flow_plan(hooked) is None          # the fused block would no longer call the norm: its hook would stop firing
    pre = BranchesFirst()
    pre.n_a.register_forward_pre_hook(lambda mod, args: None)
    assert parallel_flow_plan(pre) is None


def test_a_stack_of_hand_written_blocks_links_only_what_it_accepts():
    from protoquant_amd import gptlike

    class Model(nn.Module):
        def __init__(self):
            super().__init__()
            self.h = nn.ModuleList([BranchesFirst(), OneNorm(), ScaledSum(), InputAndAttnFirst(), BranchesFirst(), BranchesFirst()])

    m = Model()
    m.h[4].n_a.register_forward_hook(lambda mod, args, out: None)
    refused, hooked = m.h[2], m.h[4]
    assert gptlike.fuse_parallel_residual(m) == 4 and gptlike.parallel_fused_blocks(m) == 4
    nxt = [getattr(b, "_rf_next", ["-"])[0] for b in m.h]
    assert nxt == [m.h[1], None, "-", None, "-", None]          # a refused block, scaled or hooked, breaks the chain: its predecessor ends with torch adds
    assert m.h[2] is refused and type(refused) is ScaledSum and m.h[4] is hooked and type(hooked) is BranchesFirst and isinstance(m.h[0], BranchesFirst)
    assert m._rf_layers == [m.h[0], m.h[1], m.h[3], m.h[5]]
