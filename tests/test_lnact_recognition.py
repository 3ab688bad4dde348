"""CPU: fuse_layernorm_layers recognises the LayerNorm-family decoders by probing their own code, changes nothing while probing, and refuses look-alikes.
The models are tiny random-init transformers decoders on the CPU whose linear layers were replaced by EMPTY qlinear modules (tests/gptlike_models.py): the
recognisers never touch a weight, so nothing here needs a GPU."""
import copy

import pytest
import torch
from torch import nn

from tests import gptlike_models as G


def _fused(model):
    from protoquant_amd.gptlike import ActQuant, LayerNormQuant
    mods = dict(model.named_modules())
    return sorted(n for n, m in mods.items() if isinstance(m, LayerNormQuant)), {n: m.kind for n, m in mods.items() if isinstance(m, ActQuant)}


# family -> (norms fused per layer, activation kind, names)
REQUIRED = {
    "gpt2": (("ln_1", "ln_2"), "gelu_tanh"),
    "starcoder2": (("input_layernorm", "post_attention_layernorm"), "gelu_tanh"),
    "gpt_neox": (("input_layernorm", "post_attention_layernorm"), "gelu_erf"),          # parallel residual
    "gpt_neox_seq": (("input_layernorm", "post_attention_layernorm"), "gelu_erf"),      # use_parallel_residual=False
}


@pytest.mark.parametrize("family", sorted(REQUIRED))
def test_required_families_are_fused_end_to_end(family):
    import protoquant_amd as pq
    model = G.fake_swap_linears(G.build(family, layers=3))
    keys = sorted(model.state_dict())
    n = pq.fuse_layernorm_layers(model)
    norms, acts = _fused(model)
    want_norms, kind = REQUIRED[family]
    assert n == 3 and len(norms) == 3 * len(want_norms) and all(x.rsplit(".", 1)[1] in want_norms for x in norms), (n, norms)
    assert len(acts) == 3 and set(acts.values()) == {kind}, acts
    assert sorted(model.state_dict()) == keys                                   # every state-dict key survives
    assert not any(isinstance(m, nn.LayerNorm) for name, m in model.named_modules() if name.rsplit(".", 1)[-1] in want_norms)
    # final norms feed the caller: left alone
    assert sum(isinstance(m, nn.LayerNorm) for m in model.modules()) == 1
    assert pq.fuse_layernorm_layers(model) == 0                                 # a second call finds nothing left


def test_other_families_fall_out_of_the_same_rules():
    """Phi: its single norm feeds attention AND the MLP (one quantisation, two consumers) and the tanh GELU is fused.  OPT: relu and the norm in front of fc1 are fused; the
    norm in front of the attention is not — OPT's attention reads hidden_states.size(), which a QTensor does not offer.  Falcon is left as it is."""
    import protoquant_amd as pq
    phi = G.fake_swap_linears(G.build("phi"))
    assert pq.fuse_layernorm_layers(phi) == 2
    norms, acts = _fused(phi)
    assert [n.rsplit(".", 1)[1] for n in norms] == ["input_layernorm"] * 2 and set(acts.values()) == {"gelu_tanh"} and len(acts) == 2
    opt = G.fake_swap_linears(G.build("opt"))
    assert pq.fuse_layernorm_layers(opt) == 2
    norms, acts = _fused(opt)
    assert [n.rsplit(".", 1)[1] for n in norms] == ["final_layer_norm"] * 2 and set(acts.values()) == {"relu"} and len(acts) == 2
    falcon = G.fake_swap_linears(G.build("falcon"))
    types = G.module_types(falcon)
    assert pq.fuse_layernorm_layers(falcon) == 0 and G.module_types(falcon) == types


def test_flags_select_the_fusions():
    import protoquant_amd as pq
    m = G.fake_swap_linears(G.build("gpt2"))
    assert pq.fuse_layernorm_layers(m, fuse_norms=False) == 2
    assert _fused(m)[0] == [] and len(_fused(m)[1]) == 2
    m = G.fake_swap_linears(G.build("gpt2"))
    assert pq.fuse_layernorm_layers(m, fuse_act=False) == 2
    assert len(_fused(m)[0]) == 4 and _fused(m)[1] == {}
    m = G.fake_swap_linears(G.build("gpt2"))
    assert pq.fuse_layernorm_layers(m, fuse_norms=False, fuse_act=False) == 0


def test_composes_with_fuse_llama_layers_in_either_order():
    import protoquant_amd as pq
    from protoquant_amd.llama import _FusedSlice
    for first in ("llama", "layernorm"):
        m = G.fake_swap_linears(G.build("starcoder2"))
        if first == "llama":
            assert pq.fuse_llama_layers(m) == 2 and pq.fuse_layernorm_layers(m) == 2
        else:
            assert pq.fuse_layernorm_layers(m) == 2 and pq.fuse_llama_layers(m) == 2
        norms, acts = _fused(m)
        assert len(norms) == 4 and len(acts) == 2
        assert sum(isinstance(x, _FusedSlice) for x in m.modules()) == 6
        assert not any(type(x).__name__ == "RMSNormQuant" for x in m.modules())


def test_probing_changes_nothing():
    """weights, RNG state, training flags, hooks, module objects: a model that is refused everywhere (swap_linears has not run) is exactly what it was, and a model
    that is accepted changes only in the replaced modules"""
    import protoquant_amd as pq
    for family in ("gpt2", "gpt_neox"):
        model = G.build(family).train()                                         # training mode: the dropouts would draw random numbers
        before = {k: v.clone() for k, v in model.state_dict().items()}
        ids = {n: id(m) for n, m in model.named_modules()}
        hooks = {n: (len(m._forward_hooks), len(m._forward_pre_hooks)) for n, m in model.named_modules()}
        rng = torch.random.get_rng_state()
        assert pq.fuse_layernorm_layers(model) == 0                             # nn.Linear / Conv1D projections: not swapped, nothing is fused
        assert torch.equal(torch.random.get_rng_state(), rng)
        assert {n: id(m) for n, m in model.named_modules()} == ids and all(m.training for m in model.modules())
        assert {n: (len(m._forward_hooks), len(m._forward_pre_hooks)) for n, m in model.named_modules()} == hooks
        after = model.state_dict()
        assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
        swapped = G.fake_swap_linears(model)
        sd = {k: v.clone() for k, v in swapped.state_dict().items()}
        rng = torch.random.get_rng_state()
        assert pq.fuse_layernorm_layers(swapped) == 2
        assert torch.equal(torch.random.get_rng_state(), rng) and all(m.training for m in swapped.modules())
        after = swapped.state_dict()
        assert list(after) == list(sd) and all(torch.equal(after[k], sd[k]) for k in sd)
        assert all(len(m._forward_hooks) == 0 and len(m._forward_pre_hooks) == 0 for m in swapped.modules())


def test_activation_kinds_are_told_by_behaviour():
    from protoquant_amd.gptlike import activation_kind
    tf = pytest.importorskip("transformers")
    A = tf.activations.ACT2FN
    assert activation_kind(nn.ReLU()) == "relu" and activation_kind(torch.relu) == "relu" and activation_kind(A["relu"]) == "relu"
    assert activation_kind(nn.GELU()) == "gelu_erf" and activation_kind(A["gelu"]) == "gelu_erf" and activation_kind(torch.nn.functional.gelu) == "gelu_erf"
    assert activation_kind(nn.GELU(approximate="tanh")) == "gelu_tanh" and activation_kind(A["gelu_new"]) == "gelu_tanh" and activation_kind(A["gelu_pytorch_tanh"]) == "gelu_tanh"
    for name in ("quick_gelu", "gelu_10", "relu2", "silu", "gelu_fast", "tanh", "sigmoid", "mish", "relu6", "leaky_relu"):
        if name in A:
            got = activation_kind(A[name])
            assert got is None or (name == "gelu_fast" and got == "gelu_tanh"), (name, got)
    assert activation_kind(nn.PReLU()) is None and activation_kind(nn.Identity()) is None and activation_kind(None) is None

    class Raises(nn.Module):
        def forward(self, x):
            raise RuntimeError("no")
    assert activation_kind(Raises()) is None


class _Block(nn.Module):
    """GPT-2's data flow written out, from empty qlinear modules"""

    def __init__(self, H=32, act=None, norm=None):
        super().__init__()
        from protoquant_amd.qlinear import qlinear
        self.ln_1, self.ln_2 = (norm or nn.LayerNorm)(H), (norm or nn.LayerNorm)(H)
        self.c_attn, self.c_proj = qlinear(H, H), qlinear(H, H)
        self.mlp = _MLP(H, act)

    def forward(self, x):
        x = x + self.c_proj(self.c_attn(self.ln_1(x)))
        return x + self.mlp(self.ln_2(x))


class _MLP(nn.Module):
    def __init__(self, H=32, act=None):
        super().__init__()
        from protoquant_amd.qlinear import qlinear
        self.c_fc, self.c_proj, self.act, self.drop = qlinear(H, 4 * H), qlinear(4 * H, H), act if act is not None else nn.GELU(), nn.Dropout(0.1)

    def forward(self, x):
        return self.drop(self.c_proj(self.act(self.c_fc(x))))


def test_look_alikes_are_refused_and_left_untouched():
    import protoquant_amd as pq
    from protoquant_amd.gptlike import fusable_activation, fusable_norms

    good = _Block()
    assert fusable_norms(good) == ["ln_1", "ln_2"] and fusable_activation(good.mlp) == ("act", "gelu_erf")

    class OwnForward(nn.LayerNorm):
        def forward(self, x):
            return super().forward(x) * 2.0

    class ReadsDtype(_Block):
        def forward(self, x):
            h = self.ln_1(x)
            x = x + self.c_proj(self.c_attn(h)).to(h.dtype)
            return x + self.mlp(self.ln_2(x))

    class AddsToNorm(_Block):
        def forward(self, x):
            x = x + self.c_proj(self.c_attn(self.ln_1(x) + 1.0))
            return x + self.mlp(self.ln_2(x))

    class ReturnsNorm(_Block):
        def forward(self, x):
            h = self.ln_1(x)
            return x + self.c_proj(self.c_attn(h)), h

    class NormTwice(_Block):
        def forward(self, x):
            self.ln_1(x)
            x = x + self.c_proj(self.c_attn(self.ln_1(x)))
            return x + self.mlp(self.ln_2(x))

    class DropBetween(_MLP):
        def forward(self, x):
            return self.c_proj(self.drop(self.act(self.c_fc(x))))

    class ScaledAct(_MLP):
        def forward(self, x):
            return self.c_proj(self.act(self.c_fc(x) * 1.0))

    class ActNotOnProjection(_MLP):
        def forward(self, x):
            return self.c_proj(self.act(x.repeat(1, 1, 4)))

    for blk, want in ((_Block(norm=OwnForward), []), (ReadsDtype(), ["ln_2"]), (AddsToNorm(), ["ln_2"]), (ReturnsNorm(), []), (NormTwice(), ["ln_2"])):
        types = G.module_types(blk)
        assert fusable_norms(blk) == want, type(blk).__name__
        assert G.module_types(blk) == types
    noaffine = _Block()
    noaffine.ln_1 = nn.LayerNorm(32, elementwise_affine=False)
    assert fusable_norms(noaffine) == ["ln_2"]
    two_d = _Block()
    two_d.ln_1 = nn.LayerNorm((1, 32))
    assert "ln_1" not in fusable_norms(two_d)
    A = pytest.importorskip("transformers").activations.ACT2FN
    for mlp in (DropBetween(), ScaledAct(), ActNotOnProjection(), _MLP(act=A["quick_gelu"]), _MLP(act=nn.SiLU()), _MLP(act=nn.PReLU())):
        types = G.module_types(mlp)
        assert fusable_activation(mlp) is None, type(mlp).__name__
        assert G.module_types(mlp) == types
    # whole blocks through the entry point: refused parts stay the objects they were
    for blk in (ReadsDtype(), AddsToNorm()):
        ln1 = blk.ln_1
        assert pq.fuse_layernorm_layers(blk) == 1 and blk.ln_1 is ln1 and type(blk.ln_2).__name__ == "LayerNormQuant" and type(blk.mlp.act).__name__ == "ActQuant"
    d = nn.ModuleList([_Block(norm=OwnForward)])
    d[0].mlp = DropBetween()
    types = G.module_types(d)
    assert pq.fuse_layernorm_layers(d) == 0 and G.module_types(d) == types
    # a model on which swap_linears has not run
    plain = G.build("gpt2")
    types = G.module_types(plain)
    assert pq.fuse_layernorm_layers(plain) == 0 and G.module_types(plain) == types
