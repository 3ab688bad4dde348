"""Which routers of real model code fuse_moe_routers takes (protoquant_amd.moe_router.router_parts: a probe of the class's own forward on the CPU) and which it
refuses: no GPU, no library call — tiny transformers models built from a config on the CPU.  "Taken": the router object stays, with the same parameters and state-dict
keys, as an instance of a class derived from its own; "refused": fuse_moe_routers returns 0 and every module object, class and state-dict key is what it was.

| family                       | outcome on transformers 5.15                                                                       |
| Mixtral                      | taken: softmax_topk, renormalised, f32 scores                                                      |
| Qwen3-MoE, Qwen2-MoE, OLMoE  | taken: softmax_topk, the flag read from norm_topk_prob at run time, scores in the logits' dtype    |
| GPT-OSS                      | taken: topk_softmax, with its bias                                                                 |
| GraniteMoe                   | taken: topk_softmax; returns (indices, scores, logits) with f32 logits, which the probe records    |
| DeepSeek-V3                  | refused: a correction-bias buffer (and a sigmoid, grouped top-k forward)                           |
| Phi-MoE                      | refused: the router is a subclass of nn.Linear (sparsemixer)                                       |
| DeepSeek-V4                  | refused: the probe finds none of the three recipes                                                 |
| a dense Llama                | refused: no router                                                                                 |
| a router carrying a hook     | refused                                                                                            |"""
import pytest
import torch
from torch import nn

tr = pytest.importorskip("transformers")

import protoquant_amd as pq                          # noqa: E402
from protoquant_amd import moe                       # noqa: E402
from protoquant_amd import serialize as S            # noqa: E402
from protoquant_amd.moe_router import RouterParts, router_parts   # noqa: E402
from tests import moe_models as M                    # noqa: E402

TAKEN = {
    # family: (kind, renormalise, renorm_attr, scores_f32, logits_f32, flatten, has_bias, (pos_logits, pos_scores, pos_indices))
    "mixtral": ("softmax_topk", True, None, True, False, True, False, (0, 1, 2)),
    "qwen3_moe": ("softmax_topk", True, "norm_topk_prob", False, False, True, False, (0, 1, 2)),
    "qwen2_moe": ("softmax_topk", False, "norm_topk_prob", False, False, True, False, (0, 1, 2)),
    "olmoe": ("softmax_topk", False, "norm_topk_prob", False, False, True, False, (0, 1, 2)),
    "gpt_oss": ("topk_softmax", False, None, False, False, False, True, (0, 1, 2)),
    "granitemoe": ("topk_softmax", False, None, False, True, False, False, (2, 1, 0)),
}
REFUSED = ("deepseek_v3", "phimoe", "deepseek_v4", "llama")


def _snapshot(model):
    return [(n, id(m), type(m)) for n, m in model.named_modules()], list(model.state_dict().keys()), [id(p) for p in model.parameters()]


def _routers(model):
    return [(n, m) for n, m in model.named_modules() if getattr(m, "_pq_router", None) is not None]


@pytest.mark.parametrize("family", sorted(TAKEN))
@pytest.mark.parametrize("E,k", ((4, 2), (8, 2)))
def test_routers_of_the_table_are_taken(family, E, k):
    model = M.build(family, E=E, k=k)
    before = _snapshot(model)
    classes = {n: type(m) for n, m in model.named_modules()}
    kind, renorm, attr, s32, l32, flat, bias, pos = TAKEN[family]
    found = {n: router_parts(m) for n, m in model.named_modules() if router_parts(m) is not None}
    assert len(found) == 2 and _snapshot(model) == before, "the probe changes nothing"
    for n, parts in found.items():
        flag = bool(getattr(model.get_submodule(n), attr)) if attr else renorm
        assert parts == RouterParts(E, 64, bias, pos[0], pos[1], pos[2], kind, flag, attr, s32, l32, flat), (n, parts)
    assert pq.fuse_moe_routers(model) == 2
    after = _snapshot(model)
    assert [(n, i) for n, i, _ in after[0]] == [(n, i) for n, i, _ in before[0]], "the module objects are the same"
    assert after[1:] == before[1:], "state-dict keys and parameter objects are unchanged"
    changed = [n for (n, _, c0), (_, _, c1) in zip(before[0], after[0]) if c0 is not c1]
    assert sorted(changed) == sorted(found), "only the routers got a new class"
    for n, r in _routers(model):
        assert isinstance(r, classes[n]) and type(r) is not classes[n] and type(r).__name__ == classes[n].__name__
    assert pq.fuse_moe_routers(model) == 0, "a second call finds nothing to do"


@pytest.mark.parametrize("family", sorted(TAKEN))
def test_cpu_forward_is_the_models_own_and_router_logits_are_still_recorded(family):
    ids = torch.randint(3, M.VOCAB, (2, 9), generator=torch.Generator().manual_seed(4))
    plain, model = M.build(family), M.build(family)          # (the same seed.  A twin, not the same model before and after: transformers leaves its output-capturing
    kw = dict(output_router_logits=True) if family != "granitemoe" else {}      # hooks on the routers at the first forward, and a router carrying a hook is refused)
    with torch.no_grad():
        ref = plain(ids, output_hidden_states=True, **kw)
    assert pq.fuse_moe_routers(model) == 2
    assert not kw or pq.fuse_moe_routers(plain) == 0, "after a recording forward the routers carry transformers' hooks: fuse_moe_routers is called before the first forward"
    with torch.no_grad():
        got = model(ids, output_hidden_states=True, **kw)
    assert torch.equal(got.logits, ref.logits) and all(torch.equal(a, b) for a, b in zip(got.hidden_states, ref.hidden_states))
    if kw:
        assert len(got.router_logits) == 2 and all(torch.equal(a, b) for a, b in zip(got.router_logits, ref.router_logits))
        assert tuple(got.router_logits[0].shape) == (18, 4)


def test_norm_topk_prob_is_followed_at_run_time_and_probed_at_both_values():
    for value in (True, False):
        model = M.build("qwen3_moe", norm_topk_prob=value)
        parts = [router_parts(m) for m in model.modules() if router_parts(m) is not None]
        assert len(parts) == 2 and all(p.renorm_attr == "norm_topk_prob" and p.renormalise is value and p.kind == "softmax_topk" for p in parts)

    class Liar(type(model.model.layers[0].mlp.gate)):          # says norm_topk_prob and does not follow it: refused
        def forward(self, hidden_states):
            keep, self.norm_topk_prob = self.norm_topk_prob, True
            try:
                return super().forward(hidden_states)
            finally:
                self.norm_topk_prob = keep

    gate = model.model.layers[0].mlp.gate
    gate.__class__ = Liar
    assert router_parts(gate) is None


@pytest.mark.parametrize("family", REFUSED)
def test_refused_families_are_left_as_they_are(family):
    model = M.build(family)
    before = _snapshot(model)
    assert all(router_parts(m) is None for m in model.modules())
    assert pq.fuse_moe_routers(model) == 0
    assert _snapshot(model) == before and not _routers(model)


def test_a_router_carrying_a_hook_is_refused():
    model = M.build("mixtral")
    g0, g1 = model.model.layers[0].mlp.gate, model.model.layers[1].mlp.gate
    handle = g0.register_forward_hook(lambda mod, args, out: None)
    pre = g1.register_forward_pre_hook(lambda mod, args: None)
    before = _snapshot(model)
    assert router_parts(g0) is None and router_parts(g1) is None and pq.fuse_moe_routers(model) == 0 and _snapshot(model) == before
    handle.remove()
    assert pq.fuse_moe_routers(model) == 1 and type(g0) is not before[0][0][2] and getattr(g1, "_pq_router", None) is None
    pre.remove()


def test_look_alikes_are_refused():
    """modules with a router's attributes whose forward is none of the three recipes, returns another convention, or has more state"""
    model = M.build("mixtral")
    Router = type(model.model.layers[0].mlp.gate)

    class Sigmoid(Router):
        def forward(self, hidden_states):
            logits = torch.nn.functional.linear(hidden_states.reshape(-1, self.hidden_dim), self.weight)
            w, ids = torch.topk(logits.sigmoid(), self.top_k, dim=-1)
            return logits, w / w.sum(-1, keepdim=True), ids

    class Scaled(Router):
        def forward(self, hidden_states):
            logits, w, ids = super().forward(hidden_states)
            return logits, w * 2.5, ids

    class NoLogits(Router):
        def forward(self, hidden_states):
            logits, w, ids = super().forward(hidden_states)
            return logits * 1.0001, w, ids

    class Pair(Router):
        def forward(self, hidden_states):
            return super().forward(hidden_states)[1:]

    class Unsorted(Router):
        def forward(self, hidden_states):
            logits, w, ids = super().forward(hidden_states)
            return logits, w.flip(-1), ids.flip(-1)

    for cls in (Sigmoid, Scaled, NoLogits, Pair, Unsorted):
        gate = model.model.layers[0].mlp.gate
        gate.__class__ = cls
        assert router_parts(gate) is None, cls.__name__
        gate.__class__ = Router
    gate = model.model.layers[0].mlp.gate
    assert router_parts(gate) is not None
    gate.register_buffer("e_score_correction_bias", torch.zeros(4))
    assert router_parts(gate) is None, "a buffer"
    del gate._buffers["e_score_correction_bias"]
    gate.extra = nn.Parameter(torch.zeros(1))
    assert router_parts(gate) is None, "a third parameter"
    del gate._parameters["extra"]
    gate.top_k = 5
    assert router_parts(gate) is None, "top_k > E"
    gate.top_k = 2
    assert router_parts(gate) is not None
    assert router_parts(nn.Linear(64, 4)) is None and router_parts(nn.Embedding(4, 64)) is None


def _prepare_experts(model):
    S.prepare_for_int8(model, predicate=lambda name, mod: not isinstance(mod, nn.Linear), moe_gates="all")      # (the MoE half of prepare_for_int8: swap_moe_experts' recognition without a GPU)


@pytest.mark.parametrize("family", ("mixtral", "gpt_oss", "qwen2_moe"))
def test_both_call_orders_with_the_experts_swap_give_the_same_modules(family):
    a, b = M.build(family), M.build(family)
    _prepare_experts(a)
    assert pq.fuse_moe_routers(a) == 2
    assert pq.fuse_moe_routers(b) == 2
    _prepare_experts(b)
    sa, sb = [(n, type(m).__name__, type(m).__mro__[1].__name__) for n, m in a.named_modules()], [(n, type(m).__name__, type(m).__mro__[1].__name__) for n, m in b.named_modules()]
    assert sa == sb and list(a.state_dict().keys()) == list(b.state_dict().keys())
    assert len(_routers(a)) == 2 and len(_routers(b)) == 2
    assert sum(isinstance(m, moe.MoEGatedMLP) for m in a.modules()) == 2 and sum(isinstance(m, moe.MoEGatedMLP) for m in b.modules()) == 2


def test_moe_block_switch_is_per_instance_and_off_by_default():
    assert moe.MoEBlock.hip_routing is False

    def tiny():
        torch.manual_seed(0)
        holder = nn.Module()
        holder.block = M.ListMoeBlock(4, 64, 32, 2)
        _prepare_experts(holder)
        return holder

    h1, h2 = tiny(), tiny()
    assert isinstance(h1.block, moe.MoEBlock) and h1.block.hip_routing is False and "hip_routing" not in h1.block.__dict__
    assert pq.fuse_moe_routers(h1) == 1 and h1.block.hip_routing is True and pq.fuse_moe_routers(h1) == 0
    assert h2.block.hip_routing is False and moe.MoEBlock.hip_routing is False, "a block that was never passed to fuse_moe_routers"
    assert isinstance(h1.block.gate, nn.Linear) and type(h1.block.gate) is nn.Linear, "the Linear router of the 4.x layout is not a router module: the block holds the switch"


def test_a_fused_model_pickles_and_deepcopies():
    """the derived class is not importable by name: a fused router is rebuilt from its original class (torch.save(model) pickles the modules)"""
    import copy
    import io
    model = M.build("mixtral")
    Router = type(model.model.layers[0].mlp.gate)
    assert pq.fuse_moe_routers(model) == 2
    buf = io.BytesIO()
    torch.save(model, buf)
    buf.seek(0)
    for clone in (torch.load(buf, weights_only=False), copy.deepcopy(model)):
        g, h = model.model.layers[0].mlp.gate, clone.model.layers[0].mlp.gate
        assert h is not g and type(h) is type(g) and isinstance(h, Router) and h._pq_router == g._pq_router
        assert torch.equal(h.weight, g.weight) and h.weight is not g.weight and list(clone.state_dict().keys()) == list(model.state_dict().keys())
        assert pq.fuse_moe_routers(clone) == 0
        ids = torch.randint(3, M.VOCAB, (1, 5), generator=torch.Generator().manual_seed(1))
        with torch.no_grad():
            assert torch.equal(clone(ids).logits, model(ids).logits)
