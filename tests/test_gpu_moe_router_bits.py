"""-m gpu: fuse_moe_routers on whole tiny decoders (tests/moe_models.py: H = 64, E = 4 and 8, k = 2, two layers).  Logits, every hidden state and a greedy generation
with the KV cache are torch.equal to a TWIN whose routers run the model's F.linear on the GPU and then QSPEC RT on the host (tests/router_spec.py) — after
swap_moe_experts(gates="all") + fuse_moe_routers for Mixtral, Qwen3-MoE, Qwen2-MoE, OLMoE, GPT-OSS and GraniteMoe in bf16, Mixtral in fp16 as well, and Qwen3-MoE (bf16)
and GraniteMoe (fp16) with fuse_moe_routers alone; both call orders of the two entries give the same modules and bits.  A fused router is one pq_moe_topk call and no torch softmax / topk / sum / div; the recorded router_logits are still there; the 4.x
ModuleList layout (MoEBlock.hip_routing) equals its torch_plumbing form fed by the host specification.

The switch is NOT bit-neutral (the softmax becomes the specified one): cosine of all logits against the bf16 original, seeds 0-7, is printed without and with it."""
import copy
import types

import pytest
import torch
import torch.nn.functional as F
from torch import nn

tr = pytest.importorskip("transformers")

from tests import moe_models as M                   # noqa: E402
from tests import router_spec as RS                 # noqa: E402
from tests.gpu_util import bits, to_gpu             # noqa: E402

pytestmark = pytest.mark.gpu

FAMILIES = ("mixtral", "qwen3_moe", "qwen2_moe", "olmoe", "gpt_oss")
NAME = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "f32"}
CODE = {"bf16": 0, "fp16": 1, "f32": 2}
FORBIDDEN = ("softmax", "topk", "sum", "div", "true_divide", "divide")


def _build(family, dtype, seed=0, E=4):
    """a float model on the GPU whose routers and experts matter (the default initialisation leaves every routing a near-tie)"""
    model = M.build(family, seed=seed, H=64, I=128, E=E, k=2)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for _, blk in M.sparse_blocks(model):
            blk.experts.gate_up_proj.normal_(0, 0.05, generator=g); blk.experts.down_proj.normal_(0, 0.05, generator=g)
            (blk.gate if hasattr(blk, "gate") else blk.router).weight.normal_(0, 0.3, generator=g)
    return model.to(dtype).cuda().eval()


def _routers(model):
    return [m for m in model.modules() if getattr(m, "_pq_router", None) is not None]


def _host_spec(logits, k, kind, renorm, out_dtype):
    """QSPEC RT on the host for GPU logits [..., E] -> (scores, int64 ids) back on the GPU"""
    lead, E = tuple(logits.shape[:-1]), logits.shape[-1]
    l2 = logits.reshape(-1, E)
    stored = bits(l2) if l2.dtype != torch.float32 else l2.detach().cpu().numpy()
    w, ids, _ = RS.moe_topk(stored, NAME[l2.dtype], k, kind, renorm, NAME[out_dtype])
    return to_gpu(w, CODE[NAME[out_dtype]]).reshape(lead + (k,)), torch.from_numpy(ids).cuda().reshape(lead + (k,))


def _host_forward(self, hidden_states):
    rec = self._pq_router
    x = hidden_states.reshape(-1, hidden_states.shape[-1]) if rec.flatten else hidden_states
    logits = F.linear(x, self.weight, self.bias if rec.has_bias else None)
    if rec.logits_f32:
        logits = logits.float()
    renorm = bool(getattr(self, rec.renorm_attr)) if rec.renorm_attr else rec.renormalise
    scores, ids = _host_spec(logits, self.top_k, rec.kind, renorm, torch.float32 if rec.scores_f32 else hidden_states.dtype)
    out = [None, None, None]
    out[rec.pos_logits], out[rec.pos_scores], out[rec.pos_indices] = logits, scores, ids
    return tuple(out)


def _twin(model):
    twin = copy.deepcopy(model)
    for r in _routers(twin):
        r.forward = types.MethodType(_host_forward, r)
    return twin


def _ids(seed=5, shape=(2, 12)):
    return torch.randint(3, M.VOCAB, shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _run(model, ids):
    with torch.no_grad():
        out = model(ids, output_hidden_states=True)
        gen = model.generate(ids[:, :6], max_new_tokens=6, min_new_tokens=6, do_sample=False, use_cache=True)
    return out.logits, out.hidden_states, gen


# (GraniteMoe: f32-widened logits into the kernel, scores in the hidden dtype, the tuple returned as (indices, scores, logits))
CASES = [(f, "bf16", E, True) for f in FAMILIES for E in (4, 8)] + [("mixtral", "fp16", 4, True), ("qwen3_moe", "bf16", 8, False), ("granitemoe", "bf16", 8, True),
                                                                   ("granitemoe", "fp16", 4, False)]


@pytest.mark.parametrize("family,dt,E,swap", CASES, ids=[f"{f}-{d}-E{E}-{'swapped' if s else 'routers_alone'}" for f, d, E, s in CASES])
def test_fused_decoder_equals_the_host_specification_twin(family, dt, E, swap):
    import protoquant_amd as pq
    dtype = torch.bfloat16 if dt == "bf16" else torch.float16
    model = _build(family, dtype, E=E)
    if swap:
        assert pq.swap_moe_experts(model, gates="all") == 2
    assert pq.fuse_moe_routers(model) == 2 and len(_routers(model)) == 2
    assert sum(isinstance(m, pq.MoEGatedMLP) for m in model.modules()) == (2 if swap else 0)
    twin = _twin(model)
    ids = _ids()
    logits, hidden, gen = _run(model, ids)
    t_logits, t_hidden, t_gen = _run(twin, ids)
    assert torch.equal(logits, t_logits), f"{int((logits != t_logits).sum())} logits differ from the twin's"
    assert len(hidden) == len(t_hidden) == 3 and all(torch.equal(a, b) for a, b in zip(hidden, t_hidden))
    assert gen.shape == (2, 12) and torch.equal(gen, t_gen)
    assert bool(torch.isfinite(logits.float()).all())


@pytest.mark.parametrize("family", ("mixtral", "gpt_oss", "qwen2_moe", "granitemoe"))
def test_both_call_orders_with_swap_moe_experts(family):
    """fuse_moe_routers before swap_moe_experts and after it, with the real swap on the GPU: the same modules, the same state-dict keys, the same bits"""
    import protoquant_amd as pq
    a, b = _build(family, torch.bfloat16, E=8), _build(family, torch.bfloat16, E=8)
    assert pq.swap_moe_experts(a, gates="all") == 2 and pq.fuse_moe_routers(a) == 2
    assert pq.fuse_moe_routers(b) == 2 and pq.swap_moe_experts(b, gates="all") == 2
    assert [(n, type(m).__name__, type(m).__mro__[1].__name__) for n, m in a.named_modules()] == [(n, type(m).__name__, type(m).__mro__[1].__name__) for n, m in b.named_modules()]
    assert list(a.state_dict().keys()) == list(b.state_dict().keys()) and len(_routers(a)) == len(_routers(b)) == 2
    la, ha, ga = _run(a, _ids())
    lb, hb, gb = _run(b, _ids())
    assert torch.equal(la, lb) and all(torch.equal(x, y) for x, y in zip(ha, hb)) and torch.equal(ga, gb)


@pytest.mark.parametrize("family", ("mixtral", "gpt_oss", "qwen3_moe"))
def test_router_logits_are_still_recorded(family):
    """output_router_logits=True after the switch: one tensor per layer, in the router's own dtype and shape; the first layer's are the un-fused model's bit for bit (its
    input does not depend on any routing), and every layer's are the host twin's"""
    import protoquant_amd as pq
    plain = _build(family, torch.bfloat16)
    assert pq.swap_moe_experts(plain, gates="all") == 2
    fused = copy.deepcopy(plain)
    assert pq.fuse_moe_routers(fused) == 2
    twin = _twin(fused)
    ids = _ids(7)
    with torch.no_grad():
        a, b, c = (m(ids, output_router_logits=True).router_logits for m in (plain, fused, twin))
    assert len(a) == len(b) == len(c) == 2
    assert all(x.shape == y.shape == (24, 4) and x.dtype == y.dtype for x, y in zip(a, b))
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(b, c))


class _Log(torch.overrides.TorchFunctionMode):
    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_function__(self, func, types_, args=(), kwargs=None):
        self.names.append(getattr(func, "__name__", str(func)))
        return func(*args, **(kwargs or {}))


def _count_topk_calls(monkeypatch):
    from protoquant_amd import _lib
    L = _lib.lib()
    calls = []
    real = L.pq_moe_topk

    class Counting:
        def __getattr__(self, name):
            if name == "pq_moe_topk":
                return lambda *a: (calls.append(a), real(*a))[1]
            return getattr(L, name)

    monkeypatch.setattr(_lib, "lib", lambda: Counting())
    return calls


@pytest.mark.parametrize("family", ("mixtral", "gpt_oss"))
def test_a_fused_router_is_one_library_call_and_no_torch_arithmetic(family, monkeypatch):
    import protoquant_amd as pq
    model = _build(family, torch.bfloat16)
    plain_router = [m for m in model.modules() if type(m).__name__.endswith("TopKRouter")][0]
    x = torch.randn(24, 64, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).cuda()
    with _Log() as eager, torch.no_grad():
        plain_router(x)
    assert "linear" in eager.names and "softmax" in eager.names and "topk" in eager.names, eager.names
    assert pq.fuse_moe_routers(model) == 2
    calls = _count_topk_calls(monkeypatch)
    with _Log() as log, torch.no_grad():
        out = plain_router(x)
    assert len(calls) == 1, "one pq_moe_topk call (one kernel launch: moe_topk_kernels.hip has one kernel and its dispatcher launches once)"
    assert log.names.count("linear") == 1 and not [n for n in log.names if n in FORBIDDEN or n in ("to", "float", "type_as")], log.names
    assert len(out) == 3 and out[2].dtype == torch.int64


def _list_block(norm_topk_prob, dtype=torch.bfloat16, E=8):
    import protoquant_amd as pq
    torch.manual_seed(11)
    holder = nn.ModuleDict({"mlp": M.ListMoeBlock(E, 64, 128, 2, norm_topk_prob=norm_topk_prob)})
    with torch.no_grad():
        holder["mlp"].gate.weight.normal_(0, 0.3)
    holder = holder.to(dtype).cuda()
    assert pq.swap_moe_experts(holder) == 1 and isinstance(holder["mlp"], pq.MoEBlock)
    return holder


@pytest.mark.parametrize("norm_topk_prob", (True, False))
def test_module_list_layout_with_hip_routing(norm_topk_prob, monkeypatch):
    import protoquant_amd as pq
    holder = _list_block(norm_topk_prob)
    block = holder["mlp"]
    x = (torch.randn(2, 19, 64, generator=torch.Generator().manual_seed(3)) * 2).to(torch.bfloat16).cuda()
    with _Log() as eager, torch.no_grad():
        y_eager = block(x)
    assert block.hip_routing is False and "softmax" in eager.names and "topk" in eager.names
    assert pq.fuse_moe_routers(holder) == 1 and block.hip_routing is True and block.renormalise is norm_topk_prob
    calls = _count_topk_calls(monkeypatch)
    with _Log() as log, torch.no_grad():
        y = block(x)
    assert len(calls) == 1 and calls[0][12] == 0, "one pq_moe_topk call whose int32 ids go straight into moe_route"
    assert not [n for n in log.names if n in FORBIDDEN], log.names
    # the twin: the block's own Linear router, QSPEC RT on the host, the experts with the stock torch ops of route_plan / combine
    with torch.no_grad():
        x2 = x.reshape(-1, 64)
        w, ids = _host_spec(block.gate(x2), 2, "softmax_topk", norm_topk_prob, torch.bfloat16)
        block.experts.torch_plumbing = True
        want = block.experts(x2, ids, w).reshape(x.shape)
        block.experts.torch_plumbing = False
    assert torch.equal(y, want)
    cos = float(F.cosine_similarity(y.float().flatten(), y_eager.float().flatten(), dim=0))
    print(f"ListMoeBlock norm_topk_prob={norm_topk_prob}: cosine(hip_routing, eager routing) = {cos:.6f}, {int((y != y_eager).sum())} of {y.numel()} outputs differ")
    assert cos > 0.999


@pytest.mark.parametrize("family", FAMILIES)
def test_cosine_against_the_bf16_original_without_and_with_the_switch(family):
    """reported, seeds 0-7: the cosine of all logits of the swapped model against the bf16 original, without and with fuse_moe_routers.  The switch is not bit-neutral;
    what it may not do is move the model away from the original by more than the int8 experts already do (held loosely: the figures are in the README)."""
    import protoquant_amd as pq
    ids = _ids(9, (2, 24))
    without, with_ = [], []
    for seed in range(8):
        original = _build(family, torch.bfloat16, seed=seed, E=8)
        swapped = copy.deepcopy(original)
        assert pq.swap_moe_experts(swapped, gates="all") == 2
        fused = copy.deepcopy(swapped)
        assert pq.fuse_moe_routers(fused) == 2
        with torch.no_grad():
            ref, a, b = (m(ids).logits.float().flatten() for m in (original, swapped, fused))
        without.append(float(F.cosine_similarity(ref, a, dim=0)))
        with_.append(float(F.cosine_similarity(ref, b, dim=0)))
    print(f"{family}: cosine against the bf16 original, seeds 0-7: swapped {min(without):.5f} .. {max(without):.5f} (mean {sum(without) / 8:.5f}); "
          f"swapped + fused routers {min(with_):.5f} .. {max(with_):.5f} (mean {sum(with_) / 8:.5f})")
    assert min(with_) >= min(without) - 0.01, (without, with_)
