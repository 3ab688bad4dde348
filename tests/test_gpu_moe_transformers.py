"""-m gpu: swap_moe_experts on the real transformers decoders (fused-parameter experts, tests/moe_models.py): how many layers are swapped, one swapped layer bit for bit
against the C oracle's chain and against the per-expert ModuleList path, the logits against the float model, prefill and cached decode, the refused families, one
hipGraph, and the serialised form.  Every model is tiny, built from a config with a seeded random initialisation, once per (family, dtype)."""
import copy
import os

import numpy as np
import pytest
import torch
from torch import nn

tr = pytest.importorskip("transformers")

from oracle import c_oracle as C                    # noqa: E402
from tests import moe_models as M                   # noqa: E402
from tests.gpu_util import bits, same               # noqa: E402

pytestmark = pytest.mark.gpu

DT = {"bf16": (torch.bfloat16, 0), "fp16": (torch.float16, 1)}
BLOCK_ONLY = ("mixtral", "qwen3_moe", "olmoe")      # the block is a router and routed experts, nothing else: MoEBlock over the ModuleList layout can stand in its place
SHAPE = dict(H=256, I=384, E=8, k=2)


def _same_t(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    bad = a.view(torch.int16) != b.view(torch.int16)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {a.numel()} elements differ"


def _make(family, dtype, seed=0, **shape):
    """float model on the GPU with experts and routers that matter (the default initialisation, std 0.02, leaves the experts a rounding error of the residual and
    every routing a near-tie) + the swapped copy + the float expert parameters of every sparse block, saved on the CPU before the swap"""
    import protoquant_amd as pq
    model = M.build(family, seed=seed, **(shape or SHAPE))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for _, blk in M.sparse_blocks(model):
            blk.experts.gate_up_proj.normal_(0, 0.05, generator=g); blk.experts.down_proj.normal_(0, 0.05, generator=g)
            router = blk.gate if hasattr(blk, "gate") else blk.router
            router.weight.normal_(0, 0.3, generator=g)
    model = model.to(dtype).cuda().eval()
    names = [n for n, _ in M.sparse_blocks(model)]
    saved = {n: (b.experts.gate_up_proj.detach().cpu().clone(), b.experts.down_proj.detach().cpu().clone()) for n, b in M.sparse_blocks(model)}
    swapped = copy.deepcopy(model)
    count = pq.swap_moe_experts(swapped)
    return dict(float=model, swapped=swapped, count=count, names=names, saved=saved, family=family)


_CACHE: dict = {}


@pytest.fixture(scope="module")
def models():
    def get(family, dt="bf16", **shape):
        key = (family, dt, tuple(sorted(shape.items())))
        if key not in _CACHE:
            _CACHE[key] = _make(family, DT[dt][0], **shape)
        return _CACHE[key]
    yield get
    _CACHE.clear()


def _ids(shape=(2, 48), seed=5):
    return torch.randint(3, M.VOCAB, shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _capture_experts(model, block_name, ids):
    """the (hidden, indices, weights) a block's experts module is called with, and what it returns, during model(ids)"""
    ex = model.get_submodule(block_name).experts
    got = {}
    h = ex.register_forward_hook(lambda mod, args, out: got.update(args=tuple(a.detach().clone() for a in args), out=out.detach().clone()))
    try:
        with torch.no_grad():
            logits = model(ids).logits
    finally:
        h.remove()
    return got["args"], got["out"], logits


def _oracle_layer(x, idx, w, gate_up, down, code):
    """The layer restated on the CPU: C oracle for the quantisations and the two int8 linears per expert over the float parameters as they were before the swap
    (gate rows first), protoquant_amd.moe.route_plan / combine — the combine's definition — for the order of the sum."""
    from protoquant_amd import moe
    x, idx, w = x.cpu(), idx.cpu(), w.cpu()
    E, I = gate_up.shape[0], down.shape[2]
    xq, xs = C.quant_rowwise(bits(x), code)
    row_index, offsets, rows_of, slot_of = moe.route_plan(idx, E)
    y = np.zeros((idx.numel(), x.shape[1]), np.uint16)
    for e in range(E):
        lo, hi = int(offsets[e]), int(offsets[e + 1])
        if hi == lo:
            continue
        toks = row_index[lo:hi].long().numpy()
        gq, gs = C.quant_rowwise(bits(gate_up[e]), code)
        gu = C.qlinear_s8(xq[toks], xs[toks], gq, gs, None, code)
        hq, hs, _ = C.silu_mul_quant_rowwise(gu[:, :I], gu[:, I:], code, want_h=False)
        dq, ds = C.quant_rowwise(bits(down[e]), code)
        y[lo:hi] = C.qlinear_s8(hq, hs, dq, ds, None, code)
    yt = torch.from_numpy(y.view(np.int16)).view(x.dtype)
    return bits(moe.combine(yt, rows_of, slot_of, w))


# ------------------------------------------------------------------------------------------------ 1. count
@pytest.mark.parametrize("family", M.SWAPPED)
def test_every_sparse_layer_is_swapped_and_the_float_experts_are_gone(models, family):
    import protoquant_amd as pq
    m = models(family)
    assert m["count"] == len(m["names"]) == (1 if family == "deepseek_v3" else 2)
    sd = m["swapped"].state_dict()
    assert not any(k.endswith("gate_up_proj") or k.endswith("down_proj") for k in sd)
    for n in m["names"]:
        blk, was = m["swapped"].get_submodule(n), m["float"].get_submodule(n)
        assert isinstance(blk.experts, pq.MoEGatedMLP) and type(blk) is type(was)          # the block, its router and its shared experts: the model's own classes
        assert {c for c, _ in blk.named_children()} == {c for c, _ in was.named_children()}
        assert sd[n + ".experts.gate_up.wq"].shape == (8, 768, 256) and sd[n + ".experts.down.wq"].shape == (8, 256, 384)


def test_qwen2_moe_with_dense_and_sparse_layers(models):
    import protoquant_amd as pq
    model = M.build("qwen2_moe", layers=4, decoder_sparse_step=2, mlp_only_layers=[3], **SHAPE).to(torch.bfloat16).cuda()
    kinds = [type(l.mlp).__name__ for l in model.model.layers]
    assert kinds == ["Qwen2MoeMLP", "Qwen2MoeSparseMoeBlock", "Qwen2MoeMLP", "Qwen2MoeMLP"]
    assert pq.swap_moe_experts(model) == 1
    assert [type(l.mlp).__name__ for l in model.model.layers] == kinds and isinstance(model.model.layers[1].mlp.experts, pq.MoEGatedMLP)
    with torch.no_grad():
        assert torch.isfinite(model(_ids()).logits.float()).all()


# ------------------------------------------------------------------------------------------------ 2. one swapped layer against the oracle
CASES = [(f, dt, {}) for f in M.SWAPPED for dt in DT] + [
    ("mixtral", "bf16", dict(H=320, I=200, E=8, k=2)),       # neither K a multiple of 128: the padded-K experts
    ("qwen3_moe", "fp16", dict(H=320, I=200, E=8, k=2)),
    ("mixtral", "bf16", dict(H=256, I=128, E=64, k=8)),      # most experts see a handful of rows, some none
    ("olmoe", "bf16", dict(H=256, I=384, E=8, k=8)),         # k = E: every expert sees every token
    ("mixtral", "fp16", dict(H=256, I=128, E=1, k=1)),
]


@pytest.mark.parametrize("family,dt,shape", CASES, ids=lambda v: v if isinstance(v, str) else "-".join(f"{k}{x}" for k, x in v.items()) or "base")
def test_a_swapped_layer_equals_the_oracle_chain(models, family, dt, shape):
    m = models(family, dt, **shape)
    name = m["names"][-1]                                    # the last sparse layer: its input went through the swapped layers before it
    (x, idx, w), out, _ = _capture_experts(m["swapped"], name, _ids())
    E = (shape or SHAPE)["E"]
    assert x.shape == (96, (shape or SHAPE)["H"]) and idx.shape == w.shape == (96, (shape or SHAPE)["k"]) and x.dtype == DT[dt][0]
    assert int(idx.min()) >= 0 and int(idx.max()) < E
    gate_up, down = m["saved"][name]
    same(out, _oracle_layer(x, idx, w, gate_up, down, DT[dt][1]), f"{family} {dt} {name}")


# ------------------------------------------------------------------------------------------------ 3. against the per-expert ModuleList path
def _old_way_block(m, name, dtype):
    """the block's experts split into E (gate, up, down) nn.Linear triples in the 4.x layout, with the block's router weight, swapped the old way (-> MoEBlock)"""
    import protoquant_amd as pq
    blk = m["float"].get_submodule(name)
    gate_up, down = (t.cuda() for t in m["saved"][name])
    old = M.ListMoeBlock.from_stacked(blk.gate.weight.detach(), gate_up, down, blk.gate.top_k, norm_topk_prob=getattr(blk.gate, "norm_topk_prob", True))
    holder = nn.ModuleDict({"mlp": old})
    assert pq.swap_moe_experts(holder) == 1 and isinstance(holder["mlp"], pq.MoEBlock)
    return holder["mlp"]


@pytest.mark.parametrize("dt", tuple(DT))
@pytest.mark.parametrize("family", BLOCK_ONLY + ("qwen2_moe",))
def test_fused_parameter_swap_equals_the_module_list_swap(models, family, dt):
    m = models(family, dt)
    ids = _ids()
    name = m["names"][-1]
    (x, idx, w), out, logits = _capture_experts(m["swapped"], name, ids)
    old = _old_way_block(m, name, DT[dt][0])
    new_experts = m["swapped"].get_submodule(name).experts
    assert torch.equal(old.experts.gate_up.wq, new_experts.gate_up.wq) and torch.equal(old.experts.gate_up.ws, new_experts.gate_up.ws)
    assert torch.equal(old.experts.down.wq, new_experts.down.wq) and torch.equal(old.experts.down.ws, new_experts.down.ws)
    with torch.no_grad():
        _same_t(old(x.reshape(2, 48, -1)).reshape(x.shape), out, f"{family} {dt}: routed experts of {name}")      # (MoEBlock routes by itself: the router's recipe restated)
    if family not in BLOCK_ONLY:
        return                                                # (a Qwen2-MoE block adds its shared expert: the ModuleList block cannot stand in the model)
    whole = copy.deepcopy(m["float"])
    for n in m["names"]:
        parent, leaf = n.rsplit(".", 1)
        setattr(whole.get_submodule(parent), leaf, _old_way_block(m, n, DT[dt][0]))
    with torch.no_grad():
        _same_t(whole(ids).logits, logits, f"{family} {dt}: logits")


# ------------------------------------------------------------------------------------------------ 4. close to the float model
# Measured on these seeded models (bf16, all logits of [2, 48] ids against the float model): mixtral 0.99746, qwen3_moe 0.99868, olmoe 0.99900, qwen2_moe 0.99843,
# deepseek_v3 0.99972, granitemoe 0.99460, phimoe 0.99086.  What pulls a family down is not the experts' arithmetic (that is bit-exact against the oracle above) but single
# positions whose top-k flips under the int8 noise of the layer before (worst position: 0.69 for phimoe, whose sparsemixer thresholds the logits; 0.82 for granitemoe,
# 0.85 for mixtral): the floor of a family is the 0.995 of the Llama test where it holds, and the next 0.005 step below the measurement where it does not.  The MEDIAN
# position is the statement about every token — a dropped shared expert or a wrong renormalisation moves all of them.
COSINE_FLOOR = {"granitemoe": 0.99, "phimoe": 0.99}


@pytest.mark.parametrize("family", M.SWAPPED)
def test_swapped_logits_are_close_to_the_float_model(models, family):
    m = models(family)
    ids = _ids()
    with torch.no_grad():
        a, b = m["float"](ids).logits.float(), m["swapped"](ids).logits.float()
    assert a.shape == b.shape == (2, 48, M.VOCAB)
    cos = torch.nn.functional.cosine_similarity(a.reshape(1, -1), b.reshape(1, -1)).item()
    worst = torch.nn.functional.cosine_similarity(a.reshape(96, -1), b.reshape(96, -1)).min().item()
    median = torch.nn.functional.cosine_similarity(a.reshape(96, -1), b.reshape(96, -1)).median().item()
    print(f"COSINE {family} bf16: all logits {cos:.5f}, worst position {worst:.5f}, median position {median:.5f}")
    assert cos > COSINE_FLOOR.get(family, 0.995), f"{family}: cosine {cos} against the float model"
    assert median > 0.995, f"{family}: median cosine over the positions {median}"


# ------------------------------------------------------------------------------------------------ 5. prefill and cached decode
@pytest.mark.parametrize("family", BLOCK_ONLY)
def test_prefill_and_cached_decode_equal_the_module_list_swap(models, family):
    m = models(family)
    new = m["swapped"]
    old = copy.deepcopy(m["float"])
    for n in m["names"]:
        parent, leaf = n.rsplit(".", 1)
        setattr(old.get_submodule(parent), leaf, _old_way_block(m, n, torch.bfloat16))
    ids = _ids(seed=9)
    outs = []
    for model in (new, old):
        with torch.no_grad():
            g = model.generate(ids, max_new_tokens=8, min_new_tokens=8, do_sample=False, use_cache=True, output_logits=True, return_dict_in_generate=True, pad_token_id=0, eos_token_id=None)
        outs.append(g)
    assert outs[0].sequences.shape == (2, 56) and torch.equal(outs[0].sequences, outs[1].sequences)
    assert len(outs[0].logits) == 8
    for step in (0, 7):                                       # the prefill's last position, and the last cached step (T = 2 rows through every MoE layer)
        assert outs[0].logits[step].shape == (2, M.VOCAB) and torch.equal(outs[0].logits[step], outs[1].logits[step]), f"{family}: logits of step {step} differ"


# ------------------------------------------------------------------------------------------------ 6. refused families run unchanged
@pytest.mark.parametrize("family", M.REFUSED)
def test_a_refused_family_is_left_alone_and_runs_unchanged(family):
    import protoquant_amd as pq
    model = M.build(family, **SHAPE).to(torch.bfloat16).cuda()
    ids = _ids()
    with torch.no_grad():
        before = model(ids).logits
    mods = [(n, id(x)) for n, x in model.named_modules()]
    assert pq.swap_moe_experts(model) == 0 and [(n, id(x)) for n, x in model.named_modules()] == mods
    with torch.no_grad():
        _same_t(model(ids).logits, before, family)


def test_swap_linears_leaves_the_phimoe_router_its_forward():
    import protoquant_amd as pq
    model = M.build("phimoe", **SHAPE).to(torch.bfloat16).cuda()
    router = model.model.layers[0].mlp.router
    ids = _ids()
    with torch.no_grad():
        want = model(ids).logits.float()
    pq.swap_linears(model, predicate=lambda n, mod: n != "lm_head")
    assert pq.swap_moe_experts(model) == 2
    assert model.model.layers[0].mlp.router is router and type(router).__name__ == "PhimoeTopKRouter" and isinstance(model.model.layers[0].self_attn.q_proj, pq.qlinear)
    with torch.no_grad():
        logits, weights, selected = router(torch.randn(7, 256, device="cuda").to(torch.bfloat16))
        got = model(ids).logits.float()
    assert logits.shape == (7, 8) and weights.shape == selected.shape == (7, 2)
    cos = torch.nn.functional.cosine_similarity(got.reshape(1, -1), want.reshape(1, -1)).item()
    print(f"COSINE phimoe bf16 with swap_linears: {cos:.5f}")
    assert cos > 0.99, cos                                      # measured 0.99474 (every linear layer but lm_head int8 as well): the same rule as COSINE_FLOOR, the next 0.005 step below


# ------------------------------------------------------------------------------------------------ 7. one graph
def test_a_swapped_mixtral_block_in_one_graph(models):
    block = models("mixtral")["swapped"].model.layers[0].mlp
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(2, 24, 256, device="cuda", generator=gen).to(torch.bfloat16)
    x2 = (torch.randn(2, 24, 256, device="cuda", generator=gen) * 1.5).to(torch.bfloat16)
    s, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.stream(s):
        block(x)                                              # warm-up on the capture stream: the workspaces exist before the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=s):
            out = block(x)
    with torch.no_grad():
        want1, want2 = block(x.clone()), block(x2)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    _same_t(out, want1, "replay, the captured input")
    x.copy_(x2)
    out.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    _same_t(out, want2, "replay, a second input (another routing)")
    assert not torch.equal(want1, want2)


# ------------------------------------------------------------------------------------------------ the constructor and the serialised form
def test_from_stacked_gives_the_codes_of_the_per_expert_slices():
    import protoquant_amd as pq
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        g = torch.Generator().manual_seed(2)
        E, H, I = 5, 200, 72
        gate_up = (torch.randn(E, 2 * I, H, generator=g) * 0.1).to(dtype).cuda()
        down = (torch.randn(E, H, I, generator=g) * 0.1).to(dtype).cuda()
        down[2, 7] = 0                                          # an all-zero output channel
        a = pq.MoEGatedMLP.from_stacked(gate_up, down)
        lins = []
        for e in range(E):
            trio = [nn.Linear(H, I, bias=False), nn.Linear(H, I, bias=False), nn.Linear(I, H, bias=False)]
            for lin, wt in zip(trio, (gate_up[e, :I], gate_up[e, I:], down[e])):
                lin.weight = nn.Parameter(wt.clone())
            lins.append(tuple(trio))
        b = pq.MoEGatedMLP.from_experts(lins)
        for x, y in ((a.gate_up, b.gate_up), (a.down, b.down)):
            assert x.wq.shape == y.wq.shape and torch.equal(x.wq, y.wq) and torch.equal(x.ws, y.ws) and x.bias is None and y.bias is None
        wq, ws = C.quant_rowwise(bits(gate_up[3].cpu()), {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}[dtype])
        same(a.gate_up.wq[3], wq, "expert 3's codes against the oracle"); same(a.gate_up.ws[3], ws, "expert 3's scales against the oracle")
    with pytest.raises(ValueError):
        pq.MoEGatedMLP.from_stacked(gate_up.transpose(1, 2), down)


def test_a_real_mixtral_checkpoint_round_trips(models, tmp_path):
    """float state dict -> convert_checkpoint(model = a meta instance) -> file -> a meta model prepared without weights -> the swapped model's bits"""
    import protoquant_amd as pq
    from protoquant_amd import serialize as S
    m = models("mixtral")
    cfg = m["float"].config
    sd = {k: v.detach().cpu() for k, v in m["float"].state_dict().items()}
    with torch.device("meta"):
        meta = tr.AutoModelForCausalLM.from_config(cfg).to(torch.bfloat16)
    conv = S.convert_checkpoint(sd, model=meta)
    p = m["names"][0] + "."
    assert p + "experts.gate_up_proj" not in conv and p + "gate.wq" not in conv and conv[p + "gate.weight"].dtype == torch.bfloat16
    ex = m["swapped"].get_submodule(m["names"][0]).experts
    assert torch.equal(conv[p + "experts.gate_up.wq"], ex.gate_up.wq.cpu()) and torch.equal(conv[p + "experts.down.ws"], ex.down.ws.cpu())
    assert conv[p + "experts.gate_up.wq"].shape == (8, 768, 256) and conv["model.layers.0.self_attn.q_proj.wq"].dtype == torch.int8
    with pytest.raises(KeyError):
        S.convert_checkpoint({k: v for k, v in sd.items() if not k.endswith("experts.down_proj")}, model=meta)
    path = os.path.join(tmp_path, "mixtral.int8.safetensors")
    S.save_quantized(conv, path)
    back = S.load_quantized(path)
    with torch.device("meta"):
        fresh = tr.AutoModelForCausalLM.from_config(cfg).to(torch.bfloat16)
    S.prepare_for_int8(fresh)
    missing, unexpected = fresh.load_state_dict(back, strict=True, assign=True)
    assert not missing and not unexpected and not any(t.device.type == "meta" for t in fresh.state_dict().values())
    ref = pq.swap_linears(copy.deepcopy(m["swapped"]))
    ids = _ids()
    fresh.model.rotary_emb = ref.model.rotary_emb              # (inv_freq is a non-persistent buffer: not in a state dict, computed by the constructor)
    with torch.no_grad():
        fresh = fresh.cuda().eval()
        _same_t(fresh(ids).logits, ref(ids).logits, "loaded model against the model swapped in memory")
