"""-m gpu: the clamped gates through MoEGatedMLP and through real decoders.  The layer with each gate kind, with and without biases, against the eager int8 chain per
expert (qlinear -> glu_quantize -> qlinear -> index_add_), bit for bit, at a prefill size (the 64-row tiles), at decode sizes (the weight-streaming kernel), on both
plumbings, in a replayed hipGraph and at GPT-OSS's real widths; from_stacked on GPT-OSS's storage order; tiny GPT-OSS and DeepSeek-V4 decoders swapped with
gates="all": what changed, the logits against the bf16 original, cached decode on both plumbings, and the serialised form loaded into a meta-device model."""
import copy
import os

import pytest
import torch
from torch import nn

tr = pytest.importorskip("transformers")

from tests import moe_models as M                   # noqa: E402

pytestmark = pytest.mark.gpu

GATES = {"clamped_silu": dict(gate_kind="clamped_silu", gate_limit=7.0), "alpha_sigmoid": dict(gate_kind="alpha_sigmoid", gate_limit=7.0, gate_alpha=1.702)}


def _same(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{what}: {int((a.view(torch.int16) != b.view(torch.int16)).sum())} of {a.numel()} elements differ"


def _params(E, H, I, bias, seed, dtype, scale=0.08):
    """standard-order float parameters: gate_up [E, 2 I, H], down [E, H, I] (+ biases), large enough that gate and up pass the limit now and then"""
    g = torch.Generator().manual_seed(seed)
    gu = (torch.randn(E, 2 * I, H, generator=g) * scale * 4).to(dtype).cuda()
    dn = (torch.randn(E, H, I, generator=g) * scale).to(dtype).cuda()
    gub = (torch.randn(E, 2 * I, generator=g) * 2).to(dtype).cuda() if bias else None
    dnb = torch.randn(E, H, generator=g).to(dtype).cuda() if bias else None
    return gu, dn, gub, dnb


def _routing(T, E, k, seed, dtype):
    g = torch.Generator(device="cuda").manual_seed(seed)
    logits = torch.randn(T, E, generator=g, device="cuda") + torch.linspace(1.5, -1.5, E, device="cuda")[None, :]
    wts, ids = torch.topk(torch.softmax(logits, dim=1), k, dim=-1)
    return ids, (wts / wts.sum(dim=-1, keepdim=True)).to(dtype)


def _eager_chain(params, gate, x, ids, w):
    """the model's loop over the experts with every expert an int8 chain of its own: qlinear (per-token quantisation + int8 GEMM + bias) -> glu_quantize -> qlinear ->
    (y + b) * w -> index_add_ into zeros"""
    import protoquant_amd as pq
    gu, dn, gub, dnb = params
    E, I = gu.shape[0], dn.shape[2]
    final = torch.zeros_like(x)
    mask = torch.nn.functional.one_hot(ids, num_classes=E).permute(2, 1, 0)
    clamped = 0
    for e in range(E):
        slot, tok = torch.where(mask[e])
        if tok.numel() == 0:
            continue
        lin_gu, lin_dn = nn.Linear(gu.shape[2], 2 * I, bias=gub is not None, dtype=x.dtype, device="cuda"), nn.Linear(I, dn.shape[1], bias=dnb is not None, dtype=x.dtype, device="cuda")
        with torch.no_grad():
            lin_gu.weight.copy_(gu[e]); lin_dn.weight.copy_(dn[e])
            if gub is not None:
                lin_gu.bias.copy_(gub[e]); lin_dn.bias.copy_(dnb[e])
        y1 = pq.qlinear.from_linear(lin_gu)(x[tok])
        clamped += int((y1.float().abs() > gate["gate_limit"]).sum())
        h = pq.glu_quantize(y1[:, :I], y1[:, I:], gate["gate_kind"], gate["gate_limit"], gate.get("gate_alpha"))
        y2 = pq.qlinear.from_linear(lin_dn)(h)
        final.index_add_(0, tok, (y2 * w[tok, slot, None]).to(x.dtype))
    return final, clamped


# T = 300: 64-row tiles; T k <= 64 grouped rows: the weight-streaming kernel (GroupedQLinear.stream_rows)
@pytest.mark.parametrize("E,k,T", ((8, 2, 300), (32, 4, 16), (32, 4, 1), (8, 2, 32)))
@pytest.mark.parametrize("bias", (False, True), ids=("nobias", "bias"))
@pytest.mark.parametrize("kind", sorted(GATES))
def test_layer_equals_the_eager_int8_chain_on_both_plumbings(kind, bias, E, k, T):
    import protoquant_amd as pq
    H, I = 256, 384
    dtype = torch.bfloat16 if (E + T) % 2 == 0 else torch.float16
    params = _params(E, H, I, bias, E + T, dtype)
    moe = pq.MoEGatedMLP.from_stacked(*params, **GATES[kind])
    assert moe.gate_kind == kind and (moe.gate_up.bias is not None) == bias and (moe.down.bias is not None) == bias and kind in repr(moe)
    x = (torch.randn(T, H, device="cuda", generator=torch.Generator(device="cuda").manual_seed(T)) * 1.5).to(dtype)
    ids, w = _routing(T, E, k, T, dtype)
    got = moe(x, ids, w)
    moe.torch_plumbing = True
    try:
        _same(got, moe(x, ids, w), "HIP plumbing vs torch plumbing")
    finally:
        moe.torch_plumbing = False
    want, clamped = _eager_chain(params, GATES[kind], x, ids, w)
    assert clamped > 0, "the clamp must be live in this test"
    _same(got, want, f"{kind}: layer vs the eager int8 chain")
    silu = pq.MoEGatedMLP.from_stacked(*params)(x, ids, w)
    assert not torch.equal(silu, got), "the gate kind must matter"


def test_layer_at_the_real_gpt_oss_widths():
    """H = I = 2880: neither GEMM's K is a multiple of 128 (zero-tailed codes), rows of 360 vectors in the producer kernel"""
    import protoquant_amd as pq
    E, k, H, I = 4, 2, 2880, 2880
    params = _params(E, H, I, True, 3, torch.bfloat16, scale=0.02)
    moe = pq.MoEGatedMLP.from_stacked(*params, **GATES["alpha_sigmoid"])
    for T in (70, 8):
        x = torch.randn(T, H, device="cuda").to(torch.bfloat16)
        ids, w = _routing(T, E, k, T, torch.bfloat16)
        want, clamped = _eager_chain(params, GATES["alpha_sigmoid"], x, ids, w)
        assert clamped > 0
        _same(moe(x, ids, w), want, f"2880 x 2880, T = {T}")


@pytest.mark.parametrize("kind", sorted(GATES))
def test_whole_forward_in_a_graph_replays_for_another_routing(kind):
    import protoquant_amd as pq
    E, k, T, H, I = 16, 4, 64, 256, 128
    moe = pq.MoEGatedMLP.from_stacked(*_params(E, H, I, True, 5, torch.bfloat16), **GATES[kind])
    x = torch.randn(T, H, device="cuda").to(torch.bfloat16)
    ids, w = _routing(T, E, k, 1, torch.bfloat16)
    s, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        moe(x, ids, w)                                            # warm-up on the capture stream: its workspace exists before the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=s):
            out = moe(x, ids, w)
    ids2, w2 = _routing(T, E, k, 2, torch.bfloat16)
    x2 = (torch.randn(T, H, device="cuda") * 2).to(torch.bfloat16)
    ids.copy_(ids2); w.copy_(w2); x.copy_(x2)
    out.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    _same(out, moe(x2, ids2, w2), "replay under a second routing")
    del graph
    pq.clear_workspaces()


def test_from_stacked_on_gpt_oss_storage_quantise_and_permute_commute():
    """GPT-OSS's [E, H, 2 I] interleaved gate_up_proj -> the standard order: the codes of the converted float tensor are the permuted codes of the stored one"""
    import protoquant_amd as pq
    from protoquant_amd import moe as moe_mod
    g = torch.Generator().manual_seed(4)
    E, H, I = 3, 200, 72
    gu_t = (torch.randn(E, H, 2 * I, generator=g) * 0.1).to(torch.bfloat16).cuda()          # stored [E, in, out], gate / up in alternating columns
    dn_t = (torch.randn(E, I, H, generator=g) * 0.1).to(torch.bfloat16).cuda()
    gub = torch.randn(E, 2 * I, generator=g).to(torch.bfloat16).cuda()
    dnb = torch.randn(E, H, generator=g).to(torch.bfloat16).cuda()
    m = pq.MoEGatedMLP.from_stacked(gu_t, dn_t, gub, dnb, transposed=True, interleaved=True, **GATES["alpha_sigmoid"])
    # quantise the stored tensor's output channels first (rows of its transpose), permute the codes afterwards
    q = pq.GroupedQLinear.from_weight(gu_t.transpose(1, 2).contiguous())
    perm = torch.cat([torch.arange(0, 2 * I, 2), torch.arange(1, 2 * I, 2)]).cuda()
    assert torch.equal(m.gate_up.wq, q.wq[:, perm]) and torch.equal(m.gate_up.ws, q.ws[:, perm]) and torch.equal(m.gate_up.bias, gub[:, perm])
    d = pq.GroupedQLinear.from_weight(dn_t.transpose(1, 2).contiguous())
    assert torch.equal(m.down.wq, d.wq) and torch.equal(m.down.ws, d.ws) and torch.equal(m.down.bias, dnb)
    std = moe_mod.standard_stacked(gu_t, dn_t, gub, dnb, True, True)
    again = pq.MoEGatedMLP.from_stacked(*std, **GATES["alpha_sigmoid"])
    assert torch.equal(again.gate_up.wq, m.gate_up.wq) and torch.equal(again.down.wq, m.down.wq)
    with pytest.raises(ValueError):
        pq.MoEGatedMLP.from_stacked(gu_t, dn_t, transposed=False)
    with pytest.raises(ValueError):
        pq.MoEGatedMLP.from_stacked(gu_t, dn_t, gub[:, :5], dnb, transposed=True, interleaved=True)


# ------------------------------------------------------------------------------------------------ real decoders
FAMILIES = ("gpt_oss", "deepseek_v4")
SHAPE = dict(H=256, I=384, E=8, k=2)
# Measured on these seeded models (bf16, all logits of [2, 48] ids against the bf16 original; printed by the test): the floor is the 0.995 of the other families where it
# holds, else the next 0.005 step below the measurement, as COSINE_FLOOR in tests/test_gpu_moe_transformers.py.
COSINE_FLOOR = {}


def _make(family, seed=0):
    import protoquant_amd as pq
    model = M.build(family, seed=seed, **SHAPE)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for _, blk in M.sparse_blocks(model):
            for n, p in blk.experts.named_parameters(recurse=False):
                p.normal_(0, 0.5 if n.endswith("bias") else 0.05, generator=g)
            router = blk.gate if hasattr(blk, "gate") else blk.router
            router.weight.normal_(0, 0.3, generator=g)
    model = model.to(torch.bfloat16).cuda().eval()
    swapped = copy.deepcopy(model)
    count = pq.swap_moe_experts(swapped, gates="all")
    return dict(float=model, swapped=swapped, count=count, names=[n for n, _ in M.sparse_blocks(model)])


_CACHE: dict = {}


@pytest.fixture(scope="module")
def models():
    def get(family):
        if family not in _CACHE:
            _CACHE[family] = _make(family)
        return _CACHE[family]
    yield get
    _CACHE.clear()


def _ids(shape=(2, 48), seed=5):
    return torch.randint(3, M.VOCAB, shape, generator=torch.Generator().manual_seed(seed)).cuda()


@pytest.mark.parametrize("family", FAMILIES)
def test_every_sparse_layer_is_swapped_and_only_the_experts_change(models, family):
    import protoquant_amd as pq
    m = models(family)
    assert m["count"] == len(m["names"]) == 2
    was = {n: type(x) for n, x in m["float"].named_modules()}
    changed = {n for n, x in m["swapped"].named_modules() if n in was and type(x) is not was[n]}
    assert changed == {n + ".experts" for n in m["names"]}
    sd = m["swapped"].state_dict()
    assert not any(k.endswith("gate_up_proj") or k.endswith("down_proj") or k.endswith("proj_bias") for k in sd)
    for n in m["names"]:
        ex = m["swapped"].get_submodule(n).experts
        assert isinstance(ex, pq.MoEGatedMLP) and ex.gate_kind == ("alpha_sigmoid" if family == "gpt_oss" else "clamped_silu")
        assert sd[n + ".experts.gate_up.wq"].shape == (8, 768, 256) and sd[n + ".experts.down.wq"].shape == (8, 256, 384)
        assert ((n + ".experts.gate_up.bias") in sd) == (family == "gpt_oss") == ((n + ".experts.down.bias") in sd)
    plain = copy.deepcopy(m["float"])
    assert pq.swap_moe_experts(plain) == 0                      # the default call still refuses both families


@pytest.mark.parametrize("family", FAMILIES)
def test_swapped_logits_are_close_to_the_bf16_original(models, family):
    m = models(family)
    ids = _ids()
    with torch.no_grad():
        a, b = m["float"](ids).logits.float(), m["swapped"](ids).logits.float()
    assert a.shape == b.shape == (2, 48, M.VOCAB)
    cos = torch.nn.functional.cosine_similarity(a.reshape(1, -1), b.reshape(1, -1)).item()
    per = torch.nn.functional.cosine_similarity(a.reshape(96, -1), b.reshape(96, -1))
    print(f"\nCOSINE {family} bf16: all logits {cos:.5f}, worst position {per.min().item():.5f}, median position {per.median().item():.5f}")
    assert cos > COSINE_FLOOR.get(family, 0.995), f"{family}: cosine {cos} against the bf16 original"
    assert per.median().item() > 0.995


@pytest.mark.parametrize("family", FAMILIES)
def test_cached_decode_is_the_same_on_both_plumbings(models, family):
    import protoquant_amd as pq
    model = models(family)["swapped"]
    ids = _ids(seed=9)
    outs = []
    for torch_plumbing in (False, True):
        pq.MoEGatedMLP.torch_plumbing = torch_plumbing
        try:
            with torch.no_grad():
                outs.append(model.generate(ids, max_new_tokens=8, min_new_tokens=8, do_sample=False, use_cache=True, output_logits=True, return_dict_in_generate=True,
                                           pad_token_id=0, eos_token_id=None))
        finally:
            pq.MoEGatedMLP.torch_plumbing = False
    assert outs[0].sequences.shape == (2, 56) and torch.equal(outs[0].sequences, outs[1].sequences) and len(outs[0].logits) == 8
    for step in range(8):                                        # step 0: the prefill (96 rows); later steps: 2 tokens x k = 4 grouped rows, the weight-streaming kernel
        assert torch.equal(outs[0].logits[step], outs[1].logits[step]), f"{family}: logits of step {step} differ"


@pytest.mark.parametrize("family", FAMILIES)
def test_a_checkpoint_round_trips_through_a_meta_device_model(models, family, tmp_path):
    """float state dict -> convert_checkpoint(model = a meta instance, moe_gates = "all") -> file -> a meta model prepared without weights -> the swapped model's bits"""
    import protoquant_amd as pq
    from protoquant_amd import serialize as S
    m = models(family)
    cfg = m["float"].config
    sd = {k: v.detach().cpu() for k, v in m["float"].state_dict().items()}
    with torch.device("meta"):
        meta = tr.AutoModelForCausalLM.from_config(cfg).to(torch.bfloat16)
    untouched = S.convert_checkpoint(sd, model=meta)
    p = m["names"][0] + ".experts."
    assert p + "gate_up_proj" in untouched and p + "gate_up.wq" not in untouched             # the default still copies these experts through
    conv = S.convert_checkpoint(sd, model=meta, moe_gates="all")
    ex = m["swapped"].get_submodule(m["names"][0]).experts
    assert p + "gate_up_proj" not in conv and p + "gate_up_proj_bias" not in conv and p + "down_proj_bias" not in conv
    assert torch.equal(conv[p + "gate_up.wq"], ex.gate_up.wq.cpu()) and torch.equal(conv[p + "down.ws"], ex.down.ws.cpu()) and conv[p + "gate_up.wq"].shape == (8, 768, 256)
    if family == "gpt_oss":
        assert torch.equal(conv[p + "gate_up.bias"], ex.gate_up.bias.cpu()) and torch.equal(conv[p + "down.bias"], ex.down.bias.cpu())
    with pytest.raises(KeyError):
        S.convert_checkpoint({k: v for k, v in sd.items() if not k.endswith("experts.down_proj")}, model=meta, moe_gates="all")
    path = os.path.join(tmp_path, f"{family}.int8.safetensors")
    S.save_quantized(conv, path)
    back = S.load_quantized(path)
    with torch.device("meta"):
        fresh = tr.AutoModelForCausalLM.from_config(cfg).to(torch.bfloat16)
    S.prepare_for_int8(fresh, moe_gates="all")
    missing, unexpected = fresh.load_state_dict(back, strict=True, assign=True)
    assert not missing and not unexpected and not any(t.device.type == "meta" for t in fresh.state_dict().values())
    ref = pq.swap_linears(copy.deepcopy(m["swapped"]))
    persistent = set(ref.state_dict())
    for name, buf in ref.named_buffers():                        # (inv_freq and its kin are non-persistent buffers: not in a state dict, computed by the constructor)
        if name not in persistent:
            parent, leaf = name.rsplit(".", 1)
            fresh.get_submodule(parent)._buffers[leaf] = buf
    ids = _ids()
    with torch.no_grad():
        fresh = fresh.cuda().eval()
        _same(fresh(ids).logits, ref(ids).logits, "loaded model against the model swapped in memory")
    got = fresh.get_submodule(m["names"][0]).experts
    assert (got.gate_kind, got.gate_limit, got.gate_alpha) == (ex.gate_kind, ex.gate_limit, ex.gate_alpha)
