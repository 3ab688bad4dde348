"""-m gpu: fuse_olmo_layers on whole OLMo-2 and OLMo-3 decoders, held to BITS.  tests/olmo_twin.py builds tiny seeded models in code: 2 and 3 layers, GQA with 4 query
and 2 kv heads, hidden 256 and 320 (320: padded K), intermediate 640 and 696, bf16 at both sizes and fp16 once, sliding layers included for OLMo-3.

a. fuse_olmo_layers(model) (fuse_residual=False: one quantisation and one GEMM for q / k / v, q_norm / k_norm on column slices) equals the swap_linears model: logits,
   every hidden state, greedy generation with the KV cache, torch.equal;
b. fuse_olmo_layers(model, fuse_residual=True) equals its TWIN (the swap_linears model whose norms call olmo_rmsnorm, torch adds kept) in the same three comparisons,
   with one refused layer (a hooked post-norm) in the middle of the stack;
c. the launches of a forward: 1 K1, 2L - 1 K1oq, 1 K1oa and 2L K1on, no eager norm module call inside the layers — where the un-switched model calls 4L eager norms;
d. the cosine of all logits to the unquantised bf16 model, seeds 0-7, for the un-switched int8 model and for the switched one: per seed the switched cosine is not
   below the un-switched one by more than the un-switched model's own max - min over the eight seeds.
   Measured on an MI355X: OLMo-2 un-switched 0.998869 .. 0.999060 (spread 1.91e-4), switched 0.998867 .. 0.999061; OLMo-3 0.998958 .. 0.999071 (spread 1.13e-4) and
   0.998961 .. 0.999071; per seed the two differ by at most 6e-6."""
import copy
import importlib

import pytest
import torch

from tests import olmo_twin as T

pytestmark = pytest.mark.gpu
tr = pytest.importorskip("transformers")

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
CASES = [("olmo2", "bf16", "aligned", 2), ("olmo2", "bf16", "ragged", 3), ("olmo3", "bf16", "aligned", 3), ("olmo3", "bf16", "ragged", 2), ("olmo2", "fp16", "aligned", 3)]
IDS = ["-".join(map(str, c)) for c in CASES]


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    from protoquant_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return protoquant_amd


def _same_bits(a: torch.Tensor, b: torch.Tensor, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ, max |d| {float((a.float() - b.float()).abs().max())}"


def _forward_both(ref, got, ids, what):
    with torch.no_grad():
        a, b = ref(ids, output_hidden_states=True), got(ids, output_hidden_states=True)
    _same_bits(b.logits, a.logits, f"{what}: logits")
    assert len(a.hidden_states) == len(b.hidden_states)
    for i, (h, hw) in enumerate(zip(b.hidden_states, a.hidden_states)):
        _same_bits(h, hw, f"{what}: hidden state {i}")
    return a.logits


def _equal_models(ref, got):
    g = torch.Generator().manual_seed(11)
    batches = [torch.randint(0, T.VOCAB, s, generator=g).cuda() for s in ((2, 48), (1, 1), (3, 7))]          # M = 96, 1 and 21 rows; 48 tokens pass the sliding window
    first = [_forward_both(ref, got, ids, f"ids {tuple(ids.shape)}") for ids in batches]
    assert all(torch.isfinite(l.float()).all() for l in first)
    # the same ids objects, other hidden states: nothing computed for the first forward may be served again
    with torch.no_grad():
        for m in (ref, got):
            m.model.embed_tokens.weight.mul_(1.5)
    for ids, l1 in zip(batches, first):
        assert not torch.equal(l1, _forward_both(ref, got, ids, f"ids {tuple(ids.shape)} after the embedding changed in place"))
    # a prefill and decode steps against the KV cache
    with torch.no_grad():
        gen = [m.generate(batches[0][:, :16], max_new_tokens=4, min_new_tokens=4, do_sample=False, use_cache=True, pad_token_id=0) for m in (ref, got)]
    assert gen[0].shape == (2, 20) and torch.equal(gen[1], gen[0]), "greedy generation differs"
    assert all(l.self_attn.qkv_fused._outs is None and l.self_attn.qkv_fused._key is None for l in T.decoder_layers(got))
    assert not any(l._rf_inbox.pending for l in T.decoder_layers(got) if hasattr(l, "_rf_inbox"))


# ---------------------------------------------------------------- a. without the switch: the swap_linears model's bits
@pytest.mark.parametrize("family,dt,geometry,layers", CASES, ids=IDS)
def test_qkv_fusion_alone_changes_no_bit(pq, family, dt, geometry, layers):
    from protoquant_amd.llama import residual_fused_layers
    b = T.build(family, DT[dt], geometry, layers=layers, seed=0)
    swapped = pq.swap_linears(b.model, fuse_gated_mlp=True)
    fused = copy.deepcopy(swapped)
    assert pq.fuse_olmo_layers(fused) == layers and residual_fused_layers(fused) == 0
    _equal_models(swapped, fused)


# ---------------------------------------------------------------- b. with the switch: the twin's bits, a refused layer in the middle
def _fused(pq, swapped, layers, refused=()):
    from protoquant_amd.llama import residual_fused_layers
    m = copy.deepcopy(swapped)
    handles = [T.decoder_layers(m)[i].post_attention_layernorm.register_forward_hook(lambda mod, a, o: None) for i in refused]
    assert pq.fuse_olmo_layers(m, fuse_residual=True) == layers and residual_fused_layers(m) == layers - len(refused)
    assert [isinstance(l, pq.PostNormFusedLayer) for l in T.decoder_layers(m)] == [i not in refused for i in range(layers)]
    return m, handles


@pytest.mark.parametrize("family,dt,geometry,layers", CASES, ids=IDS)
def test_post_norm_fused_model_equals_the_twin_bit_for_bit(pq, family, dt, geometry, layers):
    b = T.build(family, DT[dt], geometry, layers=layers, seed=0)
    swapped = pq.swap_linears(b.model, fuse_gated_mlp=True)
    fused, _ = _fused(pq, swapped, layers)
    _equal_models(T.twin(swapped), fused)


@pytest.mark.parametrize("family", ["olmo2", "olmo3"])
def test_a_refused_layer_in_the_middle_still_equals_its_twin(pq, monkeypatch, family):
    L = 3
    b = T.build(family, torch.bfloat16, "aligned", layers=L, seed=2)
    swapped = pq.swap_linears(b.model, fuse_gated_mlp=True)
    tw = T.twin(swapped, keep_stock=(1,))
    fused, _ = _fused(pq, swapped, L, refused=(1,))
    layers = T.decoder_layers(fused)
    assert layers[0]._rf_next == [None] and layers[2]._rf_next == [None] and not hasattr(layers[1], "_rf_inbox")
    kernels, eager, _ = _counters(monkeypatch, fused)
    ids = torch.randint(0, T.VOCAB, (2, 24), generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad():
        fused(ids)
    # layers 0 and 2: K1 (no hand-over reaches them), K1oq, K1oa, two K1on; layer 1 as before the switch: its four eager norms
    assert kernels == {"K1": 2, "K1oq": 2, "K1oa": 2, "K1on": 4}, kernels
    assert eager == {(1, n): 1 for n in ("post_attention_layernorm", "post_feedforward_layernorm", "self_attn.q_norm", "self_attn.k_norm")}, eager
    _equal_models(tw, fused)


# ---------------------------------------------------------------- c. the launches of a forward
def _counters(monkeypatch, model):
    """call counters on the four functions olmo.py launches, and on every stock RMSNorm MODULE inside the decoder layers (the eager chains)"""
    OM = importlib.import_module("protoquant_amd.olmo")
    kernels = {"K1": 0, "K1oq": 0, "K1oa": 0, "K1on": 0}
    eager = {}

    def counting(name, fn):
        def run(*a, **kw):
            kernels[name] += 1
            return fn(*a, **kw)
        return run
    for name, attr in (("K1", "quantize"), ("K1oq", "olmo_postnorm_add_quantize"), ("K1oa", "olmo_postnorm_add"), ("K1on", "olmo_rmsnorm")):
        monkeypatch.setattr(OM, attr, counting(name, getattr(OM, attr)))
    handles = []
    for i, layer in enumerate(T.decoder_layers(model)):
        for n, mod in layer.named_modules():
            if type(mod).__name__.endswith("RMSNorm") and not isinstance(mod, OM.OlmoRMSNorm):
                def hook(m, a, o, key=(i, n)):
                    eager[key] = eager.get(key, 0) + 1
                handles.append(mod.register_forward_hook(hook))
    return kernels, eager, handles


@pytest.mark.parametrize("family", ["olmo2", "olmo3"])
def test_launch_counts(pq, monkeypatch, family):
    L = 4
    b = T.build(family, torch.bfloat16, "ragged", layers=L, seed=1)
    swapped = pq.swap_linears(b.model, fuse_gated_mlp=True)
    fused, _ = _fused(pq, swapped, L)
    ids = torch.randint(0, T.VOCAB, (1, 40), device="cuda")
    kernels, eager, handles = _counters(monkeypatch, fused)          # (hooks registered AFTER the fusion: they only count)
    assert len(handles) == 2 * L                                      # the two post-norm modules per layer: still there, never called
    adds = []
    for rep in range(2):          # (the second forward: nothing was left over from the first)
        for k in kernels:
            kernels[k] = 0
        eager.clear()
        with torch.no_grad():
            out = fused(ids, output_hidden_states=True)
        assert kernels == {"K1": 1, "K1oq": 2 * L - 1, "K1oa": 1, "K1on": 2 * L}, (rep, kernels)
        assert eager == {}, f"eager norm calls inside the decoder layers: {eager}"
        adds.append(out.logits)
    assert torch.equal(adds[0], adds[1])
    # the un-switched model: 4L eager norm chains, none of the fused launches
    unfused = copy.deepcopy(swapped)
    assert pq.fuse_olmo_layers(unfused) == L
    kernels, eager, handles = _counters(monkeypatch, unfused)
    assert len(handles) == 4 * L
    with torch.no_grad():
        unfused(ids)
    assert kernels == {"K1": 0, "K1oq": 0, "K1oa": 0, "K1on": 0} and len(eager) == 4 * L and set(eager.values()) == {1}


def test_nothing_stays_pending_after_an_exception(pq):
    L = 3
    b = T.build("olmo2", torch.bfloat16, "aligned", layers=L, seed=5)
    fused, _ = _fused(pq, pq.swap_linears(b.model, fuse_gated_mlp=True), L)
    layers = T.decoder_layers(fused)
    ids = torch.randint(0, T.VOCAB, (1, 12), device="cuda")
    with torch.no_grad():
        want = fused(ids).logits
    seen = []

    def boom(mod, args, kwargs):
        seen.append(mod._rf_inbox.pending)          # layer 0 has handed its codes over: pending at this very moment
        raise RuntimeError("inside the stack")
    h = layers[1].register_forward_pre_hook(boom, with_kwargs=True)
    with pytest.raises(RuntimeError, match="inside the stack"), torch.no_grad():
        fused(ids)
    h.remove()
    assert seen == [True] and not any(l._rf_inbox.pending for l in layers)
    with torch.no_grad():
        _same_bits(fused(ids).logits, want, "the forward after the exception")
        _same_bits(copy.deepcopy(fused)(ids).logits, want, "a deep copy")


# ---------------------------------------------------------------- d. against the unquantised model
SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)


@pytest.mark.parametrize("family", ["olmo2", "olmo3"])
def test_cosine_of_all_logits_to_the_unquantised_model(pq, family):
    """Per seed (2 layers, `aligned`, bf16, ids [2, 96]): the cosine of all logits of the unquantised bf16 model to the int8 model without the switch (eager norms) and
    with it (the specified norm).  The switch replaces the eager norm by NO1-NO5, which differs from it only by the pinned summation order: it must not cost accuracy.
    Asserted per seed, relative and not a fixed number: switched >= un-switched - spread, where spread is the un-switched model's own max - min over the eight seeds,
    recomputed here."""
    rows = []
    for seed in SEEDS:
        b = T.build(family, torch.bfloat16, "aligned", layers=2, seed=seed)
        ref = copy.deepcopy(b.model)
        swapped = pq.swap_linears(b.model, fuse_gated_mlp=True)
        unfused = copy.deepcopy(swapped)
        assert pq.fuse_olmo_layers(unfused) == 2
        fused, _ = _fused(pq, swapped, 2)
        ids = torch.randint(0, T.VOCAB, (2, 96), generator=torch.Generator().manual_seed(5)).cuda()
        with torch.no_grad():
            a, u, f = (m(ids).logits.float().flatten() for m in (ref, unfused, fused))
        cos = lambda p, q: float(torch.dot(p, q) / (p.norm() * q.norm()))          # noqa: E731
        rows.append((seed, cos(a, u), cos(a, f)))
    spread = max(r[1] for r in rows) - min(r[1] for r in rows)
    for seed, cu, cf in rows:
        print(f"{family} seed {seed}: cosine of all logits to the unquantised bf16 model: without the switch {cu:.6f}, post-norm-fused {cf:.6f}")
    print(f"{family}: un-switched {min(r[1] for r in rows):.6f} .. {max(r[1] for r in rows):.6f} (spread {spread:.6f}), switched {min(r[2] for r in rows):.6f} .. "
          f"{max(r[2] for r in rows):.6f}")
    for seed, cu, cf in rows:
        assert cf >= cu - spread, (family, seed, cu, cf, spread)
