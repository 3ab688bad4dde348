"""-m gpu: fuse_gemma_postnorm_residual on whole Gemma-2 and Gemma-3 (text) decoders, held to BITS.  tests/gemma_twin.py builds tiny models in code.

a. the model after swap_linears + fuse_gemma_layers + fuse_gemma_postnorm_residual equals an unfused TWIN (tests/gemma_postnorm_twin.py: gemma_twin's twin whose two
   post-norms per layer are the specified norm by the library's own kernel, followed by the layer's torch add), bit for bit: logits, every hidden state, greedy
   generation with the KV cache — bf16 at hidden 256 and 320, fp16 once, 2 and 3 layers;
b. the launches of a forward: 2L - 1 K1pang and one K1pa, one K1ng (the first layer's input_layernorm), no K1ang, no eager post-norm call (Gemma-2: no eager RMSNorm
   module call at all inside the decoder layers);
c. a model with one refused layer in the middle (a hook on its post-norm) still equals its twin, and that layer's predecessor ends with K1pa;
d. after an exception inside the stack nothing stays pending; a deep copy starts with empty hand-overs;
e. the cosine of all logits to the unquantised bf16 original, beside that of the same int8 model without the switch."""
import copy
import importlib

import pytest
import torch

from tests import gemma_postnorm_twin as PT
from tests import gemma_twin as T

pytestmark = pytest.mark.gpu
tr = pytest.importorskip("transformers")

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    from protoquant_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return protoquant_amd


def _fused(pq, swapped, layers, refused=()):
    from protoquant_amd.llama import residual_fused_layers
    m = copy.deepcopy(swapped)
    assert pq.fuse_gemma_layers(m) == layers and residual_fused_layers(m) == 0
    handles = [getattr(T.decoder_layers(m)[i], "post_attention_layernorm").register_forward_hook(lambda mod, a, o: None) for i in refused]
    assert pq.fuse_gemma_postnorm_residual(m) == layers - len(refused) and residual_fused_layers(m) == layers - len(refused)
    assert [isinstance(l, pq.SandwichFusedLayer) for l in T.decoder_layers(m)] == [i not in refused for i in range(layers)]
    return m, handles


def _same_bits(a: torch.Tensor, b: torch.Tensor, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ, max |d| {float((a.float() - b.float()).abs().max())}"


def _forward_both(tw, fused, ids, what):
    with torch.no_grad():
        a, b = tw(ids, output_hidden_states=True), fused(ids, output_hidden_states=True)
    _same_bits(b.logits, a.logits, f"{what}: logits")
    assert len(a.hidden_states) == len(b.hidden_states)
    for i, (h, hw) in enumerate(zip(b.hidden_states, a.hidden_states)):
        _same_bits(h, hw, f"{what}: hidden state {i}")
    return a.logits


def _equal_to_the_twin(tw, fused, layers):
    g = torch.Generator().manual_seed(11)
    batches = [torch.randint(0, T.VOCAB, s, generator=g).cuda() for s in ((2, 48), (1, 1), (3, 7))]          # M = 96, 1 and 21 rows
    first = [_forward_both(tw, fused, ids, f"ids {tuple(ids.shape)}") for ids in batches]
    assert all(torch.isfinite(l.float()).all() for l in first)
    # the same ids objects, other hidden states: nothing computed for the first forward may be served again
    with torch.no_grad():
        for m in (tw, fused):
            m.model.embed_tokens.weight.mul_(1.5)
    for ids, l1 in zip(batches, first):
        assert not torch.equal(l1, _forward_both(tw, fused, ids, f"ids {tuple(ids.shape)} after the embedding changed in place"))
    # a prefill and decode steps against the KV cache
    with torch.no_grad():
        gen = [m.generate(batches[0][:, :16], max_new_tokens=4, min_new_tokens=4, do_sample=False, use_cache=True, pad_token_id=0) for m in (tw, fused)]
    assert gen[0].shape == (2, 20) and torch.equal(gen[1], gen[0]), "greedy generation differs from the twin's"
    assert all(l.self_attn.qkv_fused._outs is None and l.self_attn.qkv_fused._key is None for l in T.decoder_layers(fused))
    assert not any(l._rf_inbox.pending for l in T.decoder_layers(fused) if hasattr(l, "_rf_inbox"))


CASES_A = [("gemma2", "bf16", "aligned", 2), ("gemma2", "bf16", "ragged", 3), ("gemma3", "bf16", "aligned", 3), ("gemma3", "bf16", "ragged", 2), ("gemma2", "fp16", "aligned", 3)]


@pytest.mark.parametrize("family,dt,geometry,layers", CASES_A, ids=["-".join(map(str, c)) for c in CASES_A])
def test_sandwich_fused_model_equals_the_twin_bit_for_bit(pq, family, dt, geometry, layers):
    b = T.build(family, DT[dt], geometry, layers=layers, seed=0)
    swapped = pq.swap_linears(b.model)
    tw = PT.twin(swapped, family)
    fused, _ = _fused(pq, swapped, layers)
    _equal_to_the_twin(tw, fused, layers)


# ---------------------------------------------------------------- b. the launches of a forward
def _counters(monkeypatch, model):
    """call counters on the four norm functions gemma.py launches, and on every stock RMSNorm MODULE inside the decoder layers (the eager chains)"""
    GM = importlib.import_module("protoquant_amd.gemma")
    kernels = {"K1pang": 0, "K1pa": 0, "K1ng": 0, "K1ang": 0}
    eager = {}

    def counting(name, fn):
        def run(*a, **kw):
            kernels[name] += 1
            return fn(*a, **kw)
        return run
    for name, attr in (("K1pang", "gemma_postnorm_add_rmsnorm_quantize"), ("K1pa", "gemma_postnorm_add"), ("K1ng", "gemma_rmsnorm_quantize"),
                       ("K1ang", "add_gemma_rmsnorm_quantize")):
        monkeypatch.setattr(GM, attr, counting(name, getattr(GM, attr)))
    handles = []
    for i, layer in enumerate(T.decoder_layers(model)):
        for n, mod in layer.named_modules():
            if type(mod).__name__.endswith("RMSNorm"):
                def hook(m, a, o, key=(i, n)):
                    eager[key] = eager.get(key, 0) + 1
                handles.append(mod.register_forward_hook(hook))
    return kernels, eager, handles


@pytest.mark.parametrize("family", ["gemma2", "gemma3"])
def test_launch_counts(pq, monkeypatch, family):
    L = 4
    b = T.build(family, torch.bfloat16, "ragged", layers=L, seed=1)
    fused, _ = _fused(pq, pq.swap_linears(b.model), L)
    kernels, eager, handles = _counters(monkeypatch, fused)          # (hooks registered AFTER the fusion: they only count)
    assert len(handles) >= 2 * L
    ids = torch.randint(0, T.VOCAB, (1, 40), device="cuda")
    for rep in range(2):          # (the second forward: nothing was left over from the first)
        for k in kernels:
            kernels[k] = 0
        eager.clear()
        with torch.no_grad(), T.record(fused) as calls:
            fused(ids)
        assert kernels == {"K1pang": 2 * L - 1, "K1pa": 1, "K1ng": 1, "K1ang": 0}, (rep, kernels)
        post = {k: v for k, v in eager.items() if k[1] in PT.POST_NORMS}
        assert post == {}, f"eager post-norm calls: {post}"
        if family == "gemma2":
            assert eager == {}, f"eager RMSNorm calls inside the decoder layers: {eager}"
        else:
            assert set(n for _, n in eager) <= {"self_attn.q_norm", "self_attn.k_norm"}, eager          # Gemma-3's q_norm / k_norm stay the model's code
        n = {}
        for c in calls:
            k = c.kind + ("+residual" if c.kind == "norm" and "residual" in c.inputs else "")
            n[k] = n.get(k, 0) + 1
        assert n == {"layer": L, "qkv": L, "slice": 3 * L, "o_proj": L, "gate_up": L, "down": L, "norm+residual": 2 * L - 1, "norm": 1}, (rep, n)
        # the hand-over: layer i + 1's input_layernorm is called by layer i, with layer i's MLP output, and what it returns is layer i's output
        per = {}
        for c in calls:
            per.setdefault(c.layer, {}).setdefault(c.role, []).append(c)
        for i in range(L):
            assert len(per[i]["input_layernorm"]) == 1 and len(per[i]["pre_feedforward_layernorm"]) == 1
            c = per[i]["pre_feedforward_layernorm"][0]
            assert torch.equal(c.inputs["residual"], per[i][""][0].inputs["x"]) and torch.equal(c.inputs["x"], per[i]["self_attn.o_proj"][0].output)
            if i + 1 < L:
                c = per[i + 1]["input_layernorm"][0]
                assert torch.equal(c.inputs["x"], per[i]["mlp.down"][0].output) and torch.equal(c.inputs["residual"], per[i]["pre_feedforward_layernorm"][0].output[1])
                assert torch.equal(c.output[1], per[i][""][0].output) and torch.equal(per[i + 1][""][0].inputs["x"], per[i][""][0].output)


# ---------------------------------------------------------------- c. a refused layer in the middle
def test_a_refused_layer_in_the_middle_still_equals_its_twin(pq, monkeypatch):
    L = 3
    b = T.build("gemma2", torch.bfloat16, "aligned", layers=L, seed=2)
    swapped = pq.swap_linears(b.model)
    tw = PT.twin(swapped, "gemma2", keep_stock=(1,))
    fused, _ = _fused(pq, swapped, L, refused=(1,))
    layers = T.decoder_layers(fused)
    assert layers[0]._rf_next == [None] and layers[2]._rf_next == [None] and not hasattr(layers[1], "_rf_inbox")
    kernels, eager, _ = _counters(monkeypatch, fused)
    ids = torch.randint(0, T.VOCAB, (2, 24), generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad():
        fused(ids)
    # layers 0 and 2: K1ng (no hand-over reaches them), K1pang, K1pa; layer 1 as before the switch: two K1ng and its two eager post-norms
    assert kernels == {"K1pang": 2, "K1pa": 2, "K1ng": 4, "K1ang": 0}, kernels
    assert eager == {(1, "post_attention_layernorm"): 1, (1, "post_feedforward_layernorm"): 1}, eager
    _equal_to_the_twin(tw, fused, L)


# ---------------------------------------------------------------- d. nothing stays pending; copies start empty
def test_nothing_stays_pending_after_an_exception_and_copies_start_empty(pq):
    L = 3
    b = T.build("gemma2", torch.bfloat16, "aligned", layers=L, seed=5)
    fused, _ = _fused(pq, pq.swap_linears(b.model), L)
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
    # a deep copy made while a hand-over is pending starts empty, and computes the same bits
    t = torch.zeros(1, 12, 256, dtype=torch.bfloat16, device="cuda")
    layers[1]._rf_inbox.put(t, pq.quantize(t))
    assert layers[1]._rf_inbox.pending
    cp = copy.deepcopy(fused)
    layers[1]._rf_inbox.clear()
    cl = T.decoder_layers(cp)
    assert not any(l._rf_inbox.pending for l in cl) and [l._rf_next[0] for l in cl] == cl[1:] + [None] and all(a is not b for a, b in zip(cl, layers))
    with torch.no_grad():
        _same_bits(cp(ids).logits, want, "the deep copy")


# ---------------------------------------------------------------- e. against the unquantised model
SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)
# Measured on an MI355X over SEEDS (2 layers, `aligned`, bf16, ids [2, 96]), the cosine of all logits of the int8 model WITHOUT the switch to the unquantised bf16 model:
#   Gemma-2  0.999484 0.999473 0.999470 0.999448 0.999454 0.999389 0.999513 0.999479   spread (max - min) 1.25e-4
#   Gemma-3  0.999456 0.999404 0.999455 0.999456 0.999432 0.999407 0.999492 0.999384   spread (max - min) 1.08e-4
# and the sandwich-fused model gave the same six digits for every seed.  SPREAD is that measured spread: the fused cosine may fall below the unfused one of the same
# seed by no more than it.  The test prints the spread it recomputes beside it.
SPREAD = {"gemma2": 1.25e-4, "gemma3": 1.08e-4}


@pytest.mark.parametrize("family", ["gemma2", "gemma3"])
def test_cosine_of_all_logits_to_the_unquantised_model(pq, family):
    """Per seed (2 layers, `aligned`, bf16, ids [2, 96]): the cosine of all logits of the unquantised bf16 model to the int8 model without the switch
    (fuse_gemma_layers alone: eager post-norms) and with it (the specified post-norm).  The switch replaces the eager post-norm by NG1-NG5, which differs from it only
    by the pinned summation order: it must not cost accuracy.  Asserted per seed: fused >= unfused - SPREAD, the spread (max - min) that the UNFUSED cosine showed
    over SEEDS when it was measured (the figures stand beside SPREAD above); README "Gemma" carries the seed-0 values."""
    rows = []
    for seed in SEEDS:
        b = T.build(family, torch.bfloat16, "aligned", layers=2, seed=seed)
        ref = copy.deepcopy(b.model)
        swapped = pq.swap_linears(b.model)
        unfused = copy.deepcopy(swapped)
        assert pq.fuse_gemma_layers(unfused) == 2
        fused, _ = _fused(pq, swapped, 2)
        ids = torch.randint(0, T.VOCAB, (2, 96), generator=torch.Generator().manual_seed(5)).cuda()
        with torch.no_grad():
            a, u, f = (m(ids).logits.float().flatten() for m in (ref, unfused, fused))
        cos = lambda p, q: float(torch.dot(p, q) / (p.norm() * q.norm()))          # noqa: E731
        rows.append((seed, cos(a, u), cos(a, f)))
    spread = max(r[1] for r in rows) - min(r[1] for r in rows)
    for seed, cu, cf in rows:
        print(f"{family} seed {seed}: cosine of all logits to the unquantised bf16 model: without the switch {cu:.6f}, sandwich-fused {cf:.6f}")
    print(f"{family}: spread of the unfused cosine over seeds {SEEDS}: {spread:.6f}")
    for seed, cu, cf in rows:
        assert cf >= cu - SPREAD[family], (family, seed, cu, cf, SPREAD[family])
