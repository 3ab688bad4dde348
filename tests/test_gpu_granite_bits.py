"""-m gpu: fuse_granite_residual on tiny GraniteForCausalLM models (tests/granite_twin.py): the fused model against the SAME model after swap_linears +
fuse_llama_layers alone — logits, every hidden state and greedy generation with the KV cache are the same bits; one forward of L layers launches 1 K1n, 2L - 1 K1ma and
1 K1mo and no torch multiply or add inside the layers, where the baseline launches 2L multiplies, 2L adds and 2L K1n; the same with a refused layer in the middle."""
import pytest
import torch

from protoquant_amd import granite  # noqa: F401  (the module this file is about)
from tests import granite_twin as G
from tests.llama_twin import VOCAB, decoder_layers

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}
CASES = [("bf16", "aligned", 2), ("bf16", "ragged", 3), ("fp16", "aligned", 3), ("fp16", "ragged", 2), ("f32", "ragged", 2)]


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    from protoquant_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return protoquant_amd


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ, max |d| {float((a.float() - b.float()).abs().max())}"


def _compare_forwards(base, fused, batches, what):
    for ids in batches:
        with torch.no_grad():
            ob, of = base(ids, output_hidden_states=True), fused(ids, output_hidden_states=True)
        assert bool(torch.isfinite(ob.logits.float()).all())
        _same_bits(of.logits, ob.logits, f"{what} ids {tuple(ids.shape)}: logits")
        assert len(of.hidden_states) == len(ob.hidden_states)
        for i, (h, hw) in enumerate(zip(of.hidden_states, ob.hidden_states)):
            _same_bits(h, hw, f"{what} ids {tuple(ids.shape)}: hidden state {i}")
    with torch.no_grad():
        gb, gf = (m.generate(batches[0][:, :16], max_new_tokens=12, min_new_tokens=12, do_sample=False, use_cache=True, pad_token_id=0) for m in (base, fused))
    assert gb.shape == (batches[0].shape[0], 28) and torch.equal(gf, gb), f"{what}: greedy generation differs"
    assert not any(l._rf_inbox.pending for l in decoder_layers(fused) if hasattr(l, "_rf_inbox"))


def _batches():
    g = torch.Generator().manual_seed(11)
    return [torch.randint(3, VOCAB, s, generator=g).cuda() for s in ((2, 40), (1, 1), (3, 7))]          # 80, 1 and 21 rows


@pytest.mark.parametrize("dt,geometry,layers", CASES, ids=[f"{a}-{b}-{c}L" for a, b, c in CASES])
def test_fused_model_holds_the_bits_and_the_launch_counts(pq, dt, geometry, layers):
    from protoquant_amd.llama import residual_fused_layers
    base, fused = G.pair(pq, G.build(DT[dt], geometry, layers))
    assert residual_fused_layers(base) == 0 and residual_fused_layers(fused) == layers
    assert all(isinstance(l, pq.ScaledResidualFusedLayer) and l.residual_multiplier == 0.22 for l in decoder_layers(fused))
    assert list(fused.state_dict().keys()) == list(base.state_dict().keys())
    batches = _batches()
    _compare_forwards(base, fused, batches, f"{dt} {geometry} {layers} layers")
    for model, want in ((base, dict(K1n=2 * layers, K1a=0, K1ma=0, K1mo=0, mul=2 * layers, add=2 * layers)),
                        (fused, dict(K1n=1, K1a=0, K1ma=2 * layers - 1, K1mo=1, mul=0, add=0))):
        with G.counted(model) as counts, torch.no_grad():
            model(batches[2], use_cache=False)
        assert counts == want, (counts, want)
    # the multiplier is read at every call: changed on both models, the bits stay the same and are others than before
    with torch.no_grad():
        before = fused(batches[2]).logits
        for m in (base, fused):
            for l in decoder_layers(m):
                l.residual_multiplier = 0.5
        lb, lf = base(batches[2]).logits, fused(batches[2]).logits
    _same_bits(lf, lb, "after residual_multiplier changed")
    assert not torch.equal(lf, before)


@pytest.mark.parametrize("dt,geometry", [("bf16", "ragged"), ("fp16", "aligned")])
def test_a_refused_layer_in_the_middle_ends_the_chain_with_k1mo(pq, dt, geometry):
    from protoquant_amd.llama import residual_fused_layers
    layers = 3
    base, fused = G.pair(pq, G.build(DT[dt], geometry, layers, seed=1), refuse=1)
    fl = decoder_layers(fused)
    assert residual_fused_layers(fused) == 2 and not isinstance(fl[1], pq.ScaledResidualFusedLayer) and fl[0]._rf_next == [None] and fl[2]._rf_next == [None]
    batches = _batches()
    _compare_forwards(base, fused, batches, f"{dt} {geometry}, layer 1 refused")
    with G.counted(fused) as counts, torch.no_grad():
        fused(batches[2], use_cache=False)
    # layers 0 and 2: their own input norm, K1ma after the attention, K1mo at the end; layer 1: the eager flow
    assert counts == dict(K1n=4, K1a=0, K1ma=2, K1mo=2, mul=2, add=2), counts


def test_logits_stay_where_they_were_against_the_unquantised_model(pq):
    """the cosine of all logits to the unquantised bf16 model is a property of the int8 path, reported in the README; the switch leaves it unchanged (the same bits)"""
    cos = []
    for seed in range(2):
        model = G.build(torch.bfloat16, "aligned", 2, seed=seed)
        ids = torch.randint(3, VOCAB, (2, 32), generator=torch.Generator().manual_seed(seed)).cuda()
        with torch.no_grad():
            ref = model(ids).logits.float()
        base, fused = G.pair(pq, model)
        with torch.no_grad():
            lb, lf = base(ids).logits, fused(ids).logits
        _same_bits(lf, lb, f"seed {seed}")
        cos.append(float(torch.nn.functional.cosine_similarity(lf.float().flatten(), ref.flatten(), dim=0)))
    print("cosine of the fused int8 logits to the unquantised bf16 model:", cos)
    assert all(c == c for c in cos)
