"""-m gpu: fuse_llama_layers(fuse_residual=True) — the two residual adds of a decoder layer inside the RMSNorm + quantisation kernels that follow them (K1a).  The add is
one binary32 add and one storage rounding either way (QSPEC A1), so the residual-fused model is held to the fused model WITHOUT it bit for bit: logits, every recorded
hidden state, greedy generation with the KV cache.  Plus the hand-over discipline: 2L - 1 fused add-norms and one plain input norm per forward, nothing pending after a
forward (one that raised included) or in a deep copy, a layer called alone, a refused layer in the middle of the stack."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
tr = pytest.importorskip("transformers")


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    from protoquant_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return protoquant_amd


def _llama(layers=3):
    cfg = tr.LlamaConfig(vocab_size=512, hidden_size=256, intermediate_size=640, num_hidden_layers=layers, num_attention_heads=4, num_key_value_heads=2,
                         max_position_embeddings=256)
    return tr.LlamaForCausalLM(cfg)


def _qwen3(layers=3):
    cfg = tr.Qwen3Config(vocab_size=512, hidden_size=256, intermediate_size=640, num_hidden_layers=layers, num_attention_heads=4, num_key_value_heads=2, head_dim=64,
                         max_position_embeddings=256)
    return tr.Qwen3ForCausalLM(cfg)


def _pair(pq, make, layers=3, seed=0):
    """(fused without the residual fusion, fused with it): the same weights"""
    from protoquant_amd.llama import fuse_llama_layers, residual_fused_layers
    torch.manual_seed(seed)
    model = make(layers).to(torch.bfloat16).cuda().eval()
    with torch.no_grad():
        for l in model.model.layers:        # non-trivial norm weights
            l.input_layernorm.weight.copy_((1 + 0.1 * torch.randn(256)).to(torch.bfloat16))
            l.post_attention_layernorm.weight.copy_((1 + 0.1 * torch.randn(256)).to(torch.bfloat16))
    pq.swap_linears(model, fuse_gated_mlp=True)
    a, b = model, copy.deepcopy(model)
    keys = list(b.state_dict().keys())
    assert fuse_llama_layers(a) == layers and residual_fused_layers(a) == 0
    assert fuse_llama_layers(b, fuse_residual=True) == layers and residual_fused_layers(b) == layers
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    return a, b, keys


def _pending(model):
    from protoquant_amd.llama import ResidualFusedLayer
    return [i for i, l in enumerate(model.model.layers) if isinstance(l, ResidualFusedLayer) and l._rf_inbox.pending]


@pytest.mark.parametrize("make", [_llama, _qwen3], ids=["llama", "qwen3"])
def test_logits_hidden_states_and_generation_are_bit_identical(pq, make):
    from protoquant_amd.llama import ResidualFusedLayer
    a, b, _ = _pair(pq, make)
    assert all(isinstance(l, ResidualFusedLayer) and isinstance(l, type(a.model.layers[0])) for l in b.model.layers)
    ids = torch.randint(0, 512, (2, 96), device="cuda")
    with torch.no_grad():
        oa, ob = a(ids, output_hidden_states=True), b(ids, output_hidden_states=True)
    assert torch.equal(oa.logits, ob.logits)
    assert len(oa.hidden_states) == len(ob.hidden_states) == 3 + 1
    for i, (ha, hb) in enumerate(zip(oa.hidden_states, ob.hidden_states)):
        assert torch.equal(ha, hb), f"hidden state {i}"
    assert _pending(b) == []
    with torch.no_grad():                       # decode shapes: one token per step against the KV cache
        ga = a.generate(ids[:, :16], max_new_tokens=16, do_sample=False, use_cache=True, pad_token_id=0)
        gb = b.generate(ids[:, :16], max_new_tokens=16, do_sample=False, use_cache=True, pad_token_id=0)
    assert ga.shape == (2, 32) and torch.equal(ga, gb)
    assert _pending(b) == []


def test_the_fused_add_norm_runs_2l_minus_1_times_and_the_plain_norm_once(pq):
    from protoquant_amd.llama import RMSNormQuant
    L = 4
    a, b, _ = _pair(pq, _llama, layers=L)
    counts = {"fused": 0, "plain": 0}

    def hook(mod, args, kwargs, out):
        counts["fused" if (kwargs.get("residual") is not None or len(args) > 1) else "plain"] += 1
    hs = [m.register_forward_hook(hook, with_kwargs=True) for m in b.modules() if isinstance(m, RMSNormQuant)]
    ids = torch.randint(0, 512, (1, 40), device="cuda")
    with torch.no_grad():
        ob = b(ids).logits
    assert counts == {"fused": 2 * L - 1, "plain": 1}, counts
    with torch.no_grad():
        assert torch.equal(a(ids).logits, ob)
    for h in hs:
        h.remove()
    # the model's input tensor is never written: the embedding output feeds layer 0 and stays what it was
    emb = b.model.embed_tokens(ids)
    keep = emb.clone()
    with torch.no_grad():
        b.model(inputs_embeds=emb)
    assert torch.equal(emb, keep)


def test_nothing_is_pending_after_a_forward_that_raised_or_in_a_deep_copy(pq):
    a, b, _ = _pair(pq, _llama)
    ids = torch.randint(0, 512, (1, 24), device="cuda")

    class Boom(RuntimeError):
        pass

    def boom(mod, args, kwargs):
        raise Boom()
    h = b.model.layers[2].mlp.register_forward_pre_hook(boom, with_kwargs=True)      # layer 1 has handed over to layer 2, which has consumed it; layer 2 raises
    with torch.no_grad(), pytest.raises(Boom):
        b(ids)
    h.remove()
    assert _pending(b) == []
    h = b.model.layers[1].self_attn.register_forward_pre_hook(boom, with_kwargs=True)
    with torch.no_grad(), pytest.raises(Boom):
        b(ids)
    h.remove()
    assert _pending(b) == []
    # a layer called alone parks a hand-over on its successor; a deep copy made then starts empty and shares nothing; the next forward of the original is still right
    x = torch.randn(1, 8, 256, device="cuda").to(torch.bfloat16)
    pos = b.model.rotary_emb(x, position_ids=torch.arange(8, device="cuda")[None])
    with torch.no_grad():
        b.model.layers[0](x, position_embeddings=pos)
    assert _pending(b) == [1]
    c = copy.deepcopy(b)
    assert _pending(c) == [] and _pending(b) == [1]
    assert c.model.layers[0]._rf_next[0] is c.model.layers[1] and c.model._rf_layers[0] is c.model.layers[0] and c.model.layers[0] is not b.model.layers[0]
    with torch.no_grad():
        want = a(ids).logits
        assert torch.equal(b(ids).logits, want) and torch.equal(c(ids).logits, want)
    assert _pending(b) == [] and _pending(c) == []


def test_a_layer_called_alone_gives_the_unfused_layers_bits(pq):
    a, b, _ = _pair(pq, _llama)
    x = torch.randn(2, 8, 256, device="cuda").to(torch.bfloat16)
    keep = x.clone()
    pos = a.model.rotary_emb(x, position_ids=torch.arange(8, device="cuda")[None])
    with torch.no_grad():
        for i in (0, 1, 2):                                   # a link of the chain, and its end (a torch add)
            assert torch.equal(a.model.layers[i](x, position_embeddings=pos), b.model.layers[i](x, position_embeddings=pos)), i
        # a hand-over parked for ANOTHER tensor is not served: layer 1 called with x right after layer 0 produced something else
        y = b.model.layers[0](x, position_embeddings=pos)
        assert torch.equal(b.model.layers[1](x, position_embeddings=pos), a.model.layers[1](x, position_embeddings=pos))
        # ... nor for the same tensor changed in place since
        y = b.model.layers[0](x, position_embeddings=pos)
        y.mul_(1.25)          # (not a power of two: RMSNorm of 2 y has the bits of RMSNorm of y, and a stale hand-over would have passed)
        assert torch.equal(b.model.layers[1](y, position_embeddings=pos), a.model.layers[1](y, position_embeddings=pos))
    assert torch.equal(x, keep)                               # the tensor a layer is called with is never written


def test_a_refused_layer_in_the_middle_breaks_the_chain_and_the_model_still_matches(pq):
    """layer 1 of 4 gets a Granite-style forward (residual_multiplier): it keeps the norm / qkv fusions, is not residual-fused, and its predecessor ends with a torch add"""
    from protoquant_amd.llama import ResidualFusedLayer, RMSNormQuant, fuse_llama_layers, residual_fused_layers
    torch.manual_seed(5)
    model = _llama(4).to(torch.bfloat16).cuda().eval()
    base = type(model.model.layers[1])

    class GraniteStyle(base):
        residual_multiplier = 0.5

        def forward(self, hidden_states, **kwargs):
            residual = hidden_states
            hidden_states, _ = self.self_attn(hidden_states=self.input_layernorm(hidden_states), **kwargs)
            hidden_states = residual + hidden_states * self.residual_multiplier
            residual = hidden_states
            hidden_states = self.mlp(self.post_attention_layernorm(hidden_states))
            return residual + hidden_states * self.residual_multiplier
    model.model.layers[1].__class__ = GraniteStyle
    pq.swap_linears(model, fuse_gated_mlp=True)
    a, b = model, copy.deepcopy(model)
    assert fuse_llama_layers(a) == 4
    assert fuse_llama_layers(b, fuse_residual=True) == 4 and residual_fused_layers(b) == 3
    lb = b.model.layers
    assert [isinstance(l, ResidualFusedLayer) for l in lb] == [True, False, True, True]
    assert isinstance(lb[1].input_layernorm, RMSNormQuant) and type(lb[1]) is GraniteStyle
    assert lb[0]._rf_next[0] is None and lb[2]._rf_next[0] is lb[3] and lb[3]._rf_next[0] is None
    ids = torch.randint(0, 512, (2, 48), device="cuda")
    with torch.no_grad():
        oa, ob = a(ids, output_hidden_states=True), b(ids, output_hidden_states=True)
    assert torch.equal(oa.logits, ob.logits) and all(torch.equal(x, y) for x, y in zip(oa.hidden_states, ob.hidden_states))
    assert _pending(b) == []
    # a second call finds nothing left to change (no layer is converted or hooked twice)
    assert fuse_llama_layers(b, fuse_residual=True) == 0 and residual_fused_layers(b) == 3 and len(b.model._rf_layers) == 3 and len(b.model._forward_hooks) == len(a.model._forward_hooks) + 1
