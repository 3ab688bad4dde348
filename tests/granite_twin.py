"""TEST INFRASTRUCTURE — tiny transformers Granite decoders for the bit-level tests of protoquant_amd/granite.py (tests/test_gpu_granite_bits.py): built in code from a
config with random initialisation (nothing is loaded from a hub), in the manner of tests/llama_twin.py, whose helpers it imports.  The reference of a fused model is
the SAME model after swap_linears + fuse_llama_layers alone: its layers run the eager `residual + hidden * residual_multiplier` (a torch multiply and a torch add) and
K1n, and QSPEC S1 / A1 say the fused kernels store those bits.  A plain module, imported explicitly: no fixtures live here."""
import contextlib
import copy

import pytest
import torch
from torch import nn

from tests.llama_twin import NORMS, VOCAB, decoder_layers

# name -> (hidden, intermediate, heads, kv heads): GQA 4 / 2; "ragged" has padded K (320 -> 384 for q / k / v and gate_up, 696 -> 768 for down) and the generic row kernel
GEOMETRIES = {"aligned": (256, 640, 4, 2), "ragged": (320, 696, 4, 2)}
# Granite-3-like scalars, none of them 1: the three that are out of scope stay the model's own code in both models
SCALARS = dict(residual_multiplier=0.22, embedding_multiplier=12.0, attention_multiplier=0.015625, logits_scaling=8.0)


def build(dtype: torch.dtype, geometry: str, layers: int, seed: int = 0, **cfg) -> nn.Module:
    """a seeded random-init GraniteForCausalLM on the GPU, .eval(), nn.Linear projections; both norm weights of every layer are 1 + 0.1 randn"""
    tr = pytest.importorskip("transformers")
    if not (hasattr(tr, "GraniteConfig") and hasattr(tr, "GraniteForCausalLM")):
        pytest.skip("the installed transformers has no GraniteForCausalLM")
    H, I, heads, kv = GEOMETRIES[geometry]
    kw = dict(vocab_size=VOCAB, hidden_size=H, intermediate_size=I, num_hidden_layers=layers, num_attention_heads=heads, num_key_value_heads=kv,
              max_position_embeddings=256, rms_norm_eps=1e-6, pad_token_id=0, bos_token_id=1, eos_token_id=2, **SCALARS)
    kw.update(cfg)
    torch.manual_seed(seed)
    model = tr.GraniteForCausalLM(tr.GraniteConfig(**kw)).to(dtype).cuda().eval()
    with torch.no_grad():
        for layer in decoder_layers(model):
            for n in NORMS:
                getattr(layer, n).weight.copy_((1 + 0.1 * torch.randn(H)).to(dtype))
    return model


def pair(pq, model: nn.Module, refuse: int | None = None):
    """(baseline, fused): two copies of `model` after swap_linears(fuse_gated_mlp=True) and fuse_llama_layers; `fused` after fuse_granite_residual as well.  refuse: the
    index of a layer whose post_attention_layernorm gets a forward hook (in both copies) before the switch runs, so that the switch refuses that layer."""
    from protoquant_amd.llama import fuse_llama_layers
    swapped = pq.swap_linears(model, fuse_gated_mlp=True)
    n = len(decoder_layers(swapped))
    assert fuse_llama_layers(swapped) == n
    base, fused = copy.deepcopy(swapped), copy.deepcopy(swapped)
    if refuse is not None:
        for m in (base, fused):
            decoder_layers(m)[refuse].post_attention_layernorm.register_forward_hook(lambda mod, args, out: None)
    want = n - (refuse is not None)
    assert pq.fuse_granite_residual(fused) == want and pq.fuse_granite_residual(fused) == 0          # (a second call finds nothing left)
    return base, fused


@contextlib.contextmanager
def counted(model: nn.Module):
    """Counts, for the forwards run inside the block: the C-ABI calls of the three norm entries (K1ma and K1mo told apart by the null weight, the way
    tests/test_gpu_gptlike_residual.py counts entries) and the torch multiplies and adds that produce a tensor of the hidden state's shape INSIDE a decoder layer."""
    from torch.utils._python_dispatch import TorchDispatchMode

    from protoquant_amd import _lib
    L = _lib.lib()
    names = ("pq_rmsnorm_quant_rowwise", "pq_add_rmsnorm_quant_rowwise", "pq_scaled_add_rmsnorm_quant_rows")
    counts = dict(K1n=0, K1a=0, K1ma=0, K1mo=0, mul=0, add=0)
    orig = {n: getattr(L, n) for n in names}
    state = dict(depth=0, shape=None)

    def wrap(n):
        def f(*a):
            counts[{"pq_rmsnorm_quant_rowwise": "K1n", "pq_add_rmsnorm_quant_rowwise": "K1a"}.get(n) or ("K1mo" if a[7] is None else "K1ma")] += 1
            return orig[n](*a)
        return f

    class Ops(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            name = func.overloadpacket.__name__ if hasattr(func, "overloadpacket") else str(func)
            if state["depth"] and name in ("mul", "add", "mul_", "add_") and isinstance(out, torch.Tensor) and tuple(out.shape) == state["shape"]:
                counts[name.rstrip("_")] += 1
            return out

    def pre(mod, args, kwargs):
        x = args[0] if args else kwargs["hidden_states"]
        state["depth"] += 1
        state["shape"] = tuple(x.shape)

    def post(mod, args, kwargs, out):
        state["depth"] -= 1

    hs = []
    for layer in decoder_layers(model):
        hs += [layer.register_forward_pre_hook(pre, with_kwargs=True), layer.register_forward_hook(post, with_kwargs=True, always_call=True)]
    try:
        for n in names:
            setattr(L, n, wrap(n))
        with Ops():
            yield counts
    finally:
        for n in names:
            setattr(L, n, orig[n])
        for h in hs:
            h.remove()
