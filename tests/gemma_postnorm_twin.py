"""TEST INFRASTRUCTURE — the unfused TWIN of a sandwich-fused Gemma-2 / Gemma-3 model (tests/test_gpu_gemma_postnorm_bits.py): tests/gemma_twin.twin(...) — the
fusable norms return the stored h of gemma_rmsnorm_quantize, the MLP is down(quantize(stored h of gelu_mul_quantize)) — whose two POST-norms per layer are GSpecNorm as
well: the specified norm (QSPEC NG1-NG5) by the library's own kernel, stored in the input dtype, followed by the layer's own torch add.

Why the twin is bit-exact: PN1 is NG1-NG5 on the sublayer output, rounded to the storage dtype — GSpecNorm's output; A1 is the layer's torch add (one binary32 add, one
storage rounding); and NG6 says the codes after it are Q1-Q6 on the rows of h as stored.  Everything else is gemma_twin's argument."""
from torch import nn

from tests import gemma_twin as T

POST_NORMS = ("post_attention_layernorm", "post_feedforward_layernorm")


def twin(swapped_model: nn.Module, family: str, keep_stock=()) -> nn.Module:
    """gemma_twin.twin(swapped_model, family) with both post-norms of every layer replaced by GSpecNorm (same weight, same eps).  keep_stock: the indices of layers
    whose post-norms stay the stock modules — the twin of a model in which fuse_gemma_postnorm_residual refused those layers"""
    t = T.twin(swapped_model, family)
    for i, layer in enumerate(T.decoder_layers(t)):
        if i in keep_stock:
            continue
        for n in POST_NORMS:
            old = getattr(layer, n)
            setattr(layer, n, T.GSpecNorm(old.weight, old.eps))
    return t
