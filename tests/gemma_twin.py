"""TEST INFRASTRUCTURE — tiny transformers Gemma / Gemma-2 / Gemma-3 (text) decoders for the bit-level tests of protoquant_amd/gemma.py (tests/test_gpu_gemma_bits.py),
modelled on tests/llama_twin.py and importing its geometries, its layer finder and its call recorder: built in code from a config with random initialisation (nothing is
loaded from a hub), and an unfused TWIN of a swapped model.

Why the twin is bit-exact: QSPEC NG6 says the codes of gemma_rmsnorm_quantize are Q1-Q6 on the rows of h AS STORED, so quantize(gemma_rmsnorm_quantize(x, w, eps,
return_h=True)[1]) — what a qlinear does with the twin norm's output — has the fused kernel's codes and scale bit for bit; GG3 says the same of gelu_mul_quantize;
FusedQLinear equals its separate projections bit for bit; and everything else (the embedding scaling, rope, attention and its softcapping, q_norm / k_norm, the
post-norms, the adds, the final norm) is the same stock op on the same bits.  So the twin equals the fused model in every bit, for every seed."""
import copy

import pytest
import torch
from torch import nn

from tests.llama_twin import GEOMETRIES, VOCAB, Built, decoder_layers, record  # noqa: F401  (re-exported: the tests use them through this module)

FAMILIES = {"gemma": ("GemmaConfig", "GemmaForCausalLM"), "gemma2": ("Gemma2Config", "Gemma2ForCausalLM"), "gemma3": ("Gemma3TextConfig", "Gemma3ForCausalLM")}
ALL_NORMS = ("input_layernorm", "post_attention_layernorm", "pre_feedforward_layernorm", "post_feedforward_layernorm")
# the norms whose output only feeds int8 projections: what fuse_gemma_layers replaces (tests/test_gemma_recognition.py holds it to that)
FUSED_NORMS = {"gemma": ("input_layernorm", "post_attention_layernorm"), "gemma2": ("input_layernorm", "pre_feedforward_layernorm"),
               "gemma3": ("input_layernorm", "pre_feedforward_layernorm")}


def build(family: str, dtype: torch.dtype, geometry: str, layers: int = 2, seed: int = 0, **cfg) -> Built:
    """A seeded random-init decoder of `family` at GEOMETRIES[geometry]; EVERY Gemma norm weight of the model (transformers initialises them to 0) is 0.3 randn.
    Skips when the installed transformers lacks the family."""
    tr = pytest.importorskip("transformers")
    cname, mname = FAMILIES[family]
    if not (hasattr(tr, cname) and hasattr(tr, mname)):
        pytest.skip(f"the installed transformers has no {mname}")
    H, I, heads, kv, hd = GEOMETRIES[geometry]
    kw = dict(vocab_size=VOCAB, hidden_size=H, intermediate_size=I, num_hidden_layers=layers, num_attention_heads=heads, num_key_value_heads=kv, head_dim=hd,
              max_position_embeddings=256, rms_norm_eps=1e-6)
    kw.update(cfg)
    torch.manual_seed(seed)
    config = getattr(tr, cname)(**kw)
    model = getattr(tr, mname)(config).to(dtype).eval()
    with torch.no_grad():
        for m in model.modules():
            if type(m).__name__.endswith("RMSNorm"):
                m.weight.copy_((0.3 * torch.randn(m.weight.shape)).to(dtype))
    model = model.cuda()
    weights = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    return Built(model, weights, config, GEOMETRIES[geometry])


class GSpecNorm(nn.Module):
    """The Gemma RMSNorm by the library's own kernel: the normalised activation h of gemma_rmsnorm_quantize (QSPEC NG1-NG5), stored in the input dtype — the rows the
    fused kernel quantises"""

    def __init__(self, weight: torch.Tensor, eps: float):
        super().__init__()
        self.weight = nn.Parameter(weight.detach().clone(), requires_grad=False)
        self.eps = float(eps)

    def forward(self, x):
        from protoquant_amd.qtensor import gemma_rmsnorm_quantize
        return gemma_rmsnorm_quantize(x, self.weight, self.eps, return_h=True)[1]


class TwinGeGLU(nn.Module):
    """down(quantize(h)) with h = the stored activation of gelu_mul_quantize (QSPEC GG1-GG2), over SEPARATE gate and up projections"""

    def __init__(self, mlp: nn.Module):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj = mlp.gate_proj, mlp.up_proj, mlp.down_proj

    def forward(self, x):
        from protoquant_amd.qtensor import gelu_mul_quantize, quantize
        h = gelu_mul_quantize(self.gate_proj(x), self.up_proj(x), return_h=True)[1]
        return self.down_proj(quantize(h))


def twin(swapped_model: nn.Module, family: str) -> nn.Module:
    """A deep copy of a model after swap_linears(model) whose fusable norms are GSpecNorm and whose MLPs are TwinGeGLU.  q / k / v stay three qlinears; the post-norms,
    q_norm / k_norm and the final norm stay stock, as they do in the fused model."""
    t = copy.deepcopy(swapped_model)
    for layer in decoder_layers(t):
        for n in FUSED_NORMS[family]:
            old = getattr(layer, n)
            setattr(layer, n, GSpecNorm(old.weight, old.eps))
        layer.mlp = TwinGeGLU(layer.mlp)
    return t
