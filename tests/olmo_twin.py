"""TEST INFRASTRUCTURE — tiny transformers OLMo-2 / OLMo-3 decoders for the bit-level tests of protoquant_amd/olmo.py (tests/test_gpu_olmo_bits.py): built in code from
a config with random initialisation (nothing is loaded from a hub), and an unfused TWIN of a swapped model.

The twin is the swap_linears model with the four norm modules of every layer — post_attention_layernorm, post_feedforward_layernorm and the attention's q_norm
and k_norm — replaced by OSpecNorm, the specified norm (QSPEC NO1-NO5) by the library's own kernel K1on, stored in the input dtype; its torch adds, its three separate
q / k / v projections and its GatedMLP are kept.

Why the twin is bit-exact: PO1 is NO1-NO5 on the sublayer output, rounded to the storage dtype — OSpecNorm's output; A1 is the layer's own torch add (one binary32
add, one storage rounding); K1oq's codes are Q1-Q6 on the rows of the sum AS STORED, which is what the qlinear / GatedMLP that receives the sum computes; FusedQLinear
equals its separate projections bit for bit, and K1on on a column slice of the fused output reads the bits the separate projection stored.  Everything else (rope,
attention, sliding windows, the final norm) is the same stock op on the same bits."""
import copy
from dataclasses import dataclass

import pytest
import torch
from torch import nn

VOCAB = 512
GEOMETRIES = {"aligned": (256, 640, 4, 2), "ragged": (320, 696, 4, 2)}          # hidden, intermediate, query heads, kv heads; 320: K is padded for the GEMMs
FAMILIES = {"olmo2": ("Olmo2Config", "Olmo2ForCausalLM"), "olmo3": ("Olmo3Config", "Olmo3ForCausalLM")}
POST_NORMS = ("post_attention_layernorm", "post_feedforward_layernorm")
QK_NORMS = ("q_norm", "k_norm")


@dataclass
class Built:
    model: nn.Module          # on the GPU, .eval(), nn.Linear projections (not yet swapped)
    config: object
    geometry: tuple


def build(family: str, dtype: torch.dtype, geometry: str, layers: int = 2, seed: int = 0) -> Built:
    """A seeded random-init decoder of `family` at GEOMETRIES[geometry]; every norm weight is 1 + 0.3 randn.  OLMo-3: a sliding window of 16 on every layer but each
    third (sliding, sliding, full), so sliding layers are included at 2 and 3 layers.  Skips when the installed transformers lacks the family."""
    tr = pytest.importorskip("transformers")
    cname, mname = FAMILIES[family]
    if not (hasattr(tr, cname) and hasattr(tr, mname)):
        pytest.skip(f"the installed transformers has no {mname}")
    H, I, heads, kv = GEOMETRIES[geometry]
    kw = dict(vocab_size=VOCAB, hidden_size=H, intermediate_size=I, num_hidden_layers=layers, num_attention_heads=heads, num_key_value_heads=kv,
              max_position_embeddings=256, rms_norm_eps=1e-6)
    if family == "olmo3":
        kw.update(sliding_window=16, layer_types=["full_attention" if i % 3 == 2 else "sliding_attention" for i in range(layers)])
    torch.manual_seed(seed)
    config = getattr(tr, cname)(**kw)
    model = getattr(tr, mname)(config).to(dtype).eval()
    with torch.no_grad():
        for m in model.modules():
            if type(m).__name__.endswith("RMSNorm"):
                m.weight.copy_((1.0 + 0.3 * torch.randn(m.weight.shape)).to(dtype))
    return Built(model.cuda(), config, GEOMETRIES[geometry])


def decoder_layers(model: nn.Module) -> list:
    return [m for m in model.modules() if all(hasattr(m, c) for c in POST_NORMS + ("self_attn", "mlp"))]


class OSpecNorm(nn.Module):
    """The OLMo RMSNorm by the library's own kernel (olmo_rmsnorm, K1on: QSPEC NO1-NO5), stored in the input dtype"""

    def __init__(self, weight: torch.Tensor, eps: float):
        super().__init__()
        self.weight = nn.Parameter(weight.detach().clone(), requires_grad=False)
        self.variance_epsilon = float(eps)

    def forward(self, x):
        from protoquant_amd.qtensor import olmo_rmsnorm
        return olmo_rmsnorm(x, self.weight, self.variance_epsilon)


def twin(swapped_model: nn.Module, keep_stock=()) -> nn.Module:
    """A deep copy of a model after swap_linears(model, fuse_gated_mlp=True) whose post-norms, q_norm and k_norm are OSpecNorm.  keep_stock: the indices of layers
    whose norms stay the stock modules — the twin of a model in which fuse_olmo_layers(fuse_residual=True) refused those layers."""
    t = copy.deepcopy(swapped_model)
    for i, layer in enumerate(decoder_layers(t)):
        if i in keep_stock:
            continue
        for owner, names in ((layer, POST_NORMS), (layer.self_attn, QK_NORMS)):
            for n in names:
                old = getattr(owner, n)
                setattr(owner, n, OSpecNorm(old.weight, old.variance_epsilon))
    return t
