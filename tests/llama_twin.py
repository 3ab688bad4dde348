"""TEST INFRASTRUCTURE — tiny transformers decoders for the bit-level tests of protoquant_amd/llama.py (tests/test_gpu_llama_bits.py): built in code from a config with
random initialisation (nothing is loaded from a hub), an unfused TWIN of a swapped model whose two norms per layer are the QSPEC norm, and a recorder of every call the
library's modules receive inside the decoder layers.  A plain module, imported explicitly: no fixtures live here.

Why the twin is bit-exact and the eager model is not: HF's RMSNorm sums the squares in torch's order, QSPEC N1-N3 pins another, so the eager chain and the fused chain differ
in ~5e-6 of the stored activations.  QSPEC N6 says the codes of rmsnorm_quantize are Q1-Q6 on the rows of h AS STORED: quantize(rmsnorm_quantize(x, w, eps, return_h=True)[1])
has the fused kernel's codes and scale bit for bit, FusedQLinear equals its separate projections bit for bit, and everything else (rope, attention, the adds, the final norm)
is the same stock op on the same bits.  So the twin equals the fused model in every bit, for every seed."""
import contextlib
import copy
import re
from dataclasses import dataclass, field

import pytest
import torch
from torch import nn

FAMILIES = {"llama": ("LlamaConfig", "LlamaForCausalLM"), "mistral": ("MistralConfig", "MistralForCausalLM"),
            "qwen2": ("Qwen2Config", "Qwen2ForCausalLM"), "qwen3": ("Qwen3Config", "Qwen3ForCausalLM")}

# name -> (hidden, intermediate, heads, kv heads, head dim)
#   aligned: every K a multiple of 128
#   ragged:  K1n at 320 columns, K1s at 696 (generic / odd row layouts); q/k/v and gate_up take _KPadded with a QTensor input (320 -> 384), down too (696 -> 768);
#            q (320 wide) and k / v (64 wide) differ: a wrong slice boundary cannot hide behind equal widths
#   wide:    the vector row layouts of K1n / K1s and a multi-tile GEMM
GEOMETRIES = {"aligned": (256, 640, 4, 2, 64), "ragged": (320, 696, 5, 1, 64), "wide": (1024, 2816, 8, 2, 128)}
VOCAB = 512
NORMS = ("input_layernorm", "post_attention_layernorm")


@dataclass
class Built:
    model: nn.Module          # on the GPU, .eval(), nn.Linear projections (not yet swapped)
    weights: dict             # the float weights of the whole model as the kernels see them (model dtype), on the CPU, by state-dict key
    config: object
    geometry: tuple


def build(family: str, dtype: torch.dtype, geometry: str, layers: int = 2, seed: int = 0, **cfg) -> Built:
    """A seeded random-init decoder of `family` at GEOMETRIES[geometry]; both norm weights of every layer are 1 + 0.1 randn.  Skips when the installed transformers
    lacks the family."""
    tr = pytest.importorskip("transformers")
    cname, mname = FAMILIES[family]
    if not (hasattr(tr, cname) and hasattr(tr, mname)):
        pytest.skip(f"the installed transformers has no {mname}")
    H, I, heads, kv, hd = GEOMETRIES[geometry]
    kw = dict(vocab_size=VOCAB, hidden_size=H, intermediate_size=I, num_hidden_layers=layers, num_attention_heads=heads, num_key_value_heads=kv, head_dim=hd,
              max_position_embeddings=256, rms_norm_eps=1e-6)
    if family == "mistral":
        kw["sliding_window"] = None
    kw.update(cfg)
    torch.manual_seed(seed)
    config = getattr(tr, cname)(**kw)
    model = getattr(tr, mname)(config).to(dtype).cuda().eval()
    with torch.no_grad():
        for layer in decoder_layers(model):
            for n in NORMS:
                getattr(layer, n).weight.copy_((1 + 0.1 * torch.randn(H)).to(dtype))
    weights = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    return Built(model, weights, config, GEOMETRIES[geometry])


def decoder_layers(model: nn.Module) -> list:
    return [m for m in model.modules() if all(hasattr(m, c) for c in NORMS + ("self_attn", "mlp"))]


class QSpecNorm(nn.Module):
    """RMSNorm by the library's own kernel: the normalised activation h of rmsnorm_quantize (QSPEC N1-N5), stored in the input dtype — the rows the fused kernel quantises"""

    def __init__(self, weight: torch.Tensor, eps: float):
        super().__init__()
        self.weight = nn.Parameter(weight.detach().clone(), requires_grad=False)
        self.variance_epsilon = float(eps)

    def forward(self, x):
        from protoquant_amd.qtensor import rmsnorm_quantize
        return rmsnorm_quantize(x, self.weight, self.variance_epsilon, return_h=True)[1]


def twin(swapped_model: nn.Module) -> nn.Module:
    """A deep copy of a model after swap_linears(..., fuse_gated_mlp=True) whose input_layernorm / post_attention_layernorm are QSpecNorm.  The final norm and Qwen3's
    q_norm / k_norm stay stock, as they do in the fused model."""
    t = copy.deepcopy(swapped_model)
    for layer in decoder_layers(t):
        for n in NORMS:
            old = getattr(layer, n)
            setattr(layer, n, QSpecNorm(old.weight, old.variance_epsilon))
    return t


# ---------------------------------------------------------------- the recorder
@dataclass
class Call:
    path: str                 # the module's name in the model
    layer: int                # index of the decoder layer it belongs to
    role: str                 # the path below the layer ("" = the layer itself)
    kind: str                 # "norm" | "qkv" | "slice" | "o_proj" | "gate_up" | "down" | "layer"
    inputs: dict = field(default_factory=dict)
    output: object = None


def _cpu(v):
    from protoquant_amd.qtensor import QTensor
    if isinstance(v, QTensor):
        return {"int_data": v.int_data.detach().cpu(), "scale": v.scale.detach().cpu(), "orig_dtype": v.orig_dtype}
    if isinstance(v, torch.Tensor):
        return v.detach().cpu()
    if isinstance(v, (tuple, list)):
        return tuple(_cpu(e) for e in v)
    return v


_LAYER_PATH = re.compile(r"(?:^|\.)layers\.(\d+)(?:\.(.*))?$")


@contextlib.contextmanager
def record(model: nn.Module):
    """Forward hooks on the library's modules inside the decoder layers — RMSNormQuant, the FusedQLinear under qkv_fused and the slices that serve q / k / v from it, o_proj,
    GatedMLP.gate_up / .down — and on the layers themselves.  Yields the list the calls are appended to, in call order: the module's path and CPU copies of its tensor
    inputs and outputs (a QTensor as its int_data, scale and orig_dtype; K1a as x, residual and the returned (QTensor, sum))."""
    from protoquant_amd.llama import RMSNormQuant, _FusedSlice, _SharedFused
    from protoquant_amd.qlinear import GatedMLP
    calls, handles = [], []
    layers = set(map(id, decoder_layers(model)))

    def kind_of(name, mod, parents):
        parent = parents.get(name.rpartition(".")[0])
        if id(mod) in layers:
            return "layer"
        if isinstance(mod, RMSNormQuant):
            return "norm"
        if isinstance(mod, _FusedSlice):
            return "slice"
        if isinstance(parent, _SharedFused) and name.endswith(".fused"):
            return "qkv"
        if name.endswith(".self_attn.o_proj"):
            return "o_proj"
        if isinstance(parent, GatedMLP):
            return {"gate_up": "gate_up", "down": "down"}.get(name.rpartition(".")[2])
        return None

    def hook_for(name, kind, layer, role):
        def hook(mod, args, kwargs, out):
            c = Call(name, layer, role, kind)
            x = args[0] if args else kwargs.get("hidden_states", kwargs.get("x"))
            c.inputs["x"] = _cpu(x)
            if kind == "norm":
                residual = kwargs.get("residual", args[1] if len(args) > 1 else None)
                if residual is not None:
                    c.inputs["residual"] = _cpu(residual)
            if kind == "slice":
                c.inputs["index"] = mod.index
            c.output = _cpu(out[0] if kind == "layer" and isinstance(out, (tuple, list)) else out)
            calls.append(c)
        return hook

    named = dict(model.named_modules())
    for name, mod in named.items():
        m = _LAYER_PATH.search(name)
        if m is None:
            continue
        kind = kind_of(name, mod, named)
        if kind is not None:
            handles.append(mod.register_forward_hook(hook_for(name, kind, int(m.group(1)), m.group(2) or ""), with_kwargs=True))
    try:
        yield calls
    finally:
        for h in handles:
            h.remove()
