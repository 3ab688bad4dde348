"""Call-site integration for IBM Granite 3.x dense decoders: the Llama data flow with a scalar on every residual add,

    r1  = x  + self_attn(input_layernorm(x))[0]    * residual_multiplier
    out = r1 + mlp(post_attention_layernorm(r1))   * residual_multiplier

``swap_linears(model, fuse_gated_mlp=True)`` and ``fuse_llama_layers(model)`` apply as they do to Llama (both norms become ``RMSNormQuant``, q / k / v one GEMM,
gate / up / down a ``GatedMLP``); ``fuse_llama_layers(fuse_residual=True)`` refuses these layers, because K1a adds an unscaled sublayer output.
``fuse_granite_residual(model)`` (opt-in, an entry of its own, run after those two) takes each scaled add into the norm + quantisation that follows it
(``scaled_add_rmsnorm_quantize``, kernel K1ma; ``scaled_add``, K1mo, at the end of a chain): see ``ScaledResidualFusedLayer``.  The product is rounded to the
storage dtype before the add (QSPEC S1), as the eager expression rounds it, so the fused model holds the bits of the unfused one.

Out of scope: ``embedding_multiplier``, ``attention_multiplier`` and ``logits_scaling`` stay the model's own code; GraniteMoe / GraniteMoeShared / GraniteMoeHybrid
layers (their post-attention norm feeds a float router, so it is no ``RMSNormQuant``, and they have no ``mlp`` child: the entry returns 0 for them and touches
nothing); ``shard_llama_layers``."""
from __future__ import annotations

import math

from torch import nn

from .llama import _CHILDREN, RMSNormQuant
from .qtensor import scaled_add, scaled_add_rmsnorm_quantize
from .residual_flow import FusedLayer, NamedFusedLayer, _forward_extra_params, _hooked, fuse_stacks, probe_named_flow

_PROBE_MULTIPLIERS = (0.5, 4.0)          # powers of two: every operation of the probe stays exact on its small integers


def _scaled_flow(m: float):
    def want(x):
        r1 = x + (x * 2.0 + 1.0) * m
        return r1 + ((r1 * 0.5 - 3.0) ** 2) * m
    return want


class _WithMultiplier:
    """`layer` as the probe's stand-in reads it, with a planted residual_multiplier"""

    def __init__(self, layer: nn.Module, m: float):
        self.__dict__["_layer"], self.__dict__["residual_multiplier"] = layer, m

    def __getattr__(self, name):
        return getattr(self.__dict__["_layer"], name)


def _is_multiplier(m) -> bool:
    return isinstance(m, (int, float)) and not isinstance(m, bool) and math.isfinite(m)


def residual_flow_is_scaled(layer: nn.Module, cls=None) -> bool:
    """True iff `cls.forward` (default: the layer's own class) IS the scaled-residual data flow on this layer, with m = self.residual_multiplier:

        r1 = x + self_attn(hidden_states=input_layernorm(x), **kwargs)[0] * m;   out = r1 + mlp(post_attention_layernorm(r1)) * m

    with each of the four children called once, every keyword argument of the layer handed to the attention unchanged, no other submodule touched and a tensor
    returned.  Probed like llama.residual_flow_is_llama, at TWO stand-in multipliers (0.5 and 4: exact on the probe's small integers), each planted as the stand-in's
    `residual_multiplier`: a forward that ignores the attribute (Llama), scales the residual instead of the sublayer output, or scales only one of the two adds
    computes something else at one of them and is refused; `m * h` and `h * m` both pass.  The layer's real `residual_multiplier` must be a finite Python int or
    float (a tensor, a bool, NaN or an infinity is refused: the kernel takes it as an argument).  transformers' GraniteDecoderLayer passes at any multiplier, 1.0
    included; a layer without the attribute does not."""
    if not _is_multiplier(getattr(layer, "residual_multiplier", None)):
        return False
    cls = cls or type(layer)
    return all(probe_named_flow(_WithMultiplier(layer, m), cls, _CHILDREN, _scaled_flow(m), attn_positional=True) for m in _PROBE_MULTIPLIERS)


class ScaledResidualFusedLayer(NamedFusedLayer):
    """A scaled-residual decoder layer (Granite) whose two residual adds, with their multiplies, run inside the RMSNorm + quantisation kernels that follow them (K1ma,
    scaled_add_rmsnorm_quantize; K1mo, scaled_add, at the end of a chain):

        h          = the QTensor handed over for this very tensor, else input_layernorm(hidden)
        attn_out   = self_attn(hidden_states=h, **kwargs)[0]
        m          = self.residual_multiplier                                      # read at every call
        hq, resid  = scaled_add_rmsnorm_quantize(attn_out, hidden, m, pan.weight, pan.eps)            # pan = post_attention_layernorm: multiply + add + norm + quant
        y          = mlp(hq)
        last of the chain:  return scaled_add(y, resid, m)                         # multiply + add, one launch
        otherwise:          hq2, out = scaled_add_rmsnorm_quantize(y, resid, m, nin.weight, nin.eps)  # nin = the NEXT layer's input_layernorm; m is THIS layer's:
                            hand hq2 to the next layer;  return out                #   each add uses the multiplier of the layer whose add it is

    What the layer returns is the real summed tensor (the bits of the eager multiply and add: QSPEC S1, A1), so hooks on the layer, output_hidden_states and the final
    norm see what they saw.  The kernels read the weight and eps of post_attention_layernorm and of the next layer's input_layernorm; those modules stay the model's,
    object for object, but are no longer CALLED for these adds, which is why fuse_granite_residual refuses a layer whose norms carry hooks.
    fuse_granite_residual makes a layer one by giving the layer object a class that derives from this one AND from its original class: the object, its four
    children under their names (state_dict keys), its other attributes, its hooks and every isinstance check on it stay as they were.  The tensor the layer was
    called with is never written; the hand-over is consumed at the next layer's entry and never served for another tensor or a tensor changed in place since."""
    _pq_prefix, _pq_residual_fused = "ScaledResidualFused", True

    def forward(self, hidden_states, *args, **kwargs):
        if args:
            self._fold_positional(args, kwargs)
        h = self._rf_inbox.take(hidden_states)
        if h is None:
            h = self.input_layernorm(hidden_states)
        attn_out = self.self_attn(hidden_states=h, **kwargs)[0]
        m, pan = self.residual_multiplier, self.post_attention_layernorm
        hq, resid = scaled_add_rmsnorm_quantize(attn_out, hidden_states, m, pan.weight, pan.variance_epsilon)
        y = self.mlp(hq)
        nxt = self._rf_next[0]
        if nxt is None:
            return scaled_add(y, resid, m)
        nin = nxt.input_layernorm
        hq2, out = scaled_add_rmsnorm_quantize(y, resid, m, nin.weight, nin.variance_epsilon)
        nxt._rf_inbox.put(out, hq2)
        return out


def fuse_granite_residual(model: nn.Module) -> int:
    """Opt-in, after swap_linears(model, fuse_gated_mlp=True) and fuse_llama_layers(model): every layer of a ModuleList that has the four children input_layernorm,
    self_attn, post_attention_layernorm and mlp, whose two norms are RMSNormQuant without forward hooks or pre-hooks, and whose class's forward passes
    residual_flow_is_scaled becomes a ScaledResidualFusedLayer (in place).  Returns the number of layers converted by THIS call; llama.residual_fused_layers(model)
    counts them over all calls.  A refused layer keeps what it had and breaks the chain: its predecessor ends with K1mo.  A layer without a residual_multiplier (Llama,
    Mistral, Qwen) is refused here — fuse_llama_layers(fuse_residual=True) is its switch — as are GraniteMoe layers (no `mlp` child, a float norm in front of the
    router), Gemma-2, OLMo-2 and Phi-3.  The module that owns the ModuleList gets an always-called forward hook that drops every pending hand-over when its forward ends.

    Per forward of an L-layer stack the norm and add work is then 1 K1n, 2L - 1 K1ma and 1 K1mo launches and no torch multiply or add inside the layers, where the
    fuse_llama_layers model runs 2L multiplies, 2L adds and 2L K1n.  Out of scope: embedding_multiplier, attention_multiplier and logits_scaling (the model's own
    code), the GraniteMoe families, shard_llama_layers."""
    def convert(layer):
        if isinstance(layer, FusedLayer) or not all(hasattr(layer, c) for c in _CHILDREN):
            return None
        norms = (layer.input_layernorm, layer.post_attention_layernorm)
        if not all(isinstance(n, RMSNormQuant) and not _hooked(n) for n in norms):
            return None
        cls = type(layer)
        if not residual_flow_is_scaled(layer, cls):
            return None
        layer._rf_argnames = _forward_extra_params(cls)[0]
        return cls
    return fuse_stacks(model, ScaledResidualFusedLayer, convert)          # (a chain that ends, ends with K1mo)
