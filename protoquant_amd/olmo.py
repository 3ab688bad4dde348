"""Call-site integration for the post-norm decoders (transformers' OLMo-2 and OLMo-3): a layer has NO input norm — it normalises the OUTPUT of each sublayer,

    r1  = x  + post_attention_layernorm(self_attn(x))
    out = r1 + post_feedforward_layernorm(mlp(r1))

and its attention normalises the whole of q and of k (``q_norm(q_proj(x))``, ``k_norm(k_proj(x))``).  The norm is ``(weight * (x.float() * rsqrt(mean(x.float()²) +
eps))).to(x.dtype)``: binary32 throughout, ONE storage rounding, gain ``w`` — neither the Llama norm (two roundings) nor the Gemma norm (gain ``1 + w``).

``fuse_olmo_layers(model)`` after ``swap_linears(model, fuse_gated_mlp=True)``:

* q / k / v share one activation quantisation and one GEMM launch, by ``fuse_llama_layers``' machinery (its classes and hooks); ``q_norm`` / ``k_norm`` then receive
  column slices of the fused output and stay the model's modules.  Nothing else changes: the model's bits are those of the ``swap_linears`` model;
* ``fuse_residual=True`` (opt-in): a layer becomes a ``PostNormFusedLayer`` — each post-norm, the residual add behind it and the quantisation of the next sublayer's
  input run in ONE kernel (``olmo_postnorm_add_quantize``, K1oq; ``olmo_postnorm_add``, K1oa, at the end of a chain), and ``q_norm`` / ``k_norm`` become
  ``OlmoRMSNorm`` (``olmo_rmsnorm``, K1on).  The norms become the specified norm (QSPEC NO1-NO5: spec-exact and eager-close) instead of the eager chain, so the
  switch changes bits against the model without it.

Nothing is recognised by class name or by import: a norm is probed (``is_olmo_rmsnorm`` runs its class's forward against the formula), the layer's forward is probed
(``residual_flow_is_postnorm``).  Out of scope: ``shard_llama_layers`` (its layers have an input norm), the final norm, the rotary embedding, and FlexOlmo (a
mixture-of-experts MLP)."""
from __future__ import annotations

import torch
from torch import nn

from .gemma import _NormStandin, _gemma_formula, _llama_formula
from .llama import _FusedSlice, _SharedFused, _install_qkv_hooks
from .qlinear import FusedQLinear, GatedMLP, qlinear
from .qtensor import olmo_postnorm_add, olmo_postnorm_add_quantize, olmo_rmsnorm, quantize
from .residual_flow import NamedFusedLayer, _forward_extra_params, _hooked, attention, fuse_stacks, probe_named_flow


class OlmoRMSNorm(nn.Module):
    """An OLMo RMSNorm by the specified norm (QSPEC NO1-NO5; kernel K1on): what q_norm / k_norm of a post-norm-fused layer become.  Holds the module's own weight
    OBJECT (not a copy: state-dict key and storage unchanged) and its eps under the name it had, `variance_epsilon`."""

    def __init__(self, weight: torch.Tensor, eps: float):
        super().__init__()
        self.weight = weight if isinstance(weight, nn.Parameter) else nn.Parameter(weight, requires_grad=False)
        self.variance_epsilon = float(eps)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return olmo_rmsnorm(x, self.weight, self.variance_epsilon)

    def extra_repr(self):
        return f"{tuple(self.weight.shape)}, eps={self.variance_epsilon}, one launch"


# ---------------------------------------------------------------- is it an OLMo norm?  (by behaviour)
def _olmo_formula(x, w, eps):
    xf = x.float()
    return (w * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps))).to(x.dtype)


def _norm_eps(m):
    """(attribute name, value) of a norm's eps — `variance_epsilon` (OLMo, Llama, T5) or `eps` — or (None, None)"""
    for name in ("variance_epsilon", "eps"):
        v = getattr(m, name, None)
        if isinstance(v, float) and v >= 0.0:
            return name, v
    return None, None


def is_olmo_rmsnorm(m) -> bool:
    """True iff `m` computes the OLMo RMSNorm: a module with a 1-D `weight`, a float `variance_epsilon` or `eps` and no other parameter, buffer or child, whose class's
    forward — run on a stand-in with a seeded non-trivial weight, on a small CPU tensor in bf16 and in f32 — returns exactly (w * (x.float() * rsqrt(mean(x²) +
    eps))).to(x.dtype).  On the bf16 operands the Llama formula (two roundings) and the Gemma formula (gain 1 + w) must both differ, so the operands tell the three
    apart; in f32 the Llama formula coincides by construction and only Gemma's is told apart.  Olmo2RMSNorm and Olmo3RMSNorm pass; LlamaRMSNorm, T5LayerNorm,
    GemmaRMSNorm, nn.LayerNorm and a subclass with another forward are refused."""
    if not isinstance(m, nn.Module) or isinstance(m, OlmoRMSNorm):
        return False
    w = getattr(m, "weight", None)
    eps_name, eps = _norm_eps(m)
    if not isinstance(w, torch.Tensor) or w.dim() != 1 or w.shape[0] < 1 or eps_name is None:
        return False
    if [n for n, _ in m.named_parameters()] + [n for n, _ in m.named_buffers()] != ["weight"] or any(True for _ in m.children()):
        return False
    g = torch.Generator().manual_seed(20240221)
    xs = torch.randn(3, 5, w.shape[0], generator=g) * torch.tensor([0.05, 1.0, 20.0]).reshape(3, 1, 1)
    ws = 0.3 * torch.randn(w.shape[0], generator=g)
    try:
        for dt in (torch.bfloat16, torch.float32):
            x, wt = xs.to(dt), ws.to(dt)
            standin = _NormStandin(type(m), wt, eps)
            standin.__dict__[eps_name] = eps
            with torch.no_grad():
                got = type(m).forward(standin, x.clone())
            want = _olmo_formula(x, wt, eps)
            if not isinstance(got, torch.Tensor) or got.dtype != want.dtype or got.shape != want.shape or not torch.equal(got, want):
                return False
            if torch.equal(_gemma_formula(x, wt, eps), want) or (dt == torch.bfloat16 and torch.equal(_llama_formula(x, wt, eps), want)):
                return False
    except Exception:          # noqa: BLE001  (whatever the forward raises on the stand-in: refused)
        return False
    return True


# ---------------------------------------------------------------- is it the post-norm data flow?  (by behaviour)
# (the attention is 2 h + 1, not the h + 1 of the flows that have an input norm: it is what tells a missing input norm apart)
_POSTNORM = {"self_attn": attention(lambda h: h * 2.0 + 1.0), "post_attention_layernorm": lambda t: t * 3.0 - 1.0, "mlp": lambda t: t * t,
             "post_feedforward_layernorm": lambda t: t * 4.0 + 5.0}


def _postnorm_flow(x):
    r1 = x + ((x * 2.0 + 1.0) * 3.0 - 1.0)
    return r1 + ((r1 * r1) * 4.0 + 5.0)


def residual_flow_is_postnorm(layer: nn.Module, cls=None) -> bool:
    """True iff `cls.forward` (default: the layer's own class) IS the post-norm data flow on this layer:

        r1  = x  + post_attention_layernorm(self_attn(hidden_states=x, **kwargs)[0])
        out = r1 + post_feedforward_layernorm(mlp(r1))

    with each of the four children called once, the attention given its input as `hidden_states=` (the form the fused layer calls it in; a positional hidden state is
    refused), every keyword argument of the layer handed to it unchanged, no other submodule touched and a tensor returned.  Probed like
    gemma.residual_flow_is_sandwich, not pattern-matched: the class's forward runs on a stand-in whose children are cheap exact functions on a tiny CPU tensor, and
    its result must EQUAL the formula.  transformers' Olmo2DecoderLayer and Olmo3DecoderLayer pass; Llama, Gemma-2 and Granite (an input norm: another submodule), a
    layer with a scaled sum, a layer that calls a dropout child and any forward that raises on the stand-in do not."""
    return probe_named_flow(layer, cls or type(layer), _POSTNORM, _postnorm_flow)


class PostNormFusedLayer(NamedFusedLayer):
    """A post-norm decoder layer (OLMo-2, OLMo-3) whose two post-norms and residual adds run inside the quantisation of the next sublayer's input (K1oq,
    olmo_postnorm_add_quantize; K1oa, olmo_postnorm_add, at the end of a chain):

        hq       = the QTensor handed over for this very tensor, else quantize(hidden)                                       # K1
        a        = self_attn(hidden_states=hq, **kwargs)[0]
        hq1, r1  = olmo_postnorm_add_quantize(a, post_attention_layernorm.weight, hidden, its eps)                         # post-norm + add + quant, one launch
        m        = mlp(hq1)
        last of the chain:  return olmo_postnorm_add(m, pfn.weight, r1, pfn.eps)                                           # pfn = post_feedforward_layernorm
        otherwise:          hq2, out = olmo_postnorm_add_quantize(m, pfn.weight, r1, pfn.eps);  hand hq2 to the next layer;  return out

    What the layer returns is the real summed tensor, so hooks, output_hidden_states and the final norm see a residual stream.  The two post-norm modules stay the
    model's modules, object for object (state-dict keys unchanged); they are no longer CALLED — only their `weight` and eps are read, and the norm is the specified
    one (QSPEC PO1) instead of the eager chain.  fuse_olmo_layers(fuse_residual=True) makes a layer one by giving the layer object a class that derives from this one
    AND from its original class: the object, its children under their names, its other attributes, its hooks and every isinstance check on it stay as they were.
    The tensor the layer was called with is never written; the hand-over is consumed at the next layer's entry and never served for another tensor or a tensor
    changed in place since."""
    _pq_prefix, _pq_residual_fused = "PostNormFused", True

    def forward(self, hidden_states, *args, **kwargs):
        if args:
            self._fold_positional(args, kwargs)
        hq = self._rf_inbox.take(hidden_states)
        if hq is None:
            hq = quantize(hidden_states, axis=-1)
        attn_out = self.self_attn(hidden_states=hq, **kwargs)[0]
        pan, pfn = self.post_attention_layernorm, self.post_feedforward_layernorm
        hq1, r1 = olmo_postnorm_add_quantize(attn_out, pan.weight, hidden_states, _norm_eps(pan)[1])
        m = self.mlp(hq1)
        nxt = self._rf_next[0]
        if nxt is None:
            return olmo_postnorm_add(m, pfn.weight, r1, _norm_eps(pfn)[1])
        hq2, out = olmo_postnorm_add_quantize(m, pfn.weight, r1, _norm_eps(pfn)[1])
        nxt._rf_inbox.put(out, hq2)
        return out


def _qkv_state(attn) -> str:
    """"plain": three qlinear projections; "fused": the three slices of one shared fused GEMM; "": anything else"""
    q, k, v = (getattr(attn, p, None) for p in ("q_proj", "k_proj", "v_proj"))
    if all(isinstance(p, qlinear) for p in (q, k, v)):
        return "plain"
    if all(isinstance(p, _FusedSlice) for p in (q, k, v)) and isinstance(getattr(attn, "qkv_fused", None), _SharedFused):
        return "fused"
    return ""


def fuse_olmo_layers(model: nn.Module, fuse_qkv: bool = True, fuse_residual: bool = False) -> int:
    """Apply the fusions above to every post-norm decoder layer found in `model` (in place), after swap_linears(model, fuse_gated_mlp=True); returns the number of
    layers changed by THIS call (a second call finds nothing left to change and returns 0).  A layer is a member of a ModuleList that has exactly the four children
    self_attn, post_attention_layernorm, mlp and post_feedforward_layernorm, whose q_proj / k_proj / v_proj are qlinear (or already this function's slices) and whose
    class's forward passes residual_flow_is_postnorm: a Llama, Gemma or Mixtral model is left exactly as it was.

    * fuse_qkv: q / k / v become the slices of one FusedQLinear (llama._SharedFused / _FusedSlice and its hooks): one activation quantisation and one GEMM launch for
      the three.  q_norm and k_norm then receive column slices of the fused output and stay the model's modules.  With fuse_residual=False nothing else changes, and
      the model's bits are those of the swap_linears model.
    * fuse_residual=True (opt-in: the norms become the specified norm in place of the eager chain, so bits change): a layer becomes a PostNormFusedLayer if ALL of
      these hold — both post-norms pass is_olmo_rmsnorm and are as wide as the hidden size; neither has a forward hook or pre-hook registered (the post-norm MODULE is
      no longer called — the kernel reads its weight and eps — so a hook on it would silently stop firing); the MLP is a GatedMLP.  Under the same switch a q_norm /
      k_norm of such a layer that passes is_olmo_rmsnorm and is unhooked becomes an OlmoRMSNorm around the same weight object (state-dict key unchanged; K1on).  A
      refused layer keeps what it had and breaks the chain: its predecessor ends with K1oa.  The module that owns the ModuleList gets an always-called forward hook
      that drops every pending hand-over when its forward ends; llama.residual_fused_layers(model) counts the fused layers over all calls.

    Per forward of an L-layer stack the norm and add work is then 1 K1, 2L - 1 K1oq, 1 K1oa and 2L K1on launches, where the swap_linears model runs 4L eager norm
    chains and 2L torch adds on top of its K1 launches.  Out of scope: shard_llama_layers, the final norm, the rotary embedding, FlexOlmo."""
    changed = []          # per recognised layer: did this call change it (q / k / v fused, made a PostNormFusedLayer, or both)?

    def convert(layer):
        if {name for name, _ in layer.named_children()} != set(_POSTNORM):
            return None
        attn = layer.self_attn
        state = _qkv_state(attn)
        if not state or not residual_flow_is_postnorm(layer, _original_class(layer)):
            return None
        cls, did = None, False
        if fuse_qkv and state == "plain":
            attn.qkv_fused = _SharedFused(FusedQLinear([attn.q_proj, attn.k_proj, attn.v_proj]))
            attn.q_proj, attn.k_proj, attn.v_proj = (_FusedSlice(attn.qkv_fused, i) for i in range(3))
            _install_qkv_hooks(attn)
            did = True
        if fuse_residual and not isinstance(layer, PostNormFusedLayer) and _residual_fusable(layer):
            for name in ("q_norm", "k_norm"):
                old = getattr(attn, name, None)
                if is_olmo_rmsnorm(old) and not _hooked(old):
                    setattr(attn, name, OlmoRMSNorm(old.weight, _norm_eps(old)[1]))
            cls = type(layer)
            layer._rf_argnames = _forward_extra_params(cls)[0]
            did = True
        changed.append(did)
        return cls
    fuse_stacks(model, PostNormFusedLayer, convert)          # (a chain that ends, ends with K1oa)
    return sum(changed)


def _original_class(layer):
    """the class whose forward is the model's own: a PostNormFusedLayer's second base"""
    cls = type(layer)
    return cls.__bases__[1] if isinstance(layer, PostNormFusedLayer) else cls


def _residual_fusable(layer) -> bool:
    mlp = layer.mlp
    if not isinstance(mlp, GatedMLP):
        return False
    hidden = mlp.down.out_features
    posts = (layer.post_attention_layernorm, layer.post_feedforward_layernorm)
    return all(is_olmo_rmsnorm(p) and p.weight.shape[0] == hidden and not _hooked(p) for p in posts)
