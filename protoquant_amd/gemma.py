"""Call-site integration for the Gemma family (transformers' Gemma, Gemma-2 and Gemma-3 text decoders):

* a Gemma RMSNorm — ``((x.float() * rsqrt(mean(x²) + eps)) * (1.0 + weight.float())).type_as(x)``: the gain is ``1 + w``, everything is binary32 and there is one
  storage rounding — whose output only feeds int8 projections becomes ``GemmaRMSNormQuant`` (``gemma_rmsnorm_quantize``, kernel K1ng).  In Gemma these are
  ``input_layernorm`` and ``post_attention_layernorm``; in Gemma-2 and Gemma-3 ``input_layernorm`` and ``pre_feedforward_layernorm`` — their two post-norms feed the
  residual add and stay the model's modules;
* q / k / v share one quantisation and one GEMM launch, as ``fuse_llama_layers`` does it (its code runs);
* the GeGLU MLP, ``down(gelu_tanh(gate(x)) * up(x))``, becomes ``GatedMLP(act="gelu_tanh")``: a fused gate+up GEMM and ``gelu_mul_quantize`` (kernel K1gg);
* ``fuse_residual=True`` (opt-in): a layer whose forward is the Llama data flow — Gemma v1 — gets its two residual adds taken into the norms that follow them
  (``add_gemma_rmsnorm_quantize``, kernel K1ang), through ``llama.ResidualFusedLayer``.  Gemma-2 and Gemma-3 normalise the sublayer output BEFORE the add: refused
  by that switch;
* ``fuse_gemma_postnorm_residual(model)`` (opt-in, an entry of its own, after ``fuse_gemma_layers``): a layer whose forward is the sandwich data flow — Gemma-2 and
  Gemma-3, ``r1 = x + post_attention_layernorm(self_attn(input_layernorm(x)))``, ``out = r1 + post_feedforward_layernorm(mlp(pre_feedforward_layernorm(r1)))`` —
  becomes a ``SandwichFusedLayer``: each post-norm, the add behind it and the norm + quantisation that follows run in ONE kernel
  (``gemma_postnorm_add_rmsnorm_quantize``, K1pang; ``gemma_postnorm_add``, K1pa, at the end of a chain).  The post-norms become the specified norm (QSPEC PN1:
  NG1-NG5, spec-exact and eager-close) instead of the eager chain, so the switch changes bits against the model without it; no eager GemmaRMSNorm is left inside
  such a layer.

``swap_linears(model)`` must have run first.  Nothing is recognised by class name: a norm is probed (``is_gemma_rmsnorm`` runs its class's forward against the
formula), its use is probed (``gptlike.fusable_norms``), the activation is probed (``gptlike.activation_kind``), the MLP's forward is probed.  The embedding
scaling, the attention softcapping, the sliding windows, ``q_norm`` / ``k_norm`` and the final norm stay the model's code (Gemma-3's per-head ``q_norm`` / ``k_norm`` are taken by
``qk_norm.fuse_qk_norms``, an entry of its own, called last)."""
from __future__ import annotations

import types

import torch
from torch import nn

from .gptlike import activation_kind, fusable_norms
from .llama import RMSNormQuant, _FusedSlice, _fuse_residual, fuse_llama_layers
from .qlinear import FusedQLinear, GatedMLP, qlinear
from .qtensor import add_gemma_rmsnorm_quantize, gemma_postnorm_add, gemma_postnorm_add_rmsnorm_quantize, gemma_rmsnorm_quantize
from .residual_flow import NamedFusedLayer, _forward_extra_params, _hooked, _ProbeLayer, attention, fuse_stacks, probe_named_flow


class GemmaRMSNormQuant(RMSNormQuant):
    """A Gemma RMSNorm whose output is the per-token int8 quantisation of the normalised activation (QSPEC NG1-NG6 then Q1-Q6).  Holds the module's STORED weight w
    (state-dict compatible), not 1 + w: the kernel forms the gain.  An RMSNormQuant to everything that handles one (llama.ResidualFusedLayer calls it with
    `residual`); eps lives under the Gemma norms' own name, `eps`, so the Llama recogniser — which looks for `variance_epsilon` — never takes it for a Llama norm."""

    def __init__(self, weight: torch.Tensor, eps: float):
        super().__init__(weight, eps)
        del self.variance_epsilon
        self.eps = float(eps)

    def forward(self, x: torch.Tensor, residual: torch.Tensor | None = None):
        """Without `residual`: the QTensor of GemmaRMSNorm(x).  With it: (QTensor of GemmaRMSNorm(residual + x), residual + x) from one kernel (K1ang) — the bits
        of the torch add followed by the call without `residual`."""
        if residual is None:
            return gemma_rmsnorm_quantize(x, self.weight, self.eps)
        return add_gemma_rmsnorm_quantize(x, residual, self.weight, self.eps)

    def extra_repr(self):
        return f"{tuple(self.weight.shape)}, eps={self.eps}, gain 1 + w -> int8 per-token QTensor"


class GemmaSandwichNormQuant(GemmaRMSNormQuant):
    """The GemmaRMSNormQuant of a sandwich-fused layer (fuse_gemma_postnorm_residual gives the two norm objects this class; nothing else about them changes): its
    forward also takes the post-norm that precedes the residual add.  A class of its own because GemmaRMSNormQuant.forward(x, residual=None) is a held signature."""

    def forward(self, x: torch.Tensor, residual: torch.Tensor | None = None, post_norm=None):
        """Without `post_norm`: GemmaRMSNormQuant.forward.  With `residual` and `post_norm` (a Gemma norm module: only its `weight` and `eps` are read, it is not
        called): summed = residual + post_norm(x) by the specified norm (QSPEC PN1), and (QTensor of GemmaRMSNorm(summed), summed) from one kernel (K1pang)."""
        if post_norm is None:
            return super().forward(x, residual)
        if residual is None:
            raise ValueError("GemmaSandwichNormQuant: post_norm needs the residual its output is added to")
        return gemma_postnorm_add_rmsnorm_quantize(x, post_norm.weight, residual, self.weight, self.eps, post_norm.eps)


# ---------------------------------------------------------------- is it a Gemma norm?  (by behaviour)
class _NormStandin:
    """Stand-in for `self` in a norm class's own forward: a seeded weight, the real eps, the class's other attributes (methods bound to the stand-in)."""

    def __init__(self, cls, weight, eps):
        self.__dict__.update(_cls=cls, weight=weight, eps=eps)

    def __getattr__(self, name):
        v = getattr(self.__dict__["_cls"], name)
        return types.MethodType(v, self) if isinstance(v, types.FunctionType) else v


def _gemma_formula(x, w, eps):
    xf = x.float()
    return ((xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)) * (1.0 + w.float())).type_as(x)


def _llama_formula(x, w, eps):
    xf = x.float()
    return w * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).to(x.dtype)


def is_gemma_rmsnorm(m) -> bool:
    """True iff `m` computes the Gemma RMSNorm: a module with a 1-D `weight`, a float `eps` and no other parameter or buffer, whose class's forward — run on a
    stand-in with a seeded non-trivial weight, on a small CPU tensor in bf16 and in f32 — returns exactly ((x.float() * rsqrt(mean(x²) + eps)) * (1.0 +
    w.float())).type_as(x).  The Llama formula (gain w, two roundings) evaluated on the same operands must differ, so the operands tell the two apart: LlamaRMSNorm,
    nn.LayerNorm and a subclass with another forward are refused."""
    if not isinstance(m, nn.Module) or isinstance(m, RMSNormQuant):
        return False
    w, eps = getattr(m, "weight", None), getattr(m, "eps", None)
    if not isinstance(w, torch.Tensor) or w.dim() != 1 or w.shape[0] < 1 or not isinstance(eps, float) or not eps >= 0.0:
        return False
    if [n for n, _ in m.named_parameters()] + [n for n, _ in m.named_buffers()] != ["weight"] or any(True for _ in m.children()):
        return False
    g = torch.Generator().manual_seed(20240221)
    xs = torch.randn(3, 5, w.shape[0], generator=g) * torch.tensor([0.05, 1.0, 20.0]).reshape(3, 1, 1)
    ws = 0.3 * torch.randn(w.shape[0], generator=g)
    try:
        for dt in (torch.bfloat16, torch.float32):
            x, wt = xs.to(dt), ws.to(dt)
            with torch.no_grad():
                got = type(m).forward(_NormStandin(type(m), wt, eps), x.clone())
            want = _gemma_formula(x, wt, eps)
            if not isinstance(got, torch.Tensor) or got.dtype != want.dtype or got.shape != want.shape or not torch.equal(got, want):
                return False
            if torch.equal(_llama_formula(x, wt, eps), want):
                return False
    except Exception:          # noqa: BLE001  (whatever the forward raises on the stand-in: refused)
        return False
    return True


# ---------------------------------------------------------------- is it a GeGLU MLP?  (by behaviour)
def _mlp_flow_is_gated(mlp: nn.Module) -> bool:
    """True iff type(mlp).forward IS down_proj(act_fn(gate_proj(x)) * up_proj(x)), each child called once: probed with exact functions on small integers in the
    children's places (any other submodule is a refusal, every other attribute is the real module's), not pattern-matched."""
    calls = {"gate_proj": 0, "up_proj": 0, "down_proj": 0, "act_fn": 0}

    def counted(name, f):
        def run(t):
            calls[name] += 1
            return f(t)
        return run

    kids = {"gate_proj": counted("gate_proj", lambda t: t * 2.0), "up_proj": counted("up_proj", lambda t: t + 1.0),
            "down_proj": counted("down_proj", lambda t: t - 3.0), "act_fn": counted("act_fn", lambda t: t * t)}
    x = torch.arange(-6, 6, dtype=torch.float32).reshape(1, 3, 4)
    try:
        with torch.no_grad():
            out = type(mlp).forward(_ProbeLayer(mlp, kids), x.clone())
    except Exception:          # noqa: BLE001
        return False
    want = (x * 2.0) ** 2 * (x + 1.0) - 3.0
    return isinstance(out, torch.Tensor) and all(n == 1 for n in calls.values()) and out.shape == want.shape and torch.equal(out, want)


def _as_geglu(mlp: nn.Module):
    """GatedMLP(act="gelu_tanh") for a module whose gate_proj / up_proj / down_proj are qlinear, whose act_fn is the tanh GELU and whose forward is the gated
    flow; None for anything else"""
    g, u, d = (getattr(mlp, n, None) for n in ("gate_proj", "up_proj", "down_proj"))
    if not all(isinstance(p, qlinear) for p in (g, u, d)) or activation_kind(getattr(mlp, "act_fn", None)) != "gelu_tanh":
        return None
    if g.in_features != u.in_features or g.out_features != u.out_features or d.in_features != g.out_features or (g.bias is None) != (u.bias is None):
        return None
    if not _mlp_flow_is_gated(mlp):
        return None
    return GatedMLP(FusedQLinear([g, u]), d, act="gelu_tanh")


def _is_gemma_norm_or_fused(m) -> bool:
    return isinstance(m, GemmaRMSNormQuant) or is_gemma_rmsnorm(m)


def fuse_gemma_layers(model: nn.Module, fuse_norms: bool = True, fuse_qkv: bool = True, fuse_mlp: bool = True, fuse_residual: bool = False) -> int:
    """Apply the fusions above to every Gemma-family decoder layer found in `model` (in place), after swap_linears(model); returns the number of layers changed.
    A layer is a module with self_attn, mlp, input_layernorm and post_attention_layernorm whose input_layernorm is a Gemma norm (is_gemma_rmsnorm): a Llama model
    is left exactly as it was.  Per layer, in this order:

    * norms (fuse_norms): every Gemma norm child that gptlike.fusable_norms accepts — the layer's own forward, probed, uses its output only as the input of int8
      projections — becomes GemmaRMSNormQuant.  The probe runs before the MLP is replaced, on its qlinear projections; a norm whose consumers are not int8
      (fuse_mlp with projections that were not swapped) is refused and stays the model's module, object for object;
    * q / k / v (fuse_qkv): fuse_llama_layers' fusion, by its code;
    * MLP (fuse_mlp): gate_proj / up_proj / down_proj all qlinear, activation_kind(act_fn) == "gelu_tanh" and the gated forward -> GatedMLP(act="gelu_tanh").
      With fuse_mlp=False the model's MLP keeps running on the swapped projections (torch's gelu and mul, then K1) — the choice for decode batches of a few rows
      if K1gg measures slower there (README).

    fuse_residual=True (opt-in): afterwards llama's residual fusion runs on the layers recognised here (and no others) — every one whose two norms are GemmaRMSNormQuant and whose forward passes
    llama.residual_flow_is_llama becomes a ResidualFusedLayer, with K1ang in K1a's place.  That is Gemma v1; Gemma-2 and Gemma-3 layers are refused and run as
    before.  llama.residual_fused_layers(model) counts them."""
    n, mine = 0, set()
    for layer in list(model.modules()):
        attn, mlp = getattr(layer, "self_attn", None), getattr(layer, "mlp", None)
        if attn is None or mlp is None or not hasattr(layer, "input_layernorm") or not hasattr(layer, "post_attention_layernorm"):
            continue
        if not _is_gemma_norm_or_fused(layer.input_layernorm):
            continue
        mine.add(id(layer))
        did = False
        if fuse_norms:
            for name in fusable_norms(layer, candidate=is_gemma_rmsnorm):
                old = getattr(layer, name)
                setattr(layer, name, GemmaRMSNormQuant(old.weight, old.eps))
                did = True
        if fuse_qkv:
            unfused = isinstance(getattr(attn, "q_proj", None), qlinear)
            fuse_llama_layers(layer, fuse_norms=False, fuse_qkv=True)          # (norms untouched; q / k / v that are not three qlinears are left alone)
            did = did or (unfused and isinstance(attn.q_proj, _FusedSlice))
        if fuse_mlp:
            fused = _as_geglu(mlp)
            if fused is not None:
                layer.mlp = fused
                did = True
        n += int(did)
    if fuse_residual:
        _fuse_residual(model, only=mine)          # the layers recognised above and no others: a Llama layer that fuse_llama_layers prepared is not this call's to change
    return n


# ---------------------------------------------------------------- the sandwich residual flow of Gemma-2 / Gemma-3 (opt-in)
_SANDWICH = {"input_layernorm": lambda t: t * 2.0, "self_attn": attention(lambda h: h + 1.0), "post_attention_layernorm": lambda t: t * 3.0 - 1.0,
             "pre_feedforward_layernorm": lambda t: t * 0.5 - 3.0, "mlp": lambda t: t * t, "post_feedforward_layernorm": lambda t: t * 4.0 + 5.0}


def _sandwich_flow(x):
    r1 = x + ((x * 2.0 + 1.0) * 3.0 - 1.0)
    return r1 + ((r1 * 0.5 - 3.0) ** 2 * 4.0 + 5.0)


def residual_flow_is_sandwich(layer: nn.Module, cls=None) -> bool:
    """True iff `cls.forward` (default: the layer's own class) IS the sandwich data flow on this layer:

        r1  = x  + post_attention_layernorm(self_attn(hidden_states=input_layernorm(x), **kwargs)[0])
        out = r1 + post_feedforward_layernorm(mlp(pre_feedforward_layernorm(r1)))

    with each of the six children called once, the attention given its input as `hidden_states=` (the form the fused layer calls it in; a positional hidden state is
    refused), every keyword argument of the layer handed to it unchanged, no other submodule touched and a tensor
    returned.  Probed like llama.residual_flow_is_llama, not pattern-matched: the class's forward runs on a stand-in whose children are cheap exact functions on a
    tiny CPU tensor, and its result must EQUAL the formula.  transformers' Gemma2DecoderLayer and Gemma3DecoderLayer pass; Gemma v1 and Llama (no post-norms),
    OLMo-2 (post-norms only), Gemma-3n (further submodules) and any forward that raises on the stand-in do not."""
    return probe_named_flow(layer, cls or type(layer), _SANDWICH, _sandwich_flow)


class SandwichFusedLayer(NamedFusedLayer):
    """A sandwich-flow decoder layer (Gemma-2, Gemma-3) whose two post-norms and residual adds run inside the norm + quantisation kernels that follow them (K1pang,
    gemma_postnorm_add_rmsnorm_quantize; K1pa, gemma_postnorm_add, at the end of a chain):

        h        = the QTensor handed over for this very tensor, else input_layernorm(hidden)
        a        = self_attn(hidden_states=h, **kwargs)[0]
        hq, r1   = pre_feedforward_layernorm(a, residual=hidden, post_norm=post_attention_layernorm)       # post-norm + add + norm + quant, one launch
        m        = mlp(hq)
        last of the chain:  return gemma_postnorm_add(m, pfn.weight, r1, pfn.eps)                          # post-norm + add, one launch; pfn = post_feedforward_layernorm
        otherwise:          hq2, out = NEXT layer's input_layernorm(m, residual=r1, post_norm=pfn);  hand hq2 to the next layer;  return out

    What the layer returns is the real summed tensor, so hooks, output_hidden_states and the final norm see a residual stream.  The two post-norm modules stay the
    model's modules, object for object (state-dict keys unchanged); they are no longer CALLED — only their `weight` and `eps` are read, and the norm is the specified
    one (QSPEC PN1) instead of the eager chain.  fuse_gemma_postnorm_residual makes a layer one by giving the layer object a class that derives from this one AND
    from its original class: the object, its children under their names, its other attributes, its hooks and every isinstance check on it stay as they were.  The
    tensor the layer was called with is never written; the hand-over is consumed at the next layer's entry and never served for another tensor or a tensor changed in
    place since."""
    _pq_prefix, _pq_residual_fused = "SandwichFused", True

    def forward(self, hidden_states, *args, **kwargs):
        if args:
            self._fold_positional(args, kwargs)
        h = self._rf_inbox.take(hidden_states)
        if h is None:
            h = self.input_layernorm(hidden_states)
        attn_out = self.self_attn(hidden_states=h, **kwargs)[0]
        hq, r1 = self.pre_feedforward_layernorm(attn_out, residual=hidden_states, post_norm=self.post_attention_layernorm)
        m = self.mlp(hq)
        pfn = self.post_feedforward_layernorm
        nxt = self._rf_next[0]
        if nxt is None:
            return gemma_postnorm_add(m, pfn.weight, r1, pfn.eps)
        hq2, out = nxt.input_layernorm(m, residual=r1, post_norm=pfn)
        nxt._rf_inbox.put(out, hq2)
        return out


def fuse_gemma_postnorm_residual(model: nn.Module) -> int:
    """Opt-in, after fuse_gemma_layers(model) (which it leaves exactly as it was: a separate entry, so nothing changes for a caller who does not ask): every layer
    of a ModuleList becomes a SandwichFusedLayer (in place) if ALL of these hold — it has the six children input_layernorm, self_attn, post_attention_layernorm,
    pre_feedforward_layernorm, mlp and post_feedforward_layernorm; input_layernorm and pre_feedforward_layernorm are GemmaRMSNormQuant (the two objects become
    GemmaSandwichNormQuant, whose forward also takes the post-norm; weight, eps and state-dict keys stay); both post-norms pass
    is_gemma_rmsnorm and are as wide as those; neither post-norm has a forward hook or pre-hook registered (the post-norm MODULE is no longer called — the kernel
    reads its weight and eps — so a hook on it would silently stop firing: such a layer is refused); and the class's forward passes residual_flow_is_sandwich.
    A refused layer keeps everything it had and breaks the chain: its predecessor ends with K1pa.  The post-norms become the specified norm (QSPEC PN1) instead of
    the eager chain, so the model's bits change against the model without this switch.  The module that owns the ModuleList gets an always-called forward hook that
    drops every pending hand-over when its forward ends.  Returns the number of layers changed by THIS call (a second call finds nothing left to change and returns
    0); llama.residual_fused_layers(model) counts them over all calls."""
    def convert(layer):
        if isinstance(layer, SandwichFusedLayer) or not all(hasattr(layer, c) for c in _SANDWICH):
            return None
        n1, n2 = layer.input_layernorm, layer.pre_feedforward_layernorm
        if not (isinstance(n1, GemmaRMSNormQuant) and isinstance(n2, GemmaRMSNormQuant)) or n1.weight.shape != n2.weight.shape:
            return None
        posts = (layer.post_attention_layernorm, layer.post_feedforward_layernorm)
        if not all(is_gemma_rmsnorm(p) and p.weight.shape == n1.weight.shape and not _hooked(p) for p in posts):
            return None
        cls = type(layer)
        if not residual_flow_is_sandwich(layer, cls):
            return None
        n1.__class__ = n2.__class__ = GemmaSandwichNormQuant          # (the same objects: they learn the post_norm argument)
        layer._rf_argnames = _forward_extra_params(cls)[0]
        return cls
    return fuse_stacks(model, SandwichFusedLayer, convert)          # (a chain that ends, ends with K1pa)
