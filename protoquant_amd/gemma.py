"""Call-site integration for the Gemma family (transformers' Gemma, Gemma-2 and Gemma-3 text decoders):

* a Gemma RMSNorm — ``((x.float() * rsqrt(mean(x²) + eps)) * (1.0 + weight.float())).type_as(x)``: the gain is ``1 + w``, everything is binary32 and there is one
  storage rounding — whose output only feeds int8 projections becomes ``GemmaRMSNormQuant`` (``gemma_rmsnorm_quantize``, kernel K1ng).  In Gemma these are
  ``input_layernorm`` and ``post_attention_layernorm``; in Gemma-2 and Gemma-3 ``input_layernorm`` and ``pre_feedforward_layernorm`` — their two post-norms feed the
  residual add and stay the model's modules;
* q / k / v share one quantisation and one GEMM launch, as ``fuse_llama_layers`` does it (its code runs);
* the GeGLU MLP, ``down(gelu_tanh(gate(x)) * up(x))``, becomes ``GatedMLP(act="gelu_tanh")``: a fused gate+up GEMM and ``gelu_mul_quantize`` (kernel K1gg);
* ``fuse_residual=True`` (opt-in): a layer whose forward is the Llama data flow — Gemma v1 — gets its two residual adds taken into the norms that follow them
  (``add_gemma_rmsnorm_quantize``, kernel K1ang), through ``llama.ResidualFusedLayer``.  Gemma-2 and Gemma-3 normalise the sublayer output BEFORE the add: refused.

``swap_linears(model)`` must have run first.  Nothing is recognised by class name: a norm is probed (``is_gemma_rmsnorm`` runs its class's forward against the
formula), its use is probed (``gptlike.fusable_norms``), the activation is probed (``gptlike.activation_kind``), the MLP's forward is probed.  The embedding
scaling, the attention softcapping, the sliding windows, ``q_norm`` / ``k_norm`` and the final norm stay the model's code."""
from __future__ import annotations

import types

import torch
from torch import nn

from .gptlike import activation_kind, fusable_norms
from .llama import RMSNormQuant, _FusedSlice, _fuse_residual, fuse_llama_layers
from .qlinear import FusedQLinear, GatedMLP, qlinear
from .qtensor import add_gemma_rmsnorm_quantize, gemma_rmsnorm_quantize


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
class _MLPStandin:
    """Stand-in for `self` in an MLP class's own forward: the three projections and the activation are exact functions on small integers; any other submodule is
    a refusal; every other attribute is the real module's."""

    def __init__(self, mlp, children):
        self.__dict__["_mlp"] = mlp
        self.__dict__.update(children)

    def __getattr__(self, name):
        v = getattr(self.__dict__["_mlp"], name)
        if isinstance(v, nn.Module):
            raise RuntimeError(f"forward reads the submodule {name!r}")
        return v


def _mlp_flow_is_gated(mlp: nn.Module) -> bool:
    """True iff type(mlp).forward IS down_proj(act_fn(gate_proj(x)) * up_proj(x)), each child called once: probed with exact functions, not pattern-matched."""
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
            out = type(mlp).forward(_MLPStandin(mlp, kids), x.clone())
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
