"""Call-site integration for the per-head ``q_norm`` / ``k_norm`` of transformers' Qwen3, Qwen3-MoE and Gemma-3 text decoders: an attention that normalises every
HEAD of q and of k (rows of ``head_dim`` elements) before the rotary embedding,

    q = q_norm(q_proj(x).view(B, T, H, D))                      (Qwen3;   Gemma-3: q_norm(q_proj(x).view(B, T, H, D).transpose(1, 2)))

Each of these calls is the eager RMSNorm chain — about eight launches, twice per layer.  ``fuse_qk_norms(model)`` replaces such a norm by ``HeadRMSNorm``: one launch
of ``head_rmsnorm`` (kernel K1hn), which norms the heads where they lie — a column slice of the fused q/k/v output, or its transposed view — without a copy.  The norm
becomes the specified norm (QSPEC HN1: N1-N5 for the Llama form, NG1-NG5 for the Gemma form; spec-exact and eager-close) instead of the eager chain, so the switch
changes bits against the model without it.

Nothing is recognised by class name: a norm is probed (``head_norm_kind`` runs its class's forward against the formulas).  The entry is opt-in and independent of
``swap_linears`` — the kernel takes any float tensor.  Call it LAST: the other entries' CPU probes may run the real attention forward, and a ``HeadRMSNorm`` raises on
CPU tensors like everything in the library; called before them, they refuse the affected layers (the model still runs, with less fused).  OLMo's whole-width q/k norm
(one row of ``H * D``) belongs to ``fuse_olmo_layers``; Cohere's is a mean-subtracting LayerNorm with a 2-D weight; both are left alone.  Out of scope: the rotary
embedding, norming q and k in a single launch, an in-place form, ``shard_llama_layers``, a CPU path."""
from __future__ import annotations

import torch
from torch import nn

from .gemma import _NormStandin, _gemma_formula, _llama_formula
from .olmo import OlmoRMSNorm, _norm_eps, _olmo_formula
from .qtensor import head_rmsnorm
from .residual_flow import _hooked


class HeadRMSNorm(nn.Module):
    """A per-head RMSNorm by the specified norm (QSPEC HN1; kernel K1hn): what q_norm / k_norm become under fuse_qk_norms.  Holds the module's own weight OBJECT (not a
    copy: state-dict key and storage unchanged) and its eps under the name it had (`variance_epsilon` or `eps`).  kind: "llama" (gain w, x * rs rounded first) or
    "gemma" (gain 1 + w, one rounding)."""

    def __init__(self, weight: torch.Tensor, eps: float, kind: str, eps_name: str = "variance_epsilon"):
        super().__init__()
        if kind not in ("llama", "gemma"):
            raise ValueError(f"HeadRMSNorm: kind must be 'llama' or 'gemma', got {kind!r}")
        if eps_name not in ("variance_epsilon", "eps"):
            raise ValueError(f"HeadRMSNorm: eps_name must be 'variance_epsilon' or 'eps', got {eps_name!r}")
        self.weight = weight if isinstance(weight, nn.Parameter) else nn.Parameter(weight, requires_grad=False)
        self.kind = kind
        self._eps_name = eps_name
        setattr(self, eps_name, float(eps))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return head_rmsnorm(x, self.weight, getattr(self, self._eps_name), self.kind)

    def extra_repr(self):
        gain = "gain 1 + w, " if self.kind == "gemma" else ""
        return f"{tuple(self.weight.shape)}, eps={getattr(self, self._eps_name)}, {gain}per head, one launch"


def head_norm_kind(m):
    """"llama", "gemma" or None: which RMSNorm `m` computes, decided by behaviour.  `m` must be a module with a 1-D `weight`, a float `variance_epsilon` or `eps` and no
    other parameter, buffer or child; its class's forward — run on a stand-in with a seeded non-trivial weight, on a small CPU tensor in bf16 and in f32 — must return
    exactly the Llama formula (w * (x.float() * rs).to(x.dtype): Qwen3RMSNorm, LlamaRMSNorm) or exactly the Gemma formula (((x.float() * rs) * (1 + w.float())).type_as(x):
    Gemma3RMSNorm, GemmaRMSNorm) in both dtypes, with the other one and the OLMo formula (gain w, one rounding) differing on the bf16 operands.  In f32 the Llama and
    OLMo formulas coincide by construction, and the Llama formula is accepted there as "llama".  Olmo2RMSNorm, nn.LayerNorm, a subclass with another forward, a norm
    with a buffer, an OlmoRMSNorm and a HeadRMSNorm give None."""
    if not isinstance(m, nn.Module) or isinstance(m, (HeadRMSNorm, OlmoRMSNorm)):
        return None
    w = getattr(m, "weight", None)
    eps_name, eps = _norm_eps(m)
    if not isinstance(w, torch.Tensor) or w.dim() != 1 or w.shape[0] < 1 or eps_name is None:
        return None
    if [n for n, _ in m.named_parameters()] + [n for n, _ in m.named_buffers()] != ["weight"] or any(True for _ in m.children()):
        return None
    g = torch.Generator().manual_seed(20240221)
    xs = torch.randn(3, 5, w.shape[0], generator=g) * torch.tensor([0.05, 1.0, 20.0]).reshape(3, 1, 1)
    ws = 0.3 * torch.randn(w.shape[0], generator=g)
    formulas = {"llama": _llama_formula, "gemma": _gemma_formula}
    kinds = []
    try:
        for dt in (torch.bfloat16, torch.float32):
            x, wt = xs.to(dt), ws.to(dt)
            standin = _NormStandin(type(m), wt, eps)
            standin.__dict__[eps_name] = eps
            with torch.no_grad():
                got = type(m).forward(standin, x.clone())
            if not isinstance(got, torch.Tensor) or got.dtype != dt or got.shape != x.shape:
                return None
            want = {k: f(x, wt, eps) for k, f in formulas.items()}
            if torch.equal(want["llama"], want["gemma"]):
                return None          # (the operands do not tell the two apart)
            hit = [k for k in formulas if torch.equal(got, want[k])]
            if len(hit) != 1:
                return None
            if dt == torch.bfloat16 and torch.equal(got, _olmo_formula(x, wt, eps)):
                return None          # (gain w with ONE rounding is OLMo's norm, and the operands must tell it apart)
            kinds.append(hit[0])
    except Exception:          # noqa: BLE001  (whatever the forward raises on the stand-in: refused)
        return None
    return kinds[0] if kinds[0] == kinds[1] else None


def fuse_qk_norms(model: nn.Module) -> int:
    """Replace the per-head q_norm / k_norm of every attention found in `model` (in place) by a HeadRMSNorm (one launch of head_rmsnorm, K1hn, in place of the eager
    chain); returns the number of norm modules replaced by THIS call (a second call returns 0).  An attention is any module that has children `q_norm` and `k_norm`
    and an integer `head_dim`.  Each of the two is replaced on its own, if its head_norm_kind is not None, its weight has exactly head_dim elements and it carries no
    forward hook or pre-hook (the module is no longer called, so a hook on it would silently stop firing).  The new module holds the same weight object (state-dict
    keys and storage unchanged) and the eps under the name it had.  Qwen3, Qwen3-MoE and Gemma-3 are taken; OLMo-2 / OLMo-3 (a weight H * D wide: fuse_olmo_layers'),
    Cohere (a LayerNorm with a 2-D weight), Llama / Mistral / Qwen2 (no such children) and an attention whose norms are already OlmoRMSNorm or HeadRMSNorm are left
    exactly as they were.

    Opt-in and independent of swap_linears; the norms become the specified norm (QSPEC HN1), so the bits change against the model without it: spec-exact, eager-close.
    Call it LAST, after fuse_llama_layers / fuse_gemma_layers / fuse_gemma_postnorm_residual / swap_moe_experts: their CPU probes may run the attention's forward, and
    a HeadRMSNorm raises on CPU tensors; called first, those entries refuse the affected layers."""
    replaced = 0
    for attn in list(model.modules()):
        children = dict(attn.named_children())
        head_dim = getattr(attn, "head_dim", None)
        if "q_norm" not in children or "k_norm" not in children or not isinstance(head_dim, int) or isinstance(head_dim, bool):
            continue
        for name in ("q_norm", "k_norm"):
            old = children[name]
            kind = head_norm_kind(old)
            if kind is None or old.weight.shape[0] != head_dim or _hooked(old):
                continue
            eps_name, eps = _norm_eps(old)
            setattr(attn, name, HeadRMSNorm(old.weight, eps, kind, eps_name))
            replaced += 1
    return replaced
