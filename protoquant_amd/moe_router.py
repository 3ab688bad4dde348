"""The expert selection of a decoder's mixture-of-experts routers on the library's kernel: fuse_moe_routers(model) gives every router module it recognises a forward
that runs the router's own F.linear and then ONE moe_topk launch (C-ABI pq_moe_topk, kernel K-rt; QSPEC RT1-RT5) where the model's code runs a softmax, a top-k, a sum,
a division and a cast.  Opt-in, an entry of its own: independent of swap_moe_experts and valid before or after it.

Recognition is by behaviour, never by name or import (router_parts): a leaf module with a 2-D `weight` [E, H], optionally a 1-D `bias` [E], an integer `top_k` and
nothing else that computes — and whose class forward, run on the CPU in float32 on planted weights and a seeded input with well separated logits, returns a tuple that
holds F.linear(x, W, b), the [T, k] indices and the [T, k] scores of one of the three recipes the kernel serves.  transformers 5's MixtralTopKRouter, Qwen2MoeTopKRouter,
Qwen3MoeTopKRouter, OlmoeTopKRouter ("softmax_topk"), GptOssTopKRouter and GraniteMoeTopKRouter ("topk_softmax") pass; DeepSeek-V3's router (a correction-bias buffer,
sigmoid, grouped top-k), Phi-MoE's (sparsemixer) and DeepSeek-V4's do not and stay the very same objects.

A recognised router keeps its parameters and its state-dict keys and gets a class DERIVED FROM ITS OWN, so isinstance(router, OriginalClass) — what transformers'
OutputRecorder records router_logits through — keeps holding.  On CPU tensors the new forward is the original class's: the model's own code, not a fallback of the
library.  The switch is not bit-neutral: the softmax becomes the specified one (exp_spec, a pinned summation order) and equal logits go to the lower expert id."""
from __future__ import annotations

import copy
from typing import NamedTuple

import torch
import torch.nn.functional as F
from torch import nn

from .moe import MoEBlock, moe_topk

# the probe's tolerance on the scores: both sides are binary32 evaluations of the same recipe on the same logits (each within a few units of 2^-24 of the exact value)
PROBE_RTOL, PROBE_ATOL = 2e-5, 1e-7
_PROBE_TOKENS = 64


class RouterParts(NamedTuple):
    """What router_parts reports of a router it recognises: where its forward returns what, and the recipe."""
    num_experts: int
    hidden: int
    has_bias: bool
    pos_logits: int           # position of F.linear(x, W, b) in the returned tuple
    pos_scores: int
    pos_indices: int
    kind: str                 # "softmax_topk" | "topk_softmax"
    renormalise: bool         # softmax_topk: the k probabilities are divided by their sum (read from renorm_attr at run time when the module has one)
    renorm_attr: str | None   # "norm_topk_prob" where the module's forward follows that attribute
    scores_f32: bool          # the scores come back in float32 whatever the input's dtype (Mixtral); else in the input's dtype
    logits_f32: bool          # the returned logits are the F.linear output widened to float32 (GraniteMoe); else the F.linear output itself
    flatten: bool             # the forward collapses the leading axes of its input to rows


def _reference(logits: torch.Tensor, k: int, kind: str, renorm: bool):
    if kind == "softmax_topk":
        w, ids = torch.topk(torch.softmax(logits.float(), dim=-1), k, dim=-1)
        return (w / w.sum(dim=-1, keepdim=True) if renorm else w), ids
    v, ids = torch.topk(logits.float(), k, dim=-1)
    return torch.softmax(v, dim=-1), ids


def _planted(E: int, H: int, has_bias: bool, dtype):
    """weights, bias and input of the probe: seeded, and in float32 every row's logits pairwise at least 4 / E apart, so that no recipe's top-k hangs on a rounding.
    Token t reads column t mod H of the weight alone; that column is a permutation of a grid of step 8 / E, and the bias moves an expert by less than a quarter step."""
    g = torch.Generator().manual_seed(20240)
    step = 8.0 / E
    grid = (torch.arange(E, dtype=torch.float32) - (E - 1) / 2) * step
    W = torch.randn(E, H, generator=g) * 0.1
    x = torch.zeros(_PROBE_TOKENS, H)
    for t in range(_PROBE_TOKENS):
        W[:, t % H] = grid[torch.randperm(E, generator=g)]
        x[t, t % H] = 1.0
    b = ((torch.rand(E, generator=g) - 0.5) * (step / 2)).to(dtype) if has_bias else None
    return W.to(dtype), b, x.to(dtype)


def _run(mod: nn.Module, cls, W, b, x, top_k: int, attrs: dict):
    """the class's own forward on a shallow copy of the module that holds the planted parameters (the module itself is not touched)"""
    probe = copy.copy(mod)
    probe.__dict__["_parameters"] = {"weight": nn.Parameter(W, requires_grad=False)}
    if b is not None:
        probe.__dict__["_parameters"]["bias"] = nn.Parameter(b, requires_grad=False)
    probe.__dict__["_buffers"], probe.__dict__["_modules"] = {}, {}
    probe.__dict__["top_k"] = top_k
    probe.__dict__.update(attrs)
    try:
        with torch.no_grad():
            out = cls.forward(probe, x)
    except Exception:
        return None
    return out if isinstance(out, tuple) and all(isinstance(o, torch.Tensor) for o in out) else None


def router_parts(mod: nn.Module):
    """RouterParts of a module that is a router the kernel can stand behind (see the module docstring), else None.  Runs the module's class forward on the CPU; changes
    nothing."""
    if getattr(mod, "_pq_router", None) is not None:
        return None
    cls = type(mod)
    params = dict(mod.named_parameters(recurse=False))
    if "weight" not in params or not set(params) <= {"weight", "bias"} or list(mod.named_buffers(recurse=False)) or list(mod.children()):
        return None
    if cls.forward is nn.Linear.forward or isinstance(mod, nn.Linear):
        return None
    if any(len(getattr(mod, h, ())) for h in ("_forward_hooks", "_forward_pre_hooks", "_backward_hooks", "_backward_pre_hooks")):
        return None
    W, b = params["weight"], params.get("bias")
    if W.dim() != 2 or not W.is_floating_point() or (b is not None and (b.dim() != 1 or b.shape[0] != W.shape[0])):
        return None
    E, H = W.shape
    top_k = getattr(mod, "top_k", None)
    if not isinstance(top_k, int) or isinstance(top_k, bool) or not 1 <= top_k <= min(E, 64) or E > 1024:
        return None
    if any(isinstance(getattr(mod, n, E), int) and getattr(mod, n, E) != E for n in ("num_experts", "num_local_experts")):
        return None
    kp = top_k if E == 1 else min(top_k, max(1, E // 2))          # fewer than E experts: renormalised and plain scores then differ by far more than the tolerance
    Wp, bp, xp = _planted(E, H, b is not None, torch.float32)
    renorm_attr = "norm_topk_prob" if isinstance(getattr(mod, "norm_topk_prob", None), bool) else None
    found = None
    for value in ((True, False) if renorm_attr else (None,)):
        out = _run(mod, cls, Wp, bp, xp, kp, {renorm_attr: value} if renorm_attr else {})
        if out is None or len(out) < 3:
            return None
        logits = F.linear(xp, Wp, bp)
        pos_l = [i for i, o in enumerate(out) if o.shape == logits.shape and o.is_floating_point() and torch.equal(o.float(), logits)]
        pos_i = [i for i, o in enumerate(out) if tuple(o.shape) == (_PROBE_TOKENS, kp) and not o.is_floating_point() and not o.is_complex() and o.dtype != torch.bool]
        pos_s = [i for i, o in enumerate(out) if tuple(o.shape) == (_PROBE_TOKENS, kp) and o.is_floating_point() and i not in pos_l]
        if len(pos_l) != 1 or len(pos_i) != 1 or len(pos_s) != 1 or len(out) != 3:
            return None
        # softmax -> top-k -> renormalise and top-k -> softmax are ONE function in exact arithmetic: where both are within the tolerance, the recipe whose plain-torch
        # evaluation gives the module's very bits is the one the module runs (same operations, same machine); failing that, the first that is close
        close, exact = [], []
        for kind, renorm in (("softmax_topk", False), ("softmax_topk", True), ("topk_softmax", False)):
            w, ids = _reference(logits, kp, kind, renorm)
            if torch.equal(out[pos_i[0]].long(), ids) and torch.allclose(out[pos_s[0]].float(), w, rtol=PROBE_RTOL, atol=PROBE_ATOL):
                close.append((kind, renorm))
                if torch.equal(out[pos_s[0]].float(), w):
                    exact.append((kind, renorm))
        match = (exact or close or [None])[0]
        if match is None or (value is not None and match[0] == "softmax_topk" and match[1] != value and E > 1):
            return None
        here = (pos_l[0], pos_s[0], pos_i[0], match[0])
        if found is not None and here != found[:4]:
            return None
        found = here + (match[1],)
    follows_attr = renorm_attr is not None and found[3] == "softmax_topk"
    # the dtypes it answers in, and whether it collapses leading axes: one more run, in bfloat16 on a 3-D input
    Wb, bb, xb = _planted(E, H, b is not None, torch.bfloat16)
    out = _run(mod, cls, Wb, bb, xb.reshape(2, _PROBE_TOKENS // 2, H), kp, {})
    if out is None or len(out) != 3:
        return None
    lo, sc, ix = out[found[0]], out[found[1]], out[found[2]]
    if lo.dtype not in (torch.bfloat16, torch.float32) or sc.dtype not in (torch.bfloat16, torch.float32) or ix.is_floating_point():
        return None
    flat, deep = (_PROBE_TOKENS,), (2, _PROBE_TOKENS // 2)
    shapes = {tuple(lo.shape[:-1]), tuple(sc.shape[:-1]), tuple(ix.shape[:-1])}
    if shapes not in ({flat}, {deep}):
        return None
    return RouterParts(E, H, b is not None, found[0], found[1], found[2], found[3], bool(getattr(mod, renorm_attr)) if follows_attr else bool(found[4]), renorm_attr if follows_attr else None, sc.dtype == torch.float32,
                       lo.dtype == torch.float32, shapes == {flat})


def _fused_forward(self, hidden_states: torch.Tensor):
    rec: RouterParts = self._pq_router
    if hidden_states.device.type != "cuda":
        return self._pq_router_class.forward(self, hidden_states)          # the model's own code
    x = hidden_states.reshape(-1, hidden_states.shape[-1]) if rec.flatten else hidden_states
    logits = F.linear(x, self.weight, self.bias if rec.has_bias else None)
    if rec.logits_f32:
        logits = logits.float()
    renorm = bool(getattr(self, rec.renorm_attr)) if rec.renorm_attr else rec.renormalise
    scores, ids = moe_topk(logits, self.top_k, rec.kind, renorm, out_dtype=torch.float32 if rec.scores_f32 else hidden_states.dtype, ids_dtype=torch.int64)
    out = [None, None, None]
    out[rec.pos_logits], out[rec.pos_scores], out[rec.pos_indices] = logits, scores, ids
    return tuple(out)


_DERIVED: dict = {}


def _rebuild(cls, state):
    """what pickle and deepcopy call for a fused router: an instance of the ORIGINAL class (found by its name, as for any module) given the derived class again"""
    obj = cls.__new__(cls)
    obj.__dict__.update(state)
    obj.__class__ = _derived(cls)
    return obj


def _reduce_ex(self, protocol):
    return _rebuild, (self._pq_router_class, self.__dict__.copy())


def _derived(cls):
    """the class a fused router of class `cls` gets: made once per class, not importable by name — so its instances pickle (torch.save(model)) and deepcopy through
    _rebuild, which needs only the original class and this module"""
    if cls not in _DERIVED:
        _DERIVED[cls] = type(cls.__name__, (cls,), {"forward": _fused_forward, "__module__": cls.__module__, "__doc__": cls.__doc__, "_pq_router_class": cls,
                                                    "__reduce_ex__": _reduce_ex})
    return _DERIVED[cls]


def fuse_moe_routers(model: nn.Module) -> int:
    """Give, in place, every router of the model that router_parts recognises the one-launch forward, and set hip_routing on every MoEBlock.  Returns the number of
    routers and blocks changed (0: nothing recognised, or a second call).  Parameters, state-dict keys and every other module stay what they were."""
    n = 0
    for mod in list(model.modules()):
        if isinstance(mod, MoEBlock):
            if not mod.hip_routing:
                mod.hip_routing = True
                n += 1
            continue
        parts = router_parts(mod)
        if parts is not None:
            cls = type(mod)
            mod.__class__ = _derived(cls)
            mod.__dict__["_pq_router"] = parts
            n += 1
    return n
