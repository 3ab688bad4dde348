"""Call-site integration for Llama-family decoder layers (transformers' LlamaDecoderLayer shape: input_layernorm -> self_attn with
q_proj / k_proj / v_proj / o_proj -> post_attention_layernorm -> mlp), SURVEY.md §8(f)1-2 applied to a whole model:

* both RMSNorms of a layer are fused into the activation quantisation of the projections they feed (``rmsnorm_quantize``: the
  normalised activation never reaches HBM, the norm costs no traffic beyond the quantisation that had to happen anyway);
* q / k / v share that one quantisation and ONE GEMM launch (``FusedQLinear``, N = hidden + 2 * kv);
* gate / up / down are a ``GatedMLP`` (fused gate+up GEMM, silu*mul fused into the quantisation of down's input).

The stock attention code keeps calling ``self.q_proj(h)``, ``self.k_proj(h)``, ``self.v_proj(h)``: ``h`` is now a per-token
``QTensor`` (it only needs ``.shape`` besides being handed to the projections), the first call runs the fused GEMM and the other
two return their column slices of its output.  Attention itself (rope, SDPA), the residual adds, the final norm and the embedding
stay stock torch-ROCm ops.  ``swap_linears(model, fuse_gated_mlp=True)`` must have run first.

``fuse_llama_layers(model, fuse_residual=True)`` (opt-in) also takes the two residual adds of a layer into the norm that follows them
(``add_rmsnorm_quantize``, kernel K1a: the residual stream is stored once and normalised from registers): see ``ResidualFusedLayer``."""
from __future__ import annotations

import torch
from torch import nn

from .qlinear import FusedQLinear, GatedMLP, qlinear
from .qtensor import QTensor, add_rmsnorm_quantize, rmsnorm_quantize
from .residual_flow import NamedFusedLayer, _forward_extra_params, attention, fuse_stacks, probe_named_flow
from .residual_flow import _HandOver  # noqa: F401  (the name under which it was introduced here stays importable)


class RMSNormQuant(nn.Module):
    """RMSNorm whose output is the per-token int8 quantisation of the normalised activation (QSPEC N1-N6 then Q1-Q6)."""

    def __init__(self, weight: torch.Tensor, eps: float):
        super().__init__()
        self.weight = nn.Parameter(weight.detach().clone(), requires_grad=False)
        self.variance_epsilon = float(eps)

    def forward(self, x: torch.Tensor, residual: torch.Tensor | None = None):
        """Without `residual`: the QTensor of RMSNorm(x).  With it: (QTensor of RMSNorm(residual + x), residual + x) from one kernel (K1a) — the bits of the
        torch add followed by the call without `residual`."""
        if residual is None:
            return rmsnorm_quantize(x, self.weight, self.variance_epsilon)
        return add_rmsnorm_quantize(x, residual, self.weight, self.variance_epsilon)

    def extra_repr(self):
        return f"{tuple(self.weight.shape)}, eps={self.variance_epsilon} -> int8 per-token QTensor"


class _FusedSlice(nn.Module):
    """Projection number `index` of a FusedQLinear shared by sibling slices.  The attention module's forward pre-hook (installed by
    fuse_llama_layers) runs the fused GEMM ONCE per forward on the hidden states it is called with; the slices, called with that
    same object by the stock attention code, return their parts of it.  Called with anything else (outside the attention forward, a
    different tensor), a slice computes its result from its own input — correct, just not shared."""

    def __init__(self, shared: "_SharedFused", index: int):
        super().__init__()
        self._shared = [shared]            # (a list: the shared module is registered once, on its owner)
        self.index = index

    def forward(self, x):
        return self._shared[0].part(x, self.index)


class _SharedFused(nn.Module):
    """The fused q/k/v GEMM of one attention module and its per-forward result: begin() at the attention's entry, end() at its exit
    (always: exceptions included), so nothing outlives the forward, a recomputed forward (activation checkpointing) recomputes, and
    an input changed in place between two forwards is never served stale."""

    def __init__(self, fused: FusedQLinear):
        super().__init__()
        self.fused = fused
        self._key, self._outs = None, None

    def begin(self, x):
        self._key, self._outs = x, self.fused(x)

    def end(self):
        self._key, self._outs = None, None

    def part(self, x, index):
        if self._outs is not None and self._key is x:
            return self._outs[index]
        return self.fused(x)[index]


def _qkv_pre_hook(mod, args, kwargs):
    x = kwargs.get("hidden_states", args[0] if args else None)
    if x is not None:
        mod.qkv_fused.begin(x)          # (looked up on the module, not captured: a deep copy of the model shares nothing with its original)


def _qkv_post_hook(mod, args, kwargs, out):
    mod.qkv_fused.end()


def _install_qkv_hooks(attn: nn.Module) -> None:
    attn.register_forward_pre_hook(_qkv_pre_hook, with_kwargs=True)
    attn.register_forward_hook(_qkv_post_hook, with_kwargs=True, always_call=True)


def _is_rmsnorm(m) -> bool:
    return hasattr(m, "weight") and hasattr(m, "variance_epsilon") and isinstance(getattr(m, "weight"), torch.Tensor) and m.weight.dim() == 1


# ---------------------------------------------------------------- the residual adds fused into the norms that follow them (opt-in)
_CHILDREN = {"input_layernorm": lambda t: t * 2.0, "self_attn": attention(lambda h: h + 1.0), "post_attention_layernorm": lambda t: t * 0.5 - 3.0,
             "mlp": lambda t: t * t}


def _llama_flow(x):
    r1 = x + (x * 2.0 + 1.0)
    return r1 + (r1 * 0.5 - 3.0) ** 2


def residual_flow_is_llama(layer: nn.Module, cls=None) -> bool:
    """True iff `cls.forward` (default: the layer's own class) IS the Llama data flow on this layer:

        r1 = x + self_attn(hidden_states=input_layernorm(x), **kwargs)[0];   out = r1 + mlp(post_attention_layernorm(r1))

    with each of the four children called once, every keyword argument of the layer handed to the attention unchanged, no other submodule touched and a tensor
    returned.  Probed, not pattern-matched: the class's forward runs on a stand-in whose children are cheap exact functions on a tiny CPU tensor, and its result
    must EQUAL the formula.  transformers' Llama, Mistral, Qwen2 and Qwen3 layers pass; Granite (residual_multiplier != 1), Gemma-2 and OLMo-2 (post-norms),
    Phi-3 (dropout children), Cohere (parallel block) and any forward that raises on the stand-in do not."""
    return probe_named_flow(layer, cls or type(layer), _CHILDREN, _llama_flow, attn_positional=True)


class ResidualFusedLayer(NamedFusedLayer):
    """A Llama-flow decoder layer whose two residual adds run inside the RMSNorm + quantisation kernels that follow them (K1a, add_rmsnorm_quantize):

        h          = the QTensor handed over for this very tensor, else input_layernorm(hidden)
        attn_out   = self_attn(hidden_states=h, **kwargs)[0]
        hq, resid  = post_attention_layernorm(attn_out, residual=hidden)         # add + norm + quant, one launch
        m          = mlp(hq)
        last of the chain:  return resid + m                                     # a torch add
        otherwise:          hq2, out = NEXT layer's input_layernorm(m, residual=resid);  hand hq2 to the next layer;  return out

    What the layer returns is the real summed tensor (the bits of the two torch adds: QSPEC A1), so hooks, output_hidden_states and the final norm see what they saw.
    fuse_llama_layers(fuse_residual=True) makes a layer one by giving the layer object a class that derives from this one AND from its original class: the object, its
    four children under their names (state_dict keys), its other attributes, its hooks and every isinstance check on it stay as they were.  The tensor the layer was
    called with is never written; the hand-over is consumed at the next layer's entry and never served for another tensor or a tensor changed in place since."""
    _pq_prefix = "ResidualFused"

    def forward(self, hidden_states, *args, **kwargs):
        if args:
            self._fold_positional(args, kwargs)
        h = self._rf_inbox.take(hidden_states)
        if h is None:
            h = self.input_layernorm(hidden_states)
        attn_out = self.self_attn(hidden_states=h, **kwargs)[0]
        hq, resid = self.post_attention_layernorm(attn_out, residual=hidden_states)
        m = self.mlp(hq)
        nxt = self._rf_next[0]
        if nxt is None:
            return resid + m
        hq2, out = nxt.input_layernorm(m, residual=resid)
        nxt._rf_inbox.put(out, hq2)
        return out


def _fuse_residual(model: nn.Module, only=None) -> int:
    """only (default: every layer): the ids of the layers that may be changed — gemma.fuse_gemma_layers passes the layers it recognised"""
    def convert(layer):
        if isinstance(layer, ResidualFusedLayer) or not all(hasattr(layer, c) for c in _CHILDREN) or (only is not None and id(layer) not in only):
            return None
        if not (isinstance(layer.input_layernorm, RMSNormQuant) and isinstance(layer.post_attention_layernorm, RMSNormQuant)):
            return None
        cls = type(layer)
        if not residual_flow_is_llama(layer, cls):
            return None
        layer._rf_argnames = _forward_extra_params(cls)[0]
        return cls
    return fuse_stacks(model, ResidualFusedLayer, convert)          # (a chain that ends, ends with a torch add)


def residual_fused_layers(model: nn.Module) -> int:
    """the number of residual-fused decoder layers in `model`: the ResidualFusedLayer modules fuse_llama_layers(fuse_residual=True) made and the ResidualFusedBlock
    modules gptlike.fuse_layernorm_residual made, over all calls"""
    return sum(1 for m in model.modules() if isinstance(m, ResidualFusedLayer) or getattr(type(m), "_pq_residual_fused", False))


def fuse_llama_layers(model: nn.Module, fuse_norms: bool = True, fuse_qkv: bool = True, fuse_residual: bool = False) -> int:
    """Apply the fusions above to every decoder layer found in `model` (in place); returns the number of layers changed.

    fuse_residual=True (opt-in; the default leaves everything as it was): afterwards, every layer of a ModuleList whose two norms are RMSNormQuant and whose class's
    forward passes residual_flow_is_llama becomes a ResidualFusedLayer.  A refused layer keeps the fusions above and breaks the chain (its predecessor ends with a
    torch add).  The module that owns the ModuleList gets an always-called forward hook that drops every pending hand-over when its forward ends.  The return value
    is unchanged; residual_fused_layers(model) counts the residual-fused layers.  A layer whose norms are LayerNorms (StarCoder2: this data flow, LayerNormQuant norms) is
    ignored here: that switch is gptlike.fuse_layernorm_residual(model) (kernel K1al).  (shard_llama_layers is not covered: its residual stream is replicated over the ranks
    and its layers keep the torch adds.)"""
    n = 0
    for layer in model.modules():
        attn, mlp = getattr(layer, "self_attn", None), getattr(layer, "mlp", None)
        if attn is None or mlp is None or not hasattr(layer, "input_layernorm") or not hasattr(layer, "post_attention_layernorm"):
            continue
        q, k, v = (getattr(attn, p, None) for p in ("q_proj", "k_proj", "v_proj"))
        if not all(isinstance(p, qlinear) for p in (q, k, v)):
            continue
        if fuse_qkv:
            attn.qkv_fused = _SharedFused(FusedQLinear([q, k, v]))
            attn.q_proj, attn.k_proj, attn.v_proj = (_FusedSlice(attn.qkv_fused, i) for i in range(3))
            _install_qkv_hooks(attn)
        if fuse_norms and _is_rmsnorm(layer.input_layernorm):
            layer.input_layernorm = RMSNormQuant(layer.input_layernorm.weight, layer.input_layernorm.variance_epsilon)
        mlp_ok = isinstance(mlp, GatedMLP) or all(isinstance(getattr(mlp, p, None), qlinear) for p in ("gate_proj", "up_proj"))
        if fuse_norms and _is_rmsnorm(layer.post_attention_layernorm) and mlp_ok:
            layer.post_attention_layernorm = RMSNormQuant(layer.post_attention_layernorm.weight, layer.post_attention_layernorm.variance_epsilon)
        n += 1
    if fuse_residual:
        _fuse_residual(model)
    return n


# ---------------------------------------------------------------- BASELINE config 5: the same layers column-sharded over the ranks of one node
class _ShardedInputProj(nn.Module):
    """o_proj of a head-sharded attention: called by the stock attention code with THIS rank's heads of the attention output [..., H / G]; the int8-code exchange of
    ColumnShardedQLinear.forward_sharded_input rebuilds the whole projection (this rank's output channels, then the all-gather of the output shards)."""

    def __init__(self, sharded):
        super().__init__()
        self.sharded = sharded

    def forward(self, x):
        return self.sharded.forward_sharded_input(x)


def _rows_of(lin: nn.Linear, lo: int, hi: int, device) -> nn.Linear:
    sub = nn.Linear(lin.in_features, hi - lo, bias=lin.bias is not None, device=device, dtype=lin.weight.dtype)
    with torch.no_grad():
        sub.weight.copy_(lin.weight[lo:hi])
        if lin.bias is not None:
            sub.bias.copy_(lin.bias[lo:hi])
    return sub


def _q_rows(mod, lo: int, hi: int, device) -> qlinear:
    """rows [lo, hi) of a projection as a qlinear on `device`: an nn.Linear's slice is quantised there; a qlinear's int8 codes, scales and bias are SLICED (per-channel
    quantisation is row-local: the slice of the codes is the codes of the slice) — an int8 checkpoint is sharded without its bf16 weights ever existing."""
    if isinstance(mod, qlinear):
        bias = mod.bias[lo:hi].to(device).contiguous() if mod.bias is not None else None
        dt = mod.bias.dtype if mod.bias is not None else torch.bfloat16
        qt = QTensor(mod.wq[lo:hi].to(device).contiguous(), mod.ws[lo:hi].to(device).contiguous(), 1, dt, torch.Size((hi - lo, mod.in_features)))
        return qlinear.from_qtensor(qt, bias)
    return qlinear.from_linear(_rows_of(mod, lo, hi, device))


def _is_proj(m) -> bool:
    return isinstance(m, (nn.Linear, qlinear))


def shard_llama_layers(model: nn.Module, world: int | None = None, rank: int | None = None, group=None, native=None, device=None,
                       shard_lm_head: bool = True) -> int:
    """BASELINE config 5 as a call site: every linear of every Llama-family decoder layer of `model` — nn.Linear (call this INSTEAD of swap_linears) or already a
    qlinear / GatedMLP (a model loaded from an int8 checkpoint, or after swap_linears: codes and scales are sliced, nothing is re-quantised) — becomes this
    rank's COLUMN shard of the int8 layer — north_star's scheme — and the stock attention / residual code keeps running unchanged, on this rank's heads:

    * q / k / v: the rank's heads (q rows [r H/G, (r+1) H/G), k / v rows of its KV heads) as ONE fused local GEMM on the replicated, RMSNorm-fused int8 input; their
      outputs are consumed by the rank's own attention heads — nothing is gathered (HF's attention infers the head count from the projection's width);
    * o: the rank's output channels; its input — the rank's heads of the attention output — is exchanged as int8 codes (forward_sharded_input), its output shards are
      all-gathered (the residual stream stays replicated);
    * gate / up / down: ColumnShardedGatedMLP (int8-code exchange between them, all-gather of down's output shards);
    * lm_head (shard_lm_head): column-sharded over the vocabulary, logits all-gathered.
    The weights may live anywhere (CPU included): each layer's slices are copied to `device` (default: the current CUDA device) and quantised there, so a model
    larger than one GPU's share can be sharded layer by layer.  native: an RcclColumnGather (libpq_rccl.so) — otherwise torch.distributed collectives over `group`.
    Needs heads % G == 0, kv_heads % G == 0, intermediate % G == 0.  Returns the number of layers changed."""
    import torch.distributed as dist

    from .sharded import ColumnShardedGatedMLP, ColumnShardedQLinear, shard_bounds
    if (world is None) != (rank is None):
        raise ValueError("shard_llama_layers: pass world and rank together (or neither: the communicator's / process group's)")
    if world is None:
        world, rank = (native.world, native.rank) if native is not None else (dist.get_world_size(group), dist.get_rank(group))
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    n = 0
    for layer in model.modules():
        attn, mlp = getattr(layer, "self_attn", None), getattr(layer, "mlp", None)
        if attn is None or mlp is None or not hasattr(layer, "input_layernorm") or not hasattr(layer, "post_attention_layernorm"):
            continue
        q, k, v, o = (getattr(attn, p, None) for p in ("q_proj", "k_proj", "v_proj", "o_proj"))
        if isinstance(mlp, GatedMLP):          # swap_linears(fuse_gated_mlp=True): gate and up are the two row blocks of one fused weight
            I_ = mlp.gate_up.splits[0]
            gu_w = mlp.gate_up
            mk = lambda a, b: qlinear.from_qtensor(QTensor(gu_w.wq[a:b], gu_w.ws[a:b], 1, torch.bfloat16, torch.Size((b - a, gu_w.in_features))),      # noqa: E731
                                                   gu_w.bias[a:b] if gu_w.bias is not None else None)
            g, u, d = mk(0, I_), mk(I_, 2 * I_), mlp.down
        else:
            g, u, d = (getattr(mlp, p, None) for p in ("gate_proj", "up_proj", "down_proj"))
        if not all(_is_proj(p) for p in (q, k, v, o, g, u, d)):
            continue
        hd = int(attn.head_dim)
        nq, nkv = q.out_features // hd, k.out_features // hd
        if nq % world or nkv % world or g.out_features % world or o.in_features != q.out_features:
            raise ValueError(f"shard_llama_layers: {nq} heads / {nkv} KV heads / intermediate {g.out_features} do not split over {world} ranks")
        ql, qh = rank * (nq // world) * hd, (rank + 1) * (nq // world) * hd
        kl, kh = rank * (nkv // world) * hd, (rank + 1) * (nkv // world) * hd
        attn.qkv_fused = _SharedFused(FusedQLinear([_q_rows(q, ql, qh, device), _q_rows(k, kl, kh, device), _q_rows(v, kl, kh, device)]))
        attn.q_proj, attn.k_proj, attn.v_proj = (_FusedSlice(attn.qkv_fused, i) for i in range(3))
        _install_qkv_hooks(attn)
        ol, oh = shard_bounds(o.out_features, world, rank)
        attn.o_proj = _ShardedInputProj(ColumnShardedQLinear(_q_rows(o, ol, oh, device), o.out_features, group, native))
        il, ih = shard_bounds(g.out_features, world, rank)
        hl, hh = shard_bounds(d.out_features, world, rank)
        layer.mlp = ColumnShardedGatedMLP(FusedQLinear([_q_rows(g, il, ih, device), _q_rows(u, il, ih, device)]), _q_rows(d, hl, hh, device),
                                          d.out_features, g.out_features, group, native, world, rank)
        for name in ("input_layernorm", "post_attention_layernorm"):
            nm = getattr(layer, name)
            if _is_rmsnorm(nm):
                setattr(layer, name, RMSNormQuant(nm.weight.to(device), nm.variance_epsilon))
        n += 1
    head = getattr(model, "lm_head", None)
    if shard_lm_head and n and _is_proj(head):
        lo, hi = shard_bounds(head.out_features, world, rank)
        model.lm_head = ColumnShardedQLinear(_q_rows(head, lo, hi, device), head.out_features, group, native)
    return n
