"""Mixture-of-experts layers on the int8 path: the E expert MLPs of a decoder block as TWO grouped GEMM launches (qlinear_s8_grouped: one launch over all experts)
instead of 3 E launches of qlinear, ONE activation quantisation instead of one per expert, and the routing sort and the combine as kernels of the library.

GroupedQLinear   E experts' linear layers as one [E, N, K] int8 weight + [E, N] scales (+ bias)
moe_route        topk_ids[T, k] -> (row_index, offsets, rows_of, slot_of[, xs_sorted]): the (token, slot) pairs sorted by expert (C-ABI pq_moe_route, kernel R)
moe_combine      out[t] = sum of the token's k expert rows times their routing weights, rounded as an eager loop over the experts rounds (C-ABI pq_moe_combine, kernel C)
MoEGatedMLP      forward(hidden[T, H], topk_ids[T, k], topk_weights[T, k]): quantise once -> moe_route (which also puts the row scales in grouped order) -> grouped
                 gate+up GEMM reading the codes through the row index -> silu_mul_quantize -> grouped down GEMM -> moe_combine: library launches only, no torch
                 kernel in between but the cast of the weights (and the zero-tailed copy of the codes where in_features is not a multiple of 128)
swap_moe_experts replaces the routed experts of a decoder's sparse MoE blocks, in either layout model code holds them in: an `experts` module with two stacked
                 parameters gate_up_proj [E, 2 I, H] / down_proj [E, H, I] called as experts(hidden, top_k_index, top_k_weights) (fused_experts_parts: only that module is
                 replaced, by MoEGatedMLP — router, shared experts and the block's return type stay the model's), or a ModuleList `experts` of gated MLPs next to a
                 Linear router `gate` (moe_block_parts: the block is replaced by MoEBlock).  With gates=... also the experts whose gate is not a plain silu —
                 GPT-OSS's clamped alpha-sigmoid, DeepSeek-V4's clamped silu (clamped_experts_parts; glu_quantize stands where silu_mul_quantize does)

route_plan and combine are the same two steps as pure tensor code that runs on any device: the DEFINITION moe_route and moe_combine are held to, element for element and
bit for bit (tests/test_gpu_moe_route.py, tests/test_gpu_moe_combine.py), and what MoEGatedMLP runs with torch_plumbing = True (A/B: tools/moe_layer_bench.py).  The expert
SELECTION — router GEMM, softmax, top-k, renormalisation — stays the model's torch code by default: its bits decide which expert a token goes to.  moe_topk (C-ABI
pq_moe_topk, kernel K-rt) is everything behind the router GEMM in one launch, to a specification of its own (QSPEC RT); fuse_moe_routers (moe_router.py) and
MoEBlock.hip_routing switch it on.
Nothing here reads a routing result on the host: the forward is capturable into a hipGraph and replayable for other routings."""
from __future__ import annotations

import inspect
from typing import NamedTuple

import torch
from torch import nn

from . import _lib as L
from .qlinear import FusedQLinear, GatedMLP, _check_operand, _is_silu, _KPadded, _round_k, _workspace, is_plain_linear, qlinear, qlinear_s8_grouped, qlinear_s8_grouped_stream
from .qtensor import QTensor, glu_params, glu_quantize, quantize, silu_mul_quantize


# Grouped rows up to which GroupedQLinear.forward takes the weight-streaming grouped kernel.  From profiles/r11_moe_decode_bench.txt: the largest of 64 / 32 / 16 / 0 at which
# no recorded row is more than 3 % slower than the tile path.
STREAM_ROWS_DEFAULT = 64


class GroupedQLinear(_KPadded, nn.Module):
    """E linear layers of one shape held together: wq int8 [E, N, K], ws f32 [E, N], bias [E, N] or None.  in_features that is not a multiple of 128 is served as in
    qlinear (_KPadded): a zero-padded copy of the weight, made lazily, and zero-tailed activation codes — same bits.
    stream_rows (class attribute, settable per instance): a forward with 0 < M_total <= stream_rows grouped rows — a decode step — goes through the weight-streaming
    grouped kernel (qlinear_s8_grouped_stream), any other through the 64-row tiles (qlinear_s8_grouped); same bits either way.  M_total is a shape, known on the host:
    nothing synchronises and a captured step keeps its path.  0 = always the tiles; at most 64."""

    stream_rows = STREAM_ROWS_DEFAULT

    def __init__(self, num_experts: int, in_features: int, out_features: int, bias: bool = False, device=None, dtype=None):
        super().__init__()
        self.num_experts, self.in_features, self.out_features = num_experts, in_features, out_features
        dtype = dtype or torch.bfloat16
        self.register_buffer("wq", torch.zeros((num_experts, out_features, in_features), dtype=torch.int8, device=device))
        self.register_buffer("ws", torch.ones((num_experts, out_features), dtype=torch.float32, device=device))
        if bias:
            self.register_buffer("bias", torch.zeros((num_experts, out_features), dtype=dtype, device=device))
        else:
            self.bias = None

    @classmethod
    def _from_parts(cls, wq: torch.Tensor, ws: torch.Tensor, bias) -> "GroupedQLinear":
        m = cls.__new__(cls)
        nn.Module.__init__(m)
        m.num_experts, m.out_features, m.in_features = wq.shape
        m.register_buffer("wq", wq.contiguous())
        m.register_buffer("ws", ws.contiguous())
        if bias is not None:
            m.register_buffer("bias", bias.contiguous())
        else:
            m.bias = None
        return m

    @classmethod
    def from_linears(cls, linears) -> "GroupedQLinear":
        """One expert per element: an nn.Linear (quantised per output channel, as qlinear.from_linear) or an existing qlinear / FusedQLinear, whose codes and scales are
        stacked as they are — nothing is quantised twice."""
        parts = [l if hasattr(l, "wq") else qlinear.from_linear(l) for l in linears]
        if not parts:
            raise ValueError("GroupedQLinear.from_linears: no experts")
        if any(p.wq.shape != parts[0].wq.shape for p in parts) or any((p.bias is None) != (parts[0].bias is None) for p in parts):
            raise ValueError("GroupedQLinear.from_linears: the experts must share one shape, and all or none may have a bias")
        return cls._from_parts(torch.stack([p.wq for p in parts]), torch.stack([p.ws for p in parts]),
                               torch.stack([p.bias for p in parts]) if parts[0].bias is not None else None)

    @classmethod
    def from_weight(cls, weight: torch.Tensor, bias=None) -> "GroupedQLinear":
        """A 3-D expert parameter weight[E, N, K] (y_e = x @ weight[e].T): per-output-channel quantisation of every expert in one pass — kernel K1 over the E * N rows of
        the flattened weight, the bits per-expert quantisation gives.  bias: [E, N] or None."""
        w = weight.detach()
        L.require_gpu(w, "GroupedQLinear.from_weight(weight)")
        if w.dim() != 3:
            raise ValueError("from_weight expects a 3-D [E, N, K] weight")
        E, N, K = w.shape
        q = quantize(w.reshape(E * N, K), axis=-1)
        return cls._from_parts(q.int_data.reshape(E, N, K), q.scale.reshape(E, N), bias.detach().clone() if bias is not None else None)

    def codes_for_gemm(self, codes: torch.Tensor) -> torch.Tensor:
        """int8 [R, in_features] -> the operand the grouped GEMM reads: itself, or a zero-tailed copy of the next multiple of 128 columns"""
        K, kp = self.in_features, _round_k(self.in_features)
        if kp == K:
            return codes
        buf = torch.empty((codes.shape[0], kp), dtype=torch.int8, device=codes.device)
        buf[:, :K].copy_(codes)
        buf[:, K:].zero_()
        return buf

    def forward(self, xq: QTensor, offsets: torch.Tensor, row_index: torch.Tensor | None = None, xs: torch.Tensor | None = None) -> torch.Tensor:
        """xq: per-token QTensor [R, in_features].  Without row_index its rows are the grouped rows themselves; with it grouped row r reads row row_index[r] of xq and xs
        carries the row scales already gathered into grouped order (default: gathered here).  Returns y[M_total, out_features] in xq.orig_dtype."""
        if not isinstance(xq, QTensor) or xq.axis != 1 or xq.shape[-1] != self.in_features:
            raise ValueError("GroupedQLinear: input must be a per-token QTensor [R, in_features]")
        codes = self.codes_for_gemm(xq.int_data.reshape(-1, self.in_features))
        if xs is None:
            xs = xq.scale if row_index is None else xq.scale.index_select(0, row_index)
        wq, _ = self._wq_for_gemm()
        M_total = codes.shape[0] if row_index is None else row_index.numel()
        grouped = qlinear_s8_grouped_stream if 0 < M_total <= self.stream_rows else qlinear_s8_grouped
        return grouped(codes, xs, wq, self.ws, self.bias, offsets, xq.orig_dtype, row_index=row_index)

    def extra_repr(self):
        return (f"num_experts={self.num_experts}, in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"stream_rows={self.stream_rows}")


def route_plan(topk_ids: torch.Tensor, num_experts: int):
    """The (token, slot) pairs of a routing sorted by expert — pure tensor code, runs on any device, reads nothing on the host.
    topk_ids: integer [T, k], every id in [0, num_experts).  Returns
      row_index  int32 [T * k]  the token of grouped row r (stable sort: inside an expert the pairs keep their (token, slot) order)
      offsets    int32 [E + 1]  rows offsets[e] .. offsets[e + 1] - 1 belong to expert e
      rows_of    int64 [T, k]   the grouped rows of token t, ordered by EXPERT id (the order in which an eager loop over the experts adds them up)
      slot_of    int64 [T, k]   the slot j of topk_ids[t] each of those rows came from (to pick the routing weight)"""
    T, k = topk_ids.shape
    flat = topk_ids.reshape(-1).to(torch.int64)
    sorted_ids, order = torch.sort(flat, stable=True)
    row_index = torch.div(order, k, rounding_mode="floor").to(torch.int32)
    edges = torch.arange(num_experts + 1, device=flat.device, dtype=torch.int64)
    offsets = torch.searchsorted(sorted_ids, edges, right=False).to(torch.int32)      # (bincount + cumsum without bincount's device -> host read of the largest id)
    pos = torch.empty_like(order)
    pos[order] = torch.arange(T * k, device=flat.device, dtype=torch.int64)           # grouped row of pair t * k + j (a permutation: no duplicate index)
    slot_of = torch.argsort(topk_ids.to(torch.int64), dim=1, stable=True)
    rows_of = pos.reshape(T, k).gather(1, slot_of)
    return row_index, offsets, rows_of, slot_of


def combine(y: torch.Tensor, rows_of: torch.Tensor, slot_of: torch.Tensor, topk_weights: torch.Tensor) -> torch.Tensor:
    """out[t] = sum over the experts of token t, in ascending expert id, of y[row] * w, every product and every partial sum rounded to y's dtype, starting from zero: the
    bits of `final = zeros; for e in range(E): final.index_add_(0, tokens_e, out_e * w_e[:, None])`.  Deterministic: a gather and k adds, no atomics."""
    T, k = rows_of.shape
    w = topk_weights.to(y.dtype).gather(1, slot_of)
    parts = y.index_select(0, rows_of.reshape(-1)).reshape(T, k, y.shape[1])
    acc = torch.zeros((T, y.shape[1]), dtype=y.dtype, device=y.device)
    for s in range(k):
        acc = acc + parts[:, s] * w[:, s, None]
    return acc


def moe_route(topk_ids: torch.Tensor, num_experts: int, xs: torch.Tensor | None = None):
    """route_plan as ONE call of the library (C-ABI pq_moe_route: one launch while T k <= 4096, three beyond): topk_ids integer [T, k] (int32 or int64) on the GPU ->
    (row_index int32 [T k], offsets int32 [E + 1], rows_of int32 [T, k], slot_of int32 [T, k]) and, with xs (f32 [T], the tokens' row scales), xs_sorted = xs[row_index]
    as a fifth element.  Equal to route_plan element for element for ids in [0, num_experts); an id outside is clamped into the range by the kernel."""
    L.require_gpu(topk_ids, "moe_route(topk_ids)")
    if topk_ids.dim() != 2 or topk_ids.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"moe_route: topk_ids must be an int32 or int64 [T, k] tensor, got {topk_ids.dtype} {tuple(topk_ids.shape)}")
    dev = topk_ids.device
    ids = L.row_major_2d(topk_ids)
    T, k = ids.shape
    if xs is not None:
        _check_operand(xs, "xs", dev, torch.float32, T)
    row_index = torch.empty((T * k,), dtype=torch.int32, device=dev)
    offsets = torch.empty((num_experts + 1,), dtype=torch.int32, device=dev)
    rows_of = torch.empty((T, k), dtype=torch.int32, device=dev)
    slot_of = torch.empty((T, k), dtype=torch.int32, device=dev)
    xs_sorted = torch.empty((T * k,), dtype=torch.float32, device=dev) if xs is not None else None
    with torch.cuda.device(dev):
        wbytes = L.lib().pq_moe_route_workspace_bytes(T, k, num_experts)
        wsp = _workspace(dev, wbytes) if wbytes else None
        L.check(L.lib().pq_moe_route(ids.data_ptr(), 1 if ids.dtype == torch.int64 else 0, L.ld(ids), T, k, num_experts, offsets.data_ptr(), row_index.data_ptr(),
                                     rows_of.data_ptr(), slot_of.data_ptr(), xs.data_ptr() if xs is not None else None,
                                     xs_sorted.data_ptr() if xs is not None else None, wsp.data_ptr() if wsp is not None else None, wbytes, L.stream_ptr(ids)), "moe_route")
    return (row_index, offsets, rows_of, slot_of) if xs is None else (row_index, offsets, rows_of, slot_of, xs_sorted)


def moe_combine(y: torch.Tensor, rows_of: torch.Tensor, slot_of: torch.Tensor, topk_weights: torch.Tensor) -> torch.Tensor:
    """combine as ONE launch of the library (C-ABI pq_moe_combine): y [M_total, H] bf16 / fp16 / f32 (last dim contiguous), rows_of / slot_of int32 [T, k] as moe_route
    returns them, topk_weights [T, k] (cast to y's dtype if it is not) -> out [T, H], the bits of combine(y, rows_of, slot_of, topk_weights): the k rows of a token are
    read once and the sums stay in registers."""
    L.require_gpu(y, "moe_combine(y)")
    dev = y.device
    code = L.dtype_code(y.dtype)
    y = L.row_major_2d(y)
    if rows_of.dim() != 2 or rows_of.shape != slot_of.shape or tuple(topk_weights.shape) != tuple(rows_of.shape):
        raise ValueError(f"moe_combine: rows_of, slot_of and topk_weights must share one [T, k] shape, got {tuple(rows_of.shape)}, {tuple(slot_of.shape)}, {tuple(topk_weights.shape)}")
    _check_operand(rows_of, "rows_of", dev, torch.int32)
    _check_operand(slot_of, "slot_of", dev, torch.int32)
    rows_of, slot_of = rows_of.contiguous(), slot_of.contiguous()
    w = L.row_major_2d(topk_weights if topk_weights.dtype == y.dtype else topk_weights.to(y.dtype))
    _check_operand(w, "topk_weights", dev, y.dtype)
    T, k = rows_of.shape
    M, H = y.shape
    out = torch.empty((T, H), dtype=y.dtype, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().pq_moe_combine(y.data_ptr(), L.ld(y), code, M, rows_of.data_ptr(), slot_of.data_ptr(), w.data_ptr(), L.ld(w), T, k, H, out.data_ptr(), max(H, 1),
                                       L.stream_ptr(y)), "moe_combine")
    return out


def moe_topk(logits: torch.Tensor, top_k: int, kind: str = "softmax_topk", renormalise: bool = False, out_dtype: torch.dtype | None = None,
             ids_dtype: torch.dtype = torch.int64):
    """The expert selection behind a router's GEMM as ONE launch of the library (C-ABI pq_moe_topk, kernel K-rt; QSPEC RT1-RT5): logits [..., E] bf16 / fp16 / f32 on the
    GPU (leading axes collapsed to rows; a view whose last axis is not contiguous is copied once) -> (weights [..., top_k] in out_dtype — default: the logits' dtype —,
    ids [..., top_k] int64 or int32, slot 0 the largest logit, equal logits to the lower expert id).
    kind "softmax_topk": softmax over all experts, the k largest, with renormalise divided by their sum (Mixtral, Qwen-MoE, OLMoE); "topk_softmax": the k largest logits,
    softmax over those (GPT-OSS; renormalise changes nothing).  The softmax is the specified one (exp_spec, a pinned summation order), not the vendor's."""
    if kind not in L.ROUTER_KINDS:
        raise ValueError(f"moe_topk: unknown kind {kind!r}, expected one of {tuple(L.ROUTER_KINDS)}")
    L.require_gpu(logits, "moe_topk(logits)")
    if ids_dtype not in (torch.int32, torch.int64):
        raise TypeError(f"moe_topk: ids_dtype must be torch.int32 or torch.int64, got {ids_dtype}")
    if logits.dim() < 1:
        raise ValueError("moe_topk: logits must have at least one axis")
    code = L.dtype_code(logits.dtype)
    w_dtype = logits.dtype if out_dtype is None else out_dtype
    w_code = L.dtype_code(w_dtype)
    lead, E = tuple(logits.shape[:-1]), logits.shape[-1]
    x2 = L.row_major_2d(logits if logits.dim() == 2 else logits.reshape(-1, E))
    T, k, dev = x2.shape[0], int(top_k), logits.device
    weights = torch.empty((T, max(k, 0)), dtype=w_dtype, device=dev)
    ids = torch.empty((T, max(k, 0)), dtype=ids_dtype, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().pq_moe_topk(x2.data_ptr(), code, L.ld(x2), T, E, k, L.ROUTER_KINDS[kind], 1 if renormalise else 0, weights.data_ptr(), w_code, max(k, 1),
                                    ids.data_ptr(), 1 if ids_dtype == torch.int64 else 0, max(k, 1), L.stream_ptr(x2)), "moe_topk")
    return weights.reshape(lead + (k,)), ids.reshape(lead + (k,))


GATE_KINDS = ("silu", "clamped_silu", "alpha_sigmoid")


def _gate_kinds(gates) -> tuple:
    """the `gates` argument of swap_moe_experts / prepare_for_int8 / convert_checkpoint as a tuple of kinds: "all", one kind, or an iterable of kinds"""
    kinds = GATE_KINDS if gates == "all" else ((gates,) if isinstance(gates, str) else tuple(gates))
    if any(k not in GATE_KINDS for k in kinds):
        raise ValueError(f"unknown gate kind in {gates!r}: expected \"all\" or any of {GATE_KINDS}")
    return kinds


def standard_stacked(gate_up_proj: torch.Tensor, down_proj: torch.Tensor, gate_up_bias=None, down_bias=None, transposed: bool = False, interleaved: bool = False):
    """Stacked expert parameters in the order model code stores them -> (gate_up [E, 2 I, H], down [E, H, I], gate_up_bias [E, 2 I] | None, down_bias [E, H] | None) in the
    order the library reads: y = x @ W[e].T, per expert the gate rows, then the up rows.  transposed: the parameters are stored [E, in, out] (y = x @ W[e]);
    interleaved: gate / up alternate along the output axis (even outputs become rows 0 .. I - 1, odd outputs rows I .. 2 I - 1, the bias permuted alike)."""
    gu, dn = gate_up_proj, down_proj
    if transposed:
        gu, dn = gu.transpose(1, 2), dn.transpose(1, 2)
    if interleaved:
        gu = torch.cat([gu[:, 0::2], gu[:, 1::2]], dim=1)
        if gate_up_bias is not None:
            gate_up_bias = torch.cat([gate_up_bias[:, 0::2], gate_up_bias[:, 1::2]], dim=1)
    return gu.contiguous(), dn.contiguous(), gate_up_bias, down_bias


class MoEGatedMLP(nn.Module):
    """The E gated expert MLPs of a mixture-of-experts block: out[t] = sum_j w[t, j] * down_e(act(gate_e(x_t), up_e(x_t))), e = topk_ids[t, j].
    gate_up: GroupedQLinear [E, 2 I, H] (gate rows, then up rows, per expert); down: GroupedQLinear [E, H, I]; a bias of `down` is added before the routing weight
    multiplies, (x @ W + b) * w.
    gate_kind (plain attributes, not part of the state dict): "silu" — act = silu(g) * u (silu_mul_quantize); "clamped_silu" — silu(min(g, L)) * clamp(u, +-L), L =
    gate_limit (DeepSeek-V4); "alpha_sigmoid" — (clamp(u, +-L) + 1) * gc * sigmoid(gate_alpha * gc), gc = min(g, L) (GPT-OSS); the last two through glu_quantize.
    torch_plumbing = True runs the routing sort and the combine as the stock torch ops of route_plan / combine instead of the library's kernels — same bits (A/B, tests)."""

    torch_plumbing = False

    def __init__(self, gate_up: GroupedQLinear, down: GroupedQLinear, gate_kind: str = "silu", gate_limit: float | None = None, gate_alpha: float | None = None):
        super().__init__()
        if gate_up.num_experts != down.num_experts or gate_up.out_features != 2 * down.in_features:
            raise ValueError("MoEGatedMLP: gate_up must map to 2 x down.in_features, for the same experts")
        if gate_kind not in GATE_KINDS:
            raise ValueError(f"MoEGatedMLP: unknown gate_kind {gate_kind!r}, expected one of {GATE_KINDS}")
        if gate_kind != "silu":
            _, gate_limit, gate_alpha = glu_params(gate_kind, gate_limit, gate_alpha)
            if gate_kind == "clamped_silu":
                gate_alpha = None
        elif gate_limit is not None or gate_alpha is not None:
            raise ValueError("MoEGatedMLP: gate_limit / gate_alpha belong to the clamped gate kinds, not to \"silu\"")
        self.gate_up, self.down = gate_up, down
        self.num_experts = gate_up.num_experts
        self.gate_kind, self.gate_limit, self.gate_alpha = gate_kind, gate_limit, gate_alpha

    @classmethod
    def from_experts(cls, experts) -> "MoEGatedMLP":
        """experts: GatedMLP modules (their codes are stacked as they are) or (gate, up, down) triples of nn.Linear."""
        mlps = [e if isinstance(e, GatedMLP) else GatedMLP.from_linears(*e) for e in experts]
        return cls(GroupedQLinear.from_linears([m.gate_up for m in mlps]), GroupedQLinear.from_linears([m.down for m in mlps]))

    @classmethod
    def from_stacked(cls, gate_up_proj: torch.Tensor, down_proj: torch.Tensor, gate_up_bias: torch.Tensor | None = None, down_bias: torch.Tensor | None = None,
                     transposed: bool = False, interleaved: bool = False, gate_kind: str = "silu", gate_limit: float | None = None,
                     gate_alpha: float | None = None) -> "MoEGatedMLP":
        """The experts as model code holds them since transformers 5: gate_up_proj [E, 2 I, H] (per expert the gate rows, then the up rows; y = x @ W[e].T) and
        down_proj [E, H, I], float, on the GPU — or, with transposed / interleaved, GPT-OSS's storage: gate_up_proj [E, H, 2 I] with gate / up in alternating columns,
        down_proj [E, I, H], gate_up_bias [E, 2 I] interleaved alike, down_bias [E, H].  The conversion to the standard order (standard_stacked) happens once, here.
        Every row is quantised per output channel (GroupedQLinear.from_weight): the codes and scales from_experts gives for the E (gate, up, down) slices taken as
        nn.Linear layers; per-channel quantisation commutes with the row permutation."""
        if gate_up_proj.dim() != 3 or down_proj.dim() != 3:
            raise ValueError(f"MoEGatedMLP.from_stacked: expected 3-D stacked parameters, got {tuple(gate_up_proj.shape)} and {tuple(down_proj.shape)}")
        gu, dn, gub, dnb = standard_stacked(gate_up_proj, down_proj, gate_up_bias, down_bias, transposed, interleaved)
        if gu.shape[0] != dn.shape[0] or gu.shape[2] != dn.shape[1] or gu.shape[1] != 2 * dn.shape[2]:
            raise ValueError(f"MoEGatedMLP.from_stacked: expected gate_up_proj [E, 2 I, H] and down_proj [E, H, I]{' (stored transposed)' if transposed else ''}, "
                             f"got {tuple(gate_up_proj.shape)} and {tuple(down_proj.shape)}")
        for b, n, what in ((gub, gu.shape[1], "gate_up_bias"), (dnb, dn.shape[1], "down_bias")):
            if b is not None and tuple(b.shape) != (gu.shape[0], n):
                raise ValueError(f"MoEGatedMLP.from_stacked: {what} must be [E, {n}], got {tuple(b.shape)}")
        return cls(GroupedQLinear.from_weight(gu, gub), GroupedQLinear.from_weight(dn, dnb), gate_kind, gate_limit, gate_alpha)

    def forward(self, hidden: torch.Tensor, topk_ids: torch.Tensor, topk_weights: torch.Tensor) -> torch.Tensor:
        H = hidden.shape[-1]
        x2 = hidden.reshape(-1, H)
        T = x2.shape[0]
        ids, w = topk_ids.reshape(T, -1), topk_weights.reshape(T, -1)
        inter = self.down.in_features
        xq = quantize(x2, axis=-1)                                     # ONE quantisation for all experts
        if self.torch_plumbing:
            row_index, offsets, rows_of, slot_of = route_plan(ids, self.num_experts)
            xs = None                                                  # (gathered by GroupedQLinear.forward: an index_select)
        else:
            row_index, offsets, rows_of, slot_of, xs = moe_route(ids, self.num_experts, xs=xq.scale.reshape(-1))
        gu = self.gate_up(xq, offsets, row_index, xs)                  # [T k, 2 I]: the codes are read where the tokens lie
        if self.gate_kind == "silu":
            h = silu_mul_quantize(gu[:, :inter], gu[:, inter:])        # sorted rows: int8 codes + row scales
        else:
            h = glu_quantize(gu[:, :inter], gu[:, inter:], self.gate_kind, self.gate_limit, self.gate_alpha)
        y = self.down(h, offsets)
        if self.torch_plumbing:
            return combine(y, rows_of, slot_of, w).reshape(hidden.shape)
        return moe_combine(y, rows_of, slot_of, w).reshape(hidden.shape)

    def extra_repr(self):
        if self.gate_kind == "silu":
            return "gate_kind=silu"
        return f"gate_kind={self.gate_kind}, gate_limit={self.gate_limit}" + (f", gate_alpha={self.gate_alpha}" if self.gate_alpha is not None else "")


class MoEBlock(nn.Module):
    """What swap_moe_experts puts in place of a sparse MoE block: the block's own router (`gate`) and routing recipe — softmax over the experts in f32, top-k,
    optional renormalisation, weights cast to the hidden dtype — in front of MoEGatedMLP.
    hip_routing = True (set per instance by fuse_moe_routers) runs that recipe as ONE moe_topk launch whose int32 ids go straight into moe_route; the softmax is then the
    specified one (QSPEC RT3), close to eager's but not its bits."""

    hip_routing = False

    def __init__(self, gate: nn.Module, experts: MoEGatedMLP, top_k: int, renormalise: bool, return_router_logits: bool):
        super().__init__()
        self.gate, self.experts = gate, experts
        self.top_k, self.renormalise, self.return_router_logits = top_k, renormalise, return_router_logits

    def forward(self, hidden_states: torch.Tensor):
        x2 = hidden_states.reshape(-1, hidden_states.shape[-1])
        router_logits = self.gate(x2)
        if self.hip_routing:
            weights, selected = moe_topk(router_logits, self.top_k, "softmax_topk", self.renormalise, out_dtype=hidden_states.dtype, ids_dtype=torch.int32)
            out = self.experts(x2, selected, weights).reshape(hidden_states.shape)
            return (out, router_logits) if self.return_router_logits else out
        weights = torch.softmax(router_logits, dim=1, dtype=torch.float)
        weights, selected = torch.topk(weights, self.top_k, dim=-1)
        if self.renormalise:
            weights = weights / weights.sum(dim=-1, keepdim=True)
        out = self.experts(x2, selected, weights.to(hidden_states.dtype)).reshape(hidden_states.shape)
        return (out, router_logits) if self.return_router_logits else out


_EXPERT_NAMES = (("gate_proj", "up_proj", "down_proj"), ("w1", "w3", "w2"))


def _expert_linears(mod: nn.Module):
    """(gate, up, down) of a gated expert MLP with a silu — Llama-style names or Mixtral's w1 / w3 / w2 — or None"""
    for names in _EXPERT_NAMES:
        g, u, d = (getattr(mod, n, None) for n in names)
        if all(is_plain_linear(l) for l in (g, u, d)):
            if not _is_silu(getattr(mod, "act_fn", None)) or len(list(mod.children())) > 4:
                return None
            if g.in_features != u.in_features or g.out_features != u.out_features or d.in_features != g.out_features or d.out_features != g.in_features:
                return None
            if (g.bias is None) != (u.bias is None):
                return None
            return g, u, d
    return None


def moe_block_parts(mod: nn.Module):
    """A module shaped like a sparse MoE block — exactly two children, a ModuleList `experts` of gated silu MLPs of one shape and a Linear router `gate` with one
    output per expert, and a top-k count among its attributes — as (experts' linears, top_k, renormalise, return_router_logits); else None.  Recognised by shape,
    not by import (no dependency on transformers)."""
    experts, gate = getattr(mod, "experts", None), getattr(mod, "gate", None)
    if not isinstance(experts, nn.ModuleList) or len(experts) == 0 or not is_plain_linear(gate) or gate.out_features != len(experts):
        return None
    if {n for n, _ in mod.named_children()} != {"experts", "gate"}:
        return None                                   # (shared experts, gates on the shared path, ...: not this block)
    top_k = getattr(mod, "top_k", None)
    if top_k is None:
        top_k = getattr(mod, "num_experts_per_tok", None)
    if not isinstance(top_k, int) or not 1 <= top_k <= len(experts):
        return None
    lins = [_expert_linears(e) for e in experts]
    if any(l is None for l in lins) or any(l[0].weight.shape != lins[0][0].weight.shape or (l[2].bias is None) != (lins[0][2].bias is None) or
                                           (l[0].bias is None) != (lins[0][0].bias is None) for l in lins):
        return None
    # Mixtral renormalises the top-k weights always; Qwen-MoE-style blocks say so in norm_topk_prob
    renorm = bool(getattr(mod, "norm_topk_prob", True))
    returns_logits = bool(getattr(mod, "return_router_logits", type(mod).__name__.endswith("SparseMoeBlock")))
    return lins, top_k, renorm, returns_logits


class FusedExperts(NamedTuple):
    """What fused_experts_parts reports of an experts module it recognises.  Only ONE layout is recognised, so the last three fields are fixed by it — no bias, gate rows
    first; a module with biases or another order is refused, not reported with other values.  They are spelled out because they are what the caller relies on
    (prepare_for_int8 sizes the receiving module from them) and what tests/test_moe_model_recognition.py checks against the module's own forward."""
    num_experts: int
    hidden: int
    intermediate: int
    gate_up_bias: bool
    down_bias: bool
    gate_first: bool          # rows 0 .. I - 1 of gate_up_proj[e] are the gate (the argument of the silu), rows I .. 2 I - 1 the up projection


_FUSED_FLAGS = (("has_gate", True), ("has_bias", False), ("is_transposed", False), ("is_concatenated", True))


def fused_experts_parts(mod: nn.Module):
    """A module that holds the routed experts of a sparse MoE block as two stacked parameters and is called as mod(hidden[T, H], top_k_index[T, k], top_k_weights[T, k])
    — transformers 5's MixtralExperts, Qwen2MoeExperts / Qwen3MoeExperts, OlmoeExperts, DeepseekV3Experts, PhimoeExperts, GraniteMoeExperts — as FusedExperts; else None.
    (Refused among the classes of transformers 5.15: GptOssExperts, DeepseekV4Experts, and every other class with a gate, a bias or a storage order of its own.)
    MoEGatedMLP.forward has that signature and that arithmetic, so such a module is replaced alone: whatever produces the indices and the weights (softmax or sigmoid,
    grouped top-k, sparsemixer), shared experts and the block's return value stay the model's code.  Recognised by shape and attributes, not by import.  Every part of
    the module's arithmetic must be the library's, so anything else about it refuses it:
      * parameters other than gate_up_proj [E, 2 I, H] and down_proj [E, H, I] (biases: GPT-OSS), buffers, child modules other than the activation
      * an act_fn that is missing or not a silu (GPT-OSS has none: its clamped alpha-sigmoid gate is a method), a gate_up_proj stored [E, H, 2 I] or with interleaved gate /
        up columns: where the two shapes coincide (H = 2 I) the flags the model code sets on its experts classes decide (is_transposed, is_concatenated, has_bias, has_gate)
      * a gate of the class's own: transformers routes every gate that is not act_fn(gate) * up through a method `_apply_gate` of the experts class (its decorator
        installs `_default_apply_gate` where the class has none) — DeepSeek-V4's experts have the shapes, the silu, the flags and the signature of Mixtral's and clamp
        gate and up to +-swiglu_limit in theirs — so a class whose `_apply_gate` is not that default is refused
      * a forward whose positional arguments are not (hidden, indices, weights) in that order, judged by substrings of their names.  That last check is a guard against a
        swapped argument ORDER only; it is no evidence of the arithmetic (GPT-OSS's names pass it).
    What attributes cannot show — a forward that writes another arithmetic inline — is not detected here."""
    if isinstance(mod, (nn.ModuleList, MoEGatedMLP)):
        return None
    own_gate = getattr(type(mod), "_apply_gate", None)
    if own_gate is not None and getattr(own_gate, "__name__", "") != "_default_apply_gate":
        return None
    params, act = dict(mod.named_parameters(recurse=False)), getattr(mod, "act_fn", None)
    if set(params) != {"gate_up_proj", "down_proj"} or list(mod.named_buffers(recurse=False)) or not _is_silu(act):
        return None
    if any(c is not act for c in mod.children()):
        return None
    gu, dn = params["gate_up_proj"], params["down_proj"]
    if gu.dim() != 3 or dn.dim() != 3 or not gu.is_floating_point() or gu.dtype != dn.dtype:
        return None
    E, H, I = gu.shape[0], gu.shape[2], dn.shape[2]
    if E < 1 or tuple(gu.shape) != (E, 2 * I, H) or tuple(dn.shape) != (E, H, I):
        return None
    if any(getattr(mod, flag, want) is not want for flag, want in _FUSED_FLAGS):
        return None
    if any(isinstance(getattr(mod, n, E), int) and getattr(mod, n, E) != E for n in ("num_experts", "num_local_experts")):
        return None
    try:
        names = [p.name.lower() for p in inspect.signature(type(mod).forward).parameters.values() if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)][1:]
    except (TypeError, ValueError):
        return None
    if len(names) != 3 or not any(t in names[1] for t in ("ind", "idx", "ids")) or not any(t in names[2] for t in ("weight", "score", "prob")):
        return None
    return FusedExperts(E, H, I, False, False, True)


class ClampedExperts(NamedTuple):
    """What clamped_experts_parts reports of an experts module whose gate is one of the two clamped kinds: the shapes, which biases it has, how the parameters are
    stored (standard_stacked turns them into the library's order) and the gate (MoEGatedMLP's gate_kind / gate_limit / gate_alpha)."""
    num_experts: int
    hidden: int
    intermediate: int
    gate_up_bias: bool
    down_bias: bool
    transposed: bool          # gate_up_proj is [E, H, 2 I], down_proj [E, I, H]: y = x @ W[e]
    interleaved: bool         # gate / up alternate along the output axis of gate_up_proj (and of its bias) instead of lying in two halves
    gate_kind: str            # "clamped_silu" | "alpha_sigmoid"
    limit: float
    alpha: float | None


def _probe_gate(mod: nn.Module, interleaved: bool, kind: str, limit: float, alpha) -> bool:
    """Attributes cannot prove what an _apply_gate computes: run the module's own on a small fixed CPU tensor — gate and up values inside and beyond +-limit, both
    signs, laid out as the module is claimed to read them — and compare with the float64 restatement of the claimed kind."""
    base = torch.tensor([-3.0, -1.5, -1.0, -0.6, -0.1, 0.0, 0.3, 0.9, 1.0, 1.25, 2.0, 4.0], dtype=torch.float64) * limit
    g = torch.stack([base, base.flip(0) * 0.7, base * 0.31])
    u = torch.stack([base.roll(5), base * 0.45, base.flip(0) * 1.1])
    packed = torch.stack([g, u], dim=-1).reshape(3, -1) if interleaved else torch.cat([g, u], dim=-1)
    gc, uc = g.clamp(max=limit), u.clamp(min=-limit, max=limit)
    want = gc * torch.sigmoid(gc) * uc if kind == "clamped_silu" else (uc + 1) * (gc * torch.sigmoid(alpha * gc))
    try:
        with torch.no_grad():
            got = mod._apply_gate(packed)
    except Exception:
        return False
    return isinstance(got, torch.Tensor) and got.shape == want.shape and bool(torch.allclose(got.to(torch.float64), want, rtol=1e-9, atol=1e-12))


def clamped_experts_parts(mod: nn.Module):
    """A fused-parameter experts module (called as mod(hidden[T, H], indices[T, k], weights[T, k]), as fused_experts_parts describes) whose gate is a method
    `_apply_gate` of its class and computes one of the two clamped gates MoEGatedMLP serves — transformers 5's GptOssExperts ("alpha_sigmoid": parameters stored
    [E, in, out], gate / up in alternating columns, biases) and DeepseekV4Experts ("clamped_silu": Mixtral's storage) — as ClampedExperts; else None, and None for every
    module fused_experts_parts accepts.  Recognised by shapes, parameter names, the flags model code sets on its experts classes (is_transposed, is_concatenated,
    has_bias) and the attributes `limit` / `alpha`, never by import; and since attributes do not say what the gate computes, the module's own _apply_gate is probed
    (_probe_gate): a class that clamps differently, uses another alpha than it states or adds no 1 to `up` is refused."""
    if isinstance(mod, (nn.ModuleList, MoEGatedMLP)) or fused_experts_parts(mod) is not None:
        return None
    own_gate = getattr(type(mod), "_apply_gate", None)
    if own_gate is None or getattr(own_gate, "__name__", "") == "_default_apply_gate":
        return None
    params, act = dict(mod.named_parameters(recurse=False)), getattr(mod, "act_fn", None)
    has_bias = getattr(mod, "has_bias", False)
    names = {"gate_up_proj", "down_proj"} | ({"gate_up_proj_bias", "down_proj_bias"} if has_bias is True else set())
    if has_bias not in (True, False) or set(params) != names or list(mod.named_buffers(recurse=False)) or any(c is not act for c in mod.children()):
        return None
    transposed, concatenated = getattr(mod, "is_transposed", False), getattr(mod, "is_concatenated", True)
    if transposed not in (True, False) or concatenated not in (True, False) or getattr(mod, "has_gate", True) is not True:
        return None
    gu, dn = params["gate_up_proj"], params["down_proj"]
    if gu.dim() != 3 or dn.dim() != 3 or not gu.is_floating_point() or any(p.dtype != gu.dtype for p in params.values()):
        return None
    E = gu.shape[0]
    H, I = (gu.shape[1], dn.shape[1]) if transposed else (gu.shape[2], dn.shape[2])
    if E < 1 or tuple(gu.shape) != ((E, H, 2 * I) if transposed else (E, 2 * I, H)) or tuple(dn.shape) != ((E, I, H) if transposed else (E, H, I)):
        return None
    if has_bias and (tuple(params["gate_up_proj_bias"].shape) != (E, 2 * I) or tuple(params["down_proj_bias"].shape) != (E, H)):
        return None
    if any(isinstance(getattr(mod, n, E), int) and getattr(mod, n, E) != E for n in ("num_experts", "num_local_experts")):
        return None
    limit, alpha = getattr(mod, "limit", None), getattr(mod, "alpha", None)
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and -float("inf") < v < float("inf")      # noqa: E731
    if not number(limit) or limit <= 0 or (alpha is not None and not number(alpha)):
        return None
    kind = "alpha_sigmoid" if alpha is not None else "clamped_silu"
    if (kind == "clamped_silu") != _is_silu(act):              # DeepSeek-V4's silu is its act_fn; GPT-OSS has none (its sigmoid is written in the method)
        return None
    try:
        sig = [p.name.lower() for p in inspect.signature(type(mod).forward).parameters.values() if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)][1:]
    except (TypeError, ValueError):
        return None
    if len(sig) != 3 or not any(t in sig[1] for t in ("ind", "idx", "ids")) or not any(t in sig[2] for t in ("weight", "score", "prob")):
        return None
    if not _probe_gate(mod, not concatenated, kind, float(limit), None if alpha is None else float(alpha)):
        return None
    return ClampedExperts(E, H, I, has_bias, has_bias, transposed, not concatenated, kind, float(limit), None if alpha is None else float(alpha))


def swap_moe_experts(model: nn.Module, gates=("silu",)) -> int:
    """Replace, in place, the routed experts of every sparse MoE block of the model: a fused-parameter experts module (fused_experts_parts) by MoEGatedMLP, a block in the
    ModuleList layout (moe_block_parts) by MoEBlock.  The experts' weights are quantised per output channel, the router stays what it was.  Returns the number of
    blocks whose experts were replaced (0: a dense model, or a layout that is refused, is left untouched — the very same module objects).
    gates: the gate kinds to swap — "silu" (the default: the layouts above), "clamped_silu" (DeepSeek-V4) and "alpha_sigmoid" (GPT-OSS), recognised by
    clamped_experts_parts and swapped only when named; "all" names all three."""
    kinds = _gate_kinds(gates)
    n = 0
    for name, child in list(model.named_children()):
        parts = moe_block_parts(child) if "silu" in kinds else None
        clamped = clamped_experts_parts(child) if parts is None and len(kinds) > ("silu" in kinds) else None
        if parts is not None:
            lins, top_k, renorm, returns_logits = parts
            setattr(model, name, MoEBlock(child.gate, MoEGatedMLP.from_experts(lins), top_k, renorm, returns_logits))
            n += 1
        elif "silu" in kinds and fused_experts_parts(child) is not None:
            setattr(model, name, MoEGatedMLP.from_stacked(child.gate_up_proj.detach(), child.down_proj.detach()))
            n += 1
        elif clamped is not None and clamped.gate_kind in kinds:
            bias = (child.gate_up_proj_bias.detach(), child.down_proj_bias.detach()) if clamped.gate_up_bias else (None, None)
            setattr(model, name, MoEGatedMLP.from_stacked(child.gate_up_proj.detach(), child.down_proj.detach(), *bias, transposed=clamped.transposed,
                                                          interleaved=clamped.interleaved, gate_kind=clamped.gate_kind, gate_limit=clamped.limit, gate_alpha=clamped.alpha))
            n += 1
        else:
            n += swap_moe_experts(child, kinds)
    return n
