"""Hadamard-rotated int8 linear layers: x W^T = (x R)(W R)^T for an orthogonal R.  With R = diag(H_B, .., H_B) / sqrt(B), a block-diagonal normalised Hadamard matrix,
one outlier channel of an activation row is spread over its whole block of B elements BEFORE the per-token quantiser spends its 255 levels on the row's largest element;
the weight is rotated once, when the layer is swapped.  Calibration-free and exact in real arithmetic (no statistics are collected: this is not PTQ calibration).

    hadamard(x, block)            the rotation alone (kernel K1h, transform-only form)
    hadamard_quantize(x, block)   the rotation and the per-token quantisation in ONE pass (K1h) — quantize(hadamard(x)) bit for bit (QSPEC H1-H5)
    gated_hadamard_quantize(g, u, act, block)   the gated activation of an MLP, its rotation and its quantisation in ONE pass (K1gh) — hadamard_quantize of
                                  silu_mul_quantize's / gelu_mul_quantize's h, bit for bit (QSPEC GH1)
    RotatedQLinear                a qlinear whose weight is rotated and whose forward rotates + quantises its input with hadamard_quantize; forward_rotated takes
                                  codes of the rotated activation (gated_hadamard_quantize's)
    rotate_linears(model, ..)     opt-in: chosen nn.Linear -> RotatedQLinear
    rotate_gated_mlps(model, ..)  opt-in: a Llama-shaped MLP -> GatedMLP(fused gate+up, RotatedQLinear down): gate+up GEMM -> K1gh -> down GEMM

Call order: rotate_gated_mlps (whole MLPs whose down_proj is to be rotated) and / or rotate_linears (single layers) first; then swap_linears for the rest; then the
fuse_* entries.  Those leave a RotatedQLinear alone (qlinear.is_code_fed): its input is NOT taken into a fused producer.  What stays unfused: a down_proj rotated by
rotate_linears alone (not as part of a GatedMLP) gets the stock MLP's float activation and runs K1h itself, rotated q/k/v projections are not fused into one GEMM, and a
norm in front of a rotated projection stays the eager norm.  A GatedMLP built by rotate_gated_mlps has no torch arithmetic inside: fuse_llama_layers accepts it as it
accepts every GatedMLP, so both norms of the layer still fuse.  There is no CPU path.  Out of scope: rotating the residual stream offline, an RMSNorm / LayerNorm
producer in front of rotated gate/up or q/k/v projections (its pinned summation order is tied to K1n's layout), fuse_gemma_layers recognising a rotated GeGLU (the
gelu_tanh kind is reachable through gated_hadamard_quantize and a hand-built GatedMLP(act="gelu_tanh") only), the clamped MoE gates and GroupedQLinear,
non-power-of-two Hadamard factors, the sharded modules, convert_checkpoint."""
from __future__ import annotations

import torch
from torch import nn

from . import _lib as L
from .qlinear import FusedQLinear, GatedMLP, _is_silu, is_plain_linear, qlinear
from .qtensor import QTensor, _alloc, _check_match, _check_out, _launch, _on_gpu, _pack, _ptr, _rows_view, _rows_view_of_out, quantize

MIN_BLOCK, MAX_BLOCK = 16, 4096


def default_block(cols: int) -> int:
    """the largest power of two that divides cols, at most 4096"""
    return min(MAX_BLOCK, cols & -cols)


def _block_of(what: str, cols: int, block) -> int:
    if block is None:
        block = default_block(cols) if cols > 0 else MIN_BLOCK
    if isinstance(block, bool) or not isinstance(block, int):
        raise TypeError(f"{what}: block must be an int or None, got {type(block).__name__}")
    if block < MIN_BLOCK or block > MAX_BLOCK or block & (block - 1):
        raise ValueError(f"{what}: block must be a power of two, {MIN_BLOCK} .. {MAX_BLOCK}, got {block}")
    if cols % block:
        raise ValueError(f"{what}: block {block} does not divide the last dimension {cols}")
    return block


def hadamard(x: torch.Tensor, block: int | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Every block of `block` consecutive elements of the last axis of x times the normalised Hadamard matrix H_block / sqrt(block), in ONE kernel (K1h, the transform-only
    form): f32 butterflies in ascending stride, one scaling, one rounding to x's dtype (QSPEC H1-H4).  block=None: min(4096, the largest power of two dividing the last
    dimension); a block below 16, no power of two, or not dividing the last dimension is a ValueError.  The leading axes are collapsed as quantize collapses them; `out`
    (optional, x's shape and dtype) receives the result and may not overlap x.  Returns a tensor of x's shape."""
    what = "hadamard"
    _on_gpu(what, x=x)
    if x.dim() < 1:
        raise ValueError(f"{what}: x needs at least 1 dimension")
    _check_out(what, out, x)
    code = L.dtype_code(x.dtype)
    block = _block_of(what, x.shape[-1], block)
    x2 = _rows_view(x)
    rows, cols = x2.shape
    h = torch.empty(x.shape, dtype=x.dtype, device=x.device) if out is None else out
    h2 = _rows_view_of_out(h, rows, cols, what)
    if rows == 0 or cols == 0:
        return h
    _launch(what, x.device, L.lib().pq_hadamard_quant_rows, x2.data_ptr(), code, rows, cols, L.ld(x2), block, None, 0, None, h2.data_ptr(), L.ld(h2), L.stream_ptr(x))
    return h


def hadamard_quantize(x: torch.Tensor, block: int | None = None, return_h: bool = False):
    """quantize(hadamard(x, block), axis=-1) in ONE pass (kernel K1h): the rotated activation is transformed, reduced and encoded in registers and LDS and never goes to
    HBM in the input dtype — the traffic of quantize itself.  Codes and scales are those of the two-step form bit for bit (QSPEC H1-H5: Q1-Q6 on h as stored).
    return_h=True also returns h = hadamard(x, block) (stored by the same kernel).  `block` as hadamard."""
    what = "hadamard_quantize"
    _on_gpu(what, x=x)
    if x.dim() < 1:
        raise ValueError(f"{what}: x needs at least 1 dimension")
    code = L.dtype_code(x.dtype)
    block = _block_of(what, x.shape[-1], block)
    x2 = _rows_view(x)
    rows, cols = x2.shape
    q, scale, h = _alloc(rows, cols, x, return_h, host_ones_when_empty=True)
    _launch(what, x.device, L.lib().pq_hadamard_quant_rows, x2.data_ptr(), code, rows, cols, L.ld(x2), block, q.data_ptr(), max(cols, 1), scale.data_ptr(), _ptr(h),
            max(cols, 1), L.stream_ptr(x))
    return _pack(x, q, scale, h)


def gated_hadamard_quantize(g: torch.Tensor, u: torch.Tensor, act: str = "silu", block: int | None = None, return_h: bool = False):
    """hadamard_quantize(h0, block) for h0 = the gated activation of g and u as stored — act "silu": silu_mul_quantize's h (QSPEC S1-S5), "gelu_tanh": gelu_mul_quantize's
    (GG1-GG3) — in ONE pass (kernel K1gh): h0 is computed in registers in front of K1h's first LDS pass and never goes to HBM.  Codes and scales are those of the
    two-launch composition bit for bit (QSPEC GH1).  g and u have the same shape and dtype and may be the column halves of one fused gate+up output.  return_h=True also
    returns the ROTATED activation hadamard(h0, block) (stored by the same kernel; h0 itself is never stored).  `block` as hadamard."""
    what = "gated_hadamard_quantize"
    _on_gpu(what, g=g, u=u)
    if act not in L.GATE_KINDS:
        raise ValueError(f"{what}: unknown act {act!r}, expected one of {sorted(L.GATE_KINDS)}")
    _check_match(what, "g", g, "u", u, devices=False)
    code = L.dtype_code(g.dtype)
    block = _block_of(what, g.shape[-1], block)
    g2, u2 = _rows_view(g), _rows_view(u)
    rows, cols = g2.shape
    q, scale, h = _alloc(rows, cols, g, return_h, host_ones_when_empty=True)
    _launch(what, g.device, L.lib().pq_gated_hadamard_quant_rows, g2.data_ptr(), L.ld(g2), u2.data_ptr(), L.ld(u2), code, rows, cols, L.GATE_KINDS[act], block, q.data_ptr(),
            max(cols, 1), scale.data_ptr(), _ptr(h), max(cols, 1), L.stream_ptr(g))
    return _pack(g, q, scale, h)


class RotatedQLinear(qlinear):
    """A qlinear on the rotated problem: `wq` / `ws` hold the per-channel quantisation of W R (R = diag(H_block) / sqrt(block) along in_features) and forward quantises
    x R with hadamard_quantize, so y approximates x W^T as qlinear does, with the outlier channels of x spread over their blocks first.  The block lives in the persistent
    int64 buffer `rot_block` (state_dict / load_state_dict / torch.save round-trip).  A QTensor input is refused: its codes are not rotated."""

    code_fed = False          # (qlinear.is_code_fed: no other producer's codes fit the rotated weight)

    def __init__(self, in_features: int, out_features: int, bias: bool = True, device=None, dtype=None, block: int | None = None):
        super().__init__(in_features, out_features, bias, device, dtype)
        self.register_buffer("rot_block", torch.tensor(_block_of("RotatedQLinear", in_features, block), dtype=torch.int64, device=device))

    @classmethod
    def from_linear(cls, lin: nn.Linear, block: int | None = None) -> "RotatedQLinear":
        """lin.weight [N, K] rotated along K in f32 (its rows run along K: the activation's kernel), cast to the weight dtype, then quantised per output channel as
        qlinear.from_linear quantises it."""
        w = lin.weight.detach()
        L.require_gpu(w, "RotatedQLinear.from_linear(weight)")
        block = _block_of("RotatedQLinear.from_linear", lin.in_features, block)
        m = cls.__new__(cls)
        nn.Module.__init__(m)
        m.in_features, m.out_features = lin.in_features, lin.out_features
        qw = quantize(hadamard(w.float(), block).to(w.dtype), axis=-1)
        m.register_buffer("wq", qw.int_data)
        m.register_buffer("ws", qw.scale)
        if lin.bias is not None:
            m.register_buffer("bias", lin.bias.detach().clone())
        else:
            m.bias = None
        m.register_buffer("rot_block", torch.tensor(block, dtype=torch.int64, device=w.device))
        m.__dict__["_block"], m.__dict__["_block_key"] = block, (m.rot_block._version, m.rot_block.data_ptr())      # (known here: forward reads no device value)
        return m

    @property
    def block(self) -> int:
        """the rotation block as a Python int; read from `rot_block` once (a device read) and again after load_state_dict replaced the buffer's contents"""
        key = (self.rot_block._version, self.rot_block.data_ptr())
        if self.__dict__.get("_block_key") != key or self.__dict__.get("_block") is None:
            self.__dict__["_block"] = int(self.rot_block.item())
            self.__dict__["_block_key"] = key
        return self.__dict__["_block"]

    def forward(self, x) -> torch.Tensor:
        if isinstance(x, QTensor):
            raise TypeError("RotatedQLinear: a QTensor input is refused — its codes are those of the unrotated activation; pass the float tensor")
        if x.shape[-1] != self.in_features:
            raise ValueError(f"RotatedQLinear: expected last dim {self.in_features}, got {x.shape[-1]}")
        return super().forward(hadamard_quantize(x, self.block))

    def forward_rotated(self, xq: QTensor) -> torch.Tensor:
        """the GEMM alone on a per-token QTensor that the caller DECLARES to hold codes of the rotated activation x R with this layer's block (gated_hadamard_quantize's,
        hadamard_quantize's): nothing here can tell them from other codes"""
        if not isinstance(xq, QTensor):
            raise TypeError("RotatedQLinear.forward_rotated: expected a per-token QTensor of the rotated activation; forward takes the float tensor")
        return super().forward(xq)

    def extra_repr(self):
        return f"{super().extra_repr()}, rot_block={self.__dict__.get('_block', '?')}"


def rotate_linears(model: nn.Module, predicate=None, block: int | None = None) -> int:
    """Replace every nn.Linear of `model` (in place) that is_plain_linear admits and for which predicate(name, module) is true (None: all) by a RotatedQLinear of `block`
    (None: per layer, the largest power of two dividing its in_features, at most 4096); returns the number replaced.  `name` is the child's name in its parent, as in
    swap_linears.  A module that already is a qlinear (a RotatedQLinear included) is never touched, and neither is a layer whose in_features no block of at least 16
    divides.  Opt-in; call it BEFORE swap_linears (which then takes the remaining nn.Linear layers) and the fuse_* entries."""
    n = 0
    for name, child in list(model.named_children()):
        if isinstance(child, qlinear):
            continue
        if is_plain_linear(child) and (predicate is None or predicate(name, child)):
            b = default_block(child.in_features) if block is None else block
            if b >= MIN_BLOCK and child.in_features % b == 0:
                setattr(model, name, RotatedQLinear.from_linear(child, b))
                n += 1
        else:
            n += rotate_linears(child, predicate, block)
    return n


def _rotatable_mlp(mod: nn.Module, block):
    """qlinear._as_gated_mlp's conditions (plain nn.Linear gate_proj / up_proj / down_proj, a SiLU act_fn, matching widths, gate and up both with or both without a
    bias) and a legal block for the intermediate width: that block, or None"""
    g, u, d = (getattr(mod, n, None) for n in ("gate_proj", "up_proj", "down_proj"))
    if not all(is_plain_linear(l) for l in (g, u, d)) or not _is_silu(getattr(mod, "act_fn", None)):
        return None
    if g.in_features != u.in_features or g.out_features != u.out_features or d.in_features != g.out_features or (g.bias is None) != (u.bias is None):
        return None
    b = default_block(d.in_features) if block is None else block
    return b if b >= MIN_BLOCK and d.in_features % b == 0 else None


def rotate_gated_mlps(model: nn.Module, predicate=None, block: int | None = None) -> int:
    """Replace every Llama-shaped MLP of `model` (in place) — what swap_linears(fuse_gated_mlp=True) would take — for which predicate(name, module) is true (None: all) and
    whose intermediate width has a legal block (`block`, or None: the largest power of two dividing it, at most 4096, at least 16) by
    GatedMLP(FusedQLinear.from_linears(gate, up), RotatedQLinear.from_linear(down, block)): one fused gate+up GEMM, K1gh (silu * mul, the rotation and the quantisation in
    one launch), the down GEMM on the rotated weight.  Anything else is left untouched, object for object; returns the number replaced (a second call: 0).  Opt-in; call
    it BEFORE swap_linears (which takes the remaining nn.Linear layers) and the fuse_* entries, as rotate_linears."""
    n = 0
    for name, child in list(model.named_children()):
        b = _rotatable_mlp(child, block) if predicate is None or predicate(name, child) else None
        if b is not None:
            L.require_gpu(child.down_proj.weight, "rotate_gated_mlps(down_proj.weight)")      # (before anything is built: a CPU model is refused with the model unchanged)
            setattr(model, name, GatedMLP(FusedQLinear.from_linears(child.gate_proj, child.up_proj), RotatedQLinear.from_linear(child.down_proj, b)))
            n += 1
        elif not isinstance(child, (qlinear, GatedMLP)):
            n += rotate_gated_mlps(child, predicate, block)
    return n
