"""Hadamard-rotated int8 linear layers: x W^T = (x R)(W R)^T for an orthogonal R.  With R = diag(H_B, .., H_B) / sqrt(B), a block-diagonal normalised Hadamard matrix,
one outlier channel of an activation row is spread over its whole block of B elements BEFORE the per-token quantiser spends its 255 levels on the row's largest element;
the weight is rotated once, when the layer is swapped.  Calibration-free and exact in real arithmetic (no statistics are collected: this is not PTQ calibration).

    hadamard(x, block)            the rotation alone (kernel K1h, transform-only form)
    hadamard_quantize(x, block)   the rotation and the per-token quantisation in ONE pass (K1h) — quantize(hadamard(x)) bit for bit (QSPEC H1-H5)
    RotatedQLinear                a qlinear whose weight is rotated and whose forward rotates + quantises its input with hadamard_quantize
    rotate_linears(model, ..)     opt-in: chosen nn.Linear -> RotatedQLinear

Call order: rotate_linears first, for the chosen layers (typically down_proj, whose input carries the outlier channels); then swap_linears for the rest; then the fuse_*
entries.  Those leave a RotatedQLinear alone (qlinear.is_code_fed): its input is NOT taken into a fused producer — a rotated down_proj gets the stock MLP's float
activation and runs K1h itself (silu_mul_quantize cannot feed it), rotated q/k/v projections are not fused into one GEMM, and a norm in front of a rotated projection
stays the eager norm.  There is no CPU path.  Out of scope: rotating the residual stream offline, fusing the rotation into the norm / activation producers,
non-power-of-two Hadamard factors, the sharded modules, GroupedQLinear, convert_checkpoint."""
from __future__ import annotations

import torch
from torch import nn

from . import _lib as L
from .qlinear import is_plain_linear, qlinear
from .qtensor import QTensor, _alloc, _check_out, _launch, _on_gpu, _pack, _ptr, _rows_view, _rows_view_of_out, quantize

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
