"""QTensor + quantize()/dequantize(): the Python surface BASELINE.json's north_star names.

The reference's own definitions are absent from the mount (/root/reference holds only
CODE_OF_CONDUCT.md:1-80), so signatures are build-defined and numerics follow
QSPEC v2.  All arithmetic happens in libpq_hip.so (HIP, gfx950)."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _lib as L


@dataclass
class QTensor:
    """Dynamic symmetric int8 tensor: `int_data` (int8, original shape), `scale` (fp32, one per
    kept index), `axis` = the reduced (quantised-over) axis of the 2-D view, `orig_dtype`."""
    int_data: torch.Tensor
    scale: torch.Tensor
    axis: int
    orig_dtype: torch.dtype
    shape: torch.Size

    def dequantize(self, dtype: torch.dtype | None = None) -> torch.Tensor:
        return dequantize(self, dtype)

    @property
    def device(self):
        return self.int_data.device

    def to(self, device) -> "QTensor":
        return QTensor(self.int_data.to(device), self.scale.to(device), self.axis, self.orig_dtype, self.shape)

    def __repr__(self):
        return (f"QTensor(shape={tuple(self.shape)}, axis={self.axis}, orig_dtype={self.orig_dtype}, "
                f"device={self.int_data.device})")


def _as_2d(x: torch.Tensor, axis: int):
    """Collapse x to the 2-D matrix whose reduced axis is `axis` (last -> rows x cols reduce over
    cols; first of a 2-D tensor -> reduce over rows)."""
    nd = x.dim()
    if nd == 0:
        raise ValueError("quantize() needs at least 1 dimension")
    a = axis % nd
    if a == nd - 1:
        lead = 1
        for d in x.shape[:-1]:
            lead *= d
        return x.reshape(lead, x.shape[-1]), 1
    if nd == 2 and a == 0:
        return x, 0
    raise ValueError("quantize(): axis must be the last axis, or axis 0 of a 2-D tensor")


def quantize(x: torch.Tensor, axis: int = -1) -> QTensor:
    """Dynamic symmetric int8 quantisation. axis=-1: per-token (one scale per row of the flattened
    [..., C] tensor, kernel K1); axis=0 on a 2-D tensor: per-channel along the strided axis (K2)."""
    L.require_gpu(x, "quantize(x)")
    code = L.dtype_code(x.dtype)
    x2, red = _as_2d(x, axis)
    x2 = L.row_major_2d(x2)
    rows, cols = x2.shape
    q = torch.empty((rows, cols), dtype=torch.int8, device=x.device)
    scale = torch.empty((rows if red == 1 else cols,), dtype=torch.float32, device=x.device)
    fn = L.lib().pq_quant_rowwise if red == 1 else L.lib().pq_quant_colwise
    with torch.cuda.device(x.device):
        L.check(fn(x2.data_ptr(), code, rows, cols, L.ld(x2), q.data_ptr(), max(cols, 1), scale.data_ptr(),
                   L.stream_ptr(x)), "quantize")
    return QTensor(q.reshape(x.shape), scale, red, x.dtype, x.shape)


def _rows_view(t: torch.Tensor) -> torch.Tensor:
    """[..., C] -> a 2-D [rows, C] view with unit column stride (column slices of a wider matrix stay views)."""
    lead = 1
    for d in t.shape[:-1]:
        lead *= d
    t2 = t if t.dim() == 2 else t.reshape(lead, t.shape[-1])
    return L.row_major_2d(t2)


def silu_mul_quantize(g: torch.Tensor, u: torch.Tensor, return_h: bool = False):
    """quantize(F.silu(g) * u, axis=-1) in ONE pass (kernel K1 fused into its producer): the activation of a gated
    MLP's down projection is computed, reduced and encoded in registers and never goes to HBM in bf16.
    g and u may be column slices of one fused gate+up output.  Numerics: QSPEC S1-S6 then Q1-Q6.
    return_h=True also returns h = silu(g)*u in the input dtype (stored by the same kernel)."""
    L.require_gpu(g, "silu_mul_quantize(g)")
    L.require_gpu(u, "silu_mul_quantize(u)")
    if g.shape != u.shape or g.dtype != u.dtype or g.device != u.device or g.dim() < 1:
        raise ValueError(f"silu_mul_quantize: g {tuple(g.shape)} {g.dtype} and u {tuple(u.shape)} {u.dtype} must match")
    code = L.dtype_code(g.dtype)
    g2, u2 = _rows_view(g), _rows_view(u)
    rows, cols = g2.shape
    q = torch.empty((rows, cols), dtype=torch.int8, device=g.device)
    scale = torch.empty((rows,), dtype=torch.float32, device=g.device)
    h = torch.empty((rows, cols), dtype=g.dtype, device=g.device) if return_h else None
    with torch.cuda.device(g.device):
        L.check(L.lib().pq_silu_mul_quant_rowwise(g2.data_ptr(), L.ld(g2), u2.data_ptr(), L.ld(u2), code, rows, cols,
                                                  q.data_ptr(), max(cols, 1), scale.data_ptr(),
                                                  h.data_ptr() if return_h else None, max(cols, 1), L.stream_ptr(g)),
                "silu_mul_quantize")
    qt = QTensor(q.reshape(g.shape), scale, 1, g.dtype, g.shape)
    return (qt, h.reshape(g.shape)) if return_h else qt


def glu_params(kind: str, limit, alpha=None):
    """(kind code, limit, alpha) of a clamped gate as pq_glu_quant_rowwise takes them, checked: kind "clamped_silu" (DeepSeek-V4: silu(min(g, L)) * clamp(u, +-L)) or
    "alpha_sigmoid" (GPT-OSS: (clamp(u, +-L) + 1) * gc * sigmoid(alpha * gc), gc = min(g, L)), limit finite and > 0, alpha finite (required for alpha_sigmoid only)."""
    if kind not in L.GLU_KINDS:
        raise ValueError(f"glu_quantize: unknown kind {kind!r}, expected one of {sorted(L.GLU_KINDS)}")
    if limit is None or not 0.0 < float(limit) < float("inf"):
        raise ValueError(f"glu_quantize: limit must be finite and > 0, got {limit!r}")
    if alpha is None:
        if kind == "alpha_sigmoid":
            raise ValueError("glu_quantize: kind 'alpha_sigmoid' needs alpha")
        alpha = 0.0
    if not -float("inf") < float(alpha) < float("inf"):
        raise ValueError(f"glu_quantize: alpha must be finite, got {alpha!r}")
    return L.GLU_KINDS[kind], float(limit), float(alpha)


def glu_quantize(g: torch.Tensor, u: torch.Tensor, kind: str, limit: float, alpha: float | None = None, return_h: bool = False):
    """quantize(h, axis=-1) in ONE pass for the clamped gates of GPT-OSS's and DeepSeek-V4's experts (glu_params names them), the way silu_mul_quantize fuses
    F.silu(g) * u: h is computed, reduced and encoded in registers.  g and u may be the column halves of one fused gate+up output.  Numerics: QSPEC G1-G6 — for
    bf16 / fp16 rows h holds the values transformers' _apply_gate stores, rounding for rounding; the limit is rounded to the rows' dtype as torch.clamp rounds it.
    return_h=True also returns h in the input dtype (stored by the same kernel)."""
    L.require_gpu(g, "glu_quantize(g)")
    L.require_gpu(u, "glu_quantize(u)")
    if g.shape != u.shape or g.dtype != u.dtype or g.device != u.device or g.dim() < 1:
        raise ValueError(f"glu_quantize: g {tuple(g.shape)} {g.dtype} and u {tuple(u.shape)} {u.dtype} must match")
    kcode, limit, alpha = glu_params(kind, limit, alpha)
    code = L.dtype_code(g.dtype)
    g2, u2 = _rows_view(g), _rows_view(u)
    rows, cols = g2.shape
    q = torch.empty((rows, cols), dtype=torch.int8, device=g.device)
    scale = torch.empty((rows,), dtype=torch.float32, device=g.device)
    h = torch.empty((rows, cols), dtype=g.dtype, device=g.device) if return_h else None
    with torch.cuda.device(g.device):
        L.check(L.lib().pq_glu_quant_rowwise(g2.data_ptr(), L.ld(g2), u2.data_ptr(), L.ld(u2), code, rows, cols, kcode, limit, alpha, q.data_ptr(), max(cols, 1),
                                             scale.data_ptr(), h.data_ptr() if return_h else None, max(cols, 1), L.stream_ptr(g)), "glu_quantize")
    qt = QTensor(q.reshape(g.shape), scale, 1, g.dtype, g.shape)
    return (qt, h.reshape(g.shape)) if return_h else qt


def _silu_pair(g, u, what):
    L.require_gpu(g, f"{what}(g)")
    L.require_gpu(u, f"{what}(u)")
    if g.shape != u.shape or g.dtype != u.dtype or g.device != u.device or g.dim() < 1:
        raise ValueError(f"{what}: g {tuple(g.shape)} {g.dtype} and u {tuple(u.shape)} {u.dtype} must match")
    return L.dtype_code(g.dtype), _rows_view(g), _rows_view(u)


def silu_mul_rowamax(g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """First half of silu_mul_quantize for a column-sharded intermediate: per token, the f32 BIT PATTERN (int32 tensor [rows]) of max |silu(g)*u| over the
    columns this rank holds.  Non-negative floats (and NaNs, above +Inf) order as integers: an integer MAX over the ranks is the exact row amax."""
    code, g2, u2 = _silu_pair(g, u, "silu_mul_rowamax")
    rows, cols = g2.shape
    amax = torch.empty((rows,), dtype=torch.int32, device=g.device)
    with torch.cuda.device(g.device):
        L.check(L.lib().pq_silu_mul_rowamax(g2.data_ptr(), L.ld(g2), u2.data_ptr(), L.ld(u2), code, rows, cols, amax.data_ptr(), L.stream_ptr(g)), "silu_mul_rowamax")
    return amax


def silu_mul_quantize_with_amax(g: torch.Tensor, u: torch.Tensor, amax_bits: torch.Tensor, out: torch.Tensor | None = None) -> QTensor:
    """Second half: the int8 codes of THESE columns against the row amax given as f32 bit patterns (int32 [rows], the max over every rank's columns), and the
    row scales amax / 127.  Column block and scale vector of the unsharded silu_mul_quantize, bit for bit.  `out`: optional int8 [rows, cols] destination."""
    code, g2, u2 = _silu_pair(g, u, "silu_mul_quantize_with_amax")
    rows, cols = g2.shape
    if amax_bits.dtype != torch.int32 or amax_bits.shape != (rows,) or amax_bits.device != g.device or not amax_bits.is_contiguous():
        raise ValueError(f"silu_mul_quantize_with_amax: amax_bits must be a contiguous int32 [{rows}] tensor on {g.device}")
    if out is None:
        q = torch.empty((rows, cols), dtype=torch.int8, device=g.device)
    else:
        q = out
        if q.dtype != torch.int8 or q.shape != (rows, cols) or q.device != g.device or (cols > 1 and q.stride(1) != 1):
            raise ValueError(f"silu_mul_quantize_with_amax: out must be an int8 [{rows}, {cols}] tensor with contiguous rows")
    scale = torch.empty((rows,), dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):
        L.check(L.lib().pq_silu_mul_quant_rowwise_amax(g2.data_ptr(), L.ld(g2), u2.data_ptr(), L.ld(u2), code, rows, cols, amax_bits.data_ptr(),
                                                       q.data_ptr(), L.ld(q) if rows > 1 else max(cols, 1), scale.data_ptr(), L.stream_ptr(g)), "silu_mul_quantize_with_amax")
    return QTensor(q if out is not None else q.reshape(g.shape), scale, 1, g.dtype, g.shape)


def rowamax(x: torch.Tensor) -> torch.Tensor:
    """First half of quantize(x, axis=-1) for an activation whose COLUMNS are sharded over ranks: per token, the f32 bit pattern (int32 [rows]) of max |x| over
    the columns this rank holds; an integer MAX over the ranks is the exact, NaN-propagating row amax."""
    L.require_gpu(x, "rowamax(x)")
    code = L.dtype_code(x.dtype)
    x2 = _rows_view(x)
    rows, cols = x2.shape
    amax = torch.empty((rows,), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        L.check(L.lib().pq_quant_rowamax(x2.data_ptr(), code, rows, cols, L.ld(x2), amax.data_ptr(), L.stream_ptr(x)), "rowamax")
    return amax


def quantize_with_amax(x: torch.Tensor, amax_bits: torch.Tensor, out: torch.Tensor | None = None) -> QTensor:
    """Second half: the int8 codes of THESE columns against the row amax given as f32 bit patterns (int32 [rows]: the max over every rank's columns) and the
    row scales — the column block and the scale vector of quantize(x_whole, axis=-1), bit for bit."""
    L.require_gpu(x, "quantize_with_amax(x)")
    code = L.dtype_code(x.dtype)
    x2 = _rows_view(x)
    rows, cols = x2.shape
    if amax_bits.dtype != torch.int32 or amax_bits.shape != (rows,) or amax_bits.device != x.device or not amax_bits.is_contiguous():
        raise ValueError(f"quantize_with_amax: amax_bits must be a contiguous int32 [{rows}] tensor on {x.device}")
    if out is None:
        q = torch.empty((rows, cols), dtype=torch.int8, device=x.device)
    else:
        q = out
        if q.dtype != torch.int8 or q.shape != (rows, cols) or q.device != x.device or (cols > 1 and q.stride(1) != 1):
            raise ValueError(f"quantize_with_amax: out must be an int8 [{rows}, {cols}] tensor with contiguous rows")
    scale = torch.empty((rows,), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        L.check(L.lib().pq_quant_rowwise_amax(x2.data_ptr(), code, rows, cols, L.ld(x2), amax_bits.data_ptr(), q.data_ptr(), L.ld(q) if rows > 1 else max(cols, 1),
                                              scale.data_ptr(), L.stream_ptr(x)), "quantize_with_amax")
    return QTensor(q if out is not None else q.reshape(x.shape), scale, 1, x.dtype, x.shape)


def rmsnorm_quantize(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6, return_h: bool = False):
    """quantize(weight * (x.float() * rsqrt(mean(x.float()**2, -1) + eps)).to(x.dtype), axis=-1) in ONE pass (kernel K1
    fused into RMSNorm): the normalised activation feeding q/k/v or gate/up is reduced, scaled and encoded in registers.
    Numerics: QSPEC N1-N6 (pinned reduction order) then Q1-Q6.  return_h=True also returns the normalised activation."""
    L.require_gpu(x, "rmsnorm_quantize(x)")
    L.require_gpu(weight, "rmsnorm_quantize(weight)")
    if x.dim() < 1 or weight.dim() != 1 or weight.shape[0] != x.shape[-1] or weight.dtype != x.dtype or weight.device != x.device:
        raise ValueError(f"rmsnorm_quantize: x {tuple(x.shape)} {x.dtype} needs a weight of shape ({x.shape[-1] if x.dim() else '?'},) "
                         f"and the same dtype/device, got {tuple(weight.shape)} {weight.dtype}")
    code = L.dtype_code(x.dtype)
    x2 = _rows_view(x)
    w = weight.contiguous()
    rows, cols = x2.shape
    q = torch.empty((rows, cols), dtype=torch.int8, device=x.device)
    scale = torch.empty((rows,), dtype=torch.float32, device=x.device)
    h = torch.empty((rows, cols), dtype=x.dtype, device=x.device) if return_h else None
    with torch.cuda.device(x.device):
        L.check(L.lib().pq_rmsnorm_quant_rowwise(x2.data_ptr(), L.ld(x2), w.data_ptr(), float(eps), code, rows, cols, q.data_ptr(),
                                                 max(cols, 1), scale.data_ptr(), h.data_ptr() if return_h else None, max(cols, 1),
                                                 L.stream_ptr(x)), "rmsnorm_quantize")
    qt = QTensor(q.reshape(x.shape), scale, 1, x.dtype, x.shape)
    return (qt, h.reshape(x.shape)) if return_h else qt


def _rows_view_of_out(out: torch.Tensor, rows: int, cols: int, what: str) -> torch.Tensor:
    """the 2-D [rows, cols] view of a destination tensor — a VIEW (never a copy: the kernel writes through it) with unit column stride"""
    try:
        o2 = out if out.dim() == 2 else out.view(rows, cols)
    except RuntimeError:
        o2 = None
    if o2 is None or (cols > 1 and o2.stride(1) != 1) or (rows > 1 and o2.stride(0) < cols):
        raise ValueError(f"{what}: out must be viewable as [{rows}, {cols}] rows with contiguous columns, got strides {tuple(out.stride())}")
    return o2


def add_rmsnorm_quantize(x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6, out: torch.Tensor | None = None, return_h: bool = False):
    """summed = residual + x, then rmsnorm_quantize(summed, weight, eps) — in ONE kernel (K1a): the new residual stream is stored once and normalised, reduced and
    encoded from the registers that hold it.  Returns (QTensor, summed) or (QTensor, summed, h) with return_h=True; every one of them holds the bits of
    rmsnorm_quantize(residual + x, weight, eps, return_h=True) with the add done by torch (QSPEC A1: one binary32 add, one storage rounding, then N1-N6, Q1-Q6).
    x and residual have the same shape, dtype and device.  `out` (optional, the same shape and dtype) receives the sum and may be x or residual themselves; any
    other tensor that overlaps an input is refused.  `summed` has x's shape."""
    L.require_gpu(x, "add_rmsnorm_quantize(x)")
    L.require_gpu(residual, "add_rmsnorm_quantize(residual)")
    L.require_gpu(weight, "add_rmsnorm_quantize(weight)")
    if x.dim() < 1 or x.shape != residual.shape or x.dtype != residual.dtype or x.device != residual.device:
        raise ValueError(f"add_rmsnorm_quantize: x {tuple(x.shape)} {x.dtype} {x.device} and residual {tuple(residual.shape)} {residual.dtype} {residual.device} must match")
    if weight.dim() != 1 or weight.shape[0] != x.shape[-1] or weight.dtype != x.dtype or weight.device != x.device:
        raise ValueError(f"add_rmsnorm_quantize: x {tuple(x.shape)} {x.dtype} needs a weight of shape ({x.shape[-1]},) and the same dtype/device, "
                         f"got {tuple(weight.shape)} {weight.dtype}")
    if out is not None:
        L.require_gpu(out, "add_rmsnorm_quantize(out)")
        if out.shape != x.shape or out.dtype != x.dtype or out.device != x.device:
            raise ValueError(f"add_rmsnorm_quantize: out {tuple(out.shape)} {out.dtype} must have x's shape {tuple(x.shape)} and dtype {x.dtype}")
    code = L.dtype_code(x.dtype)
    x2, r2 = _rows_view(x), _rows_view(residual)
    rows, cols = x2.shape
    summed = torch.empty(x.shape, dtype=x.dtype, device=x.device) if out is None else out
    s2 = _rows_view_of_out(summed, rows, cols, "add_rmsnorm_quantize")
    if rows == 0 or cols == 0:          # nothing to add: the empty sum through K1n (scales of empty rows are 1, QSPEC Q3)
        res = rmsnorm_quantize(summed, weight, eps, return_h)
        return (res[0], summed, res[1]) if return_h else (res, summed)
    w = weight.contiguous()
    q = torch.empty((rows, cols), dtype=torch.int8, device=x.device)
    scale = torch.empty((rows,), dtype=torch.float32, device=x.device)
    h = torch.empty((rows, cols), dtype=x.dtype, device=x.device) if return_h else None
    with torch.cuda.device(x.device):
        L.check(L.lib().pq_add_rmsnorm_quant_rowwise(x2.data_ptr(), L.ld(x2), r2.data_ptr(), L.ld(r2), s2.data_ptr(), L.ld(s2), w.data_ptr(), float(eps), code, rows, cols,
                                                     q.data_ptr(), cols, scale.data_ptr(), h.data_ptr() if return_h else None, cols, L.stream_ptr(x)),
                "add_rmsnorm_quantize")
    qt = QTensor(q.reshape(x.shape), scale, 1, x.dtype, x.shape)
    return (qt, summed, h.reshape(x.shape)) if return_h else (qt, summed)


def _residual_multiplier(what: str, multiplier) -> float:
    """`multiplier` as the C-ABI takes it: a finite Python int or float (a tensor would be a device value the kernel cannot take as an argument; bool is no number here)"""
    if isinstance(multiplier, bool) or not isinstance(multiplier, (int, float)):
        raise TypeError(f"{what}: multiplier must be a Python int or float, got {type(multiplier).__name__}")
    m = float(multiplier)
    if m != m or m in (float("inf"), float("-inf")):
        raise ValueError(f"{what}: multiplier must be finite, got {multiplier!r}")
    return m


def _scaled_operands(what: str, x, residual, out):
    """the shape / dtype / device checks of K1a on x, residual and the optional destination of the sum"""
    L.require_gpu(x, f"{what}(x)")
    L.require_gpu(residual, f"{what}(residual)")
    if x.dim() < 1 or x.shape != residual.shape or x.dtype != residual.dtype or x.device != residual.device:
        raise ValueError(f"{what}: x {tuple(x.shape)} {x.dtype} {x.device} and residual {tuple(residual.shape)} {residual.dtype} {residual.device} must match")
    if out is not None:
        L.require_gpu(out, f"{what}(out)")
        if out.shape != x.shape or out.dtype != x.dtype or out.device != x.device:
            raise ValueError(f"{what}: out {tuple(out.shape)} {out.dtype} must have x's shape {tuple(x.shape)} and dtype {x.dtype}")


def scaled_add_rmsnorm_quantize(x: torch.Tensor, residual: torch.Tensor, multiplier, weight: torch.Tensor, eps: float = 1e-6, out: torch.Tensor | None = None,
                                return_h: bool = False):
    """summed = residual + x * multiplier, then rmsnorm_quantize(summed, weight, eps) — in ONE kernel (K1ma): the scaled residual add of the Granite decoders taken into the
    norm + quantisation that follows it.  Returns (QTensor, summed) or (QTensor, summed, h) with return_h=True; every one of them holds the bits of
    add_rmsnorm_quantize(x * multiplier, residual, weight, eps, return_h=True) with the product computed by torch (QSPEC S1: one binary32 product, rounded to the storage
    dtype BEFORE the add — two roundings, never a fused multiply-add; then A1, N1-N6, Q1-Q6).  `multiplier` is a finite Python int or float (a tensor is a TypeError); it
    is rounded once to binary32, as torch rounds a Python scalar.  x, residual, weight, `out` and the aliasing rule as add_rmsnorm_quantize.  There is no CPU path."""
    what = "scaled_add_rmsnorm_quantize"
    m = _residual_multiplier(what, multiplier)
    _scaled_operands(what, x, residual, out)
    L.require_gpu(weight, f"{what}(weight)")
    if weight.dim() != 1 or weight.shape[0] != x.shape[-1] or weight.dtype != x.dtype or weight.device != x.device:
        raise ValueError(f"{what}: x {tuple(x.shape)} {x.dtype} needs a weight of shape ({x.shape[-1]},) and the same dtype/device, "
                         f"got {tuple(weight.shape)} {weight.dtype}")
    code = L.dtype_code(x.dtype)
    x2, r2 = _rows_view(x), _rows_view(residual)
    rows, cols = x2.shape
    summed = torch.empty(x.shape, dtype=x.dtype, device=x.device) if out is None else out
    s2 = _rows_view_of_out(summed, rows, cols, what)
    if rows == 0 or cols == 0:          # nothing to add: the empty sum through K1n (scales of empty rows are 1, QSPEC Q3)
        res = rmsnorm_quantize(summed, weight, eps, return_h)
        return (res[0], summed, res[1]) if return_h else (res, summed)
    w = weight.contiguous()
    q = torch.empty((rows, cols), dtype=torch.int8, device=x.device)
    scale = torch.empty((rows,), dtype=torch.float32, device=x.device)
    h = torch.empty((rows, cols), dtype=x.dtype, device=x.device) if return_h else None
    with torch.cuda.device(x.device):
        L.check(L.lib().pq_scaled_add_rmsnorm_quant_rows(x2.data_ptr(), L.ld(x2), r2.data_ptr(), L.ld(r2), m, s2.data_ptr(), L.ld(s2), w.data_ptr(), float(eps), code, rows,
                                                         cols, q.data_ptr(), cols, scale.data_ptr(), h.data_ptr() if return_h else None, cols, L.stream_ptr(x)), what)
    qt = QTensor(q.reshape(x.shape), scale, 1, x.dtype, x.shape)
    return (qt, summed, h.reshape(x.shape)) if return_h else (qt, summed)


def scaled_add(x: torch.Tensor, residual: torch.Tensor, multiplier, out: torch.Tensor | None = None) -> torch.Tensor:
    """residual + x * multiplier in ONE kernel (K1mo, the add-only form of K1ma: the end of a chain of Granite layers) — the bits of the torch expression (QSPEC S1, A1:
    the product is rounded to the storage dtype before the add).  Operands, `multiplier`, `out` and the aliasing rule as scaled_add_rmsnorm_quantize.  Returns the sum."""
    what = "scaled_add"
    m = _residual_multiplier(what, multiplier)
    _scaled_operands(what, x, residual, out)
    code = L.dtype_code(x.dtype)
    x2, r2 = _rows_view(x), _rows_view(residual)
    rows, cols = x2.shape
    summed = torch.empty(x.shape, dtype=x.dtype, device=x.device) if out is None else out
    s2 = _rows_view_of_out(summed, rows, cols, what)
    if rows == 0 or cols == 0:
        return summed
    with torch.cuda.device(x.device):
        L.check(L.lib().pq_scaled_add_rmsnorm_quant_rows(x2.data_ptr(), L.ld(x2), r2.data_ptr(), L.ld(r2), m, s2.data_ptr(), L.ld(s2), None, 0.0, code, rows, cols, None, cols,
                                                         None, None, cols, L.stream_ptr(x)), what)
    return summed


def layernorm_quantize(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None, eps: float = 1e-5, return_h: bool = False):
    """quantize(F.layer_norm(x, (C,), weight, bias, eps), axis=-1) in ONE pass (kernel K1l: K1 fused into LayerNorm): the normalised activation feeding c_attn /
    q, k, v / c_fc is reduced, normalised and encoded in registers.  `weight` is required (a LayerNorm without affine parameters is refused); `bias` may be None.
    Numerics: QSPEC L1-L6 (two-pass mean and variance in a pinned reduction order, one storage rounding) then Q1-Q6.  return_h=True also returns the normalised
    activation in the input dtype (stored by the same kernel)."""
    L.require_gpu(x, "layernorm_quantize(x)")
    if weight is None:
        raise ValueError("layernorm_quantize: weight is None — a LayerNorm without affine parameters (elementwise_affine=False) is not supported")
    L.require_gpu(weight, "layernorm_quantize(weight)")
    if x.dim() < 1 or weight.dim() != 1 or weight.shape[0] != x.shape[-1] or weight.dtype != x.dtype or weight.device != x.device:
        raise ValueError(f"layernorm_quantize: x {tuple(x.shape)} {x.dtype} needs a weight of shape ({x.shape[-1] if x.dim() else '?'},) "
                         f"and the same dtype/device, got {tuple(weight.shape)} {weight.dtype}")
    if bias is not None:
        L.require_gpu(bias, "layernorm_quantize(bias)")
        if bias.shape != weight.shape or bias.dtype != x.dtype or bias.device != x.device:
            raise ValueError(f"layernorm_quantize: bias {tuple(bias.shape)} {bias.dtype} must match the weight {tuple(weight.shape)} {weight.dtype}")
    code = L.dtype_code(x.dtype)
    x2 = _rows_view(x)
    w = weight.contiguous()
    b = bias.contiguous() if bias is not None else None
    rows, cols = x2.shape
    q = torch.empty((rows, cols), dtype=torch.int8, device=x.device)
    scale = torch.empty((rows,), dtype=torch.float32, device=x.device) if cols > 0 else torch.ones((rows,), dtype=torch.float32, device=x.device)
    h = torch.empty((rows, cols), dtype=x.dtype, device=x.device) if return_h else None
    with torch.cuda.device(x.device):
        L.check(L.lib().pq_layernorm_quant_rowwise(x2.data_ptr(), L.ld(x2), w.data_ptr(), b.data_ptr() if b is not None else None, float(eps), code, rows, cols,
                                                   q.data_ptr(), max(cols, 1), scale.data_ptr(), h.data_ptr() if return_h else None, max(cols, 1),
                                                   L.stream_ptr(x)), "layernorm_quantize")
    qt = QTensor(q.reshape(x.shape), scale, 1, x.dtype, x.shape)
    return (qt, h.reshape(x.shape)) if return_h else qt


def add_layernorm_quantize(x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None, eps: float = 1e-5, out: torch.Tensor | None = None,
                           return_h: bool = False):
    """summed = residual + x, then layernorm_quantize(summed, weight, bias, eps) — in ONE kernel (K1al): the new residual stream is stored once and normalised, reduced
    and encoded from the registers that hold it.  Returns (QTensor, summed) or (QTensor, summed, h) with return_h=True; every one of them holds the bits of
    layernorm_quantize(residual + x, weight, bias, eps, return_h=True) with the add done by torch (QSPEC A1: one binary32 add, one storage rounding, then L1-L6, Q1-Q6).
    x and residual have the same shape, dtype and device; `bias` may be None.  `out` (optional, the same shape and dtype) receives the sum and may be x or residual
    themselves; any other tensor that overlaps an input is refused.  `summed` has x's shape."""
    L.require_gpu(x, "add_layernorm_quantize(x)")
    L.require_gpu(residual, "add_layernorm_quantize(residual)")
    if weight is None:
        raise ValueError("add_layernorm_quantize: weight is None — a LayerNorm without affine parameters (elementwise_affine=False) is not supported")
    L.require_gpu(weight, "add_layernorm_quantize(weight)")
    if x.dim() < 1 or x.shape != residual.shape or x.dtype != residual.dtype or x.device != residual.device:
        raise ValueError(f"add_layernorm_quantize: x {tuple(x.shape)} {x.dtype} {x.device} and residual {tuple(residual.shape)} {residual.dtype} {residual.device} must match")
    if weight.dim() != 1 or weight.shape[0] != x.shape[-1] or weight.dtype != x.dtype or weight.device != x.device:
        raise ValueError(f"add_layernorm_quantize: x {tuple(x.shape)} {x.dtype} needs a weight of shape ({x.shape[-1]},) and the same dtype/device, "
                         f"got {tuple(weight.shape)} {weight.dtype}")
    if bias is not None:
        L.require_gpu(bias, "add_layernorm_quantize(bias)")
        if bias.shape != weight.shape or bias.dtype != x.dtype or bias.device != x.device:
            raise ValueError(f"add_layernorm_quantize: bias {tuple(bias.shape)} {bias.dtype} must match the weight {tuple(weight.shape)} {weight.dtype}")
    if out is not None:
        L.require_gpu(out, "add_layernorm_quantize(out)")
        if out.shape != x.shape or out.dtype != x.dtype or out.device != x.device:
            raise ValueError(f"add_layernorm_quantize: out {tuple(out.shape)} {out.dtype} must have x's shape {tuple(x.shape)} and dtype {x.dtype}")
    code = L.dtype_code(x.dtype)
    x2, r2 = _rows_view(x), _rows_view(residual)
    rows, cols = x2.shape
    summed = torch.empty(x.shape, dtype=x.dtype, device=x.device) if out is None else out
    s2 = _rows_view_of_out(summed, rows, cols, "add_layernorm_quantize")
    if rows == 0 or cols == 0:          # nothing to add: the empty sum through K1l (scales of empty rows are 1, QSPEC Q3)
        res = layernorm_quantize(summed, weight, bias, eps, return_h)
        return (res[0], summed, res[1]) if return_h else (res, summed)
    w = weight.contiguous()
    b = bias.contiguous() if bias is not None else None
    q = torch.empty((rows, cols), dtype=torch.int8, device=x.device)
    scale = torch.empty((rows,), dtype=torch.float32, device=x.device)
    h = torch.empty((rows, cols), dtype=x.dtype, device=x.device) if return_h else None
    with torch.cuda.device(x.device):
        L.check(L.lib().pq_add_layernorm_quant_rowwise(x2.data_ptr(), L.ld(x2), r2.data_ptr(), L.ld(r2), s2.data_ptr(), L.ld(s2), w.data_ptr(),
                                                       b.data_ptr() if b is not None else None, float(eps), code, rows, cols, q.data_ptr(), cols, scale.data_ptr(),
                                                       h.data_ptr() if return_h else None, cols, L.stream_ptr(x)), "add_layernorm_quantize")
    qt = QTensor(q.reshape(x.shape), scale, 1, x.dtype, x.shape)
    return (qt, summed, h.reshape(x.shape)) if return_h else (qt, summed)


def _check_ln_group(what: str, x: torch.Tensor, weight, bias, suffix: str = ""):
    """the affine parameters of one LayerNorm group against the rows they normalise (the messages of layernorm_quantize)"""
    if weight is None:
        raise ValueError(f"{what}: weight{suffix} is None — a LayerNorm without affine parameters (elementwise_affine=False) is not supported")
    L.require_gpu(weight, f"{what}(weight{suffix})")
    if weight.dim() != 1 or weight.shape[0] != x.shape[-1] or weight.dtype != x.dtype or weight.device != x.device:
        raise ValueError(f"{what}: x {tuple(x.shape)} {x.dtype} needs a weight{suffix} of shape ({x.shape[-1]},) and the same dtype/device, "
                         f"got {tuple(weight.shape)} {weight.dtype}")
    if bias is not None:
        L.require_gpu(bias, f"{what}(bias{suffix})")
        if bias.shape != weight.shape or bias.dtype != x.dtype or bias.device != x.device:
            raise ValueError(f"{what}: bias{suffix} {tuple(bias.shape)} {bias.dtype} must match the weight{suffix} {tuple(weight.shape)} {weight.dtype}")


def _parallel_launch(what: str, a2, b2, c2, s2, groups, return_h: bool, like: torch.Tensor):
    """One launch of pq_parallel_layernorm_quant_rowwise on 2-D row views (a2, b2, s2 None: no add); groups: one or two (weight, bias, eps).  Returns per group
    (QTensor, h or None)."""
    rows, cols = c2.shape
    code = L.dtype_code(c2.dtype)
    dev = c2.device
    ptr = lambda t: t.data_ptr() if t is not None else None          # noqa: E731
    ldo = lambda t: L.ld(t) if t is not None else 0                  # noqa: E731
    outs, args = [], []
    for g in (0, 1):
        if g < len(groups):
            w, b, eps = groups[g]
            w = w.contiguous()
            b = b.contiguous() if b is not None else None
            q = torch.empty((rows, cols), dtype=torch.int8, device=dev)
            scale = torch.empty((rows,), dtype=torch.float32, device=dev)
            h = torch.empty((rows, cols), dtype=c2.dtype, device=dev) if return_h else None
            outs.append((q, scale, h))
            args.append((w, b, float(eps)))
        else:
            outs.append((None, None, None))
            args.append((None, None, 0.0))
    with torch.cuda.device(dev):
        L.check(L.lib().pq_parallel_layernorm_quant_rowwise(
            ptr(a2), ldo(a2), ptr(b2), ldo(b2), c2.data_ptr(), L.ld(c2), ptr(s2), ldo(s2),
            ptr(args[0][0]), ptr(args[0][1]), args[0][2], ptr(args[1][0]), ptr(args[1][1]), args[1][2], code, rows, cols,
            ptr(outs[0][0]), cols, ptr(outs[0][1]), ptr(outs[0][2]), cols, ptr(outs[1][0]), cols if outs[1][0] is not None else 0, ptr(outs[1][1]), ptr(outs[1][2]),
            cols if outs[1][2] is not None else 0, L.stream_ptr(c2)), what)
    return [(QTensor(q.reshape(like.shape), scale, 1, like.dtype, like.shape), h.reshape(like.shape) if h is not None else None) for q, scale, h in outs[:len(groups)]]


def add2_layernorm_quantize(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None, eps: float = 1e-5,
                            weight2: torch.Tensor | None = None, bias2: torch.Tensor | None = None, eps2: float | None = None, out: torch.Tensor | None = None,
                            return_h: bool = False):
    """summed = (a + b) + c — two adds in THIS association, each rounded to the storage dtype (QSPEC A2) — then layernorm_quantize(summed, weight, bias, eps) and, with
    `weight2`, layernorm_quantize(summed, weight2, bias2, eps2) as well, in ONE kernel (K1pl): the parallel residual of a GPT-NeoX / Phi block and the norm(s) of the next
    block.  The sum is stored once; its mean and variance are computed once and serve both norms.  Returns (QTensor, summed) or (QTensor, QTensor2, summed), with h (and
    h2) appended under return_h=True; every one of them holds the bits of the two torch adds followed by layernorm_quantize(..., return_h=True) per norm.  Addition
    commutes, so a and b may be swapped, but the three may not be regrouped: pass them in the order the model adds them.  a, b and c have the same shape, dtype and
    device; the biases may be None; eps2 defaults to eps.  `out` (optional, the same shape and dtype) receives the sum and may be a, b or c themselves; any other tensor
    that overlaps an input is refused.  `summed` has a's shape."""
    what = "add2_layernorm_quantize"
    for name, t in (("a", a), ("b", b), ("c", c)):
        L.require_gpu(t, f"{what}({name})")
    for name, t in (("b", b), ("c", c)):
        if a.dim() < 1 or a.shape != t.shape or a.dtype != t.dtype or a.device != t.device:
            raise ValueError(f"{what}: a {tuple(a.shape)} {a.dtype} {a.device} and {name} {tuple(t.shape)} {t.dtype} {t.device} must match")
    _check_ln_group(what, a, weight, bias)
    two = weight2 is not None
    if two:
        _check_ln_group(what, a, weight2, bias2, "2")
    elif bias2 is not None or eps2 is not None:
        raise ValueError(f"{what}: bias2 / eps2 are given without weight2 (the second norm is absent as a whole)")
    if out is not None:
        L.require_gpu(out, f"{what}(out)")
        if out.shape != a.shape or out.dtype != a.dtype or out.device != a.device:
            raise ValueError(f"{what}: out {tuple(out.shape)} {out.dtype} must have a's shape {tuple(a.shape)} and dtype {a.dtype}")
    eps2 = eps if eps2 is None else eps2
    L.dtype_code(a.dtype)
    a2, b2, c2 = _rows_view(a), _rows_view(b), _rows_view(c)
    rows, cols = a2.shape
    summed = torch.empty(a.shape, dtype=a.dtype, device=a.device) if out is None else out
    s2 = _rows_view_of_out(summed, rows, cols, what)
    if rows == 0 or cols == 0:          # nothing to add: the empty sum through K1l (scales of empty rows are 1, QSPEC Q3)
        res = [layernorm_quantize(summed, w, bi, e, True) for w, bi, e in ([(weight, bias, eps)] + ([(weight2, bias2, eps2)] if two else []))]
    else:
        res = _parallel_launch(what, a2, b2, c2, s2, [(weight, bias, eps)] + ([(weight2, bias2, eps2)] if two else []), return_h, a)
    ret = tuple(r[0] for r in res) + (summed,)
    return ret + tuple(r[1] for r in res) if return_h else ret


def layernorm_quantize2(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None, weight2: torch.Tensor, bias2: torch.Tensor | None, eps: float = 1e-5,
                        eps2: float | None = None, return_h: bool = False):
    """layernorm_quantize(x, weight, bias, eps) and layernorm_quantize(x, weight2, bias2, eps2) in ONE kernel (K1l2, the "dual norm" of the first block of a GPT-NeoX
    stack with a parallel residual): x is read once, its mean and variance are computed once and each norm applies its own eps, affine map and quantisation.  Returns
    (QTensor, QTensor2) or (QTensor, QTensor2, h, h2) with return_h=True, the bits of the two separate calls.  The biases may be None; eps2 defaults to eps."""
    what = "layernorm_quantize2"
    L.require_gpu(x, f"{what}(x)")
    if x.dim() < 1:
        raise ValueError(f"{what}: x needs at least 1 dimension")
    _check_ln_group(what, x, weight, bias)
    _check_ln_group(what, x, weight2, bias2, "2")
    eps2 = eps if eps2 is None else eps2
    L.dtype_code(x.dtype)
    x2 = _rows_view(x)
    rows, cols = x2.shape
    if rows == 0 or cols == 0:
        res = [layernorm_quantize(x, w, bi, e, True) for w, bi, e in ((weight, bias, eps), (weight2, bias2, eps2))]
    else:
        res = _parallel_launch(what, None, None, x2, None, [(weight, bias, eps), (weight2, bias2, eps2)], return_h, x)
    ret = tuple(r[0] for r in res)
    return ret + tuple(r[1] for r in res) if return_h else ret


def act_quantize(x: torch.Tensor, kind: str, return_h: bool = False):
    """quantize(act(x), axis=-1) in ONE pass (kernel K1u) for the unary activation of a plain two-linear MLP: kind "relu" (torch.relu), "gelu_tanh" (gelu_new,
    gelu_pytorch_tanh) or "gelu_erf" (F.gelu's default).  x may be a column slice of a wider tensor.  Numerics: QSPEC U1-U4 then Q1-Q6 — relu holds torch's bits;
    both GELUs are within 1 ulp of the input dtype of the exact value, closer to it than torch's eager kernels are, and not bit-identical to those.
    return_h=True also returns h = act(x) in the input dtype (stored by the same kernel)."""
    L.require_gpu(x, "act_quantize(x)")
    if kind not in L.ACT_KINDS:
        raise ValueError(f"act_quantize: unknown kind {kind!r}, expected one of {sorted(L.ACT_KINDS)}")
    if x.dim() < 1:
        raise ValueError("act_quantize: x needs at least 1 dimension")
    code = L.dtype_code(x.dtype)
    x2 = _rows_view(x)
    rows, cols = x2.shape
    q = torch.empty((rows, cols), dtype=torch.int8, device=x.device)
    scale = torch.empty((rows,), dtype=torch.float32, device=x.device) if cols > 0 else torch.ones((rows,), dtype=torch.float32, device=x.device)
    h = torch.empty((rows, cols), dtype=x.dtype, device=x.device) if return_h else None
    with torch.cuda.device(x.device):
        L.check(L.lib().pq_act_quant_rowwise(x2.data_ptr(), L.ld(x2), code, rows, cols, L.ACT_KINDS[kind], q.data_ptr(), max(cols, 1), scale.data_ptr(),
                                             h.data_ptr() if return_h else None, max(cols, 1), L.stream_ptr(x)), "act_quantize")
    qt = QTensor(q.reshape(x.shape), scale, 1, x.dtype, x.shape)
    return (qt, h.reshape(x.shape)) if return_h else qt


def _check_norm_weight(what: str, x: torch.Tensor, weight: torch.Tensor):
    if x.dim() < 1 or weight.dim() != 1 or weight.shape[0] != x.shape[-1] or weight.dtype != x.dtype or weight.device != x.device:
        raise ValueError(f"{what}: x {tuple(x.shape)} {x.dtype} needs a weight of shape ({x.shape[-1] if x.dim() else '?'},) "
                         f"and the same dtype/device, got {tuple(weight.shape)} {weight.dtype}")


def gemma_rmsnorm_quantize(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6, return_h: bool = False):
    """quantize(((x.float() * rsqrt(mean(x.float()**2, -1) + eps)) * (1.0 + weight.float())).to(x.dtype), axis=-1) in ONE pass (kernel K1ng: K1 fused into
    GemmaRMSNorm — Gemma, Gemma-2, Gemma-3).  `weight` is the module's STORED weight w; the gain is 1 + w.  Numerics: QSPEC NG1-NG6 (N1-N4's pinned reduction
    order, then binary32 throughout and ONE storage rounding — rmsnorm_quantize with 1 + w as its weight gives other bits) then Q1-Q6.  return_h=True also returns
    the normalised activation in the input dtype (stored by the same kernel)."""
    L.require_gpu(x, "gemma_rmsnorm_quantize(x)")
    L.require_gpu(weight, "gemma_rmsnorm_quantize(weight)")
    _check_norm_weight("gemma_rmsnorm_quantize", x, weight)
    code = L.dtype_code(x.dtype)
    x2 = _rows_view(x)
    w = weight.contiguous()
    rows, cols = x2.shape
    q = torch.empty((rows, cols), dtype=torch.int8, device=x.device)
    scale = torch.empty((rows,), dtype=torch.float32, device=x.device) if cols > 0 else torch.ones((rows,), dtype=torch.float32, device=x.device)
    h = torch.empty((rows, cols), dtype=x.dtype, device=x.device) if return_h else None
    with torch.cuda.device(x.device):
        L.check(L.lib().pq_gemma_rmsnorm_quant_rowwise(x2.data_ptr(), L.ld(x2), w.data_ptr(), float(eps), code, rows, cols, q.data_ptr(), max(cols, 1),
                                                       scale.data_ptr(), h.data_ptr() if return_h else None, max(cols, 1), L.stream_ptr(x)), "gemma_rmsnorm_quantize")
    qt = QTensor(q.reshape(x.shape), scale, 1, x.dtype, x.shape)
    return (qt, h.reshape(x.shape)) if return_h else qt


def add_gemma_rmsnorm_quantize(x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6, out: torch.Tensor | None = None,
                               return_h: bool = False):
    """summed = residual + x, then gemma_rmsnorm_quantize(summed, weight, eps) — in ONE kernel (K1ang).  Returns (QTensor, summed) or (QTensor, summed, h) with
    return_h=True; every one of them holds the bits of gemma_rmsnorm_quantize(residual + x, weight, eps, return_h=True) with the add done by torch (QSPEC A1, then
    NG1-NG6, Q1-Q6).  x and residual have the same shape, dtype and device.  `out` (optional, the same shape and dtype) receives the sum and may be x or residual
    themselves; any other tensor that overlaps an input is refused.  `summed` has x's shape."""
    L.require_gpu(x, "add_gemma_rmsnorm_quantize(x)")
    L.require_gpu(residual, "add_gemma_rmsnorm_quantize(residual)")
    L.require_gpu(weight, "add_gemma_rmsnorm_quantize(weight)")
    if x.dim() < 1 or x.shape != residual.shape or x.dtype != residual.dtype or x.device != residual.device:
        raise ValueError(f"add_gemma_rmsnorm_quantize: x {tuple(x.shape)} {x.dtype} {x.device} and residual {tuple(residual.shape)} {residual.dtype} {residual.device} must match")
    _check_norm_weight("add_gemma_rmsnorm_quantize", x, weight)
    if out is not None:
        L.require_gpu(out, "add_gemma_rmsnorm_quantize(out)")
        if out.shape != x.shape or out.dtype != x.dtype or out.device != x.device:
            raise ValueError(f"add_gemma_rmsnorm_quantize: out {tuple(out.shape)} {out.dtype} must have x's shape {tuple(x.shape)} and dtype {x.dtype}")
    code = L.dtype_code(x.dtype)
    x2, r2 = _rows_view(x), _rows_view(residual)
    rows, cols = x2.shape
    summed = torch.empty(x.shape, dtype=x.dtype, device=x.device) if out is None else out
    s2 = _rows_view_of_out(summed, rows, cols, "add_gemma_rmsnorm_quantize")
    if rows == 0 or cols == 0:          # nothing to add: the empty sum through K1ng (scales of empty rows are 1, QSPEC Q3)
        res = gemma_rmsnorm_quantize(summed, weight, eps, return_h)
        return (res[0], summed, res[1]) if return_h else (res, summed)
    w = weight.contiguous()
    q = torch.empty((rows, cols), dtype=torch.int8, device=x.device)
    scale = torch.empty((rows,), dtype=torch.float32, device=x.device)
    h = torch.empty((rows, cols), dtype=x.dtype, device=x.device) if return_h else None
    with torch.cuda.device(x.device):
        L.check(L.lib().pq_add_gemma_rmsnorm_quant_rowwise(x2.data_ptr(), L.ld(x2), r2.data_ptr(), L.ld(r2), s2.data_ptr(), L.ld(s2), w.data_ptr(), float(eps), code, rows,
                                                           cols, q.data_ptr(), cols, scale.data_ptr(), h.data_ptr() if return_h else None, cols, L.stream_ptr(x)),
                "add_gemma_rmsnorm_quantize")
    qt = QTensor(q.reshape(x.shape), scale, 1, x.dtype, x.shape)
    return (qt, summed, h.reshape(x.shape)) if return_h else (qt, summed)


def _postnorm_operands(what: str, x, post_weight, residual, out):
    """the shared argument checks of the two sandwich calls; returns (code, x2, r2, rows, cols, summed, s2)"""
    L.require_gpu(x, f"{what}(x)")
    L.require_gpu(residual, f"{what}(residual)")
    L.require_gpu(post_weight, f"{what}(post_weight)")
    if x.dim() < 1 or x.shape != residual.shape or x.dtype != residual.dtype or x.device != residual.device:
        raise ValueError(f"{what}: x {tuple(x.shape)} {x.dtype} {x.device} and residual {tuple(residual.shape)} {residual.dtype} {residual.device} must match")
    _check_norm_weight(what, x, post_weight)
    if out is not None:
        L.require_gpu(out, f"{what}(out)")
        if out.shape != x.shape or out.dtype != x.dtype or out.device != x.device:
            raise ValueError(f"{what}: out {tuple(out.shape)} {out.dtype} must have x's shape {tuple(x.shape)} and dtype {x.dtype}")
    code = L.dtype_code(x.dtype)
    x2, r2 = _rows_view(x), _rows_view(residual)
    rows, cols = x2.shape
    summed = torch.empty(x.shape, dtype=x.dtype, device=x.device) if out is None else out
    return code, x2, r2, rows, cols, summed, _rows_view_of_out(summed, rows, cols, what)


def gemma_postnorm_add_rmsnorm_quantize(x: torch.Tensor, post_weight: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6,
                                        post_eps: float = 1e-6, out: torch.Tensor | None = None, return_h: bool = False):
    """The sandwich residual flow of Gemma-2 / Gemma-3 in ONE kernel (K1pang): x is a sublayer's output, `post_weight` / `post_eps` the post-norm on it, `residual` the
    residual stream, `weight` / `eps` the norm that follows the add.  Returns (QTensor, summed) or (QTensor, summed, h) with return_h=True, and every one of them
    holds, bit for bit, what this composition gives:

        p      = gemma_rmsnorm_quantize(x, post_weight, post_eps, return_h=True)[1]
        summed = residual + p
        QT, h  = gemma_rmsnorm_quantize(summed, weight, eps, return_h=True)

    (QSPEC PN1: p is rounded to the storage dtype and never stored; A1; then NG1-NG6 and Q1-Q6 on the rows of the sum as stored.)  x and residual have the same shape,
    dtype and device; both weights are the modules' STORED weights.  `out` (optional, the same shape and dtype) receives the sum and may be x or residual themselves;
    any other tensor that overlaps an input is refused.  `summed` has x's shape."""
    what = "gemma_postnorm_add_rmsnorm_quantize"
    code, x2, r2, rows, cols, summed, s2 = _postnorm_operands(what, x, post_weight, residual, out)
    L.require_gpu(weight, f"{what}(weight)")
    _check_norm_weight(what, x, weight)
    if rows == 0 or cols == 0:          # nothing to normalise or add: the empty sum through K1ng (scales of empty rows are 1, QSPEC Q3)
        res = gemma_rmsnorm_quantize(summed, weight, eps, return_h)
        return (res[0], summed, res[1]) if return_h else (res, summed)
    pw, w = post_weight.contiguous(), weight.contiguous()
    q = torch.empty((rows, cols), dtype=torch.int8, device=x.device)
    scale = torch.empty((rows,), dtype=torch.float32, device=x.device)
    h = torch.empty((rows, cols), dtype=x.dtype, device=x.device) if return_h else None
    with torch.cuda.device(x.device):
        L.check(L.lib().pq_gemma_postnorm_add_rmsnorm_quant_rowwise(x2.data_ptr(), L.ld(x2), pw.data_ptr(), float(post_eps), r2.data_ptr(), L.ld(r2), s2.data_ptr(), L.ld(s2),
                                                                    w.data_ptr(), float(eps), code, rows, cols, q.data_ptr(), cols, scale.data_ptr(),
                                                                    h.data_ptr() if return_h else None, cols, L.stream_ptr(x)), what)
    qt = QTensor(q.reshape(x.shape), scale, 1, x.dtype, x.shape)
    return (qt, summed, h.reshape(x.shape)) if return_h else (qt, summed)


def gemma_postnorm_add(x: torch.Tensor, post_weight: torch.Tensor, residual: torch.Tensor, post_eps: float = 1e-6, out: torch.Tensor | None = None) -> torch.Tensor:
    """summed = residual + GemmaRMSNorm(x; post_weight, post_eps) in ONE kernel (K1pa, the add-only form of K1pang: the end of a chain of sandwich-fused layers).
    Returns `summed`, the bits of

        p      = gemma_rmsnorm_quantize(x, post_weight, post_eps, return_h=True)[1]
        summed = residual + p

    and of gemma_postnorm_add_rmsnorm_quantize's `summed` (QSPEC PN1, A1).  Arguments and `out` as there."""
    what = "gemma_postnorm_add"
    code, x2, r2, rows, cols, summed, s2 = _postnorm_operands(what, x, post_weight, residual, out)
    if rows == 0 or cols == 0:
        return summed
    pw = post_weight.contiguous()
    with torch.cuda.device(x.device):
        L.check(L.lib().pq_gemma_postnorm_add_rmsnorm_quant_rowwise(x2.data_ptr(), L.ld(x2), pw.data_ptr(), float(post_eps), r2.data_ptr(), L.ld(r2), s2.data_ptr(), L.ld(s2),
                                                                    None, 0.0, code, rows, cols, None, cols, None, None, cols, L.stream_ptr(x)), what)
    return summed


def olmo_postnorm_add_quantize(x: torch.Tensor, post_weight: torch.Tensor, residual: torch.Tensor, post_eps: float = 1e-6, out: torch.Tensor | None = None):
    """The post-norm residual flow of OLMo-2 / OLMo-3 in ONE kernel (K1oq): x is a sublayer's output, `post_weight` / `post_eps` the norm on it, `residual` the
    residual stream; the sum is the input of the next sublayer's int8 projections.  Returns (QTensor, summed), which hold, bit for bit, what this composition gives:

        p      = olmo_rmsnorm(x, post_weight, post_eps)
        summed = residual + p
        QT     = quantize(summed)

    (QSPEC NO1-NO5: (x.float() * rsqrt(mean(x.float()²) + eps)) * w.float(), binary32 throughout and ONE storage rounding; PO1: p is never stored; A1; Q1-Q6 on the
    rows of the sum as stored.)  x and residual have the same shape, dtype and device.  `out` (optional, the same shape and dtype) receives the sum and may be x or
    residual themselves; any other tensor that overlaps an input is refused.  `summed` has x's shape."""
    what = "olmo_postnorm_add_quantize"
    code, x2, r2, rows, cols, summed, s2 = _postnorm_operands(what, x, post_weight, residual, out)
    if rows == 0 or cols == 0:          # nothing to normalise or add: the empty sum through K1 (scales of empty rows are 1, QSPEC Q3)
        return quantize(summed), summed
    pw = post_weight.contiguous()
    q = torch.empty((rows, cols), dtype=torch.int8, device=x.device)
    scale = torch.empty((rows,), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        L.check(L.lib().pq_olmo_postnorm_add_quant_rowwise(x2.data_ptr(), L.ld(x2), pw.data_ptr(), float(post_eps), r2.data_ptr(), L.ld(r2), s2.data_ptr(), L.ld(s2), code, rows,
                                                           cols, q.data_ptr(), cols, scale.data_ptr(), L.stream_ptr(x)), what)
    return QTensor(q.reshape(x.shape), scale, 1, x.dtype, x.shape), summed


def olmo_postnorm_add(x: torch.Tensor, post_weight: torch.Tensor, residual: torch.Tensor, post_eps: float = 1e-6, out: torch.Tensor | None = None) -> torch.Tensor:
    """summed = residual + olmo_rmsnorm(x, post_weight, post_eps) in ONE kernel (K1oa, the form of K1oq without the quantisation: the end of a chain of post-norm-fused
    layers).  Returns `summed`, the bits of olmo_postnorm_add_quantize's (QSPEC NO1-NO5, PO1, A1).  Arguments and `out` as there."""
    what = "olmo_postnorm_add"
    code, x2, r2, rows, cols, summed, s2 = _postnorm_operands(what, x, post_weight, residual, out)
    if rows == 0 or cols == 0:
        return summed
    pw = post_weight.contiguous()
    with torch.cuda.device(x.device):
        L.check(L.lib().pq_olmo_postnorm_add_quant_rowwise(x2.data_ptr(), L.ld(x2), pw.data_ptr(), float(post_eps), r2.data_ptr(), L.ld(r2), s2.data_ptr(), L.ld(s2), code, rows,
                                                           cols, None, 0, None, L.stream_ptr(x)), what)
    return summed


def olmo_rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6, out: torch.Tensor | None = None) -> torch.Tensor:
    """(weight * (x.float() * rsqrt(mean(x.float()², -1) + eps))).to(x.dtype) in ONE kernel (K1on, the norm alone: q_norm / k_norm of OLMo-2 / OLMo-3): binary32
    throughout and ONE storage rounding (QSPEC NO1-NO5: N1-N4's pinned reduction order; spec-exact, and as close to the eager chain as two correctly rounded orders of
    the same sum are).  x may be a column slice of a wider tensor (the k slice of a fused q/k/v output).  `out` (optional, x's shape and dtype) receives the result and
    may be x itself; any other tensor that overlaps x is refused.  Returns a tensor of x's shape."""
    what = "olmo_rmsnorm"
    L.require_gpu(x, f"{what}(x)")
    L.require_gpu(weight, f"{what}(weight)")
    _check_norm_weight(what, x, weight)
    if out is not None:
        L.require_gpu(out, f"{what}(out)")
        if out.shape != x.shape or out.dtype != x.dtype or out.device != x.device:
            raise ValueError(f"{what}: out {tuple(out.shape)} {out.dtype} must have x's shape {tuple(x.shape)} and dtype {x.dtype}")
    code = L.dtype_code(x.dtype)
    x2 = _rows_view(x)
    rows, cols = x2.shape
    h = torch.empty(x.shape, dtype=x.dtype, device=x.device) if out is None else out
    h2 = _rows_view_of_out(h, rows, cols, what)
    if rows == 0 or cols == 0:
        return h
    w = weight.contiguous()
    with torch.cuda.device(x.device):
        L.check(L.lib().pq_olmo_postnorm_add_quant_rowwise(x2.data_ptr(), L.ld(x2), w.data_ptr(), float(eps), None, 0, h2.data_ptr(), L.ld(h2), code, rows, cols, None, 0, None,
                                                           L.stream_ptr(x)), what)
    return h


def _head_stride_order(shape, strides):
    """the leading axes of a [..., D] tensor from the outermost to the innermost by stride (stable: equal strides keep their order)"""
    return sorted(range(len(shape) - 1), key=lambda a: -strides[a])


def _dense_head_strides(shape, strides):
    """strides of a dense tensor of `shape` whose last axis is innermost and whose leading axes are laid out in the stride order of `strides`: what eager's
    elementwise chain returns for such an input"""
    out = [0] * len(shape)
    out[-1] = 1
    step = max(int(shape[-1]), 1)
    for a in reversed(_head_stride_order(shape, strides)):
        out[a] = step
        step *= max(int(shape[a]), 1)
    return tuple(out)


def _collapse_heads(shape, strides):
    """The leading axes of a [..., D] tensor as at most two strided axes: (n_outer, ld_o, n_inner, ld_i), in elements, or None where a copy is needed.  The axes are
    ordered by stride and an axis is merged into its neighbour where stride[a] == stride[b] * size[b]; axes of one index are dropped.  q_proj(x).view(B, T, H, D) on a
    column slice of a fused q/k/v output, its .transpose(1, 2) and a contiguous tensor all collapse (the last to ONE axis: (rows, D, 1, D)).  None: the last stride is
    not 1, a stride is smaller than D (rows that overlap: an expanded axis), or more than two axes remain."""
    D = int(shape[-1])
    if D > 1 and strides[-1] != 1:
        return None
    groups = []          # (size, stride), outermost first
    for a in _head_stride_order(shape, strides):
        n, s = int(shape[a]), int(strides[a])
        if n == 1:
            continue
        if s < D:
            return None
        if groups and groups[-1][1] == s * n:
            groups[-1] = (groups[-1][0] * n, s)
        else:
            groups.append((n, s))
    if len(groups) > 2:
        return None
    if not groups:
        return (1, D, 1, D)
    if len(groups) == 1:
        return (groups[0][0], groups[0][1], 1, D)
    return (groups[0][0], groups[0][1], groups[1][0], groups[1][1])


def head_rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6, kind: str = "llama") -> torch.Tensor:
    """The RMSNorm of every row of the LAST axis of x in ONE kernel (K1hn: q_norm / k_norm of Qwen3, Qwen3-MoE and Gemma-3, whose rows are heads of head_dim
    elements), no quantisation.  kind "llama": (weight * (x.float() * rsqrt(mean(x.float()², -1) + eps)).to(x.dtype)) — x * rs rounded to the storage dtype before the
    gain (QSPEC N1-N5; Qwen3RMSNorm, LlamaRMSNorm); kind "gemma": ((x.float() * rs) * (1 + weight.float())).to(x.dtype), one rounding (NG1-NG5; Gemma3RMSNorm).  The
    bits are those of rmsnorm_quantize(..., return_h=True)[1] / gemma_rmsnorm_quantize(..., return_h=True)[1] on the same rows (QSPEC HN1): spec-exact, eager-close.
    x: [..., D] on the GPU; weight: [D], the same dtype and device.  The leading axes are collapsed into at most two strided axes (_collapse_heads), so
    q_proj(x).view(B, T, H, D) on a column slice of a fused q/k/v output, its .transpose(1, 2) and a contiguous tensor are normed where they lie, without a copy;
    anything else is copied once.  Returns a fresh dense tensor of x's shape whose axes are laid out in x's stride order, as eager's elementwise chain does.  An
    empty x returns an empty tensor without a launch."""
    what = "head_rmsnorm"
    L.require_gpu(x, f"{what}(x)")
    L.require_gpu(weight, f"{what}(weight)")
    _check_norm_weight(what, x, weight)
    if kind not in L.GAIN_KINDS:
        raise ValueError(f"{what}: kind must be one of {sorted(L.GAIN_KINDS)}, got {kind!r}")
    code = L.dtype_code(x.dtype)
    dense = _dense_head_strides(x.shape, x.stride())
    out = torch.empty_strided(x.shape, dense, dtype=x.dtype, device=x.device)
    if x.numel() == 0:
        return out
    plan = _collapse_heads(x.shape, x.stride())
    if plan is None:          # one copy, into the layout of the result
        xc = torch.empty_strided(x.shape, dense, dtype=x.dtype, device=x.device)
        xc.copy_(x)
        x, plan = xc, _collapse_heads(x.shape, dense)
    n_outer, ld_xo, n_inner, ld_xi = plan
    D = x.shape[-1]
    w = weight.contiguous()
    with torch.cuda.device(x.device):
        L.check(L.lib().pq_head_rmsnorm(x.data_ptr(), ld_xo, ld_xi, w.data_ptr(), float(eps), L.GAIN_KINDS[kind], code, n_outer, n_inner, D, out.data_ptr(),
                                        n_inner * D, D, L.stream_ptr(x)), what)
    return out


def gelu_mul_quantize(g: torch.Tensor, u: torch.Tensor, kind: str = "gelu_tanh", return_h: bool = False):
    """quantize(F.gelu(g, approximate="tanh") * u, axis=-1) in ONE pass (kernel K1gg): the activation of the down projection of a GeGLU MLP (Gemma's
    down(act_fn(gate(x)) * up(x))) is computed, reduced and encoded in registers.  g and u may be the column halves of one fused gate+up output.  Numerics: QSPEC
    GG1-GG3 — act_quantize's tanh GELU (U2) rounded to the input dtype, then the product rounded once, as the eager chain stores them — then Q1-Q6.  kind:
    "gelu_tanh" only.  return_h=True also returns h in the input dtype (stored by the same kernel)."""
    L.require_gpu(g, "gelu_mul_quantize(g)")
    L.require_gpu(u, "gelu_mul_quantize(u)")
    if kind != "gelu_tanh":
        raise ValueError(f"gelu_mul_quantize: unsupported kind {kind!r}, expected 'gelu_tanh'")
    if g.shape != u.shape or g.dtype != u.dtype or g.device != u.device or g.dim() < 1:
        raise ValueError(f"gelu_mul_quantize: g {tuple(g.shape)} {g.dtype} and u {tuple(u.shape)} {u.dtype} must match")
    code = L.dtype_code(g.dtype)
    g2, u2 = _rows_view(g), _rows_view(u)
    rows, cols = g2.shape
    q = torch.empty((rows, cols), dtype=torch.int8, device=g.device)
    scale = torch.empty((rows,), dtype=torch.float32, device=g.device) if cols > 0 else torch.ones((rows,), dtype=torch.float32, device=g.device)
    h = torch.empty((rows, cols), dtype=g.dtype, device=g.device) if return_h else None
    with torch.cuda.device(g.device):
        L.check(L.lib().pq_gelu_mul_quant_rowwise(g2.data_ptr(), L.ld(g2), u2.data_ptr(), L.ld(u2), code, rows, cols, L.ACT_KINDS[kind], q.data_ptr(), max(cols, 1),
                                                  scale.data_ptr(), h.data_ptr() if return_h else None, max(cols, 1), L.stream_ptr(g)), "gelu_mul_quantize")
    qt = QTensor(q.reshape(g.shape), scale, 1, g.dtype, g.shape)
    return (qt, h.reshape(g.shape)) if return_h else qt


def dequantize(q: QTensor, dtype: torch.dtype | None = None) -> torch.Tensor:
    """cast_rne(f32(int_data) * scale) along the kept axis -> `dtype` (default: the original dtype)."""
    dtype = dtype or q.orig_dtype
    L.require_gpu(q.int_data, "dequantize(q)")
    code = L.dtype_code(dtype)
    if q.axis == 1:
        lead = 1
        for d in q.shape[:-1]:
            lead *= d
        d2 = q.int_data.reshape(lead, q.shape[-1])
    else:
        d2 = q.int_data
    d2 = L.row_major_2d(d2)
    rows, cols = d2.shape
    out = torch.empty((rows, cols), dtype=dtype, device=d2.device)
    with torch.cuda.device(d2.device):
        L.check(L.lib().pq_dequant(d2.data_ptr(), L.ld(d2), q.scale.data_ptr(), q.axis, rows, cols, out.data_ptr(),
                                   max(cols, 1), code, L.stream_ptr(d2)), "dequantize")
    return out.reshape(q.shape)
