"""QTensor + quantize()/dequantize(): the Python surface BASELINE.json's north_star names.

The reference's own definitions are absent from the mount (/root/reference holds only
CODE_OF_CONDUCT.md:1-80), so signatures are build-defined and numerics follow
QSPEC v2.  All arithmetic happens in libpq_hip.so (HIP, gfx950).

Every row producer below is the same few steps, each of them written once (the private helpers that follow QTensor): the operands on the GPU (_on_gpu) and in
agreement (_check_match, _check_weight, _check_ln_group, _check_out), their 2-D row views (_rows_view, _add_rows), the outputs (_alloc), the launch (_launch) and the
result (_pack).  A public function is these calls in ITS order — the order decides which error a doubly wrong call gets — around its own argument list for the C entry."""
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


def _on_gpu(what: str, **operands):
    """every named operand on the GPU, in the order given (there is no CPU path).  These wrappers are the host side of a launch-bound decode step: the operand's name
    is formatted only for the operand that L.require_gpu is about to refuse (is_cuda: device.type == "cuda", which is what it tests)"""
    for name, t in operands.items():
        if not t.is_cuda:
            L.require_gpu(t, f"{what}({name})")


def _check_match(what: str, na: str, a: torch.Tensor, nb: str, b: torch.Tensor, devices: bool = True):
    """operand agreement: b has a's shape, dtype and device, and a has at least one dimension.  The message names the devices for the operands of an add and,
    as it always has, not for g and u (devices=False)"""
    if a.dim() < 1 or a.shape != b.shape or a.dtype != b.dtype or a.device != b.device:
        da, db = (f" {a.device}", f" {b.device}") if devices else ("", "")
        raise ValueError(f"{what}: {na} {tuple(a.shape)} {a.dtype}{da} and {nb} {tuple(b.shape)} {b.dtype}{db} must match")


def _check_out(what: str, out, like: torch.Tensor, name: str = "x"):
    """a caller's destination: on the GPU, with the shape, dtype and device of the operand `name`"""
    if out is not None:
        _on_gpu(what, out=out)
        if out.shape != like.shape or out.dtype != like.dtype or out.device != like.device:
            raise ValueError(f"{what}: out {tuple(out.shape)} {out.dtype} must have {name}'s shape {tuple(like.shape)} and dtype {like.dtype}")


def _add_rows(what: str, x: torch.Tensor, residual: torch.Tensor, out):
    """the rows of an add form, after its checks: (dtype code, x2, r2, rows, cols, summed, s2) — `summed` is `out` or a fresh tensor of x's shape, s2 its 2-D view"""
    code = L.dtype_code(x.dtype)
    x2, r2 = _rows_view(x), _rows_view(residual)
    rows, cols = x2.shape
    summed = torch.empty(x.shape, dtype=x.dtype, device=x.device) if out is None else out
    return code, x2, r2, rows, cols, summed, _rows_view_of_out(summed, rows, cols, what)


def _alloc(rows: int, cols: int, like: torch.Tensor, return_h: bool = False, host_ones_when_empty: bool = False, q=None, n_scales=None):
    """(q, scale, h) of a row producer: int8 [rows, cols], f32 [rows], and [rows, cols] of like's dtype or None.  The scales of rows without columns are 1 (QSPEC
    Q3).  The older C entries (K1, K1n, K1s and its halves) launch on such rows and the kernel writes the ones; the entries that go through check_row_producer
    (K1l, K1u, K1ng, K1gg) return before they launch anything when cols == 0, so their callers write the ones here: host_ones_when_empty.  The add forms never get
    here with an empty problem: they hand it to their non-add form.  q: a caller's own destination (the amax halves); n_scales: quantize's per-channel form keeps
    one scale per column."""
    dev = like.device
    q = torch.empty((rows, cols), dtype=torch.int8, device=dev) if q is None else q
    n = rows if n_scales is None else n_scales
    scale = torch.ones((n,), dtype=torch.float32, device=dev) if host_ones_when_empty and cols == 0 else torch.empty((n,), dtype=torch.float32, device=dev)
    return q, scale, torch.empty((rows, cols), dtype=like.dtype, device=dev) if return_h else None


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _launch(what: str, dev, entry, *args):
    """one call into the library on dev's current stream; a status other than 0 raises PQError naming `what`"""
    with torch.cuda.device(dev):
        L.check(entry(*args), what)


def _pack(like: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, h=None, summed=None, axis: int = 1, keep_q: bool = False):
    """the result of a row producer: the QTensor of like's shape, alone or as (QTensor[, summed][, h]).  keep_q: q is the caller's `out` and is returned as it is"""
    shape = like.shape
    qt = QTensor(q if keep_q else q.reshape(shape), scale, axis, like.dtype, shape)
    if summed is None:
        return qt if h is None else (qt, h.reshape(shape))
    return (qt, summed) if h is None else (qt, summed, h.reshape(shape))


def _with_sum(res, summed: torch.Tensor, return_h: bool):
    """an empty add problem has gone through the non-add form with `summed` as its input: its result with the sum put in"""
    return (res[0], summed, res[1]) if return_h else (res, summed)


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
    _on_gpu("quantize", x=x)
    code = L.dtype_code(x.dtype)
    x2, red = _as_2d(x, axis)
    x2 = L.row_major_2d(x2)
    rows, cols = x2.shape
    q, scale, _ = _alloc(rows, cols, x, n_scales=rows if red == 1 else cols)
    _launch("quantize", x.device, L.lib().pq_quant_rowwise if red == 1 else L.lib().pq_quant_colwise,
            x2.data_ptr(), code, rows, cols, L.ld(x2), q.data_ptr(), max(cols, 1), scale.data_ptr(), L.stream_ptr(x))
    return _pack(x, q, scale, axis=red)


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
    what = "silu_mul_quantize"
    _on_gpu(what, g=g, u=u)
    _check_match(what, "g", g, "u", u, devices=False)
    code = L.dtype_code(g.dtype)
    g2, u2 = _rows_view(g), _rows_view(u)
    rows, cols = g2.shape
    q, scale, h = _alloc(rows, cols, g, return_h)
    _launch(what, g.device, L.lib().pq_silu_mul_quant_rowwise, g2.data_ptr(), L.ld(g2), u2.data_ptr(), L.ld(u2), code, rows, cols, q.data_ptr(), max(cols, 1),
            scale.data_ptr(), _ptr(h), max(cols, 1), L.stream_ptr(g))
    return _pack(g, q, scale, h)


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
    what = "glu_quantize"
    _on_gpu(what, g=g, u=u)
    _check_match(what, "g", g, "u", u, devices=False)
    kcode, limit, alpha = glu_params(kind, limit, alpha)
    code = L.dtype_code(g.dtype)
    g2, u2 = _rows_view(g), _rows_view(u)
    rows, cols = g2.shape
    q, scale, h = _alloc(rows, cols, g, return_h)
    _launch(what, g.device, L.lib().pq_glu_quant_rowwise, g2.data_ptr(), L.ld(g2), u2.data_ptr(), L.ld(u2), code, rows, cols, kcode, limit, alpha, q.data_ptr(), max(cols, 1),
            scale.data_ptr(), _ptr(h), max(cols, 1), L.stream_ptr(g))
    return _pack(g, q, scale, h)


def _amax_outputs(what: str, like: torch.Tensor, rows: int, cols: int, amax_bits: torch.Tensor, out):
    """the second halves' checks of amax_bits and of a caller's `out`; returns (q, ld_q, scale) — q is `out` itself where one is given"""
    if amax_bits.dtype != torch.int32 or amax_bits.shape != (rows,) or amax_bits.device != like.device or not amax_bits.is_contiguous():
        raise ValueError(f"{what}: amax_bits must be a contiguous int32 [{rows}] tensor on {like.device}")
    if out is not None and (out.dtype != torch.int8 or out.shape != (rows, cols) or out.device != like.device or (cols > 1 and out.stride(1) != 1)):
        raise ValueError(f"{what}: out must be an int8 [{rows}, {cols}] tensor with contiguous rows")
    q, scale, _ = _alloc(rows, cols, like, q=out)
    return q, L.ld(q) if rows > 1 else max(cols, 1), scale


def silu_mul_rowamax(g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """First half of silu_mul_quantize for a column-sharded intermediate: per token, the f32 BIT PATTERN (int32 tensor [rows]) of max |silu(g)*u| over the
    columns this rank holds.  Non-negative floats (and NaNs, above +Inf) order as integers: an integer MAX over the ranks is the exact row amax."""
    what = "silu_mul_rowamax"
    _on_gpu(what, g=g, u=u)
    _check_match(what, "g", g, "u", u, devices=False)
    code = L.dtype_code(g.dtype)
    g2, u2 = _rows_view(g), _rows_view(u)
    rows, cols = g2.shape
    amax = torch.empty((rows,), dtype=torch.int32, device=g.device)
    _launch(what, g.device, L.lib().pq_silu_mul_rowamax, g2.data_ptr(), L.ld(g2), u2.data_ptr(), L.ld(u2), code, rows, cols, amax.data_ptr(), L.stream_ptr(g))
    return amax


def silu_mul_quantize_with_amax(g: torch.Tensor, u: torch.Tensor, amax_bits: torch.Tensor, out: torch.Tensor | None = None) -> QTensor:
    """Second half: the int8 codes of THESE columns against the row amax given as f32 bit patterns (int32 [rows], the max over every rank's columns), and the
    row scales amax / 127.  Column block and scale vector of the unsharded silu_mul_quantize, bit for bit.  `out`: optional int8 [rows, cols] destination."""
    what = "silu_mul_quantize_with_amax"
    _on_gpu(what, g=g, u=u)
    _check_match(what, "g", g, "u", u, devices=False)
    code = L.dtype_code(g.dtype)
    g2, u2 = _rows_view(g), _rows_view(u)
    rows, cols = g2.shape
    q, ld_q, scale = _amax_outputs(what, g, rows, cols, amax_bits, out)
    _launch(what, g.device, L.lib().pq_silu_mul_quant_rowwise_amax, g2.data_ptr(), L.ld(g2), u2.data_ptr(), L.ld(u2), code, rows, cols, amax_bits.data_ptr(), q.data_ptr(), ld_q,
            scale.data_ptr(), L.stream_ptr(g))
    return _pack(g, q, scale, keep_q=out is not None)


def rowamax(x: torch.Tensor) -> torch.Tensor:
    """First half of quantize(x, axis=-1) for an activation whose COLUMNS are sharded over ranks: per token, the f32 bit pattern (int32 [rows]) of max |x| over
    the columns this rank holds; an integer MAX over the ranks is the exact, NaN-propagating row amax."""
    what = "rowamax"
    _on_gpu(what, x=x)
    code = L.dtype_code(x.dtype)
    x2 = _rows_view(x)
    rows, cols = x2.shape
    amax = torch.empty((rows,), dtype=torch.int32, device=x.device)
    _launch(what, x.device, L.lib().pq_quant_rowamax, x2.data_ptr(), code, rows, cols, L.ld(x2), amax.data_ptr(), L.stream_ptr(x))
    return amax


def quantize_with_amax(x: torch.Tensor, amax_bits: torch.Tensor, out: torch.Tensor | None = None) -> QTensor:
    """Second half: the int8 codes of THESE columns against the row amax given as f32 bit patterns (int32 [rows]: the max over every rank's columns) and the
    row scales — the column block and the scale vector of quantize(x_whole, axis=-1), bit for bit."""
    what = "quantize_with_amax"
    _on_gpu(what, x=x)
    code = L.dtype_code(x.dtype)
    x2 = _rows_view(x)
    rows, cols = x2.shape
    q, ld_q, scale = _amax_outputs(what, x, rows, cols, amax_bits, out)
    _launch(what, x.device, L.lib().pq_quant_rowwise_amax, x2.data_ptr(), code, rows, cols, L.ld(x2), amax_bits.data_ptr(), q.data_ptr(), ld_q, scale.data_ptr(), L.stream_ptr(x))
    return _pack(x, q, scale, keep_q=out is not None)


def rmsnorm_quantize(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6, return_h: bool = False):
    """quantize(weight * (x.float() * rsqrt(mean(x.float()**2, -1) + eps)).to(x.dtype), axis=-1) in ONE pass (kernel K1
    fused into RMSNorm): the normalised activation feeding q/k/v or gate/up is reduced, scaled and encoded in registers.
    Numerics: QSPEC N1-N6 (pinned reduction order) then Q1-Q6.  return_h=True also returns the normalised activation."""
    what = "rmsnorm_quantize"
    _on_gpu(what, x=x, weight=weight)
    _check_weight(what, x, weight)
    code = L.dtype_code(x.dtype)
    x2 = _rows_view(x)
    w = weight.contiguous()
    rows, cols = x2.shape
    q, scale, h = _alloc(rows, cols, x, return_h)
    _launch(what, x.device, L.lib().pq_rmsnorm_quant_rowwise, x2.data_ptr(), L.ld(x2), w.data_ptr(), float(eps), code, rows, cols, q.data_ptr(), max(cols, 1), scale.data_ptr(),
            _ptr(h), max(cols, 1), L.stream_ptr(x))
    return _pack(x, q, scale, h)


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
    what = "add_rmsnorm_quantize"
    _on_gpu(what, x=x, residual=residual, weight=weight)
    _check_match(what, "x", x, "residual", residual)
    _check_weight(what, x, weight)
    _check_out(what, out, x)
    code, x2, r2, rows, cols, summed, s2 = _add_rows(what, x, residual, out)
    if rows == 0 or cols == 0:          # nothing to add: the empty sum through K1n (scales of empty rows are 1, QSPEC Q3)
        return _with_sum(rmsnorm_quantize(summed, weight, eps, return_h), summed, return_h)
    w = weight.contiguous()
    q, scale, h = _alloc(rows, cols, x, return_h)
    _launch(what, x.device, L.lib().pq_add_rmsnorm_quant_rowwise, x2.data_ptr(), L.ld(x2), r2.data_ptr(), L.ld(r2), s2.data_ptr(), L.ld(s2), w.data_ptr(), float(eps), code, rows,
            cols, q.data_ptr(), cols, scale.data_ptr(), _ptr(h), cols, L.stream_ptr(x))
    return _pack(x, q, scale, h, summed)


def _residual_multiplier(what: str, multiplier) -> float:
    """`multiplier` as the C-ABI takes it: a finite Python int or float (a tensor would be a device value the kernel cannot take as an argument; bool is no number here)"""
    if isinstance(multiplier, bool) or not isinstance(multiplier, (int, float)):
        raise TypeError(f"{what}: multiplier must be a Python int or float, got {type(multiplier).__name__}")
    m = float(multiplier)
    if m != m or m in (float("inf"), float("-inf")):
        raise ValueError(f"{what}: multiplier must be finite, got {multiplier!r}")
    return m


def scaled_add_rmsnorm_quantize(x: torch.Tensor, residual: torch.Tensor, multiplier, weight: torch.Tensor, eps: float = 1e-6, out: torch.Tensor | None = None,
                                return_h: bool = False):
    """summed = residual + x * multiplier, then rmsnorm_quantize(summed, weight, eps) — in ONE kernel (K1ma): the scaled residual add of the Granite decoders taken into the
    norm + quantisation that follows it.  Returns (QTensor, summed) or (QTensor, summed, h) with return_h=True; every one of them holds the bits of
    add_rmsnorm_quantize(x * multiplier, residual, weight, eps, return_h=True) with the product computed by torch (QSPEC S1: one binary32 product, rounded to the storage
    dtype BEFORE the add — two roundings, never a fused multiply-add; then A1, N1-N6, Q1-Q6).  `multiplier` is a finite Python int or float (a tensor is a TypeError); it
    is rounded once to binary32, as torch rounds a Python scalar.  x, residual, weight, `out` and the aliasing rule as add_rmsnorm_quantize.  There is no CPU path."""
    what = "scaled_add_rmsnorm_quantize"
    m = _residual_multiplier(what, multiplier)
    _on_gpu(what, x=x, residual=residual)
    _check_match(what, "x", x, "residual", residual)
    _check_out(what, out, x)
    _on_gpu(what, weight=weight)
    _check_weight(what, x, weight)
    code, x2, r2, rows, cols, summed, s2 = _add_rows(what, x, residual, out)
    if rows == 0 or cols == 0:          # nothing to add: the empty sum through K1n (scales of empty rows are 1, QSPEC Q3)
        return _with_sum(rmsnorm_quantize(summed, weight, eps, return_h), summed, return_h)
    w = weight.contiguous()
    q, scale, h = _alloc(rows, cols, x, return_h)
    _launch(what, x.device, L.lib().pq_scaled_add_rmsnorm_quant_rows, x2.data_ptr(), L.ld(x2), r2.data_ptr(), L.ld(r2), m, s2.data_ptr(), L.ld(s2), w.data_ptr(), float(eps), code,
            rows, cols, q.data_ptr(), cols, scale.data_ptr(), _ptr(h), cols, L.stream_ptr(x))
    return _pack(x, q, scale, h, summed)


def scaled_add(x: torch.Tensor, residual: torch.Tensor, multiplier, out: torch.Tensor | None = None) -> torch.Tensor:
    """residual + x * multiplier in ONE kernel (K1mo, the add-only form of K1ma: the end of a chain of Granite layers) — the bits of the torch expression (QSPEC S1, A1:
    the product is rounded to the storage dtype before the add).  Operands, `multiplier`, `out` and the aliasing rule as scaled_add_rmsnorm_quantize.  Returns the sum."""
    what = "scaled_add"
    m = _residual_multiplier(what, multiplier)
    _on_gpu(what, x=x, residual=residual)
    _check_match(what, "x", x, "residual", residual)
    _check_out(what, out, x)
    code, x2, r2, rows, cols, summed, s2 = _add_rows(what, x, residual, out)
    if rows == 0 or cols == 0:
        return summed
    _launch(what, x.device, L.lib().pq_scaled_add_rmsnorm_quant_rows, x2.data_ptr(), L.ld(x2), r2.data_ptr(), L.ld(r2), m, s2.data_ptr(), L.ld(s2), None, 0.0, code, rows, cols,
            None, cols, None, None, cols, L.stream_ptr(x))
    return summed


def layernorm_quantize(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None, eps: float = 1e-5, return_h: bool = False):
    """quantize(F.layer_norm(x, (C,), weight, bias, eps), axis=-1) in ONE pass (kernel K1l: K1 fused into LayerNorm): the normalised activation feeding c_attn /
    q, k, v / c_fc is reduced, normalised and encoded in registers.  `weight` is required (a LayerNorm without affine parameters is refused); `bias` may be None.
    Numerics: QSPEC L1-L6 (two-pass mean and variance in a pinned reduction order, one storage rounding) then Q1-Q6.  return_h=True also returns the normalised
    activation in the input dtype (stored by the same kernel)."""
    what = "layernorm_quantize"
    _on_gpu(what, x=x)
    _check_ln_group(what, x, weight, bias)
    code = L.dtype_code(x.dtype)
    x2 = _rows_view(x)
    w = weight.contiguous()
    b = bias.contiguous() if bias is not None else None
    rows, cols = x2.shape
    q, scale, h = _alloc(rows, cols, x, return_h, host_ones_when_empty=True)
    _launch(what, x.device, L.lib().pq_layernorm_quant_rowwise, x2.data_ptr(), L.ld(x2), w.data_ptr(), _ptr(b), float(eps), code, rows, cols, q.data_ptr(), max(cols, 1),
            scale.data_ptr(), _ptr(h), max(cols, 1), L.stream_ptr(x))
    return _pack(x, q, scale, h)


def add_layernorm_quantize(x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None, eps: float = 1e-5, out: torch.Tensor | None = None,
                           return_h: bool = False):
    """summed = residual + x, then layernorm_quantize(summed, weight, bias, eps) — in ONE kernel (K1al): the new residual stream is stored once and normalised, reduced
    and encoded from the registers that hold it.  Returns (QTensor, summed) or (QTensor, summed, h) with return_h=True; every one of them holds the bits of
    layernorm_quantize(residual + x, weight, bias, eps, return_h=True) with the add done by torch (QSPEC A1: one binary32 add, one storage rounding, then L1-L6, Q1-Q6).
    x and residual have the same shape, dtype and device; `bias` may be None.  `out` (optional, the same shape and dtype) receives the sum and may be x or residual
    themselves; any other tensor that overlaps an input is refused.  `summed` has x's shape."""
    what = "add_layernorm_quantize"
    _on_gpu(what, x=x, residual=residual)
    _ln_weight_on_gpu(what, weight)
    _check_match(what, "x", x, "residual", residual)
    _check_ln_params(what, x, weight, bias)
    _check_out(what, out, x)
    code, x2, r2, rows, cols, summed, s2 = _add_rows(what, x, residual, out)
    if rows == 0 or cols == 0:          # nothing to add: the empty sum through K1l (scales of empty rows are 1, QSPEC Q3)
        return _with_sum(layernorm_quantize(summed, weight, bias, eps, return_h), summed, return_h)
    w = weight.contiguous()
    b = bias.contiguous() if bias is not None else None
    q, scale, h = _alloc(rows, cols, x, return_h)
    _launch(what, x.device, L.lib().pq_add_layernorm_quant_rowwise, x2.data_ptr(), L.ld(x2), r2.data_ptr(), L.ld(r2), s2.data_ptr(), L.ld(s2), w.data_ptr(), _ptr(b), float(eps),
            code, rows, cols, q.data_ptr(), cols, scale.data_ptr(), _ptr(h), cols, L.stream_ptr(x))
    return _pack(x, q, scale, h, summed)


def _ln_weight_on_gpu(what: str, weight, suffix: str = ""):
    if weight is None:
        raise ValueError(f"{what}: weight{suffix} is None — a LayerNorm without affine parameters (elementwise_affine=False) is not supported")
    L.require_gpu(weight, f"{what}(weight{suffix})")


def _check_ln_params(what: str, x: torch.Tensor, weight, bias, suffix: str = ""):
    _check_weight(what, x, weight, suffix)
    if bias is not None:
        L.require_gpu(bias, f"{what}(bias{suffix})")
        if bias.shape != weight.shape or bias.dtype != x.dtype or bias.device != x.device:
            raise ValueError(f"{what}: bias{suffix} {tuple(bias.shape)} {bias.dtype} must match the weight{suffix} {tuple(weight.shape)} {weight.dtype}")


def _check_ln_group(what: str, x: torch.Tensor, weight, bias, suffix: str = ""):
    """the affine parameters of one LayerNorm group against the rows they normalise (add_layernorm_quantize puts its operand check between the two halves)"""
    _ln_weight_on_gpu(what, weight, suffix)
    _check_ln_params(what, x, weight, bias, suffix)


def _parallel_launch(what: str, a2, b2, c2, s2, groups, return_h: bool, like: torch.Tensor):
    """One launch of pq_parallel_layernorm_quant_rowwise on 2-D row views (a2, b2, s2 None: no add); groups: one or two (weight, bias, eps).  Returns per group
    (QTensor, h or None)."""
    rows, cols = c2.shape
    code = L.dtype_code(c2.dtype)
    ldo = lambda t: L.ld(t) if t is not None else 0                  # noqa: E731
    outs, args = [], []
    for g in (0, 1):
        if g < len(groups):
            w, b, eps = groups[g]
            args.append((w.contiguous(), b.contiguous() if b is not None else None, float(eps)))
            outs.append(_alloc(rows, cols, c2, return_h))
        else:
            outs.append((None, None, None))
            args.append((None, None, 0.0))
    (w1, b1, eps1), (w2, b2_, eps2) = args
    (q1, scale1, h1), (q2, scale2, h2) = outs
    _launch(what, c2.device, L.lib().pq_parallel_layernorm_quant_rowwise, _ptr(a2), ldo(a2), _ptr(b2), ldo(b2), c2.data_ptr(), L.ld(c2), _ptr(s2), ldo(s2),
            _ptr(w1), _ptr(b1), eps1, _ptr(w2), _ptr(b2_), eps2, code, rows, cols,
            _ptr(q1), cols, _ptr(scale1), _ptr(h1), cols, _ptr(q2), cols if q2 is not None else 0, _ptr(scale2), _ptr(h2), cols if h2 is not None else 0, L.stream_ptr(c2))
    return [(_pack(like, q, scale), h.reshape(like.shape) if h is not None else None) for q, scale, h in outs[:len(groups)]]


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
    _on_gpu(what, a=a, b=b, c=c)
    _check_match(what, "a", a, "b", b)
    _check_match(what, "a", a, "c", c)
    _check_ln_group(what, a, weight, bias)
    two = weight2 is not None
    if two:
        _check_ln_group(what, a, weight2, bias2, "2")
    elif bias2 is not None or eps2 is not None:
        raise ValueError(f"{what}: bias2 / eps2 are given without weight2 (the second norm is absent as a whole)")
    _check_out(what, out, a, "a")
    eps2 = eps if eps2 is None else eps2
    L.dtype_code(a.dtype)
    a2, b2, c2 = _rows_view(a), _rows_view(b), _rows_view(c)
    rows, cols = a2.shape
    summed = torch.empty(a.shape, dtype=a.dtype, device=a.device) if out is None else out
    s2 = _rows_view_of_out(summed, rows, cols, what)
    groups = [(weight, bias, eps)] + ([(weight2, bias2, eps2)] if two else [])
    if rows == 0 or cols == 0:          # nothing to add: the empty sum through K1l (scales of empty rows are 1, QSPEC Q3)
        res = [layernorm_quantize(summed, w, bi, e, True) for w, bi, e in groups]
    else:
        res = _parallel_launch(what, a2, b2, c2, s2, groups, return_h, a)
    ret = tuple(r[0] for r in res) + (summed,)
    return ret + tuple(r[1] for r in res) if return_h else ret


def layernorm_quantize2(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None, weight2: torch.Tensor, bias2: torch.Tensor | None, eps: float = 1e-5,
                        eps2: float | None = None, return_h: bool = False):
    """layernorm_quantize(x, weight, bias, eps) and layernorm_quantize(x, weight2, bias2, eps2) in ONE kernel (K1l2, the "dual norm" of the first block of a GPT-NeoX
    stack with a parallel residual): x is read once, its mean and variance are computed once and each norm applies its own eps, affine map and quantisation.  Returns
    (QTensor, QTensor2) or (QTensor, QTensor2, h, h2) with return_h=True, the bits of the two separate calls.  The biases may be None; eps2 defaults to eps."""
    what = "layernorm_quantize2"
    _on_gpu(what, x=x)
    if x.dim() < 1:
        raise ValueError(f"{what}: x needs at least 1 dimension")
    _check_ln_group(what, x, weight, bias)
    _check_ln_group(what, x, weight2, bias2, "2")
    eps2 = eps if eps2 is None else eps2
    L.dtype_code(x.dtype)
    x2 = _rows_view(x)
    rows, cols = x2.shape
    groups = [(weight, bias, eps), (weight2, bias2, eps2)]
    if rows == 0 or cols == 0:
        res = [layernorm_quantize(x, w, bi, e, True) for w, bi, e in groups]
    else:
        res = _parallel_launch(what, None, None, x2, None, groups, return_h, x)
    ret = tuple(r[0] for r in res)
    return ret + tuple(r[1] for r in res) if return_h else ret


def act_quantize(x: torch.Tensor, kind: str, return_h: bool = False):
    """quantize(act(x), axis=-1) in ONE pass (kernel K1u) for the unary activation of a plain two-linear MLP: kind "relu" (torch.relu), "gelu_tanh" (gelu_new,
    gelu_pytorch_tanh) or "gelu_erf" (F.gelu's default).  x may be a column slice of a wider tensor.  Numerics: QSPEC U1-U4 then Q1-Q6 — relu holds torch's bits;
    both GELUs are within 1 ulp of the input dtype of the exact value, closer to it than torch's eager kernels are, and not bit-identical to those.
    return_h=True also returns h = act(x) in the input dtype (stored by the same kernel)."""
    what = "act_quantize"
    _on_gpu(what, x=x)
    if kind not in L.ACT_KINDS:
        raise ValueError(f"act_quantize: unknown kind {kind!r}, expected one of {sorted(L.ACT_KINDS)}")
    if x.dim() < 1:
        raise ValueError("act_quantize: x needs at least 1 dimension")
    code = L.dtype_code(x.dtype)
    x2 = _rows_view(x)
    rows, cols = x2.shape
    q, scale, h = _alloc(rows, cols, x, return_h, host_ones_when_empty=True)
    _launch(what, x.device, L.lib().pq_act_quant_rowwise, x2.data_ptr(), L.ld(x2), code, rows, cols, L.ACT_KINDS[kind], q.data_ptr(), max(cols, 1), scale.data_ptr(), _ptr(h),
            max(cols, 1), L.stream_ptr(x))
    return _pack(x, q, scale, h)


def _check_weight(what: str, x: torch.Tensor, weight: torch.Tensor, suffix: str = ""):
    """norm parameters: `weight` is a [cols] vector of x's dtype on x's device"""
    if x.dim() < 1 or weight.dim() != 1 or weight.shape[0] != x.shape[-1] or weight.dtype != x.dtype or weight.device != x.device:
        raise ValueError(f"{what}: x {tuple(x.shape)} {x.dtype} needs a weight{suffix} of shape ({x.shape[-1] if x.dim() else '?'},) "
                         f"and the same dtype/device, got {tuple(weight.shape)} {weight.dtype}")


def gemma_rmsnorm_quantize(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6, return_h: bool = False):
    """quantize(((x.float() * rsqrt(mean(x.float()**2, -1) + eps)) * (1.0 + weight.float())).to(x.dtype), axis=-1) in ONE pass (kernel K1ng: K1 fused into
    GemmaRMSNorm — Gemma, Gemma-2, Gemma-3).  `weight` is the module's STORED weight w; the gain is 1 + w.  Numerics: QSPEC NG1-NG6 (N1-N4's pinned reduction
    order, then binary32 throughout and ONE storage rounding — rmsnorm_quantize with 1 + w as its weight gives other bits) then Q1-Q6.  return_h=True also returns
    the normalised activation in the input dtype (stored by the same kernel)."""
    what = "gemma_rmsnorm_quantize"
    _on_gpu(what, x=x, weight=weight)
    _check_weight(what, x, weight)
    code = L.dtype_code(x.dtype)
    x2 = _rows_view(x)
    w = weight.contiguous()
    rows, cols = x2.shape
    q, scale, h = _alloc(rows, cols, x, return_h, host_ones_when_empty=True)
    _launch(what, x.device, L.lib().pq_gemma_rmsnorm_quant_rowwise, x2.data_ptr(), L.ld(x2), w.data_ptr(), float(eps), code, rows, cols, q.data_ptr(), max(cols, 1),
            scale.data_ptr(), _ptr(h), max(cols, 1), L.stream_ptr(x))
    return _pack(x, q, scale, h)


def add_gemma_rmsnorm_quantize(x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6, out: torch.Tensor | None = None,
                               return_h: bool = False):
    """summed = residual + x, then gemma_rmsnorm_quantize(summed, weight, eps) — in ONE kernel (K1ang).  Returns (QTensor, summed) or (QTensor, summed, h) with
    return_h=True; every one of them holds the bits of gemma_rmsnorm_quantize(residual + x, weight, eps, return_h=True) with the add done by torch (QSPEC A1, then
    NG1-NG6, Q1-Q6).  x and residual have the same shape, dtype and device.  `out` (optional, the same shape and dtype) receives the sum and may be x or residual
    themselves; any other tensor that overlaps an input is refused.  `summed` has x's shape."""
    what = "add_gemma_rmsnorm_quantize"
    _on_gpu(what, x=x, residual=residual, weight=weight)
    _check_match(what, "x", x, "residual", residual)
    _check_weight(what, x, weight)
    _check_out(what, out, x)
    code, x2, r2, rows, cols, summed, s2 = _add_rows(what, x, residual, out)
    if rows == 0 or cols == 0:          # nothing to add: the empty sum through K1ng (scales of empty rows are 1, QSPEC Q3)
        return _with_sum(gemma_rmsnorm_quantize(summed, weight, eps, return_h), summed, return_h)
    w = weight.contiguous()
    q, scale, h = _alloc(rows, cols, x, return_h)
    _launch(what, x.device, L.lib().pq_add_gemma_rmsnorm_quant_rowwise, x2.data_ptr(), L.ld(x2), r2.data_ptr(), L.ld(r2), s2.data_ptr(), L.ld(s2), w.data_ptr(), float(eps), code,
            rows, cols, q.data_ptr(), cols, scale.data_ptr(), _ptr(h), cols, L.stream_ptr(x))
    return _pack(x, q, scale, h, summed)


def _postnorm_operands(what: str, x, post_weight, residual, out):
    """the shared argument checks of the post-norm calls, then their rows as _add_rows returns them"""
    _on_gpu(what, x=x, residual=residual, post_weight=post_weight)
    _check_match(what, "x", x, "residual", residual)
    _check_weight(what, x, post_weight)
    _check_out(what, out, x)
    return _add_rows(what, x, residual, out)


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
    _on_gpu(what, weight=weight)
    _check_weight(what, x, weight)
    if rows == 0 or cols == 0:          # nothing to normalise or add: the empty sum through K1ng (scales of empty rows are 1, QSPEC Q3)
        return _with_sum(gemma_rmsnorm_quantize(summed, weight, eps, return_h), summed, return_h)
    pw, w = post_weight.contiguous(), weight.contiguous()
    q, scale, h = _alloc(rows, cols, x, return_h)
    _launch(what, x.device, L.lib().pq_gemma_postnorm_add_rmsnorm_quant_rowwise, x2.data_ptr(), L.ld(x2), pw.data_ptr(), float(post_eps), r2.data_ptr(), L.ld(r2), s2.data_ptr(),
            L.ld(s2), w.data_ptr(), float(eps), code, rows, cols, q.data_ptr(), cols, scale.data_ptr(), _ptr(h), cols, L.stream_ptr(x))
    return _pack(x, q, scale, h, summed)


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
    _launch(what, x.device, L.lib().pq_gemma_postnorm_add_rmsnorm_quant_rowwise, x2.data_ptr(), L.ld(x2), pw.data_ptr(), float(post_eps), r2.data_ptr(), L.ld(r2), s2.data_ptr(),
            L.ld(s2), None, 0.0, code, rows, cols, None, cols, None, None, cols, L.stream_ptr(x))
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
    q, scale, _ = _alloc(rows, cols, x)
    _launch(what, x.device, L.lib().pq_olmo_postnorm_add_quant_rowwise, x2.data_ptr(), L.ld(x2), pw.data_ptr(), float(post_eps), r2.data_ptr(), L.ld(r2), s2.data_ptr(), L.ld(s2),
            code, rows, cols, q.data_ptr(), cols, scale.data_ptr(), L.stream_ptr(x))
    return _pack(x, q, scale, None, summed)


def olmo_postnorm_add(x: torch.Tensor, post_weight: torch.Tensor, residual: torch.Tensor, post_eps: float = 1e-6, out: torch.Tensor | None = None) -> torch.Tensor:
    """summed = residual + olmo_rmsnorm(x, post_weight, post_eps) in ONE kernel (K1oa, the form of K1oq without the quantisation: the end of a chain of post-norm-fused
    layers).  Returns `summed`, the bits of olmo_postnorm_add_quantize's (QSPEC NO1-NO5, PO1, A1).  Arguments and `out` as there."""
    what = "olmo_postnorm_add"
    code, x2, r2, rows, cols, summed, s2 = _postnorm_operands(what, x, post_weight, residual, out)
    if rows == 0 or cols == 0:
        return summed
    pw = post_weight.contiguous()
    _launch(what, x.device, L.lib().pq_olmo_postnorm_add_quant_rowwise, x2.data_ptr(), L.ld(x2), pw.data_ptr(), float(post_eps), r2.data_ptr(), L.ld(r2), s2.data_ptr(), L.ld(s2),
            code, rows, cols, None, 0, None, L.stream_ptr(x))
    return summed


def olmo_rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6, out: torch.Tensor | None = None) -> torch.Tensor:
    """(weight * (x.float() * rsqrt(mean(x.float()², -1) + eps))).to(x.dtype) in ONE kernel (K1on, the norm alone: q_norm / k_norm of OLMo-2 / OLMo-3): binary32
    throughout and ONE storage rounding (QSPEC NO1-NO5: N1-N4's pinned reduction order; spec-exact, and as close to the eager chain as two correctly rounded orders of
    the same sum are).  x may be a column slice of a wider tensor (the k slice of a fused q/k/v output).  `out` (optional, x's shape and dtype) receives the result and
    may be x itself; any other tensor that overlaps x is refused.  Returns a tensor of x's shape."""
    what = "olmo_rmsnorm"
    _on_gpu(what, x=x, weight=weight)
    _check_weight(what, x, weight)
    _check_out(what, out, x)
    code = L.dtype_code(x.dtype)
    x2 = _rows_view(x)
    rows, cols = x2.shape
    h = torch.empty(x.shape, dtype=x.dtype, device=x.device) if out is None else out
    h2 = _rows_view_of_out(h, rows, cols, what)
    if rows == 0 or cols == 0:
        return h
    w = weight.contiguous()
    _launch(what, x.device, L.lib().pq_olmo_postnorm_add_quant_rowwise, x2.data_ptr(), L.ld(x2), w.data_ptr(), float(eps), None, 0, h2.data_ptr(), L.ld(h2), code, rows, cols,
            None, 0, None, L.stream_ptr(x))
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
    _on_gpu(what, x=x, weight=weight)
    _check_weight(what, x, weight)
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
    _launch(what, x.device, L.lib().pq_head_rmsnorm, x.data_ptr(), ld_xo, ld_xi, w.data_ptr(), float(eps), L.GAIN_KINDS[kind], code, n_outer, n_inner, D, out.data_ptr(),
            n_inner * D, D, L.stream_ptr(x))
    return out


def gelu_mul_quantize(g: torch.Tensor, u: torch.Tensor, kind: str = "gelu_tanh", return_h: bool = False):
    """quantize(F.gelu(g, approximate="tanh") * u, axis=-1) in ONE pass (kernel K1gg): the activation of the down projection of a GeGLU MLP (Gemma's
    down(act_fn(gate(x)) * up(x))) is computed, reduced and encoded in registers.  g and u may be the column halves of one fused gate+up output.  Numerics: QSPEC
    GG1-GG3 — act_quantize's tanh GELU (U2) rounded to the input dtype, then the product rounded once, as the eager chain stores them — then Q1-Q6.  kind:
    "gelu_tanh" only.  return_h=True also returns h in the input dtype (stored by the same kernel)."""
    what = "gelu_mul_quantize"
    _on_gpu(what, g=g, u=u)
    if kind != "gelu_tanh":
        raise ValueError(f"gelu_mul_quantize: unsupported kind {kind!r}, expected 'gelu_tanh'")
    _check_match(what, "g", g, "u", u, devices=False)
    code = L.dtype_code(g.dtype)
    g2, u2 = _rows_view(g), _rows_view(u)
    rows, cols = g2.shape
    q, scale, h = _alloc(rows, cols, g, return_h, host_ones_when_empty=True)
    _launch(what, g.device, L.lib().pq_gelu_mul_quant_rowwise, g2.data_ptr(), L.ld(g2), u2.data_ptr(), L.ld(u2), code, rows, cols, L.ACT_KINDS[kind], q.data_ptr(), max(cols, 1),
            scale.data_ptr(), _ptr(h), max(cols, 1), L.stream_ptr(g))
    return _pack(g, q, scale, h)


def dequantize(q: QTensor, dtype: torch.dtype | None = None) -> torch.Tensor:
    """cast_rne(f32(int_data) * scale) along the kept axis -> `dtype` (default: the original dtype)."""
    dtype = dtype or q.orig_dtype
    _on_gpu("dequantize", q=q.int_data)
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
    _launch("dequantize", d2.device, L.lib().pq_dequant, d2.data_ptr(), L.ld(d2), q.scale.data_ptr(), q.axis, rows, cols, out.data_ptr(), max(cols, 1), code, L.stream_ptr(d2))
    return out.reshape(q.shape)
