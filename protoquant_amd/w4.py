"""Int4 weights for decode, format "W4 v1" (QSPEC W1-W4): a second, INTEGER quantisation level on top of the per-channel int8 weight.  For row n and
group j of 128 consecutive k:  g = min(18, max(1, ceil(max |wq| / 7))),  q = clamp(round_half_away(wq / g), -7, 7),  and the weight the pair stands for is the ordinary
int8 matrix W8[n, k] = q[n, k] * g[n, k / 128] (|W8| <= 126).  The GEMM on the packed weight is DEFINED as qlinear_s8 on W8 — the same bits for every output dtype, with
and without bias, whatever the plan — so the format has an exact twin in the library and prefill needs no second kernel family.

    w4_pack(wq)                    int8 codes [N, K] -> (w4 u8[N, Kp / 2], gs u8[ceil(N / 4), Kp / 128, 4]); Kp = K rounded up to 128, tail codes 0
    w4_expand(w4, gs, K)           -> W8 s8[N, K]: the format's definition in code, and the prefill path
    qlinear_w4(xq, xs, w4, gs, ..) <= 64 rows: ONE launch of the weight-streaming int4 kernel (Kp / 2 + Kp / 128 weight bytes per row instead of Kp); more rows: w4_expand
                                   into the cached workspace, then qlinear_s8
    int_mm_w4(xq, w4, gs)          the exact int32 accumulators of the streaming kernel (<= 64 rows)
    QLinearW4                      a qlinear that keeps w4 / gs instead of wq (half the weight memory)
    swap_linears_w4(model, ..)     opt-in: chosen nn.Linear -> QLinearW4; call it BEFORE swap_linears (which takes the remaining layers) and the fuse_* entries

The activation side is unchanged: dynamic per-token int8, the same codes.  The fuse_* entries read `.wq` of the linears they merge, so they leave a QLinearW4 and what
would have fed it alone (qlinear.is_code_fed).  There is no CPU path.  Out of scope: a grouped (MoE) host and GroupedQLinear, FusedQLinear / GatedMLP over W4 weights, the
sharded modules, serialize.py / convert_checkpoint (the module's state_dict is the persistent form), RotatedQLinear with W4 weights, zero points, other group sizes,
calibration, float-activation weight-only GEMMs."""
from __future__ import annotations

import torch
from torch import nn

from . import _lib as L
from .qlinear import _check_operand, _round_k, _workspace, is_plain_linear, qlinear, qlinear_s8
from .qtensor import QTensor, _launch, _on_gpu, _ptr

GROUP = 128
STREAM_ROWS_MAX = 64      # rows the weight-streaming int4 kernel serves (pq_qlinear_w4 refuses more)


def _aligned_rows(t: torch.Tensor) -> torch.Tensor:
    """a 2-D operand the 16-byte loads can walk: last dim contiguous, rows a multiple of 16 bytes apart, base 16-byte aligned (1-byte elements); copies only if it must"""
    t = L.row_major_2d(t)
    if t.data_ptr() % 16 or (t.shape[0] > 1 and t.stride(0) % 16):
        t = t.contiguous()
    return t


def _packed(what: str, w4: torch.Tensor, gs: torch.Tensor):
    """the checks of a packed weight: (w4 as the kernels walk it, N, Kp)"""
    _on_gpu(what, w4=w4, gs=gs)
    dev = w4.device
    _check_operand(w4, "w4", dev, torch.uint8); _check_operand(gs, "gs", dev, torch.uint8)
    if w4.dim() != 2 or w4.shape[1] == 0 or w4.shape[1] % (GROUP // 2):
        raise ValueError(f"{what}: w4 must be uint8 [N, Kp / 2] with Kp a positive multiple of {GROUP}, got shape {tuple(w4.shape)}")
    N, G = w4.shape[0], w4.shape[1] // (GROUP // 2)
    if tuple(gs.shape) != ((N + 3) // 4, G, 4) or not gs.is_contiguous():
        raise ValueError(f"{what}: gs must be a contiguous uint8 [{(N + 3) // 4}, {G}, 4] tensor, got shape {tuple(gs.shape)} stride {gs.stride()}")
    return _aligned_rows(w4), N, G * GROUP


def w4_pack(wq: torch.Tensor):
    """int8 codes wq [N, K] (a per-channel int8 weight: quantize(w, axis=-1).int_data, qlinear.wq; any row pitch) -> (w4, gs) of the W4 format, one launch (C-ABI
    pq_w4_pack: one wave per (row, group) — the group maximum by a wave reduction, the rule, the nibble interleave)."""
    what = "w4_pack"
    _on_gpu(what, wq=wq)
    wq = L.row_major_2d(wq)
    _check_operand(wq, "wq", wq.device, torch.int8)
    N, K = wq.shape
    if K == 0:
        raise ValueError(f"{what}: wq needs at least one column")
    kp = _round_k(K)
    w4 = torch.empty((N, kp // 2), dtype=torch.uint8, device=wq.device)
    gs = torch.empty(((N + 3) // 4, kp // GROUP, 4), dtype=torch.uint8, device=wq.device)
    if N:
        _launch(what, wq.device, L.lib().pq_w4_pack, wq.data_ptr(), L.ld(wq), N, K, w4.data_ptr(), kp // 2, gs.data_ptr(), L.stream_ptr(wq))
    return w4, gs


def _expand_into(what: str, w4, gs, N, kp, w8):
    _launch(what, w4.device, L.lib().pq_w4_expand, w4.data_ptr(), L.ld(w4), gs.data_ptr(), N, kp, w8.data_ptr(), kp, L.stream_ptr(w4))


def w4_expand(w4: torch.Tensor, gs: torch.Tensor, K: int | None = None) -> torch.Tensor:
    """The int8 weight the packed pair stands for, W8[n, k] = q[n, k] * g[n, k / 128], as s8 [N, K] (C-ABI pq_w4_expand).  K=None: all Kp columns; a K in
    (Kp - 128, Kp] returns the first K columns of the [N, Kp] result (the packed tail holds zeros)."""
    what = "w4_expand"
    w4, N, kp = _packed(what, w4, gs)
    if K is not None and not kp - GROUP < K <= kp:
        raise ValueError(f"{what}: K = {K} does not round up to the packed width {kp}")
    w8 = torch.empty((N, kp), dtype=torch.int8, device=w4.device)
    if N:
        _expand_into(what, w4, gs, N, kp, w8)
    return w8 if K is None or K == kp else w8[:, :K]


def _codes(what: str, xq: torch.Tensor, kp: int) -> torch.Tensor:
    _on_gpu(what, xq=xq)
    xq = _aligned_rows(xq)
    _check_operand(xq, "xq", xq.device, torch.int8)
    if xq.shape[1] != kp:
        raise ValueError(f"{what}: shape mismatch: x has K={xq.shape[1]}, the packed weight has Kp={kp} (pad the codes with zeros)")
    return xq


def int_mm_w4(xq: torch.Tensor, w4: torch.Tensor, gs: torch.Tensor) -> torch.Tensor:
    """acc[M, N] = xq[M, Kp] . W8[N, Kp]^T, exact int32, by the weight-streaming int4 kernel (C-ABI pq_gemm_s8w4s32; at most 64 rows) — int_mm on w4_expand's output."""
    what = "int_mm_w4"
    w4, N, kp = _packed(what, w4, gs)
    xq = _codes(what, xq, kp)
    M = xq.shape[0]
    if M > STREAM_ROWS_MAX:
        raise ValueError(f"{what}: at most {STREAM_ROWS_MAX} rows, got {M} (int_mm on w4_expand's output takes any number)")
    acc = torch.empty((M, N), dtype=torch.int32, device=xq.device)
    if M and N:
        _launch(what, xq.device, L.lib().pq_gemm_s8w4s32, xq.data_ptr(), L.ld(xq), w4.data_ptr(), L.ld(w4), gs.data_ptr(), acc.data_ptr(), N, M, N, kp, L.stream_ptr(xq))
    return acc


def qlinear_w4(xq: torch.Tensor, xs: torch.Tensor, w4: torch.Tensor, gs: torch.Tensor, ws: torch.Tensor, bias, out_dtype, out: torch.Tensor | None = None,
               stream_rows: int = STREAM_ROWS_MAX) -> torch.Tensor:
    """qlinear_s8(xq, xs, w4_expand(w4, gs), ws, bias, out_dtype) bit for bit.  Up to `stream_rows` rows (at most 64; 0: never) ONE launch of the weight-streaming int4
    kernel reads the packed weight (C-ABI pq_qlinear_w4); more rows expand it into the cached workspace (qlinear._workspace) and run qlinear_s8's tiles on that.
    xq: int8 [M, Kp] — codes of the activation with a zeroed tail where K < Kp."""
    what = "qlinear_w4"
    w4, N, kp = _packed(what, w4, gs)
    xq = _codes(what, xq, kp)
    M, dev = xq.shape[0], xq.device
    code = L.dtype_code(out_dtype)
    if bias is not None and bias.dtype != out_dtype:
        bias = bias.to(out_dtype)
    _check_operand(xs, "xs", dev, torch.float32, M); _check_operand(ws, "ws", dev, torch.float32, N)
    if bias is not None:
        _check_operand(bias, "bias", dev, out_dtype, N)
    if out is not None:
        _check_operand(out, "out", dev, out_dtype)
        if out.dim() != 2 or out.shape != (M, N) or (N > 1 and out.stride(1) != 1):
            raise ValueError(f"out must be a row-major [{M}, {N}] tensor, got {tuple(out.shape)} stride {out.stride()}")
    if M > min(stream_rows, STREAM_ROWS_MAX) and N:
        # the workspace is ONE buffer per (device, stream), and qlinear_s8 takes its split-K slabs from the front of it: W8 goes behind them
        with torch.cuda.device(dev):
            front = (L.lib().pq_qlinear_workspace_bytes(M, N, kp) + 255) & ~255
        w8 = _workspace(dev, front + N * kp)[front:front + N * kp].view(torch.int8).view(N, kp)
        _expand_into(what, w4, gs, N, kp, w8)
        return qlinear_s8(xq, xs, w8, ws, bias, out_dtype, out)
    y = out if out is not None else torch.empty((M, N), dtype=out_dtype, device=dev)
    if M and N:
        _launch(what, dev, L.lib().pq_qlinear_w4, xq.data_ptr(), L.ld(xq), xs.data_ptr(), w4.data_ptr(), L.ld(w4), gs.data_ptr(), ws.data_ptr(), _ptr(bias), y.data_ptr(),
                L.ld(y), code, M, N, kp, L.stream_ptr(xq))
    return y


class QLinearW4(qlinear):
    """A qlinear whose weight is kept in the W4 format: buffers `w4`, `gs`, `ws`, `bias` (no `wq`) — half the weight memory, and at decode (up to `stream_rows` rows) about
    0.51 of the weight bytes per GEMM.  forward quantises a float input per token (K1) or takes a per-token QTensor, as qlinear.forward; y has the bits of a qlinear that
    holds w4_expand(w4, gs, in_features) as its wq.  stream_rows = 0 forces the expand path at every row count (A/B).  state_dict round-trips through the buffers."""

    code_fed = False          # (qlinear.is_code_fed: the fuse_* entries read .wq of the linears they merge)

    def __init__(self, in_features: int, out_features: int, bias: bool = True, device=None, dtype=None):
        nn.Module.__init__(self)
        self.in_features, self.out_features, self.stream_rows = in_features, out_features, STREAM_ROWS_MAX
        kp = _round_k(in_features)
        self.register_buffer("w4", torch.zeros((out_features, kp // 2), dtype=torch.uint8, device=device))
        self.register_buffer("gs", torch.ones(((out_features + 3) // 4, kp // GROUP, 4), dtype=torch.uint8, device=device))
        self.register_buffer("ws", torch.ones((out_features,), dtype=torch.float32, device=device))
        if bias:
            self.register_buffer("bias", torch.zeros((out_features,), dtype=dtype or torch.bfloat16, device=device))
        else:
            self.bias = None

    @classmethod
    def from_qlinear(cls, m: qlinear) -> "QLinearW4":
        """the level-2 codes of m's int8 weight (w4_pack); ws and bias are m's own tensors"""
        if isinstance(m, QLinearW4) or not isinstance(m, qlinear) or not getattr(m, "code_fed", True):
            raise TypeError(f"QLinearW4.from_qlinear: expected a plain qlinear, got {type(m).__name__}")
        r = cls.__new__(cls)
        nn.Module.__init__(r)
        r.in_features, r.out_features, r.stream_rows = m.in_features, m.out_features, STREAM_ROWS_MAX
        w4, gs = w4_pack(m.wq)
        r.register_buffer("w4", w4)
        r.register_buffer("gs", gs)
        r.register_buffer("ws", m.ws)
        if m.bias is not None:
            r.register_buffer("bias", m.bias)
        else:
            r.bias = None
        return r

    @classmethod
    def from_linear(cls, lin: nn.Linear) -> "QLinearW4":
        """exactly the level-1 codes qlinear.from_linear makes (K1 over W's rows), then w4_pack"""
        return cls.from_qlinear(qlinear.from_linear(lin))

    def forward(self, x) -> torch.Tensor:
        K, N = self.in_features, self.out_features
        if x.shape[-1] != K:
            raise ValueError(f"QLinearW4: expected last dim {K}, got {x.shape[-1]}")
        kp = _round_k(K)
        if isinstance(x, QTensor):
            if x.axis != 1:
                raise ValueError("QLinearW4: a QTensor input must be quantised per token (axis=-1)")
            buf, xs, out_dtype = x.int_data.reshape(-1, K), x.scale, x.orig_dtype
            if kp != K:                                   # zero-padded K: the packed tail holds zeros, so do the codes
                src, buf = buf, torch.empty((buf.shape[0], kp), dtype=torch.int8, device=buf.device)
                buf[:, :K].copy_(src)
                buf[:, K:].zero_()
        else:
            L.require_gpu(x, "QLinearW4(x)")
            code = L.dtype_code(x.dtype)
            x2 = L.row_major_2d(x.reshape(-1, K))
            M = x2.shape[0]
            buf = torch.empty((M, kp), dtype=torch.int8, device=x.device)
            if kp != K:
                buf[:, K:].zero_()
            xs = torch.empty((M,), dtype=torch.float32, device=x.device)
            _launch("quantize", x.device, L.lib().pq_quant_rowwise, x2.data_ptr(), code, M, K, L.ld(x2), buf.data_ptr(), kp, xs.data_ptr(), L.stream_ptr(x))
            out_dtype = x.dtype
        y = qlinear_w4(buf, xs, self.w4, self.gs, self.ws, self.bias, out_dtype, stream_rows=self.stream_rows)
        return y.reshape(*x.shape[:-1], N)

    def extra_repr(self):
        return f"{super().extra_repr()}, w4, stream_rows={self.stream_rows}"


def swap_linears_w4(model: nn.Module, predicate=None) -> int:
    """Replace every nn.Linear of `model` (in place) that is_plain_linear admits and for which predicate(name, module) is true (None: all) by a QLinearW4; returns the
    number replaced (a second call: 0).  `name` is the child's name in its parent, as in swap_linears.  A module that already is a qlinear is never touched.  Opt-in; call
    it BEFORE swap_linears (which then takes the remaining nn.Linear layers) and the fuse_* entries."""
    n = 0
    for name, child in list(model.named_children()):
        if isinstance(child, qlinear):
            continue
        if is_plain_linear(child) and (predicate is None or predicate(name, child)):
            setattr(model, name, QLinearW4.from_linear(child))
            n += 1
        else:
            n += swap_linears_w4(child, predicate)
    return n
