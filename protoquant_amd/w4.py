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
    qlinear_w4_grouped(..)         the experts of a mixture-of-experts layer, stacked: w4 u8[E, N, Kp / 2], gs u8[E, ceil(N / 4), Kp / 128, 4] (per expert what w4_pack
                                   gives for wq[e]).  <= 64 grouped rows: ONE launch of the grouped weight-streaming int4 kernel over the live experts; more rows: all
                                   experts expanded into the cached workspace, then qlinear_s8_grouped.  The bits of qlinear_s8_grouped on the expanded weight either way
    int_mm_w4_grouped(..)          the exact int32 accumulators of the grouped streaming kernel (<= 64 grouped rows)
    GroupedQLinearW4               a GroupedQLinear that keeps w4 / gs instead of wq; MoEGatedMLP runs unchanged with two of them
    swap_moe_experts_w4(model, ..) opt-in: the GroupedQLinear pair of chosen MoEGatedMLP modules -> GroupedQLinearW4; call it AFTER swap_moe_experts

The activation side is unchanged: dynamic per-token int8, the same codes.  The fuse_* entries read `.wq` of the linears they merge, so they leave a QLinearW4 and what
would have fed it alone (qlinear.is_code_fed).  There is no CPU path.  Out of scope: FusedQLinear / GatedMLP over W4 weights, the sharded modules, serialize.py /
convert_checkpoint for packed weights, dense or expert (the modules' state_dict is the persistent form), MoEBlock-level changes, a grouped int4 PREFILL kernel (more than
64 grouped rows expand and run the int8 tiles), RotatedQLinear with W4 weights, zero points, other group sizes, calibration, float-activation weight-only GEMMs."""
from __future__ import annotations

import importlib

import torch
from torch import nn

from . import _lib as L
from .moe import GroupedQLinear, MoEGatedMLP
from .qlinear import (_check_operand, _epilogue_operands, _grouped_rows, _module_of, _out, _quantize_zero_tailed, _round_k, _set_buffers, _swap_children,
                      _zero_tailed, is_plain_linear, qlinear, qlinear_s8, qlinear_s8_grouped)
from .qtensor import QTensor, _launch, _on_gpu, _ptr

# qlinear.py itself (the package attribute `qlinear` is the class): its _workspace is looked up at every call, so whatever replaces qlinear._workspace serves the expand paths
_QL = importlib.import_module(".qlinear", __package__)

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
    if not (w4.is_cuda and gs.is_cuda):
        _on_gpu(what, w4=w4, gs=gs)
    dev = w4.device
    if w4.dtype != torch.uint8 or gs.dtype != torch.uint8 or gs.device != dev:
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
    if not xq.is_cuda:
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
    bias = _epilogue_operands(dev, out_dtype, xs, M, ws, bias, per=N)
    if out is not None:
        _out(out, M, N, dev, out_dtype)
    if M > min(stream_rows, STREAM_ROWS_MAX) and N:
        # the workspace is ONE buffer per (device, stream), and qlinear_s8 takes its split-K slabs from the front of it: W8 goes behind them
        with torch.cuda.device(dev):
            front = (L.lib().pq_qlinear_workspace_bytes(M, N, kp) + 255) & ~255
        w8 = _QL._workspace(dev, front + N * kp)[front:front + N * kp].view(torch.int8).view(N, kp)
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
        _set_buffers(self, torch.zeros((out_features,), dtype=dtype or torch.bfloat16, device=device) if bias else None,
                     w4=torch.zeros((out_features, kp // 2), dtype=torch.uint8, device=device),
                     gs=torch.ones(((out_features + 3) // 4, kp // GROUP, 4), dtype=torch.uint8, device=device),
                     ws=torch.ones((out_features,), dtype=torch.float32, device=device))

    @classmethod
    def from_qlinear(cls, m: qlinear) -> "QLinearW4":
        """the level-2 codes of m's int8 weight (w4_pack); ws and bias are m's own tensors"""
        if isinstance(m, QLinearW4) or not isinstance(m, qlinear) or not getattr(m, "code_fed", True):
            raise TypeError(f"QLinearW4.from_qlinear: expected a plain qlinear, got {type(m).__name__}")
        w4, gs = w4_pack(m.wq)
        r = _module_of(cls, m.bias, w4=w4, gs=gs, ws=m.ws)
        r.in_features, r.out_features, r.stream_rows = m.in_features, m.out_features, STREAM_ROWS_MAX
        return r

    @classmethod
    def from_linear(cls, lin: nn.Linear) -> "QLinearW4":
        """exactly the level-1 codes qlinear.from_linear makes (K1 over W's rows), then w4_pack"""
        return cls.from_qlinear(qlinear.from_linear(lin))

    def forward(self, x) -> torch.Tensor:
        K = self.in_features
        if x.shape[-1] != K:
            raise ValueError(f"QLinearW4: expected last dim {K}, got {x.shape[-1]}")
        if isinstance(x, QTensor) and x.axis != 1:
            raise ValueError("QLinearW4: a QTensor input must be quantised per token (axis=-1)")
        kp = _round_k(K)          # (zero-padded K: the packed tail holds zeros, so do the codes)
        if isinstance(x, QTensor):
            buf, xs, out_dtype = x.int_data.reshape(-1, K), x.scale, x.orig_dtype
            if kp != K:
                buf = _zero_tailed(buf, kp)
        else:
            (buf, xs), out_dtype = _quantize_zero_tailed(x, kp, "QLinearW4(x)"), x.dtype
        y = qlinear_w4(buf, xs, self.w4, self.gs, self.ws, self.bias, out_dtype, stream_rows=self.stream_rows)
        return y.reshape(*x.shape[:-1], self.out_features)

    def extra_repr(self):
        return f"{super().extra_repr()}, w4, stream_rows={self.stream_rows}"


def swap_linears_w4(model: nn.Module, predicate=None) -> int:
    """Replace every nn.Linear of `model` (in place) that is_plain_linear admits and for which predicate(name, module) is true (None: all) by a QLinearW4; returns the
    number replaced (a second call: 0).  `name` is the child's name in its parent, as in swap_linears.  A module that already is a qlinear is never touched.  Opt-in; call
    it BEFORE swap_linears (which then takes the remaining nn.Linear layers) and the fuse_* entries."""
    def visit(name, child):
        if isinstance(child, qlinear):
            return 0
        if is_plain_linear(child) and (predicate is None or predicate(name, child)):
            return QLinearW4.from_linear(child)
        return None
    return _swap_children(model, visit)


# ---- the experts of a mixture-of-experts layer: E packed weights stacked, the grouped contract of qlinear_s8_grouped_stream (C-ABI pq_qlinear_w4_grouped_stream)
def _grouped_call(what: str, xq, w4, gs, offsets, row_index):
    """the checks of the grouped W4 entries: (xq, w4 as the kernel walks it, E, N, Kp, M_total, the C-ABI's operand arguments up to gs_expert_stride)"""
    if not (xq.is_cuda and w4.is_cuda and gs.is_cuda):
        _on_gpu(what, xq=xq, w4=w4, gs=gs)
    dev = xq.device
    if w4.dtype != torch.uint8 or gs.dtype != torch.uint8 or w4.device != dev or gs.device != dev:
        _check_operand(w4, "w4", dev, torch.uint8); _check_operand(gs, "gs", dev, torch.uint8)
    if w4.dim() != 3 or w4.shape[0] == 0 or w4.shape[2] == 0 or w4.shape[2] % (GROUP // 2):
        raise ValueError(f"{what}: w4 must be uint8 [E, N, Kp / 2] with Kp a positive multiple of {GROUP}, got shape {tuple(w4.shape)}")
    E, N, G = w4.shape[0], w4.shape[1], w4.shape[2] // (GROUP // 2)
    quads = (N + 3) // 4
    if tuple(gs.shape) != (E, quads, G, 4) or not gs.is_contiguous():
        raise ValueError(f"{what}: gs must be a contiguous uint8 [{E}, {quads}, {G}, 4] tensor, got shape {tuple(gs.shape)} stride {gs.stride()}")
    if w4.stride(2) != 1 or w4.data_ptr() % 16 or (N > 1 and w4.stride(1) % 16) or (E > 1 and w4.stride(0) % 16):
        w4 = w4.contiguous()
    xq = _codes(what, xq, G * GROUP)
    x_args, w_args = _grouped_rows(xq, w4, G * (GROUP // 2), offsets, row_index)
    return xq, w4, E, N, G * GROUP, xq.shape[0] if row_index is None else row_index.numel(), (x_args, (*w_args, gs.data_ptr(), quads * G * 4))


def int_mm_w4_grouped(xq: torch.Tensor, w4: torch.Tensor, gs: torch.Tensor, offsets: torch.Tensor, row_index: torch.Tensor | None = None) -> torch.Tensor:
    """acc[r] = xq[src(r)] . W8[e(r)]^T, exact int32, by the grouped weight-streaming int4 kernel (C-ABI pq_gemm_s8w4s32_grouped_stream; at most 64 grouped rows) —
    int_mm_grouped_stream on the stacked w4_expand outputs.  Rows >= offsets[E] are left as allocated."""
    what = "int_mm_w4_grouped"
    xq, w4, E, N, kp, M, (x_args, w_args) = _grouped_call(what, xq, w4, gs, offsets, row_index)
    if M > STREAM_ROWS_MAX:
        raise ValueError(f"{what}: at most {STREAM_ROWS_MAX} grouped rows, got {M} (int_mm_grouped on the expanded weights takes any number)")
    acc = torch.empty((M, N), dtype=torch.int32, device=xq.device)
    if M and N:
        _launch(what, xq.device, L.lib().pq_gemm_s8w4s32_grouped_stream, *x_args, *w_args, offsets.data_ptr(), E, M, N, kp, acc.data_ptr(), N, L.stream_ptr(xq))
    return acc


def qlinear_w4_grouped(xq: torch.Tensor, xs: torch.Tensor, w4: torch.Tensor, gs: torch.Tensor, ws: torch.Tensor, bias, offsets: torch.Tensor, out_dtype,
                       row_index: torch.Tensor | None = None, out: torch.Tensor | None = None, stream_rows: int = STREAM_ROWS_MAX) -> torch.Tensor:
    """qlinear_s8_grouped(xq, xs, W8, ws, bias, offsets, out_dtype, row_index) bit for bit, W8[e] = w4_expand(w4[e], gs[e]): the operands and the contract of
    qlinear_s8_grouped (rows sorted by expert, offsets int32 [E + 1] and row_index on the device and never read on the host, xs [M_total] in grouped order, rows >=
    offsets[E] untouched) with the experts' weights stacked in the W4 format: w4 u8 [E, N, Kp / 2], gs u8 [E, ceil(N / 4), Kp / 128, 4], ws [E, N], bias [E, N] or None.
    Up to `stream_rows` grouped rows (at most 64; 0: never) ONE launch of the grouped weight-streaming int4 kernel reads the live experts' packed weights (C-ABI
    pq_qlinear_w4_grouped_stream).  More rows: ALL E experts are expanded into the cached workspace (qlinear._workspace) — E * N * Kp bytes, the size of the int8
    weight the module does not keep: 0.94 GB for eight 28672 x 4096 experts; the price of having no second prefill kernel family, as in the dense path — in one launch
    of pq_w4_expand where N % 4 == 0 (the stacked rows then share one quad layout), expert by expert otherwise, and qlinear_s8_grouped's tiles run on that.
    xq: int8 [R, Kp] — codes with a zeroed tail where K < Kp."""
    what = "qlinear_w4_grouped"
    xq, w4, E, N, kp, M, (x_args, w_args) = _grouped_call(what, xq, w4, gs, offsets, row_index)
    dev = xq.device
    code = L.dtype_code(out_dtype)
    bias = _epilogue_operands(dev, out_dtype, xs, M, ws, bias, per=(E, N))
    y = torch.empty((M, N), dtype=out_dtype, device=dev) if out is None else _out(out, M, N, dev, out_dtype)
    if M > min(stream_rows, STREAM_ROWS_MAX) and N:
        w8 = _QL._workspace(dev, E * N * kp)[:E * N * kp].view(torch.int8).view(E, N, kp)
        if N % 4 == 0 and (E == 1 or w4.stride(0) == N * w4.stride(1)):
            _expand_into(what, w4.as_strided((E * N, kp // 2), (w4.stride(1), 1)), gs, E * N, kp, w8)
        else:
            for e in range(E):
                _expand_into(what, w4[e], gs[e], N, kp, w8[e])
        return qlinear_s8_grouped(xq, xs, w8, ws, bias, offsets, out_dtype, row_index=row_index, out=y)
    if M and N:
        _launch(what, dev, L.lib().pq_qlinear_w4_grouped_stream, *x_args, xs.data_ptr(), *w_args, ws.data_ptr(), _ptr(bias), offsets.data_ptr(), E, M, N, kp,
                y.data_ptr(), L.ld(y), code, L.stream_ptr(xq))
    return y


class GroupedQLinearW4(nn.Module):
    """A GroupedQLinear whose E experts' weights are kept in the W4 format: buffers `w4` [E, N, Kp / 2], `gs` [E, ceil(N / 4), Kp / 128, 4], `ws` [E, N], `bias` [E, N]
    or None (no `wq`) — half the expert memory, and at decode about 0.51 of the weight bytes a step streams.  forward has GroupedQLinear.forward's signature and checks;
    y has the bits of a GroupedQLinear that holds the expanded weights.  stream_rows (settable per instance): up to that many grouped rows take the streaming int4
    kernel, more (or stream_rows = 0: all) expand into the workspace and run the int8 tiles (qlinear_w4_grouped).  state_dict round-trips through the buffers."""

    stream_rows = STREAM_ROWS_MAX

    def __init__(self, num_experts: int, in_features: int, out_features: int, bias: bool = False, device=None, dtype=None):
        super().__init__()
        self.num_experts, self.in_features, self.out_features = num_experts, in_features, out_features
        kp = _round_k(in_features)
        _set_buffers(self, torch.zeros((num_experts, out_features), dtype=dtype or torch.bfloat16, device=device) if bias else None,
                     w4=torch.zeros((num_experts, out_features, kp // 2), dtype=torch.uint8, device=device),
                     gs=torch.ones((num_experts, (out_features + 3) // 4, kp // GROUP, 4), dtype=torch.uint8, device=device),
                     ws=torch.ones((num_experts, out_features), dtype=torch.float32, device=device))

    @classmethod
    def from_grouped(cls, m: GroupedQLinear) -> "GroupedQLinearW4":
        """the level-2 codes of m's [E, N, K] int8 weight: ONE w4_pack over its E * N rows, the multipliers re-laid from the quads of the stacked rows into each expert's
        own ceil(N / 4) quads (rows past N hold 1) — per expert exactly w4_pack(m.wq[e]); ws and bias are m's own tensors"""
        if not isinstance(m, GroupedQLinear):
            raise TypeError(f"GroupedQLinearW4.from_grouped: expected a GroupedQLinear, got {type(m).__name__}")
        E, N, K = m.num_experts, m.out_features, m.in_features
        w4, gs = w4_pack(m.wq.reshape(E * N, K))
        G, quads = gs.shape[1], (N + 3) // 4
        g = gs.permute(0, 2, 1).reshape(-1, G)[:E * N].reshape(E, N, G)          # g[e, n, j]
        g = torch.cat([g, g.new_ones((E, quads * 4 - N, G))], dim=1)
        r = _module_of(cls, m.bias, w4=w4.view(E, N, -1), gs=g.view(E, quads, 4, G).permute(0, 1, 3, 2).contiguous(), ws=m.ws)
        r.num_experts, r.in_features, r.out_features = E, K, N
        return r

    @classmethod
    def from_weight(cls, weight: torch.Tensor, bias=None) -> "GroupedQLinearW4":
        """exactly the level-1 codes GroupedQLinear.from_weight makes, then packed"""
        return cls.from_grouped(GroupedQLinear.from_weight(weight, bias))

    @classmethod
    def from_linears(cls, linears) -> "GroupedQLinearW4":
        return cls.from_grouped(GroupedQLinear.from_linears(linears))

    codes_for_gemm = GroupedQLinear.codes_for_gemm          # (zero-tailed codes where in_features is not a multiple of 128: the packed tail holds zeros)

    def forward(self, xq: QTensor, offsets: torch.Tensor, row_index: torch.Tensor | None = None, xs: torch.Tensor | None = None) -> torch.Tensor:
        if not isinstance(xq, QTensor) or xq.axis != 1 or xq.shape[-1] != self.in_features:
            raise ValueError("GroupedQLinearW4: input must be a per-token QTensor [R, in_features]")
        codes = self.codes_for_gemm(xq.int_data.reshape(-1, self.in_features))
        if xs is None:
            xs = xq.scale if row_index is None else xq.scale.index_select(0, row_index)
        return qlinear_w4_grouped(codes, xs, self.w4, self.gs, self.ws, self.bias, offsets, xq.orig_dtype, row_index=row_index, stream_rows=self.stream_rows)

    def extra_repr(self):
        return (f"num_experts={self.num_experts}, in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, w4, "
                f"stream_rows={self.stream_rows}")


def swap_moe_experts_w4(model: nn.Module, predicate=None) -> int:
    """Replace, in place, the two GroupedQLinear members (gate_up, down) of every MoEGatedMLP of `model` for which predicate(name, module) is true (None: all) by
    GroupedQLinearW4.from_grouped; returns the number of MoEGatedMLP modules converted (a second call: 0).  `name` is the module's name in its parent, as in
    swap_linears_w4.  Opt-in; call it AFTER swap_moe_experts (which makes the MoEGatedMLP modules).  Gate kinds, the router, fuse_moe_routers and torch_plumbing are
    untouched: MoEGatedMLP reads only num_experts / in_features / out_features of its members and calls them."""
    def visit(name, child):
        if not isinstance(child, MoEGatedMLP):
            return None
        if not (isinstance(child.gate_up, GroupedQLinear) and isinstance(child.down, GroupedQLinear) and (predicate is None or predicate(name, child))):
            return 0
        child.gate_up, child.down = GroupedQLinearW4.from_grouped(child.gate_up), GroupedQLinearW4.from_grouped(child.down)
        return 1
    return _swap_children(model, visit)
