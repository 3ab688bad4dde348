"""qlinear: the nn.Linear replacement of the contract (BASELINE.json north_star) + swap_linears().

forward(x[..., K]) = K1 row-quant(x) -> K3 s8xs8->s32 MFMA GEMM -> K4 fused (row-scale x col-scale
(+bias)) epilogue, all inside libpq_hip.so.  Weights are quantised once, per output channel, when
the module is built.  Reference definitions are absent from the mount (/root/reference holds only
CODE_OF_CONDUCT.md:1-80); semantics follow QSPEC v2."""
from __future__ import annotations

import torch
from torch import nn

from . import _lib as L
from .qtensor import QTensor, _launch, _ptr, gelu_mul_quantize, quantize, silu_mul_quantize


def int_mm(xq: torch.Tensor, wq: torch.Tensor) -> torch.Tensor:
    """acc[M,N] = xq[M,K] . wq[N,K]^T, exact int32 — the GPU twin of torch._int_mm(xq, wq.t())."""
    L.require_gpu(xq, "int_mm(xq)")
    xq, wq = L.row_major_2d(xq), L.row_major_2d(wq)
    M, K = xq.shape
    N, K2 = wq.shape
    if K != K2 or xq.dtype != torch.int8 or wq.dtype != torch.int8:
        raise ValueError("int_mm expects int8 [M,K] and int8 [N,K]")
    if _pad_pays(M, N, K):
        K = _round_k(K)
        xq, wq = _zero_tailed(xq, K), _zero_tailed(wq, K)
    acc = torch.empty((M, N), dtype=torch.int32, device=xq.device)
    _launch("int_mm", xq.device, L.lib().pq_gemm_s8s8s32, xq.data_ptr(), L.ld(xq), wq.data_ptr(), L.ld(wq), acc.data_ptr(), max(N, 1), M, N, K, L.stream_ptr(xq))
    return acc


_WORKSPACES: dict = {}     # (device, stream) -> [buffer, handed out under a hipGraph capture?]
_RETIRED: list = []        # outgrown buffers whose address a captured hipGraph holds


def _workspace(device, nbytes: int) -> torch.Tensor:
    """Caller-owned scratch (split-K slabs, the one-call path's codes and scales): one buffer per (device, stream) — reuse is
    ordered by the stream, and two streams never share a buffer.  It grows geometrically (at least 2x), so a run with rising M
    reallocates O(log) times.  An outgrown buffer is simply dropped — the caching allocator hands its memory out again in stream
    order, which is safe because every use of it was enqueued on this stream before the free — UNLESS it was ever handed out while
    a hipGraph was being captured (whether it was allocated during that capture or eagerly before it, the usual warm-up): a captured
    launch keeps the raw address, so such a buffer is parked until clear_workspaces()."""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    capturing = torch.cuda.is_current_stream_capturing()
    ent = _WORKSPACES.get(key)
    if ent is None or ent[0].numel() < nbytes:
        if ent is not None and ent[1]:
            _RETIRED.append(ent[0])
        size = nbytes if ent is None else max(nbytes, 2 * ent[0].numel())
        ent = [torch.empty((size,), dtype=torch.uint8, device=device), False]
        _WORKSPACES[key] = ent
    if capturing:
        ent[1] = True          # graph-pinned from now on: replays write through this address
    return ent[0]


def clear_workspaces() -> None:
    """Drop every cached workspace (call when no captured hipGraph that used this module will be replayed again)."""
    _WORKSPACES.clear()
    _RETIRED.clear()


def _check_operand(t, name: str, dev, dtype, numel=None):
    """The C-ABI takes raw pointers: a CPU tensor, a wrong dtype or a strided vector would be read as garbage (or fault)."""
    if t.device != dev:
        raise L.PQError(f"{name} is on {t.device}, expected {dev}: protoquant_amd has no CPU fallback — move the module / tensor to the GPU")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if numel is not None and (t.dim() != 1 or t.numel() != numel or (numel > 1 and t.stride(0) != 1)):
        raise ValueError(f"{name} must be a contiguous vector of {numel} elements, got shape {tuple(t.shape)} stride {t.stride()}")


def _round_k(K: int) -> int:
    return -(-K // 128) * 128


def _zero_tailed(codes: torch.Tensor, kp: int) -> torch.Tensor:
    """int8 codes [M, K] -> the operand a GEMM over kp >= K columns reads: the codes themselves when kp == K, else a fresh [M, kp] buffer with a zeroed tail (zeros add
    nothing to an integer sum)"""
    K = codes.shape[1]
    if kp == K:
        return codes
    buf = torch.empty((codes.shape[0], kp), dtype=torch.int8, device=codes.device)
    buf[:, :K].copy_(codes)
    buf[:, K:].zero_()
    return buf


def _quantize_zero_tailed(x: torch.Tensor, kp: int, where: str):
    """float rows x[..., K] -> (codes int8 [M, kp], xs f32 [M]): kernel K1 quantises per token straight into a buffer of kp >= K columns whose tail is zeroed"""
    L.require_gpu(x, where)
    code = L.dtype_code(x.dtype)
    K = x.shape[-1]
    x2 = L.row_major_2d(x.reshape(-1, K))
    M = x2.shape[0]
    buf = torch.empty((M, kp), dtype=torch.int8, device=x.device)
    if kp != K:
        buf[:, K:].zero_()
    xs = torch.empty((M,), dtype=torch.float32, device=x.device)
    _launch("quantize", x.device, L.lib().pq_quant_rowwise, x2.data_ptr(), code, M, K, L.ld(x2), buf.data_ptr(), kp, xs.data_ptr(), L.stream_ptr(x))
    return buf, xs


def _pad_pays(M: int, N: int, K: int) -> bool:
    """The functional entry points with a K that is not a multiple of 128: the C-ABI would run its generic kernel (~300 TOPS, and ~50 when the rows are not 16-byte
    aligned) where the MFMA tiles do 2000+.  Copying BOTH operands into zero-tailed buffers of the next multiple of 128 costs two int8 copies and four small launches
    (~10 us + (M + N) K bytes); it pays from about 2^31 multiply-adds on (4096 x 4096 x 4000: 429 -> ~80 us).  Same bits: zeros add nothing to an integer sum.
    (The modules keep a padded weight copy instead of making one per call: _KPadded.)"""
    return K % 128 != 0 and K > 0 and M * N * K >= (1 << 31)


# The entries below are the host side of a launch-bound decode step: a helper is called where it stands for several checks, L.require_gpu and the dtype checks of the codes
# only once a cheap test says they will refuse, and a fresh output is allocated in place.
def _out(out: torch.Tensor, rows: int, cols: int, dev, dtype, terse: bool = False) -> torch.Tensor:
    """A caller's `out`, refused unless it is a row-major [rows, cols] tensor of `dtype` on `dev`.  terse: qlinear_s8_t's and qlinear_s8_kslabs' one refusal"""
    if terse:
        if out.device != dev or out.dtype != dtype or out.shape != (rows, cols) or (cols > 1 and out.stride(1) != 1):
            raise ValueError(f"out must be a row-major [{rows}, {cols}] {dtype} tensor on {dev}")
        return out
    _check_operand(out, "out", dev, dtype)
    if out.dim() != 2 or out.shape != (rows, cols) or (cols > 1 and out.stride(1) != 1):
        raise ValueError(f"out must be a row-major [{rows}, {cols}] tensor, got {tuple(out.shape)} stride {out.stride()}")
    return out


def _epilogue_operands(dev, out_dtype, xs, M: int, ws, bias, per):
    """What every fused entry checks about its epilogue, in this order: the bias cast to out_dtype; xs f32 [M] (None: the entry makes its own); ws f32 and bias — vectors
    of `per` elements, or contiguous [E, N] tensors where `per` is that shape (the grouped entries).  Returns the bias the library reads."""
    if bias is not None and bias.dtype != out_dtype:
        bias = bias.to(out_dtype)
    if xs is not None:
        _check_operand(xs, "xs", dev, torch.float32, M)
    if type(per) is int:
        _check_operand(ws, "ws", dev, torch.float32, per)
        if bias is not None:
            _check_operand(bias, "bias", dev, out_dtype, per)
        return bias
    _check_operand(ws, "ws", dev, torch.float32)
    if bias is not None:
        _check_operand(bias, "bias", dev, out_dtype)
    ws_fits = tuple(ws.shape) == per and ws.is_contiguous()
    if not ws_fits or (bias is not None and (tuple(bias.shape) != per or not bias.is_contiguous())):
        name, t = ("bias", bias) if ws_fits else ("ws", ws)
        raise ValueError(f"{name} must be a contiguous [{per[0]}, {per[1]}] tensor, got shape {tuple(t.shape)} stride {t.stride()}")
    return bias


def _launch_with_workspace(what: str, on: torch.Tensor, entry, query, qargs, *args, at_least: int = 0):
    """Query, workspace, launch: entry(*args, workspace | NULL, its bytes, stream) on the current stream of `on`'s device, with the bytes query(*qargs) asks for out of the
    cached workspace.  Query and launch run under the tensor's device: the planner's thresholds follow the CURRENT device's CU count.  at_least: the entry always wants a
    workspace, of that many bytes or more, and is told the size of the one it gets (pq_qlinear_dyn)."""
    dev = on.device
    with torch.cuda.device(dev):
        wbytes = query(*qargs)          # > 0: split-K pays for this shape (or the entry keeps codes and scales there)
        if at_least:
            wsp = _workspace(dev, max(wbytes, at_least))
            L.check(entry(*args, wsp.data_ptr(), wsp.numel(), L.stream_ptr(on)), what)
        else:
            L.check(entry(*args, _workspace(dev, wbytes).data_ptr() if wbytes else None, wbytes, L.stream_ptr(on)), what)


def _qlinear_s8(what: str, transposed: bool, xq, xs, wq, ws, bias, out_dtype, out):
    """qlinear_s8 / qlinear_s8_t: the output [M, N] or [N, M]"""
    xq, wq = L.row_major_2d(xq), L.row_major_2d(wq)
    M, K = xq.shape
    N = wq.shape[0]
    if wq.shape[1] != K:
        raise ValueError(f"shape mismatch: x has K={K}, weight has K={wq.shape[1]}")
    code = L.dtype_code(out_dtype)
    dev = xq.device
    if xq.dtype != torch.int8 or wq.dtype != torch.int8 or wq.device != dev:
        _check_operand(xq, "xq", dev, torch.int8); _check_operand(wq, "wq", dev, torch.int8)
    bias = _epilogue_operands(dev, out_dtype, xs, M, ws, bias, per=N)
    rows, cols = (N, M) if transposed else (M, N)
    y = torch.empty((rows, cols), dtype=out_dtype, device=dev) if out is None else _out(out, rows, cols, dev, out_dtype, terse=transposed)
    if K % 128 and _pad_pays(M, N, K):
        K = _round_k(K)
        xq, wq = _zero_tailed(xq, K), _zero_tailed(wq, K)
    lib = L.lib()
    entry, query = (lib.pq_qlinear_s8_t, lib.pq_qlinear_t_workspace_bytes) if transposed else (lib.pq_qlinear_s8, lib.pq_qlinear_workspace_bytes)
    _launch_with_workspace(what, xq, entry, query, (M, N, K), xq.data_ptr(), L.ld(xq), xs.data_ptr(), wq.data_ptr(), L.ld(wq), ws.data_ptr(),
                           bias.data_ptr() if bias is not None else None, y.data_ptr(), L.ld(y), code, M, N, K)
    return y


def qlinear_s8(xq: torch.Tensor, xs: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, bias, out_dtype,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """Fused int8 GEMM + dequant epilogue on pre-quantised operands (C-ABI pq_qlinear_s8)."""
    if not xq.is_cuda:
        L.require_gpu(xq, "qlinear_s8(xq)")
    return _qlinear_s8("qlinear_s8", False, xq, xs, wq, ws, bias, out_dtype, out)


def qlinear_s8_t(xq: torch.Tensor, xs: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, bias, out_dtype,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """The same fused GEMM + epilogue with the output TRANSPOSED: returns yt[N, M], yt[n][m] bit-identical to
    qlinear_s8(...)[m][n] (C-ABI pq_qlinear_s8_t).  The column-sharded configuration gathers these row blocks contiguously."""
    if not xq.is_cuda:
        L.require_gpu(xq, "qlinear_s8_t(xq)")
    return _qlinear_s8("qlinear_s8_t", True, xq, xs, wq, ws, bias, out_dtype, out)


def qlinear_s8_kslabs(xq_stacked: torch.Tensor, xs: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, bias, out_dtype,
                      out: torch.Tensor | None = None) -> torch.Tensor:
    """qlinear_s8 on STACKED activation codes xq_stacked[G, M, K/G] (contiguous: what an all-gather of the ranks' int8 column blocks leaves): slab s holds the
    columns [s*K/G, (s+1)*K/G) of the logical xq[M, K].  Same bits as qlinear_s8 on the row-major matrix (an integer sum has no order); the 128 x 128 ring tile
    walks the slabs in place, and so does the fused split-K of the 256 x 256 tile where the planner runs it (the Llama-70B `down` shard); every other shape takes one
    layout pass inside the call (C-ABI pq_qlinear_s8_kslabs)."""
    L.require_gpu(xq_stacked, "qlinear_s8_kslabs(xq)")
    if xq_stacked.dim() != 3 or not xq_stacked.is_contiguous():
        raise ValueError("qlinear_s8_kslabs: activation codes must be a contiguous [G, M, K/G] int8 tensor")
    G, M, kps = xq_stacked.shape
    K = G * kps
    wq = L.row_major_2d(wq)
    N = wq.shape[0]
    if wq.shape[1] != K:
        raise ValueError(f"shape mismatch: stacked x has K={K}, weight has K={wq.shape[1]}")
    code = L.dtype_code(out_dtype)
    dev = xq_stacked.device
    _check_operand(xq_stacked, "xq", dev, torch.int8); _check_operand(wq, "wq", dev, torch.int8)
    bias = _epilogue_operands(dev, out_dtype, xs, M, ws, bias, per=N)
    y = torch.empty((M, N), dtype=out_dtype, device=dev) if out is None else _out(out, M, N, dev, out_dtype, terse=True)
    slabs = (xq_stacked.data_ptr(), kps, M * kps, kps)
    # the exact query (it looks at the operands' alignment and strides): the fused split-K's hand-over slabs where the 256 x 256 tile walks the blocks in place,
    # nothing where a ring tile does, the layout pass's M * K bytes otherwise
    _launch_with_workspace("qlinear_s8_kslabs", xq_stacked, L.lib().pq_qlinear_s8_kslabs, L.lib().pq_qlinear_kslabs_workspace_bytes_for,
                           (*slabs, wq.data_ptr(), L.ld(wq), M, N, K), *slabs, xs.data_ptr(), wq.data_ptr(), L.ld(wq), ws.data_ptr(), _ptr(bias), y.data_ptr(), L.ld(y),
                           code, M, N, K)
    return y


def _grouped_rows(xq, w, width: int, offsets, row_index):
    """What the grouped entries, int8 and int4, share once xq [R, K] and the stacked weight w [E, N, width] (int8 codes, or packed int4: K / 2 bytes a row) have passed
    their own checks: offsets int32 [E + 1] and row_index int32 [M_total] are contiguous device vectors.  Returns the C-ABI's x-side arguments and its weight-side ones
    (pointer, row pitch, expert stride)."""
    dev = xq.device
    E, N = w.shape[0], w.shape[1]
    _check_operand(offsets, "offsets", dev, torch.int32, E + 1)
    if row_index is not None:
        if row_index.dim() != 1:
            raise ValueError(f"row_index must be a vector, got shape {tuple(row_index.shape)}")
        _check_operand(row_index, "row_index", dev, torch.int32, row_index.numel())
    ldw = w.stride(1) if N > 1 else width
    return ((xq.data_ptr(), L.ld(xq), row_index.data_ptr() if row_index is not None else None, xq.shape[0]),
            (w.data_ptr(), ldw, w.stride(0) if E > 1 else N * ldw))


def _grouped_operands(what: str, xq, wq, offsets, row_index):
    """Shared checks of the grouped int8 entry points: xq int8 [R, K] row-major, wq int8 [E, N, K] (K contiguous, one stride between experts).  Returns (xq, wq as the
    kernels walk them — the caller keeps both alive over the launch —, E, N, K, M_total); offsets and row_index are _grouped_rows' to check."""
    if not xq.is_cuda:
        L.require_gpu(xq, f"{what}(xq)")
    xq = L.row_major_2d(xq)
    dev = xq.device
    if xq.dtype != torch.int8 or wq.dtype != torch.int8 or wq.device != dev:
        _check_operand(xq, "xq", dev, torch.int8); _check_operand(wq, "wq", dev, torch.int8)
    if wq.dim() != 3:
        raise ValueError(f"{what}: wq must be int8 [E, N, K], got shape {tuple(wq.shape)}")
    E, N, K = wq.shape
    if xq.shape[1] != K:
        raise ValueError(f"shape mismatch: x has K={xq.shape[1]}, the experts' weights have K={K}")
    if K % 128 != 0 or K == 0:
        raise ValueError(f"{what}: K = {K} must be a positive multiple of 128 (GroupedQLinear pads its weights; pad the codes with zeros)")
    if (K > 1 and wq.stride(2) != 1) or (N > 1 and wq.stride(1) < K) or (E > 1 and wq.stride(0) < N * wq.stride(1)):
        wq = wq.contiguous()
    return xq, wq, E, N, K, (xq.shape[0] if row_index is None else row_index.numel())


def _qlinear_s8_grouped(what: str, max_rows, xq, xs, wq, ws, bias, offsets, out_dtype, row_index, out):
    """qlinear_s8_grouped / qlinear_s8_grouped_stream: one set of operand checks, then the C-ABI entry point pq_<what>"""
    xq, wq, E, N, K, M = _grouped_operands(what, xq, wq, offsets, row_index)
    if max_rows is not None and M > max_rows:
        raise ValueError(f"{what}: at most {max_rows} grouped rows, got {M} (qlinear_s8_grouped takes any number)")
    x_args, w_args = _grouped_rows(xq, wq, K, offsets, row_index)
    dev = xq.device
    code = L.dtype_code(out_dtype)
    bias = _epilogue_operands(dev, out_dtype, xs, M, ws, bias, per=(E, N))
    y = torch.empty((M, N), dtype=out_dtype, device=dev) if out is None else _out(out, M, N, dev, out_dtype)
    with torch.cuda.device(dev):
        L.check(getattr(L.lib(), "pq_" + what)(*x_args, xs.data_ptr(), *w_args, ws.data_ptr(), bias.data_ptr() if bias is not None else None, offsets.data_ptr(),
                                               E, M, N, K, y.data_ptr(), L.ld(y), code, L.stream_ptr(xq)), what)
    return y


def _int_mm_grouped(what: str, entry: str, max_rows, xq, wq, offsets, row_index, out):
    xq, wq, E, N, K, M = _grouped_operands(what, xq, wq, offsets, row_index)
    if max_rows is not None and M > max_rows:
        raise ValueError(f"{what}: at most {max_rows} grouped rows, got {M} (int_mm_grouped takes any number)")
    x_args, w_args = _grouped_rows(xq, wq, K, offsets, row_index)
    acc = torch.empty((M, N), dtype=torch.int32, device=xq.device) if out is None else _out(out, M, N, xq.device, torch.int32)
    _launch(what, xq.device, getattr(L.lib(), entry), *x_args, *w_args, offsets.data_ptr(), E, M, N, K, acc.data_ptr(), L.ld(acc), L.stream_ptr(xq))
    return acc


def qlinear_s8_grouped(xq: torch.Tensor, xs: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, bias, offsets: torch.Tensor, out_dtype,
                       row_index: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """The fused int8 GEMM + dequant epilogue over ALL experts of a mixture-of-experts layer in one launch (C-ABI pq_qlinear_s8_grouped): the rows are a token list sorted by
    expert, rows offsets[e] .. offsets[e + 1] - 1 (int32 [E + 1], on the device — it is never read on the host) go through expert e's weight wq[e] ([E, N, K] int8),
    scales ws[e] ([E, N]) and bias[e].  row_index (int32 [M_total], optional): row r reads its codes from row row_index[r] of xq, the un-permuted [T, K] code matrix;
    without it xq is already in grouped order.  xs [M_total] is always in grouped order.  Every row has the bits of qlinear_s8 run per expert on its row slice; rows
    >= offsets[E] of the output are left untouched."""
    return _qlinear_s8_grouped("qlinear_s8_grouped", None, xq, xs, wq, ws, bias, offsets, out_dtype, row_index, out)


def int_mm_grouped(xq: torch.Tensor, wq: torch.Tensor, offsets: torch.Tensor, row_index: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """The exact int32 accumulators of qlinear_s8_grouped (C-ABI pq_gemm_s8s8s32_grouped): acc[r] = xq[src(r)] . wq[e(r)]^T — int_mm per expert, in one launch."""
    return _int_mm_grouped("int_mm_grouped", "pq_gemm_s8s8s32_grouped", None, xq, wq, offsets, row_index, out)


STREAM_ROWS_MAX = 64      # grouped rows the weight-streaming grouped kernel serves (pq_qlinear_s8_grouped_stream refuses more)


def qlinear_s8_grouped_stream(xq: torch.Tensor, xs: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, bias, offsets: torch.Tensor, out_dtype,
                              row_index: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """qlinear_s8_grouped for DECODE steps — at most 64 grouped rows — through the weight-streaming grouped kernel (C-ABI pq_qlinear_s8_grouped_stream): the same operands,
    the same checks and the same bits, but every expert that owns a row has its weight streamed once, straight into MFMA operands, by several waves per 16-row block,
    instead of being staged for a 64-row tile that holds one or two rows.  offsets / row_index stay on the device; more than 64 grouped rows is an error."""
    return _qlinear_s8_grouped("qlinear_s8_grouped_stream", STREAM_ROWS_MAX, xq, xs, wq, ws, bias, offsets, out_dtype, row_index, out)


def int_mm_grouped_stream(xq: torch.Tensor, wq: torch.Tensor, offsets: torch.Tensor, row_index: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """The exact int32 accumulators of qlinear_s8_grouped_stream (C-ABI pq_gemm_s8s8s32_grouped_stream): int_mm_grouped for at most 64 grouped rows."""
    return _int_mm_grouped("int_mm_grouped_stream", "pq_gemm_s8s8s32_grouped_stream", STREAM_ROWS_MAX, xq, wq, offsets, row_index, out)


def qlinear_dyn(x: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, bias=None) -> torch.Tensor:
    """x[..., K] -> y[..., N]: dynamic per-token quant + int8 GEMM + fused dequant in ONE C-ABI call (pq_qlinear_dyn);
    the scratch (xq, xs, split-K slabs) lives in the per-device workspace."""
    L.require_gpu(x, "qlinear(x)")
    code = L.dtype_code(x.dtype)
    K = x.shape[-1]
    lead = 1
    for d in x.shape[:-1]:
        lead *= d
    x2 = L.row_major_2d(x.reshape(lead, K))
    wq = L.row_major_2d(wq)
    N = wq.shape[0]
    if wq.shape[1] != K:
        raise ValueError(f"shape mismatch: x has K={K}, weight has K={wq.shape[1]}")
    _check_operand(wq, "wq", x.device, torch.int8)
    bias = _epilogue_operands(x.device, x.dtype, None, lead, ws, bias, per=N)
    if K % 128 and _pad_pays(lead, N, K):
        xq = quantize(x2, axis=-1)
        return qlinear_s8(xq.int_data, xq.scale, wq, ws, bias, x.dtype).reshape(*x.shape[:-1], N)
    y = torch.empty((lead, N), dtype=x.dtype, device=x.device)
    lib = L.lib()
    _launch_with_workspace("qlinear_dyn", x, lib.pq_qlinear_dyn, lib.pq_qlinear_dyn_workspace_bytes, (lead, N, K), x2.data_ptr(), code, L.ld(x2),
                           wq.data_ptr(), L.ld(wq), ws.data_ptr(), _ptr(bias), y.data_ptr(), max(N, 1), lead, N, K, at_least=256)
    return y.reshape(*x.shape[:-1], N)


class _KPadded:
    """in_features that is not a multiple of 128 (GPT-2 XL's 1600, a 4000-wide projection): the MFMA tiles step through K in 128-byte K-tiles, and the C-ABI sends any
    other K to the generic kernel — 4 to 25x slower than the bf16 nn.Linear it replaces (measured: 4096 x 4096 x 4000 429 us against 99).  The modules therefore keep a
    zero-padded copy of their int8 weight, [N, round_up(K, 128)], made lazily and remade whenever `wq` changes (load_state_dict, .to()), and quantise the activation
    into a buffer of the same width whose tail is zeroed: zeros add nothing to an integer sum, so every accumulator — and every output bit — is the unpadded problem's.
    `wq` itself stays [N, K]: state dicts, fusion and sharding see the unpadded weight."""

    def _wq_for_gemm(self):
        K = self.in_features
        kp = _round_k(K)
        if kp == K or K == 0:
            return self.wq, K
        # keyed on the tensor OBJECT (held by a weak reference) and its version counter, not on its address: a weight replaced by a fresh tensor (module.to('cpu') ->
        # load_state_dict -> .to('cuda'), load_state_dict(assign=True) after a del) starts again at version 0 and can be handed the very address the caching allocator
        # just freed — an address-based key would then match and the GEMM would run on the OLD padded weight
        import weakref
        wq = self.wq
        # ... and ALSO on the address: `module.wq.data = other` / `wq.set_(...)` keep the Python object and do not bump its version
        key = (wq._version, wq.device, tuple(wq.shape), wq.data_ptr(), wq.storage_offset())
        c = self.__dict__.get("_wq_pad")
        if c is None or c[0] != key or c[2]() is not wq:
            w = wq.new_zeros((*wq.shape[:-1], kp))          # ([N, K], or GroupedQLinear's [E, N, K])
            w[..., :K].copy_(wq)
            c = (key, w, weakref.ref(wq))
            self.__dict__["_wq_pad"] = c
        return c[1], kp

    def __getstate__(self):
        """pickling / torch.save of a module: the lazily built padded copy (and the weak reference that keys it) is a cache, not state"""
        state = super().__getstate__()
        if "_wq_pad" in state:
            state = dict(state)
            del state["_wq_pad"]
        return state

    def _padded_forward(self, x, wq_pad, kp):
        """x: float [..., K] or a per-token QTensor; the GEMM runs over kp = round_up(K, 128) with zero tails on both operands."""
        if isinstance(x, QTensor):
            buf, xs, out_dtype = _zero_tailed(x.int_data.reshape(-1, self.in_features), kp), x.scale, x.orig_dtype
        else:
            (buf, xs), out_dtype = _quantize_zero_tailed(x, kp, "qlinear(x)"), x.dtype
        y = qlinear_s8(buf, xs, wq_pad, self.ws, self.bias, out_dtype)
        return y.reshape(*x.shape[:-1], self.out_features)


def gemm_operands(local: "_KPadded", codes: torch.Tensor):
    """(codes, wq) for one GEMM of a module that owns `wq`: as they are when in_features is a multiple of 128, else both zero-padded to the next one (_KPadded).
    codes: int8 [M, in_features]."""
    if local.in_features % 128 == 0 or not codes.is_cuda:      # (CPU stand-ins of the gloo host-logic tests pass through)
        return codes, local.wq
    wq, kp = local._wq_for_gemm()
    return _zero_tailed(codes, kp), wq


def _set_buffers(m: nn.Module, bias, **weights) -> nn.Module:
    """the buffers of a quantised linear module, in state_dict order: the weight's tensors (wq | w4, gs; ws), then `bias` — a buffer, or the attribute None"""
    for name, t in weights.items():
        m.register_buffer(name, t)
    if bias is not None:
        m.register_buffer("bias", bias)
    else:
        m.bias = None
    return m


def _module_of(cls, bias, **weights) -> nn.Module:
    """a `cls` made of existing tensors, past its __init__ (which would allocate them)"""
    m = cls.__new__(cls)
    nn.Module.__init__(m)
    return _set_buffers(m, bias, **weights)


class qlinear(_KPadded, nn.Module):
    """Drop-in for nn.Linear with dynamic per-token int8 activations and per-channel int8 weights."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True, device=None, dtype=None):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        _set_buffers(self, torch.zeros((out_features,), dtype=dtype or torch.bfloat16, device=device) if bias else None,
                     wq=torch.zeros((out_features, in_features), dtype=torch.int8, device=device), ws=torch.ones((out_features,), dtype=torch.float32, device=device))

    @classmethod
    def from_linear(cls, lin: nn.Linear) -> "qlinear":
        """Quantise lin.weight [N,K] per output channel on the GPU (kernel K1 over W's rows)."""
        w = lin.weight.detach()
        L.require_gpu(w, "qlinear.from_linear(weight)")
        return cls.from_qtensor(quantize(w, axis=-1), lin.bias.detach().clone() if lin.bias is not None else None)

    @classmethod
    def from_kn_weight(cls, weight_kn: torch.Tensor, bias=None) -> "qlinear":
        """A weight STORED [in_features, out_features] (y = x @ W + b: Hugging Face GPT-2's Conv1D): per-output-channel quantisation along the strided axis of the
        matrix as it lies in memory (kernel K2 — no transposed bf16 copy is made), then ONE transpose of the int8 codes into the [N, K] layout the GEMM streams.
        Codes and scales are those of from_linear on the transposed weight, bit for bit (the same max and the same quotients, reduced along the other axis)."""
        w = weight_kn.detach()
        L.require_gpu(w, "qlinear.from_kn_weight(weight)")
        if w.dim() != 2:
            raise ValueError("from_kn_weight expects a 2-D [in_features, out_features] weight")
        qw = quantize(w, axis=0)                                    # int_data [K, N], scale [N]
        K, N = w.shape
        sub = QTensor(qw.int_data.t().contiguous(), qw.scale, 1, w.dtype, torch.Size((N, K)))
        return cls.from_qtensor(sub, bias.detach().clone() if bias is not None else None)

    @classmethod
    def from_qtensor(cls, qw: QTensor, bias=None) -> "qlinear":
        if qw.axis != 1 or qw.int_data.dim() != 2:
            raise ValueError("weight QTensor must be [N,K] quantised per output channel (axis=-1)")
        m = _module_of(cls, bias, wq=qw.int_data, ws=qw.scale)
        m.out_features, m.in_features = qw.int_data.shape
        return m

    def forward(self, x) -> torch.Tensor:
        """x: a float tensor [..., K] (quantised per token here, K1), or a per-token QTensor made by quantize() /
        silu_mul_quantize() (its codes and scales go straight to the GEMM; output dtype = its orig_dtype)."""
        if x.shape[-1] != self.in_features:
            raise ValueError(f"qlinear: expected last dim {self.in_features}, got {x.shape[-1]}")
        if isinstance(x, QTensor) and x.axis != 1:
            raise ValueError("qlinear: a QTensor input must be quantised per token (axis=-1)")
        wq, kp = self._wq_for_gemm()
        if kp != self.in_features:
            return self._padded_forward(x, wq, kp)
        if isinstance(x, QTensor):
            y = qlinear_s8(x.int_data.reshape(-1, self.in_features), x.scale, self.wq, self.ws, self.bias, x.orig_dtype)
            return y.reshape(*x.shape[:-1], self.out_features)
        return qlinear_dyn(x, self.wq, self.ws, self.bias)

    def extra_repr(self):
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}"


def is_code_fed(m) -> bool:
    """A qlinear whose GEMM another producer's codes may feed (RMSNormQuant's, silu_mul_quantize's, a fused q/k/v weight): every qlinear but a subclass that transforms
    its input before quantising it (hadamard.RotatedQLinear sets `code_fed = False`: its weight is rotated, so only codes of the rotated activation fit it).  The fuse_*
    entries ask this where they used to ask isinstance(m, qlinear), and so leave such a module — and what would have fed it — alone."""
    return isinstance(m, qlinear) and getattr(m, "code_fed", True)


class FusedQLinear(_KPadded, nn.Module):
    """Horizontal fusion of projections that share one input (q/k/v, gate/up): the int8 weights are concatenated
    along N, the activation is quantised ONCE and one GEMM launch fills all outputs (better tile count on 256 CUs
    than separate N=1024 GEMMs).  Exact: weight scales are per output row, so concatenation changes no value.
    forward() returns one tensor per fused projection (views of the fused output)."""

    def __init__(self, parts):
        super().__init__()
        parts = list(parts)
        if not parts or any(p.in_features != parts[0].in_features for p in parts):
            raise ValueError("FusedQLinear: projections must share in_features")
        if any((p.bias is None) != (parts[0].bias is None) for p in parts):
            raise ValueError("FusedQLinear: either all or none of the projections may have a bias")
        self.in_features = parts[0].in_features
        self.splits = [p.out_features for p in parts]
        self.out_features = sum(self.splits)
        _set_buffers(self, torch.cat([p.bias for p in parts], dim=0).contiguous() if parts[0].bias is not None else None,
                     wq=torch.cat([p.wq for p in parts], dim=0).contiguous(), ws=torch.cat([p.ws for p in parts], dim=0).contiguous())

    @classmethod
    def from_linears(cls, *linears: nn.Linear) -> "FusedQLinear":
        return cls([qlinear.from_linear(l) for l in linears])

    def forward(self, x):
        """x: a float tensor [..., K] or a per-token QTensor (e.g. from rmsnorm_quantize)."""
        if x.shape[-1] != self.in_features or (isinstance(x, QTensor) and x.axis != 1):
            raise ValueError("FusedQLinear: input must be [..., in_features], quantised per token if a QTensor")
        wq, kp = self._wq_for_gemm()
        if kp != self.in_features:
            return torch.split(self._padded_forward(x, wq, kp), self.splits, dim=-1)
        xq = x if isinstance(x, QTensor) else quantize(x, axis=-1)
        y = qlinear_s8(xq.int_data.reshape(-1, self.in_features), xq.scale, self.wq, self.ws, self.bias, xq.orig_dtype)
        y = y.reshape(*x.shape[:-1], self.out_features)
        return torch.split(y, self.splits, dim=-1)


class GatedMLP(nn.Module):
    """The gated MLP block of BASELINE config 3 on the int8 path: down(silu(gate(x)) * up(x)).
    gate and up share one activation quantisation and one GEMM launch (FusedQLinear); silu*mul is fused into the
    quantisation of down's input (silu_mul_quantize), so between the two GEMMs only int8 codes + row scales exist.
    act="gelu_tanh" (Gemma's GeGLU; gemma.fuse_gemma_layers builds it) puts gelu_mul_quantize in silu_mul_quantize's place.  A `down` that is a
    hadamard.RotatedQLinear (hadamard.rotate_gated_mlps builds it) takes codes of the ROTATED activation: the gate, the rotation and the quantisation are one launch
    (hadamard.gated_hadamard_quantize, kernel K1gh)."""

    ACTS = ("silu", "gelu_tanh")

    def __init__(self, gate_up: FusedQLinear, down: qlinear, act: str = "silu"):
        super().__init__()
        if len(gate_up.splits) != 2 or gate_up.splits[0] != gate_up.splits[1] or gate_up.splits[0] != down.in_features:
            raise ValueError("GatedMLP: gate and up must both map to down.in_features")
        if act not in self.ACTS:
            raise ValueError(f"GatedMLP: unknown act {act!r}, expected one of {self.ACTS}")
        self.gate_up, self.down, self.act = gate_up, down, act

    @classmethod
    def from_linears(cls, gate: nn.Linear, up: nn.Linear, down: nn.Linear) -> "GatedMLP":
        return cls(FusedQLinear.from_linears(gate, up), qlinear.from_linear(down))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        g, u = self.gate_up(x)
        if not getattr(self.down, "code_fed", True):          # a RotatedQLinear: only codes of the rotated activation fit its weight
            from .hadamard import gated_hadamard_quantize
            return self.down.forward_rotated(gated_hadamard_quantize(g, u, self.act, self.down.block))
        if self.act == "gelu_tanh":          # Gemma's GeGLU: down(gelu_tanh(gate(x)) * up(x)), kernel K1gg
            return self.down(gelu_mul_quantize(g, u))
        return self.down(silu_mul_quantize(g, u))

    def extra_repr(self):
        return "" if self.act == "silu" else f"act={self.act}"


def _is_silu(act) -> bool:
    return isinstance(act, nn.SiLU) or type(act).__name__ in ("SiLU", "SiLUActivation") or act is torch.nn.functional.silu


def _as_gated_mlp(mod: nn.Module):
    """A module shaped like a Llama MLP — Linear children gate_proj / up_proj / down_proj and a SiLU act_fn — as GatedMLP."""
    g, u, d = (getattr(mod, n, None) for n in ("gate_proj", "up_proj", "down_proj"))
    if not all(isinstance(l, nn.Linear) for l in (g, u, d)) or not _is_silu(getattr(mod, "act_fn", None)):
        return None
    if g.in_features != u.in_features or g.out_features != u.out_features or d.in_features != g.out_features:
        return None
    if (g.bias is None) != (u.bias is None):
        return None
    return GatedMLP.from_linears(g, u, d)


def _is_conv1d(mod: nn.Module) -> bool:
    """transformers.pytorch_utils.Conv1D (GPT-2 family): a linear layer whose weight is stored [in_features, out_features] (recognised by shape, not by import)."""
    w = getattr(mod, "weight", None)
    return (type(mod).__name__ == "Conv1D" and isinstance(getattr(mod, "nf", None), int) and isinstance(w, torch.Tensor) and w.dim() == 2
            and w.shape[1] == mod.nf and not list(mod.children()))


def is_plain_linear(mod: nn.Module) -> bool:
    """An nn.Linear whose forward IS nn.Linear's.  A subclass that overrides forward computes something else with the same weight — Phi-MoE's router is an nn.Linear
    whose forward returns (logits, routing weights, selected experts) — and qlinear would replace that forward by y = x W^T + b: such a module is left as it is."""
    return isinstance(mod, nn.Linear) and type(mod).forward is nn.Linear.forward


def _swap_children(model: nn.Module, visit) -> int:
    """The tree walk of the swap_* functions.  visit(name, child), for every child in turn, answers a module to put in the child's place (counted once), a count — the
    child is settled: converted in place (1) or to be left alone (0) — or None: not a candidate, its own children are walked.  Returns the sum of the counts."""
    n = 0
    for name, child in list(model.named_children()):
        r = visit(name, child)
        if r is None:
            n += _swap_children(child, visit)
        elif isinstance(r, nn.Module):
            setattr(model, name, r)
            n += 1
        else:
            n += r
    return n


def swap_linears(model: nn.Module, predicate=None, fuse_gated_mlp: bool = False) -> nn.Module:
    """Replace every nn.Linear (for which predicate(name, module) is true) by qlinear, in place; Hugging Face Conv1D layers (GPT-2: weight stored [K, N]) likewise,
    through qlinear.from_kn_weight (per-channel quantisation along the strided axis, kernel K2).  A subclass of nn.Linear with a forward of its own is not a linear
    layer to this function (is_plain_linear).
    fuse_gated_mlp=True additionally replaces whole gated-MLP blocks (gate_proj / up_proj / down_proj + SiLU, the
    Llama-family MLP) by GatedMLP: one fused gate+up GEMM, silu*mul fused into the quantisation, the down GEMM."""
    def visit(name, child):
        if fuse_gated_mlp and (predicate is None or predicate(name, child)):
            fused = _as_gated_mlp(child)
            if fused is not None:
                return fused
        if is_plain_linear(child) and (predicate is None or predicate(name, child)):
            return qlinear.from_linear(child)
        if _is_conv1d(child) and (predicate is None or predicate(name, child)):
            return qlinear.from_kn_weight(child.weight, child.bias)      # Hugging Face GPT-2's Conv1D: y = x @ W[K, N] + b
        return None
    _swap_children(model, visit)
    return model
