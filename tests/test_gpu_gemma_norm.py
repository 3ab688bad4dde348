"""-m gpu: K1ng (pq_gemma_rmsnorm_quant_rowwise / gemma_rmsnorm_quantize) and K1ang (pq_add_gemma_rmsnorm_quant_rowwise / add_gemma_rmsnorm_quantize) against the CPU
specification (tests/gemma_spec.py: NG1-NG6, A1), bit for bit — codes, scales, h and the stored sum; NaNs as a class — for bf16, fp16 and f32.  Rows 1, 5 and 33
(5 and 33 leave a partial four-row block in the wave layout); widths that reach every row layout (one wave per row at 1 / 2 / 4 vectors per lane — 8 with
PQ_RMS_WAVE_MAX=512 — 256 threads per row at 1 .. 16 vectors, and on short rows with PQ_RMS_WAVE_MAX=0), the generic kernel on a ragged width, past the vector limit,
on unaligned bases and odd leading dimensions; ld_x > cols; with and without h_out; sum_out as x, as residual and as a tensor of its own; a NaN row, an Inf row and
a zero row; guarded margins around every output; and K1ang equal to the torch add followed by K1ng."""
import functools

import numpy as np
import pytest
import torch

from tests import gemma_spec as G
from tests.gemma_spec import nan_class_equal as _nan_class_equal
from tests.gpu_util import bits

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
IDS = ["bf16", "fp16", "f32"]
EPS = 1e-6
ROWS = (1, 5, 33)
# 16-bit widths (halved for f32): 1 vector; one wave x 1 vector; x 2 (a partial second slot); x 4; 256 threads x 2 (288 vectors), x 4 (576), x 8 (1152), x 16 (the vector
# limit); ragged (generic); one vector past the limit (generic)
WIDTHS = (8, 512, 520, 2048, 2304, 4608, 9216, 32768, 333, 32776)


def _cols(width, dtype):
    return width if dtype != torch.float32 else (width // 2 if width % 2 == 0 else 167)


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    from protoquant_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return protoquant_amd


@functools.lru_cache(maxsize=None)
def _case(dtype, cols):
    """33 rows of x, residual and a weight, with the specification of both kernels computed ONCE (rows are independent: the first 1 and 5 rows are their own cases).
    Row 2 holds a NaN, row 3 an Inf, row 4 is zero — in x AND in the sum."""
    g = torch.Generator().manual_seed(1000 + cols)
    scale = torch.exp(torch.empty(33, 1).uniform_(float(np.log(0.05)), float(np.log(20.0)), generator=g))
    x = (torch.randn(33, cols, generator=g) * scale).to(dtype)
    r = (torch.randn(33, cols, generator=g) * 3.0 * scale).to(dtype)
    w = (0.3 * torch.randn(cols, generator=g)).to(dtype)
    x[2, cols // 3] = float("nan")
    x[3, cols // 2] = float("inf")
    x[4], r[4] = 0.0, 0.0
    return x, r, w, G.gemma_rmsnorm_quantize_t(x, w, EPS), G.add_gemma_rmsnorm_quantize(x, r, w, EPS)


def _check_plain(pq, xd, wd, spec, rows, what):
    q_s, sc_s, h_s = spec
    qt, h = pq.gemma_rmsnorm_quantize(xd, wd, EPS, return_h=True)
    qt2 = pq.gemma_rmsnorm_quantize(xd, wd, EPS)                      # the instantiation without h_out
    torch.cuda.synchronize()
    _nan_class_equal(h, h_s[:rows], what + ": h")
    for t, tag in ((qt, ""), (qt2, " (no h)")):
        _nan_class_equal(t.scale, sc_s[:rows], what + ": scales" + tag)
        assert np.array_equal(t.int_data.cpu().numpy(), q_s[:rows]), what + ": codes" + tag


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("width", WIDTHS)
def test_k1ng_matches_the_spec(pq, dtype, width):
    cols = _cols(width, dtype)
    x, r, w, spec, _ = _case(dtype, cols)
    wd = w.cuda()
    for rows in ROWS:
        _check_plain(pq, x[:rows].cuda(), wd, spec, rows, f"K1ng {dtype} {rows}x{cols}")
    # ld_x > cols: a column block of a wider tensor, at an offset that keeps the 16-byte alignment
    wide = torch.zeros(5, cols + 32, dtype=dtype)
    wide[:, 16:16 + cols] = x[:5]
    view = wide.cuda()[:, 16:16 + cols]
    assert view.stride(0) == cols + 32
    _check_plain(pq, view, wd, spec, 5, f"K1ng {dtype} 5x{cols}, ld_x = cols + 32")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("width", WIDTHS)
def test_k1ang_matches_the_spec_and_the_pair(pq, dtype, width):
    cols = _cols(width, dtype)
    x, r, w, _, spec = _case(dtype, cols)
    q_s, sc_s, s_s, h_s = spec
    wd = w.cuda()
    for rows, out_mode in zip(ROWS, ("x", "residual", "none")):
        what = f"K1ang {dtype} {rows}x{cols} out={out_mode}"
        xd, rd = x[:rows].cuda(), r[:rows].cuda()
        with torch.no_grad():
            pair_q, pair_h = pq.gemma_rmsnorm_quantize(rd + xd, wd, EPS, return_h=True)          # the torch add followed by K1ng
            pair_s = rd + xd
        out = {"none": None, "x": xd, "residual": rd}[out_mode]
        qt, summed, h = pq.add_gemma_rmsnorm_quantize(xd, rd, wd, EPS, out=out, return_h=True)
        qt2, summed2 = pq.add_gemma_rmsnorm_quantize(x[:rows].cuda(), r[:rows].cuda(), wd, EPS)      # the instantiation without h_out
        torch.cuda.synchronize()
        assert out is None or summed is out
        _nan_class_equal(summed, s_s[:rows], what + ": sum")
        _nan_class_equal(summed2, s_s[:rows], what + ": sum (no h)")
        _nan_class_equal(h, h_s[:rows], what + ": h")
        for t, tag in ((qt, ""), (qt2, " (no h)")):
            _nan_class_equal(t.scale, sc_s[:rows], what + ": scales" + tag)
            assert np.array_equal(t.int_data.cpu().numpy(), q_s[:rows]), what + ": codes" + tag
        _nan_class_equal(summed, pair_s, what + ": sum vs the torch add")
        _nan_class_equal(h, pair_h, what + ": h vs the pair")
        _nan_class_equal(qt.scale, pair_q.scale, what + ": scales vs the pair")
        assert torch.equal(qt.int_data, pair_q.int_data), what + ": codes vs the pair"
        if out_mode != "x":
            assert torch.equal(xd.cpu().view(torch.uint8), x[:rows].contiguous().view(torch.uint8)), what + ": x was written"
        if out_mode != "residual":
            assert torch.equal(rd.cpu().view(torch.uint8), r[:rows].contiguous().view(torch.uint8)), what + ": residual was written"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("wave_max,width", [("512", 3072), ("0", 512)])
def test_wave_max_switch_changes_no_bit(pq, pq_opt, dtype, wave_max, width):
    """PQ_RMS_WAVE_MAX=512 at 3072 columns: one wave per row at 8 vectors per lane (384 vectors; 256 threads x 2 by default); PQ_RMS_WAVE_MAX=0 at 512 columns: the 256-thread
    layout on a short row.  Time only, never bits; the fixture restores the option."""
    cols = _cols(width, dtype)
    x, r, w, spec, spec_add = _case(dtype, cols)
    pq_opt("PQ_RMS_WAVE_MAX", wave_max)
    wd = w.cuda()
    for rows in ROWS:
        _check_plain(pq, x[:rows].cuda(), wd, spec, rows, f"PQ_RMS_WAVE_MAX={wave_max} K1ng {dtype} {rows}x{cols}")
        qt, summed, h = pq.add_gemma_rmsnorm_quantize(x[:rows].cuda(), r[:rows].cuda(), wd, EPS, return_h=True)
        _nan_class_equal(summed, spec_add[2][:rows], "sum")
        _nan_class_equal(h, spec_add[3][:rows], "h")
        _nan_class_equal(qt.scale, spec_add[1][:rows], "scales")
        assert np.array_equal(qt.int_data.cpu().numpy(), spec_add[0][:rows])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unaligned_bases_and_odd_leading_dimensions_take_the_generic_kernel(pq, dtype):
    cols = _cols(512, dtype)
    x, r, w, spec, spec_add = _case(dtype, cols)
    rows = 5
    big_x = torch.zeros(rows, cols + 37, dtype=dtype)
    big_r = torch.zeros(rows, cols + 11, dtype=dtype)
    big_x[:, 3:3 + cols], big_r[:, 1:1 + cols] = x[:rows], r[:rows]
    bx, br, wd = big_x.cuda(), big_r.cuda(), w.cuda()
    xv, rv = bx[:, 3:3 + cols], br[:, 1:1 + cols]
    _check_plain(pq, xv, wd, spec, rows, f"K1ng {dtype} unaligned x, odd ld")
    big_o = torch.zeros(rows, cols + 5, dtype=dtype, device="cuda")
    ov = big_o[:, 5:5 + cols]
    qt, summed, h = pq.add_gemma_rmsnorm_quantize(xv, rv, wd, EPS, out=ov, return_h=True)
    assert summed is ov
    _nan_class_equal(ov, spec_add[2][:rows], "strided sum")
    _nan_class_equal(h, spec_add[3][:rows], "h")
    _nan_class_equal(qt.scale, spec_add[1][:rows], "scales")
    assert np.array_equal(qt.int_data.cpu().numpy(), spec_add[0][:rows])
    assert not bool(big_o[:, :5].float().abs().sum() > 0), "columns outside the output view were written"
    # in place over the strided x, then over the strided residual
    for target in ("x", "residual"):
        bx2, br2 = bx.clone(), br.clone()
        xv2, rv2 = bx2[:, 3:3 + cols], br2[:, 1:1 + cols]
        qt, summed = pq.add_gemma_rmsnorm_quantize(xv2, rv2, wd, EPS, out=xv2 if target == "x" else rv2)
        _nan_class_equal(summed, spec_add[2][:rows], f"in place over strided {target}")
        assert np.array_equal(qt.int_data.cpu().numpy(), spec_add[0][:rows])
        touched, ref_big, off = (bx2, bx, 3) if target == "x" else (br2, br, 1)
        assert torch.equal(touched[:, :off], ref_big[:, :off]) and torch.equal(touched[:, off + cols:], ref_big[:, off + cols:])
        assert torch.equal((br2 if target == "x" else bx2).view(torch.uint8), (br if target == "x" else bx).view(torch.uint8))          # the other input is untouched


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,width", [(5, 512), (33, 2304), (5, 32768), (5, 333)])
def test_guarded_margins_stay_untouched(pq, dtype, rows, width):
    """every output buffer (sum, codes, scales, h) lies inside a larger allocation filled with a pattern: the kernels write their rows and nothing around them.  Raw
    C-ABI calls on interior views, 16-byte aligned for the vector layouts."""
    from protoquant_amd import _lib as L
    cols = _cols(width, dtype)
    x, r, w, spec, spec_add = _case(dtype, cols)
    xd, rd, wd = x[:rows].cuda(), r[:rows].cuda(), w.cuda()
    m = 4096          # margin in elements: a multiple of 16 bytes for every dtype
    for add in (False, True):
        sum_all = torch.full((rows * cols + 2 * m,), 7.0, dtype=dtype, device="cuda")
        h_all = torch.full((rows * cols + 2 * m,), 7.0, dtype=dtype, device="cuda")
        q_all = torch.full((rows * cols + 2 * m,), 77, dtype=torch.int8, device="cuda")
        sc_all = torch.full((rows + 2 * m,), 7.0, dtype=torch.float32, device="cuda")
        s_v, h_v, q_v, sc_v = sum_all[m:m + rows * cols], h_all[m:m + rows * cols], q_all[m:m + rows * cols], sc_all[m:m + rows]
        with torch.cuda.device(xd.device):
            if add:
                L.check(L.lib().pq_add_gemma_rmsnorm_quant_rowwise(xd.data_ptr(), cols, rd.data_ptr(), cols, s_v.data_ptr(), cols, wd.data_ptr(), EPS, L.dtype_code(dtype),
                                                                   rows, cols, q_v.data_ptr(), cols, sc_v.data_ptr(), h_v.data_ptr(), cols, L.stream_ptr(xd)), "raw K1ang")
            else:
                L.check(L.lib().pq_gemma_rmsnorm_quant_rowwise(xd.data_ptr(), cols, wd.data_ptr(), EPS, L.dtype_code(dtype), rows, cols, q_v.data_ptr(), cols,
                                                               sc_v.data_ptr(), h_v.data_ptr(), cols, L.stream_ptr(xd)), "raw K1ng")
        torch.cuda.synchronize()
        q_s, sc_s, h_s = (spec_add[0], spec_add[1], spec_add[3]) if add else spec
        _nan_class_equal(h_v.view(rows, cols), h_s[:rows], "h")
        _nan_class_equal(sc_v, sc_s[:rows], "scales")
        assert np.array_equal(q_v.view(rows, cols).cpu().numpy(), q_s[:rows])
        if add:
            _nan_class_equal(s_v.view(rows, cols), spec_add[2][:rows], "sum")
        else:
            assert bool((sum_all == 7.0).all())
        for name, buf, n, fill in (("sum", sum_all, rows * cols, 7.0), ("h", h_all, rows * cols, 7.0), ("codes", q_all, rows * cols, 77), ("scales", sc_all, rows, 7.0)):
            assert bool((buf[:m] == fill).all()) and bool((buf[m + n:] == fill).all()), f"add={add}: the margin around {name} was written"


def test_batch_shapes_module_and_empty_inputs(pq):
    """[batch, seq, hidden] inputs keep their shape; GemmaRMSNormQuant is the two functions; empty inputs launch nothing"""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 7, 512, generator=g).to(torch.bfloat16).cuda()
    r = torch.randn(2, 7, 512, generator=g).to(torch.bfloat16).cuda()
    w = (0.3 * torch.randn(512, generator=g)).to(torch.bfloat16).cuda()
    mod = pq.GemmaRMSNormQuant(w, EPS)
    assert list(mod.state_dict()) == ["weight"] and torch.equal(mod.weight, w)
    qt, s = mod(x, residual=r)
    ref = mod(r + x)
    assert s.shape == x.shape and qt.int_data.shape == x.shape and qt.scale.shape == (14,)
    assert torch.equal(s, r + x) and torch.equal(qt.int_data, ref.int_data) and torch.equal(qt.scale, ref.scale)
    q_s, sc_s, _ = G.gemma_rmsnorm_quantize_t((r + x).reshape(14, 512), w, EPS)
    assert np.array_equal(ref.int_data.reshape(14, 512).cpu().numpy(), q_s) and np.array_equal(bits(ref.scale), sc_s.view(np.uint32))
    # the gain is 1 + w: not what the Llama kernel gives for the same stored weight
    assert not torch.equal(pq.rmsnorm_quantize(r + x, w, EPS).int_data, ref.int_data)
    e = torch.empty(0, 512, dtype=torch.bfloat16, device="cuda")
    qe, se = pq.add_gemma_rmsnorm_quantize(e, e, w)
    assert se.shape == (0, 512) and qe.int_data.shape == (0, 512) and pq.gemma_rmsnorm_quantize(e, w).scale.shape == (0,)
