"""-m gpu: K1al, pq_add_layernorm_quant_rowwise / add_layernorm_quantize — the residual add fused into LayerNorm + per-token int8 quantisation.  Codes, scales, the
stored sum and h are compared bit for bit (NaNs as a class) with (a) layernorm_quantize(residual + x, return_h=True), the add done by torch on the GPU, and (b) the CPU
specification (tests/addlnorm_spec.py: A1 by torch on the CPU, L1-L6 / Q1-Q6 by tests/lnorm_spec.py), with and without a bias, over a grid that launches every
instantiation: one wave per row at 1 / 2 / 4 vectors (8 with PQ_RMS_WAVE_MAX=512), 256 threads per row at 1 .. 16 vectors (and on short rows with PQ_RMS_WAVE_MAX=0),
the generic kernel on ragged widths, unaligned bases and odd leading dimensions; out=None / x / residual; guarded margins around every output.  The kernels these
tests launch are recorded in profiles/r16_addlnorm_kernels.txt.  There is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

from tests import addlnorm_spec as A
from tests.gpu_util import bits

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
EPV = {torch.bfloat16: 8, torch.float16: 8, torch.float32: 4}
EPS = 1e-5


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    from protoquant_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return protoquant_amd


def _nan_class_equal(got: torch.Tensor, want, what):
    """float tensors: NaN positions equal, every other element bit for bit"""
    g = bits(got)
    w = bits(want) if isinstance(want, torch.Tensor) else np.asarray(want)
    if w.dtype == np.float32:
        w = w.view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    gn = torch.isnan(got.detach().float().cpu()).numpy()
    if isinstance(want, torch.Tensor):
        wn = torch.isnan(want.detach().float().cpu()).numpy()
    else:
        wt = torch.from_numpy(np.ascontiguousarray(np.asarray(want)))
        wn = torch.isnan((wt if wt.dtype == torch.float32 else wt.view(torch.int16).view(got.dtype)).float()).numpy()
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ"
    bad = (g != w) & ~wn
    assert not bad.any(), f"{what}: {int(bad.sum())} of {g.size} elements differ (first at {np.argwhere(bad)[:3].tolist()})"


def _inputs(rows, cols, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, cols, generator=g) * scale).to(dtype)
    r = (torch.randn(rows, cols, generator=g) * 3.0 * scale).to(dtype)
    w = (1.0 + 0.25 * torch.randn(cols, generator=g)).to(dtype)
    b = (0.25 * torch.randn(cols, generator=g)).to(dtype)
    return x, r, w, b


def _check(pq, x, r, w, b, what, out_mode="none", against_spec=True):
    """x, r, w, b: CPU tensors (b may be None).  Runs the fused kernel on copies on the GPU and compares with the pair (torch add + K1l) and with the CPU specification."""
    xd, rd, wd = x.cuda(), r.cuda(), w.cuda()
    bd = None if b is None else b.cuda()
    with torch.no_grad():
        s_ref = rd + xd
        q_ref, h_ref = pq.layernorm_quantize(s_ref, wd, bd, EPS, return_h=True)
        out = {"none": None, "x": xd, "residual": rd}[out_mode]
        qt, summed, h = pq.add_layernorm_quantize(xd, rd, wd, bd, EPS, out=out, return_h=True)
        qt2, summed2 = pq.add_layernorm_quantize(x.cuda(), r.cuda(), wd, bd, EPS)            # the instantiation without h_out
    torch.cuda.synchronize()
    if out is not None:
        assert summed is out
    assert summed.shape == x.shape and qt.int_data.shape == x.shape and h.shape == x.shape
    nonan = not bool(torch.isnan(s_ref.float()).any())
    if nonan:          # the issue's own statement of the contract: torch.equal with the library's two-launch form on the same GPU
        assert torch.equal(summed, s_ref) and torch.equal(h, h_ref) and torch.equal(qt.scale, q_ref.scale), what + ": torch.equal with the pair"
    _nan_class_equal(summed, s_ref, what + ": sum vs torch add")
    _nan_class_equal(h, h_ref, what + ": h vs K1l")
    _nan_class_equal(qt.scale, q_ref.scale, what + ": scales vs K1l")
    assert torch.equal(qt.int_data, q_ref.int_data), what + ": codes vs K1l"
    _nan_class_equal(summed2, s_ref, what + ": sum (no h)")
    _nan_class_equal(qt2.scale, q_ref.scale, what + ": scales (no h)")
    assert torch.equal(qt2.int_data, q_ref.int_data), what + ": codes (no h)"
    if out_mode != "x":
        assert torch.equal(xd.cpu().view(torch.uint8), x.view(torch.uint8)), what + ": x was written"
    if out_mode != "residual":
        assert torch.equal(rd.cpu().view(torch.uint8), r.view(torch.uint8)), what + ": residual was written"
    assert torch.equal(wd.cpu().view(torch.uint8), w.view(torch.uint8)) and (b is None or torch.equal(bd.cpu().view(torch.uint8), b.view(torch.uint8)))
    if against_spec:
        q_s, sc_s, s_s, h_s = A.add_layernorm_quantize(x, r, w, b, EPS)
        _nan_class_equal(summed, s_s, what + ": sum vs spec")
        _nan_class_equal(h, h_s, what + ": h vs spec")
        _nan_class_equal(qt.scale, sc_s, what + ": scales vs spec")
        assert np.array_equal(qt.int_data.cpu().numpy(), q_s), what + ": codes vs spec"


# vectors per row -> the layout it reaches by default: <= 64 / 128 / 256 one wave per row (1 / 2 / 4 vectors per lane); beyond, 256 threads x 1 / 2 / 4 / 8 / 16
VEC_COUNTS = [1, 40, 64, 65, 128, 200, 256, 257, 512, 700, 1024, 1500, 2048, 3000, 4096]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("nvec", VEC_COUNTS)
def test_every_vector_layout_matches_the_pair_and_the_spec(pq, dtype, nvec):
    cols = nvec * EPV[dtype]
    for rows in (1, 3, 5):
        x, r, w, b = _inputs(rows, cols, dtype, 100 + nvec + rows)
        for bias in (b, None):
            _check(pq, x, r, w, bias, f"{dtype} {rows}x{cols} bias={bias is not None}", out_mode=("none", "x", "residual")[(rows + (bias is None)) % 3])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("cols", [768, 2048, 4096, 8192])
def test_many_rows(pq, dtype, cols):
    x, r, w, b = _inputs(4096, cols, dtype, 7 + cols)
    _check(pq, x, r, w, b if cols != 4096 else None, f"{dtype} 4096x{cols}", out_mode="residual" if cols != 8192 else "x", against_spec=(cols == 2048))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("wave_max,nvecs", [("512", [300, 512]), ("0", [1, 64, 100, 256])])
def test_wave_max_switch_changes_no_bit(pq, pq_opt, dtype, wave_max, nvecs):
    """PQ_RMS_WAVE_MAX=512: one wave per row at 8 vectors per lane; PQ_RMS_WAVE_MAX=0: the 256-thread layout on short rows.  Time only, never bits."""
    pq_opt("PQ_RMS_WAVE_MAX", wave_max)
    for nvec in nvecs:
        for rows in (1, 5, 4096 if nvec in (512, 64) else 3, 4):
            x, r, w, b = _inputs(rows, nvec * EPV[dtype], dtype, 900 + nvec + rows)
            _check(pq, x, r, w, b if rows != 5 else None, f"PQ_RMS_WAVE_MAX={wave_max} {dtype} {rows}x{nvec} vectors", out_mode=("none", "x", "residual")[rows % 3],
                   against_spec=rows < 100)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("cols", [1, 7, 37, 255, 4097])
def test_ragged_widths_take_the_generic_kernel(pq, dtype, cols):
    for rows in (1, 3, 4, 5):
        x, r, w, b = _inputs(rows, cols, dtype, 300 + cols + rows)
        for bias in (b, None):
            _check(pq, x, r, w, bias, f"{dtype} {rows}x{cols} bias={bias is not None}", out_mode=("none", "x", "residual")[(rows + (bias is None)) % 3])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
def test_unaligned_and_strided_views(pq, dtype):
    """column slices at an odd element offset (unaligned base), odd leading dimensions, and the sum written to a strided view — directly and over x / residual"""
    rows, cols = 6, 512
    g = torch.Generator().manual_seed(44)
    big_x = torch.randn(rows, cols + 37, generator=g).to(dtype).cuda()
    big_r = (torch.randn(rows, cols + 11, generator=g) * 2).to(dtype).cuda()
    big_o = torch.zeros(rows, cols + 5, dtype=dtype, device="cuda")
    w = (1.0 + 0.25 * torch.randn(cols, generator=g)).to(dtype).cuda()
    bb = (0.25 * torch.randn(cols, generator=g)).to(dtype).cuda()
    for off_x, off_r, off_o in ((3, 1, 5), (0, 0, 0), (8, 8, 0)):
        xv, rv, ov = big_x[:, off_x:off_x + cols], big_r[:, off_r:off_r + cols], big_o[:, off_o:off_o + cols]
        big_o.zero_()
        with torch.no_grad():
            s_ref = rv + xv
            q_ref, h_ref = pq.layernorm_quantize(s_ref, w, bb, EPS, return_h=True)
            qt, summed, h = pq.add_layernorm_quantize(xv, rv, w, bb, EPS, out=ov, return_h=True)
        assert summed is ov
        _nan_class_equal(ov, s_ref, f"{dtype} strided sum {off_x, off_r, off_o}")
        _nan_class_equal(h, h_ref, "strided h")
        _nan_class_equal(qt.scale, q_ref.scale, "strided scales")
        assert torch.equal(qt.int_data, q_ref.int_data)
        mask = torch.ones_like(big_o, dtype=torch.bool)
        mask[:, off_o:off_o + cols] = False
        assert not bool(big_o[mask].float().abs().sum() > 0), "columns outside the output view were written"
        q_s, sc_s, s_s, h_s = A.add_layernorm_quantize(xv.cpu().contiguous(), rv.cpu().contiguous(), w.cpu(), bb.cpu(), EPS)
        _nan_class_equal(ov, s_s, "strided sum vs spec")
        assert np.array_equal(qt.int_data.cpu().numpy(), q_s)
    # in place over a strided x, then over a strided residual
    for target in ("x", "residual"):
        bx, br = big_x.clone(), big_r.clone()
        xv, rv = bx[:, 3:3 + cols], br[:, 1:1 + cols]
        with torch.no_grad():
            s_ref = rv + xv
            q_ref = pq.layernorm_quantize(s_ref, w, bb, EPS)
            qt, summed = pq.add_layernorm_quantize(xv, rv, w, bb, EPS, out=xv if target == "x" else rv)
        _nan_class_equal(summed, s_ref, f"{dtype} in place over strided {target}")
        assert torch.equal(qt.int_data, q_ref.int_data) and torch.equal(qt.scale, q_ref.scale)
        assert torch.equal(br if target == "x" else bx, big_r if target == "x" else big_x)          # the other input is untouched
        touched, ref_big, off = (bx, big_x, 3) if target == "x" else (br, big_r, 1)
        assert torch.equal(touched[:, :off], ref_big[:, :off]) and torch.equal(touched[:, off + cols:], ref_big[:, off + cols:])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("cols", [256, 4096, 37])
def test_special_values(pq, dtype, cols):
    """rows holding NaN, +-Inf, Inf - Inf, all zeros, -0, a row whose sum cancels to zero everywhere, and sums that overflow the storage format"""
    x, r, w, b = _inputs(11, cols, dtype, 555 + cols)
    r[10] = -x[10]                                                   # the whole row cancels: mean 0, variance 0, h = bias
    big = {torch.bfloat16: 3.0e38, torch.float16: 60000.0, torch.float32: 3.0e38}[dtype]
    x[0, 3] = float("nan")
    r[1, 5] = float("nan")
    x[2, 1], r[2, 2] = float("inf"), float("-inf")
    x[3, 7], r[3, 7] = float("inf"), float("-inf")                 # Inf - Inf: a NaN made by the add
    x[4], r[4] = 0.0, 0.0
    x[5], r[5] = -0.0, -0.0
    x[6], r[6] = 0.0, -0.0
    x[7, :] = big
    r[7, :] = big                                                    # the sum overflows to +Inf in the storage dtype (fp16: 60000 + 60000)
    x[8, 0], r[8, 0] = big, -big                                     # exact cancellation next to ordinary values
    x[9], r[9] = (x[9].float() * 1e-30).to(dtype), (r[9].float() * 1e-30).to(dtype)      # tiny rows (fp16: zeros and subnormals)
    for mode in ("none", "x", "residual"):
        for bias in (b, None):
            _check(pq, x.clone(), r.clone(), w, bias, f"{dtype} special values, {cols} columns, out={mode}, bias={bias is not None}", out_mode=mode)
    qt, s = pq.add_layernorm_quantize(x.cuda(), r.cuda(), w.cuda(), None, EPS)
    assert not bool(s[10].float().abs().sum() > 0) and not bool(qt.int_data[10].any()) and not bool(qt.int_data[4].any())      # all-zero sums: zero codes
    if dtype == torch.float16:
        assert bool(torch.isinf(s[7]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("rows,cols", [(5, 4096), (3, 520), (7, 37), (4, 32768 // 2), (1, 8192)])
def test_guarded_margins_stay_untouched(pq, dtype, rows, cols):
    """every output buffer (sum, codes, scales, h) lies inside a larger allocation filled with a pattern: the kernel writes its rows and nothing around them.  Raw
    C-ABI call on interior views, 16-byte aligned for the vector layouts."""
    from protoquant_amd import _lib as L
    x, r, w, b = _inputs(rows, cols, dtype, 70 + rows + cols)
    xd, rd, wd, bd = x.cuda(), r.cuda(), w.cuda(), b.cuda()
    m = 4096          # margin in elements: a multiple of 16 bytes for every dtype
    sum_all = torch.full((rows * cols + 2 * m,), 7.0, dtype=dtype, device="cuda")
    h_all = torch.full((rows * cols + 2 * m,), 7.0, dtype=dtype, device="cuda")
    q_all = torch.full((rows * cols + 2 * m,), 77, dtype=torch.int8, device="cuda")
    sc_all = torch.full((rows + 2 * m,), 7.0, dtype=torch.float32, device="cuda")
    s_v, h_v, q_v, sc_v = sum_all[m:m + rows * cols], h_all[m:m + rows * cols], q_all[m:m + rows * cols], sc_all[m:m + rows]
    with torch.cuda.device(xd.device):
        L.check(L.lib().pq_add_layernorm_quant_rowwise(xd.data_ptr(), cols, rd.data_ptr(), cols, s_v.data_ptr(), cols, wd.data_ptr(), bd.data_ptr(), EPS, L.dtype_code(dtype),
                                                       rows, cols, q_v.data_ptr(), cols, sc_v.data_ptr(), h_v.data_ptr(), cols, L.stream_ptr(xd)), "raw K1al")
    torch.cuda.synchronize()
    with torch.no_grad():
        s_ref = rd + xd
        q_ref, h_ref = pq.layernorm_quantize(s_ref, wd, bd, EPS, return_h=True)
    _nan_class_equal(s_v.view(rows, cols), s_ref, "sum")
    _nan_class_equal(h_v.view(rows, cols), h_ref, "h")
    assert torch.equal(q_v.view(rows, cols), q_ref.int_data) and torch.equal(sc_v, q_ref.scale)
    for name, buf, n, fill in (("sum", sum_all, rows * cols, 7.0), ("h", h_all, rows * cols, 7.0), ("codes", q_all, rows * cols, 77), ("scales", sc_all, rows, 7.0)):
        assert bool((buf[:m] == fill).all()) and bool((buf[m + n:] == fill).all()), f"the margin around {name} was written"


def test_leading_dimensions_and_batch_shapes(pq):
    """[batch, seq, hidden] inputs keep their shape; a 1-D input is one row; empty rows and empty columns go through layernorm_quantize on the empty sum"""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 7, 512, generator=g).to(torch.bfloat16).cuda()
    r = torch.randn(2, 7, 512, generator=g).to(torch.bfloat16).cuda()
    w = torch.ones(512, dtype=torch.bfloat16, device="cuda")
    b = torch.full((512,), 0.5, dtype=torch.bfloat16, device="cuda")
    qt, s = pq.add_layernorm_quantize(x, r, w, b)
    ref = pq.layernorm_quantize(r + x, w, b)
    assert s.shape == x.shape and qt.int_data.shape == x.shape and qt.scale.shape == (14,)
    assert torch.equal(s, r + x) and torch.equal(qt.int_data, ref.int_data) and torch.equal(qt.scale, ref.scale)
    qt1, s1 = pq.add_layernorm_quantize(x[0, 0], r[0, 0], w, b)
    assert s1.shape == (512,) and torch.equal(qt1.int_data, ref.int_data[0, 0]) and torch.equal(s1, s[0, 0])
    e = torch.empty(0, 512, dtype=torch.bfloat16, device="cuda")
    qe, se = pq.add_layernorm_quantize(e, e, w, b)
    assert se.shape == (0, 512) and qe.int_data.shape == (0, 512)
    e0 = torch.empty(3, 0, dtype=torch.bfloat16, device="cuda")
    w0 = torch.empty(0, dtype=torch.bfloat16, device="cuda")
    q0, s0, h0 = pq.add_layernorm_quantize(e0, e0, w0, None, return_h=True)
    assert s0.shape == (3, 0) and h0.shape == (3, 0) and torch.equal(q0.scale, pq.layernorm_quantize(e0, w0, None).scale)
    # the module: with a residual (QTensor, summed), without one what it returned before
    ln = pq.LayerNormQuant(w, b, 1e-5)
    qm, sm = ln(x, residual=r)
    assert torch.equal(sm, s) and torch.equal(qm.int_data, qt.int_data) and torch.equal(qm.scale, qt.scale)
    plain = ln(s)
    assert isinstance(plain, pq.QTensor) and torch.equal(plain.int_data, qt.int_data) and torch.equal(plain.scale, qt.scale)


def test_python_entry_refuses_overlapping_outputs(pq):
    from protoquant_amd import _lib
    x = torch.randn(8, 512, device="cuda").to(torch.bfloat16)
    r = torch.randn(8, 512, device="cuda").to(torch.bfloat16)
    w = torch.ones(512, dtype=torch.bfloat16, device="cuda")
    buf = torch.zeros(9, 512, dtype=torch.bfloat16, device="cuda")
    buf[:8] = x
    with pytest.raises(_lib.PQError, match="sum_out overlaps x"):
        pq.add_layernorm_quantize(buf[:8], r, w, None, out=buf[1:9])              # shifted by one row: overlaps x without being x
    flat = torch.zeros(8 * 512, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_lib.PQError, match="sum_out overlaps bias"):
        pq.add_layernorm_quantize(x, r, w, flat[7 * 512:], out=flat.view(8, 512))      # the bias lies in the last row of the destination
    with pytest.raises(_lib.PQError, match="sum_out overlaps weight"):
        pq.add_layernorm_quantize(x, r, flat[:512], None, out=flat.view(8, 512))
    with pytest.raises(ValueError):
        pq.add_layernorm_quantize(x, r[:, :256], w, None)
    with pytest.raises(ValueError):
        pq.add_layernorm_quantize(x, r, w, None, out=torch.empty(8, 256, dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(ValueError):
        pq.add_layernorm_quantize(x, r, w, None, out=torch.empty(512, 8, dtype=torch.bfloat16, device="cuda").t())      # no row view with contiguous columns
