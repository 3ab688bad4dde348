"""-m gpu: K1oq (olmo_postnorm_add_quantize), K1oa (olmo_postnorm_add) and K1on (olmo_rmsnorm) — pq_olmo_postnorm_add_quant_rowwise — against the CPU specification
(tests/olmo_spec.py: NO1-NO5, PO1, A1, Q1-Q6) and against the library composition of their docstrings (K1on, a torch add on the GPU, K1), bit for bit — codes, scales,
the stored sum and the norm alone; NaNs as a class — for bf16, fp16 and f32.  Rows 1, 5 and 33 (5 and 33 leave a partial four-row block in the wave layout); the widths
of tests/test_gpu_gemma_postnorm.py, which reach every row layout (one wave per row at 1 / 2 / 4 vectors per lane — 8 with PQ_RMS_WAVE_MAX=512 — 256 threads per row at
1 .. 16 vectors, and on short rows with PQ_RMS_WAVE_MAX=0), the generic kernel on a ragged width, past the vector limit, on unaligned bases and odd leading
dimensions; ld_x > cols; sum_out as x, as residual and as a tensor of its own; a NaN row, an Inf row and a zero row placed in x, so that p and the sum carry them;
guarded margins around every output; K1oa's sum equal to K1oq's and nothing else written; the row of a 33 x 2048 case whose p is changed most by its storage rounding,
which a kernel that skips that rounding fails; and K1on alone on a strided slice, the shape of the k slice of a fused q / k / v output."""
import functools

import numpy as np
import pytest
import torch

from tests import olmo_spec as O
from tests.gemma_spec import nan_class_equal as _nan_class_equal

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
IDS = ["bf16", "fp16", "f32"]
POST_EPS = 1e-5
ROWS = (1, 5, 33)
# 16-bit widths (halved for f32), as tests/test_gpu_gemma_postnorm.py: 1 vector; one wave x 1 vector; x 2 (a partial second slot); x 4; 256 threads x 2 (288 vectors),
# x 4 (576), x 8 (1152), x 16 (the vector limit); ragged (generic); one vector past the limit (generic)
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
    """33 rows of x, residual and a post-norm weight, with the specification computed ONCE (rows are independent: the first 1 and 5 rows are their own cases).  Rows are
    scaled over 0.002 .. 20.  In x, row 2 holds a NaN, row 3 an Inf and row 4 is zero — p and the sum carry them (row 4 of the sum is the residual's).
    Returns x, r, pw, (q, scale, s bits), p (the norm alone)."""
    g = torch.Generator().manual_seed(3000 + cols)
    scale = torch.exp(torch.empty(33, 1).uniform_(float(np.log(0.002)), float(np.log(20.0)), generator=g))
    x = (torch.randn(33, cols, generator=g) * scale).to(dtype)
    r = (torch.randn(33, cols, generator=g) * 2.0).to(dtype)
    pw = (1.0 + 0.3 * torch.randn(cols, generator=g)).to(dtype)
    x[2, cols // 3] = float("nan")
    x[3, cols // 2] = float("inf")
    x[4] = 0.0
    return x, r, pw, O.postnorm_add_quantize(x, pw, r, POST_EPS), O.rmsnorm(x, pw, POST_EPS)


def _check(pq, xd, rd, pwd, spec, p_spec, rows, what, out=None, pair=True):
    """K1oq, K1oa and K1on on the same operands, against the spec and (pair) against the library composition K1on + torch add + K1.  `out`: None, "x" or "residual"
    (K1on: None or "x")."""
    q_s, sc_s, s_s = spec
    x0, r0 = xd.clone(), rd.clone()
    if pair:
        with torch.no_grad():
            pair_s = rd + pq.olmo_rmsnorm(xd, pwd, POST_EPS)
            pair_q = pq.quantize(pair_s)
    x2, r2 = x0.clone(), r0.clone()          # (x0 / r0 may be strided views' clones: contiguous, the same values)
    x3 = x0.clone()
    pick = lambda a, b: {None: None, "x": a, "residual": b}[out]          # noqa: E731
    qt, summed = pq.olmo_postnorm_add_quantize(xd, pwd, rd, POST_EPS, out=pick(xd, rd))          # K1oq
    summed2 = pq.olmo_postnorm_add(x2, pwd, r2, POST_EPS, out=pick(x2, r2))                      # K1oa
    p = pq.olmo_rmsnorm(x3, pwd, POST_EPS, out=x3 if out == "x" else None)                       # K1on
    torch.cuda.synchronize()
    assert out is None or (summed is pick(xd, rd) and summed2 is pick(x2, r2))
    assert out != "x" or p is x3
    assert summed.shape == xd.shape and p.shape == xd.shape and qt.int_data.shape == xd.shape
    _nan_class_equal(summed, s_s[:rows], what + ": sum")
    _nan_class_equal(summed2, s_s[:rows], what + ": sum (K1oa)")
    assert torch.equal(summed2.view(torch.uint8), summed.view(torch.uint8)), what + ": K1oa's sum is not K1oq's"
    _nan_class_equal(p, p_spec[:rows], what + ": the norm alone (K1on)")
    _nan_class_equal(qt.scale, sc_s[:rows], what + ": scales")
    assert np.array_equal(qt.int_data.cpu().numpy(), q_s[:rows]), what + ": codes"
    if pair:
        _nan_class_equal(summed, pair_s, what + ": sum vs the composition")
        _nan_class_equal(qt.scale, pair_q.scale, what + ": scales vs the composition")
        assert torch.equal(qt.int_data, pair_q.int_data), what + ": codes vs the composition"
    for xs, rs in ((xd, rd), (x2, r2)):
        if out != "x":
            assert torch.equal(xs.view(torch.uint8), x0.view(torch.uint8)), what + ": x was written"
        if out != "residual":
            assert torch.equal(rs.view(torch.uint8), r0.view(torch.uint8)), what + ": residual was written"
    if out != "x":
        assert torch.equal(x3.view(torch.uint8), x0.view(torch.uint8)), what + ": K1on wrote x"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("width", WIDTHS)
def test_matches_the_spec_and_the_composition(pq, dtype, width):
    cols = _cols(width, dtype)
    x, r, pw, spec, p_spec = _case(dtype, cols)
    pwd = pw.cuda()
    for rows, out in zip(ROWS, ("x", "residual", None)):
        _check(pq, x[:rows].cuda(), r[:rows].cuda(), pwd, spec, p_spec, rows, f"{dtype} {rows}x{cols} out={out}", out=out)
    _check(pq, x.cuda(), r.cuda(), pwd, spec, p_spec, 33, f"{dtype} 33x{cols} out=x", out="x", pair=False)
    # ld_x > cols: a column block of a wider tensor, at an offset that keeps the 16-byte alignment; in place over it as well
    wide = torch.zeros(5, cols + 32, dtype=dtype)
    wide[:, 16:16 + cols] = x[:5]
    q_s, sc_s, s_s = spec
    for out in (None, "x"):
        for form in ("K1oq", "K1oa", "K1on"):
            wd_x = wide.cuda()
            view = wd_x[:, 16:16 + cols]
            assert view.stride(0) == cols + 32
            dst = view if out else None
            what = f"{dtype} 5x{cols} ld_x = cols + 32 out={out} {form}"
            if form == "K1oq":
                qt, got = pq.olmo_postnorm_add_quantize(view, pwd, r[:5].cuda(), POST_EPS, out=dst)
                _nan_class_equal(qt.scale, sc_s[:5], what + ": scales")
                assert np.array_equal(qt.int_data.cpu().numpy(), q_s[:5]), what
            elif form == "K1oa":
                got = pq.olmo_postnorm_add(view, pwd, r[:5].cuda(), POST_EPS, out=dst)
            else:
                got = pq.olmo_rmsnorm(view, pwd, POST_EPS, out=dst)
            _nan_class_equal(got, p_spec[:5] if form == "K1on" else s_s[:5], what)
            assert not bool(wd_x[:, :16].float().abs().sum() > 0) and not bool(wd_x[:, 16 + cols:].float().abs().sum() > 0), "columns outside the view were written"
            if out is None:
                assert torch.equal(view.cpu().view(torch.uint8), x[:5].contiguous().view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("wave_max,width", [("512", 3072), ("0", 512)])
def test_wave_max_switch_changes_no_bit(pq, pq_opt, dtype, wave_max, width):
    """PQ_RMS_WAVE_MAX=512 at 3072 columns: one wave per row at 8 vectors per lane (384 vectors; 256 threads x 2 by default); PQ_RMS_WAVE_MAX=0 at 512 columns: the
    256-thread layout on a short row.  Time only, never bits; the fixture restores the option."""
    cols = _cols(width, dtype)
    x, r, pw, spec, p_spec = _case(dtype, cols)
    pq_opt("PQ_RMS_WAVE_MAX", wave_max)
    pwd = pw.cuda()
    for rows, out in zip(ROWS, (None, "x", "residual")):
        _check(pq, x[:rows].cuda(), r[:rows].cuda(), pwd, spec, p_spec, rows, f"PQ_RMS_WAVE_MAX={wave_max} {dtype} {rows}x{cols} out={out}", out=out, pair=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unaligned_bases_and_odd_leading_dimensions_take_the_generic_kernel(pq, dtype):
    """x at a column offset of 3 elements (ld_x = cols + 37), the residual at an offset of 1, the sum at an offset of 5: nothing is 16-byte aligned"""
    cols = _cols(512, dtype)
    x, r, pw, spec, p_spec = _case(dtype, cols)
    q_s, sc_s, s_s = spec
    rows = 5
    big_x = torch.zeros(rows, cols + 37, dtype=dtype)
    big_r = torch.zeros(rows, cols + 11, dtype=dtype)
    big_x[:, 3:3 + cols], big_r[:, 1:1 + cols] = x[:rows], r[:rows]
    bx, br, pwd = big_x.cuda(), big_r.cuda(), pw.cuda()
    xv, rv = bx[:, 3:3 + cols], br[:, 1:1 + cols]
    big_o = torch.zeros(rows, cols + 5, dtype=dtype, device="cuda")
    ov = big_o[:, 5:5 + cols]
    qt, summed = pq.olmo_postnorm_add_quantize(xv, pwd, rv, POST_EPS, out=ov)
    assert summed is ov
    _nan_class_equal(ov, s_s[:rows], "strided sum")
    _nan_class_equal(qt.scale, sc_s[:rows], "scales")
    assert np.array_equal(qt.int_data.cpu().numpy(), q_s[:rows])
    assert not bool(big_o[:, :5].float().abs().sum() > 0), "columns outside the output view were written"
    big_o.zero_()
    assert pq.olmo_postnorm_add(xv, pwd, rv, POST_EPS, out=ov) is ov
    _nan_class_equal(ov, s_s[:rows], "strided sum (K1oa)")
    big_o.zero_()
    assert pq.olmo_rmsnorm(xv, pwd, POST_EPS, out=ov) is ov
    _nan_class_equal(ov, p_spec[:rows], "strided norm (K1on)")
    assert not bool(big_o[:, :5].float().abs().sum() > 0)
    _nan_class_equal(pq.olmo_rmsnorm(xv, pwd, POST_EPS), p_spec[:rows], "K1on from a strided x into a tensor of its own")
    assert torch.equal(bx.cpu().view(torch.uint8), big_x.view(torch.uint8)) and torch.equal(br.cpu().view(torch.uint8), big_r.view(torch.uint8))          # (bytes: x holds a NaN)
    # in place over the strided x, then over the strided residual; the three forms
    for target in ("x", "residual"):
        for form in ("K1oq", "K1oa", "K1on"):
            if form == "K1on" and target == "residual":
                continue
            bx2, br2 = bx.clone(), br.clone()
            xv2, rv2 = bx2[:, 3:3 + cols], br2[:, 1:1 + cols]
            dst = xv2 if target == "x" else rv2
            if form == "K1on":
                got = pq.olmo_rmsnorm(xv2, pwd, POST_EPS, out=dst)
            elif form == "K1oa":
                got = pq.olmo_postnorm_add(xv2, pwd, rv2, POST_EPS, out=dst)
            else:
                qt, got = pq.olmo_postnorm_add_quantize(xv2, pwd, rv2, POST_EPS, out=dst)
                assert np.array_equal(qt.int_data.cpu().numpy(), q_s[:rows])
                _nan_class_equal(qt.scale, sc_s[:rows], "scales")
            assert got is dst
            _nan_class_equal(got, p_spec[:rows] if form == "K1on" else s_s[:rows], f"in place over strided {target}, {form}")
            touched, ref_big, off = (bx2, bx, 3) if target == "x" else (br2, br, 1)
            assert torch.equal(touched[:, :off], ref_big[:, :off]) and torch.equal(touched[:, off + cols:], ref_big[:, off + cols:])
            assert torch.equal((br2 if target == "x" else bx2).view(torch.uint8), (br if target == "x" else bx).view(torch.uint8))          # the other input is untouched


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,width", [(5, 512), (33, 2304), (5, 32768), (5, 333)])
def test_guarded_margins_stay_untouched(pq, dtype, rows, width):
    """every output buffer (sum, codes, scales) lies inside a larger allocation filled with a pattern: K1oq writes its rows and nothing around them, K1oa and K1on write
    sum_out and NOTHING else.  Raw C-ABI calls on interior views, 16-byte aligned for the vector layouts."""
    from protoquant_amd import _lib as L
    cols = _cols(width, dtype)
    x, r, pw, spec, p_spec = _case(dtype, cols)
    q_s, sc_s, s_s = spec
    xd, rd, pwd = x[:rows].cuda(), r[:rows].cuda(), pw.cuda()
    m = 4096          # margin in elements: a multiple of 16 bytes for every dtype
    for form in ("K1oq", "K1oa", "K1on"):
        sum_all = torch.full((rows * cols + 2 * m,), 7.0, dtype=dtype, device="cuda")
        q_all = torch.full((rows * cols + 2 * m,), 77, dtype=torch.int8, device="cuda")
        sc_all = torch.full((rows + 2 * m,), 7.0, dtype=torch.float32, device="cuda")
        s_v, q_v, sc_v = sum_all[m:m + rows * cols], q_all[m:m + rows * cols], sc_all[m:m + rows]
        quant, add = form == "K1oq", form != "K1on"
        with torch.cuda.device(xd.device):
            L.check(L.lib().pq_olmo_postnorm_add_quant_rowwise(xd.data_ptr(), cols, pwd.data_ptr(), POST_EPS, rd.data_ptr() if add else None, cols if add else 0, s_v.data_ptr(), cols,
                                                               L.dtype_code(dtype), rows, cols, q_v.data_ptr() if quant else None, cols if quant else 0,
                                                               sc_v.data_ptr() if quant else None, L.stream_ptr(xd)), "raw " + form)
        torch.cuda.synchronize()
        _nan_class_equal(s_v.view(rows, cols), s_s[:rows] if add else p_spec[:rows], f"{form}: sum_out")
        if quant:
            _nan_class_equal(sc_v, sc_s[:rows], "scales")
            assert np.array_equal(q_v.view(rows, cols).cpu().numpy(), q_s[:rows])
        else:
            assert bool((q_all == 77).all()) and bool((sc_all == 7.0).all()), f"{form} wrote something else than sum_out"
        for name, buf, n, fill in (("sum", sum_all, rows * cols, 7.0), ("codes", q_all, rows * cols, 77), ("scales", sc_all, rows, 7.0)):
            assert bool((buf[:m] == fill).all()) and bool((buf[m + n:] == fill).all()), f"{form}: the margin around {name} was written"
        assert torch.equal(xd.cpu().view(torch.uint8), x[:rows].contiguous().view(torch.uint8)) and torch.equal(rd.cpu().view(torch.uint8), r[:rows].contiguous().view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES[:2], ids=IDS[:2])
def test_the_storage_rounding_of_p_happens(pq, dtype):
    """33 x 2048 (one wave per row at 4 vectors per lane), the row whose p differs from its unrounded binary32 value in the most elements — the spec shows which.  The
    unrounded variant of the spec gives OTHER sum bits on that row (asserted: the case cannot go vacuous), so a kernel that adds the binary32 p fails here.  Also at
    2304 columns (256 threads per row) and 333 (generic), rows chosen the same way."""
    for cols in (2048, 2304, 333):
        x, r, pw, spec, p_spec = _case(dtype, cols)
        pu = torch.from_numpy(O.unrounded_p(x, pw, POST_EPS))
        finite = torch.isfinite(pu).all(dim=1)
        changed = ((p_spec.float() != pu) & finite[:, None]).sum(dim=1)
        row = int(changed.argmax())
        assert int(changed[row]) > cols // 2, (cols, row, int(changed[row]))
        want = torch.from_numpy(spec[2][row:row + 1].view(np.int16).copy())
        wrong = O.unrounded_sum(x[row:row + 1], pw, r[row:row + 1], POST_EPS).view(torch.int16)
        n_wrong = int((wrong != want).sum())
        print(f"{dtype} cols {cols}: row {row}, p changed by its rounding in {int(changed[row])} elements, the unrounded sum differs in {n_wrong}")
        assert n_wrong > 0, "the unrounded variant stores the same sum: this case would show nothing"
        xd, rd = x[row:row + 1].cuda(), r[row:row + 1].cuda()
        qt, summed = pq.olmo_postnorm_add_quantize(xd, pw.cuda(), rd, POST_EPS)
        only = pq.olmo_postnorm_add(xd, pw.cuda(), rd, POST_EPS)
        assert torch.equal(summed.cpu().view(torch.int16), want) and torch.equal(only.cpu().view(torch.int16), want)
        assert not torch.equal(summed.cpu().view(torch.int16), wrong)
        assert np.array_equal(qt.int_data.cpu().numpy(), spec[0][row:row + 1])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_k1on_on_the_k_slice_of_a_fused_qkv_output(pq, dtype):
    """[batch, seq, q + k + v] with q = 256, k = v = 128: the k slice starts 256 elements in and its rows are 512 apart — K1on reads it in place (no copy) and stores
    a contiguous tensor; the module is the function"""
    g = torch.Generator().manual_seed(77)
    qkv = torch.randn(2, 7, 512, generator=g).to(dtype)
    w = (1.0 + 0.3 * torch.randn(128, generator=g)).to(dtype)
    qkv_d, wd = qkv.cuda(), w.cuda()
    k = qkv_d[..., 256:384]
    assert not k.is_contiguous()
    got = pq.olmo_rmsnorm(k, wd, 1e-6)
    assert got.shape == (2, 7, 128) and got.is_contiguous()
    want = O.rmsnorm(qkv[..., 256:384].reshape(14, 128), w, 1e-6)
    _nan_class_equal(got.reshape(14, 128), want, "K1on on the k slice")
    assert torch.equal(qkv_d.cpu(), qkv), "the fused output was written"
    mod = pq.OlmoRMSNorm(torch.nn.Parameter(wd, requires_grad=False), 1e-6)
    assert torch.equal(mod(k), got) and list(mod.state_dict()) == ["weight"] and mod.weight.data_ptr() == wd.data_ptr()


def test_batch_shapes_alias_errors_and_empty_inputs(pq):
    """[batch, seq, hidden] inputs keep their shape; an `out` that overlaps an input without being it is refused, naming the operands; empty inputs launch nothing"""
    from protoquant_amd import _lib
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 7, 512, generator=g).to(torch.bfloat16).cuda()
    r = torch.randn(2, 7, 512, generator=g).to(torch.bfloat16).cuda()
    pw = (1.0 + 0.3 * torch.randn(512, generator=g)).to(torch.bfloat16).cuda()
    qt, s = pq.olmo_postnorm_add_quantize(x, pw, r, POST_EPS)
    assert s.shape == x.shape and qt.int_data.shape == x.shape and qt.scale.shape == (14,)
    q_s, sc_s, s_s = O.postnorm_add_quantize(x.reshape(14, 512), pw, r.reshape(14, 512), POST_EPS)
    _nan_class_equal(s.reshape(14, 512), s_s, "sum")
    assert np.array_equal(qt.int_data.reshape(14, 512).cpu().numpy(), q_s)
    _nan_class_equal(qt.scale, sc_s, "scales")
    assert torch.equal(pq.olmo_postnorm_add(x, pw, r, POST_EPS), s)
    big = torch.zeros(6, 512, dtype=torch.bfloat16, device="cuda")
    x2 = x.reshape(14, 512)[:4]
    for call in (lambda: pq.olmo_postnorm_add_quantize(big[:4], pw, x2, out=big[1:5]), lambda: pq.olmo_postnorm_add(x2, pw, big[:4], out=big[2:6]),
                 lambda: pq.olmo_rmsnorm(big[:4], pw, out=big[1:5])):
        with pytest.raises(_lib.PQError, match="sum_out overlaps"):
            call()
    assert not bool(big.float().abs().sum() > 0)
    e = torch.empty(0, 512, dtype=torch.bfloat16, device="cuda")
    qe, se = pq.olmo_postnorm_add_quantize(e, pw, e)
    assert se.shape == (0, 512) and qe.int_data.shape == (0, 512) and qe.scale.shape == (0,)
    assert pq.olmo_postnorm_add(e, pw, e).shape == (0, 512) and pq.olmo_rmsnorm(e, pw).shape == (0, 512)
    z = torch.empty(3, 0, dtype=torch.bfloat16, device="cuda")
    w0 = torch.empty(0, dtype=torch.bfloat16, device="cuda")
    qz, sz = pq.olmo_postnorm_add_quantize(z, w0, z)
    assert sz.shape == (3, 0) and qz.int_data.shape == (3, 0) and qz.scale.tolist() == [1.0, 1.0, 1.0]          # QSPEC Q3
    assert pq.olmo_rmsnorm(z, w0).shape == (3, 0)
