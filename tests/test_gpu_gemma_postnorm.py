"""-m gpu: K1pang (gemma_postnorm_add_rmsnorm_quantize) and K1pa (gemma_postnorm_add) — pq_gemma_postnorm_add_rmsnorm_quant_rowwise — against the CPU specification
(tests/gemma_postnorm_spec.py: PN1, A1, NG1-NG6, Q1-Q6) and against the library composition of their docstrings (K1ng with h, a torch add on the GPU, K1ng), bit for
bit — codes, scales, the stored sum and h; NaNs as a class — for bf16, fp16 and f32.  Rows 1, 5 and 33 (5 and 33 leave a partial four-row block in the wave layout);
the widths of tests/test_gpu_gemma_norm.py, which reach every row layout (one wave per row at 1 / 2 / 4 vectors per lane — 8 with PQ_RMS_WAVE_MAX=512 — 256 threads
per row at 1 .. 16 vectors, and on short rows with PQ_RMS_WAVE_MAX=0), the generic kernel on a ragged width, past the vector limit, on unaligned bases and odd leading
dimensions; ld_x > cols; with and without h_out; sum_out as x, as residual and as a tensor of its own; post_eps != eps and post_weight != weight throughout; a NaN
row, an Inf row and a zero row placed in x, so that p and the sum carry them; guarded margins around every output; K1pa's sum equal to K1pang's and nothing else
written; and the row of a 33 x 2048 case whose p is changed most by its storage rounding, which a kernel that skips that rounding fails."""
import functools

import numpy as np
import pytest
import torch

from tests import gemma_postnorm_spec as P
from tests.gemma_spec import nan_class_equal as _nan_class_equal

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
IDS = ["bf16", "fp16", "f32"]
EPS, POST_EPS = 1e-6, 1e-5          # distinct: a kernel that uses one for both differs on the small rows
ROWS = (1, 5, 33)
# 16-bit widths (halved for f32), as tests/test_gpu_gemma_norm.py: 1 vector; one wave x 1 vector; x 2 (a partial second slot); x 4; 256 threads x 2 (288 vectors),
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
    """33 rows of x, residual, a post-norm weight and a norm weight, with the specification computed ONCE (rows are independent: the first 1 and 5 rows are their own
    cases).  Rows are scaled over 0.002 .. 20 (below ~0.003 the two eps differ in the stored p).  In x, row 2 holds a NaN, row 3 an Inf and row 4 is zero — p and
    the sum carry them (row 4 of the sum is the residual's)."""
    g = torch.Generator().manual_seed(2000 + cols)
    scale = torch.exp(torch.empty(33, 1).uniform_(float(np.log(0.002)), float(np.log(20.0)), generator=g))
    x = (torch.randn(33, cols, generator=g) * scale).to(dtype)
    r = (torch.randn(33, cols, generator=g) * 2.0).to(dtype)
    pw = (0.3 * torch.randn(cols, generator=g)).to(dtype)
    w = (0.3 * torch.randn(cols, generator=g)).to(dtype)
    x[2, cols // 3] = float("nan")
    x[3, cols // 2] = float("inf")
    x[4] = 0.0
    return x, r, pw, w, P.postnorm_add_rmsnorm_quantize(x, pw, r, w, EPS, POST_EPS)


def _check(pq, xd, rd, pwd, wd, spec, rows, what, out=None, pair=True):
    """K1pang with and without h_out and K1pa on the same operands, against the spec and (pair) against the library composition.  `out`: None, "x" or "residual"."""
    q_s, sc_s, s_s, h_s = spec
    x0, r0 = xd.clone(), rd.clone()
    if pair:
        with torch.no_grad():
            p = pq.gemma_rmsnorm_quantize(xd, pwd, POST_EPS, return_h=True)[1]
            pair_s = rd + p
            pair_q, pair_h = pq.gemma_rmsnorm_quantize(pair_s, wd, EPS, return_h=True)
    x2, r2 = x0.clone(), r0.clone()          # (x0 / r0 may be strided views' clones: contiguous, the same values)
    x3, r3 = x0.clone(), r0.clone()
    pick = lambda a, b: {None: None, "x": a, "residual": b}[out]          # noqa: E731
    qt, summed, h = pq.gemma_postnorm_add_rmsnorm_quantize(xd, pwd, rd, wd, EPS, POST_EPS, out=pick(xd, rd), return_h=True)
    qt2, summed2 = pq.gemma_postnorm_add_rmsnorm_quantize(x2, pwd, r2, wd, EPS, POST_EPS, out=pick(x2, r2))          # the instantiation without h_out
    summed3 = pq.gemma_postnorm_add(x3, pwd, r3, POST_EPS, out=pick(x3, r3))                                          # K1pa
    torch.cuda.synchronize()
    assert out is None or (summed is pick(xd, rd) and summed2 is pick(x2, r2) and summed3 is pick(x3, r3))
    assert summed.shape == xd.shape and h.shape == xd.shape and qt.int_data.shape == xd.shape
    for s, tag in ((summed, ""), (summed2, " (no h)"), (summed3, " (K1pa)")):
        _nan_class_equal(s, s_s[:rows], what + ": sum" + tag)
    assert torch.equal(summed3.view(torch.uint8), summed.view(torch.uint8)), what + ": K1pa's sum is not K1pang's"
    _nan_class_equal(h, h_s[:rows], what + ": h")
    for t, tag in ((qt, ""), (qt2, " (no h)")):
        _nan_class_equal(t.scale, sc_s[:rows], what + ": scales" + tag)
        assert np.array_equal(t.int_data.cpu().numpy(), q_s[:rows]), what + ": codes" + tag
    if pair:
        _nan_class_equal(summed, pair_s, what + ": sum vs the composition")
        _nan_class_equal(h, pair_h, what + ": h vs the composition")
        _nan_class_equal(qt.scale, pair_q.scale, what + ": scales vs the composition")
        assert torch.equal(qt.int_data, pair_q.int_data), what + ": codes vs the composition"
    for xs, rs in ((xd, rd), (x2, r2), (x3, r3)):
        if out != "x":
            assert torch.equal(xs.view(torch.uint8), x0.view(torch.uint8)), what + ": x was written"
        if out != "residual":
            assert torch.equal(rs.view(torch.uint8), r0.view(torch.uint8)), what + ": residual was written"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("width", WIDTHS)
def test_matches_the_spec_and_the_composition(pq, dtype, width):
    cols = _cols(width, dtype)
    x, r, pw, w, spec = _case(dtype, cols)
    pwd, wd = pw.cuda(), w.cuda()
    for rows, out in zip(ROWS, ("x", "residual", None)):
        _check(pq, x[:rows].cuda(), r[:rows].cuda(), pwd, wd, spec, rows, f"{dtype} {rows}x{cols} out={out}", out=out)
    _check(pq, x.cuda(), r.cuda(), pwd, wd, spec, 33, f"{dtype} 33x{cols} out=x", out="x", pair=False)
    # ld_x > cols: a column block of a wider tensor, at an offset that keeps the 16-byte alignment; in place over it as well
    wide = torch.zeros(5, cols + 32, dtype=dtype)
    wide[:, 16:16 + cols] = x[:5]
    for out in (None, "x"):
        wd_x = wide.cuda()
        view = wd_x[:, 16:16 + cols]
        assert view.stride(0) == cols + 32
        q_s, sc_s, s_s, h_s = spec
        qt, summed, h = pq.gemma_postnorm_add_rmsnorm_quantize(view, pwd, r[:5].cuda(), wd, EPS, POST_EPS, out=view if out else None, return_h=True)
        _nan_class_equal(summed, s_s[:5], f"{dtype} 5x{cols} ld_x = cols + 32 out={out}: sum")
        _nan_class_equal(h, h_s[:5], "h")
        _nan_class_equal(qt.scale, sc_s[:5], "scales")
        assert np.array_equal(qt.int_data.cpu().numpy(), q_s[:5])
        assert not bool(wd_x[:, :16].float().abs().sum() > 0) and not bool(wd_x[:, 16 + cols:].float().abs().sum() > 0), "columns outside the view were written"
        if out is None:
            assert torch.equal(view.cpu().view(torch.uint8), x[:5].contiguous().view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_two_eps_and_the_two_weights_are_told_apart(dtype):
    """(CPU only, on the spec: the GPU cases above are held to it) swapping post_eps and eps, or the two weights, changes the specified outputs of the shared case"""
    cols = _cols(512, dtype)
    x, r, pw, w, spec = _case(dtype, cols)
    swapped_eps = P.postnorm_add_rmsnorm_quantize(x, pw, r, w, POST_EPS, EPS)
    swapped_w = P.postnorm_add_rmsnorm_quantize(x, w, r, pw, EPS, POST_EPS)
    assert not np.array_equal(swapped_eps[2][5:], spec[2][5:]) and not np.array_equal(swapped_w[2][5:], spec[2][5:])
    assert not np.array_equal(swapped_w[0][5:], spec[0][5:])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("wave_max,width", [("512", 3072), ("0", 512)])
def test_wave_max_switch_changes_no_bit(pq, pq_opt, dtype, wave_max, width):
    """PQ_RMS_WAVE_MAX=512 at 3072 columns: one wave per row at 8 vectors per lane (384 vectors; 256 threads x 2 by default); PQ_RMS_WAVE_MAX=0 at 512 columns: the
    256-thread layout on a short row.  Time only, never bits; the fixture restores the option."""
    cols = _cols(width, dtype)
    x, r, pw, w, spec = _case(dtype, cols)
    pq_opt("PQ_RMS_WAVE_MAX", wave_max)
    pwd, wd = pw.cuda(), w.cuda()
    for rows, out in zip(ROWS, (None, "x", "residual")):
        _check(pq, x[:rows].cuda(), r[:rows].cuda(), pwd, wd, spec, rows, f"PQ_RMS_WAVE_MAX={wave_max} {dtype} {rows}x{cols} out={out}", out=out, pair=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unaligned_bases_and_odd_leading_dimensions_take_the_generic_kernel(pq, dtype):
    cols = _cols(512, dtype)
    x, r, pw, w, spec = _case(dtype, cols)
    q_s, sc_s, s_s, h_s = spec
    rows = 5
    big_x = torch.zeros(rows, cols + 37, dtype=dtype)
    big_r = torch.zeros(rows, cols + 11, dtype=dtype)
    big_x[:, 3:3 + cols], big_r[:, 1:1 + cols] = x[:rows], r[:rows]
    bx, br, pwd, wd = big_x.cuda(), big_r.cuda(), pw.cuda(), w.cuda()
    xv, rv = bx[:, 3:3 + cols], br[:, 1:1 + cols]
    big_o = torch.zeros(rows, cols + 5, dtype=dtype, device="cuda")
    ov = big_o[:, 5:5 + cols]
    qt, summed, h = pq.gemma_postnorm_add_rmsnorm_quantize(xv, pwd, rv, wd, EPS, POST_EPS, out=ov, return_h=True)
    assert summed is ov
    _nan_class_equal(ov, s_s[:rows], "strided sum")
    _nan_class_equal(h, h_s[:rows], "h")
    _nan_class_equal(qt.scale, sc_s[:rows], "scales")
    assert np.array_equal(qt.int_data.cpu().numpy(), q_s[:rows])
    assert not bool(big_o[:, :5].float().abs().sum() > 0), "columns outside the output view were written"
    big_o.zero_()
    assert pq.gemma_postnorm_add(xv, pwd, rv, POST_EPS, out=ov) is ov
    _nan_class_equal(ov, s_s[:rows], "strided sum (K1pa)")
    assert not bool(big_o[:, :5].float().abs().sum() > 0)
    assert torch.equal(bx.cpu().view(torch.uint8), big_x.view(torch.uint8)) and torch.equal(br.cpu().view(torch.uint8), big_r.view(torch.uint8))          # (bytes: x holds a NaN)
    # in place over the strided x, then over the strided residual; K1pang and K1pa
    for target in ("x", "residual"):
        for add_only in (False, True):
            bx2, br2 = bx.clone(), br.clone()
            xv2, rv2 = bx2[:, 3:3 + cols], br2[:, 1:1 + cols]
            dst = xv2 if target == "x" else rv2
            if add_only:
                summed = pq.gemma_postnorm_add(xv2, pwd, rv2, POST_EPS, out=dst)
            else:
                qt, summed = pq.gemma_postnorm_add_rmsnorm_quantize(xv2, pwd, rv2, wd, EPS, POST_EPS, out=dst)
                assert np.array_equal(qt.int_data.cpu().numpy(), q_s[:rows])
                _nan_class_equal(qt.scale, sc_s[:rows], "scales")
            assert summed is dst
            _nan_class_equal(summed, s_s[:rows], f"in place over strided {target}, add_only={add_only}")
            touched, ref_big, off = (bx2, bx, 3) if target == "x" else (br2, br, 1)
            assert torch.equal(touched[:, :off], ref_big[:, :off]) and torch.equal(touched[:, off + cols:], ref_big[:, off + cols:])
            assert torch.equal((br2 if target == "x" else bx2).view(torch.uint8), (br if target == "x" else bx).view(torch.uint8))          # the other input is untouched


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,width", [(5, 512), (33, 2304), (5, 32768), (5, 333)])
def test_guarded_margins_stay_untouched(pq, dtype, rows, width):
    """every output buffer (sum, codes, scales, h) lies inside a larger allocation filled with a pattern: K1pang writes its rows and nothing around them, K1pa writes
    the sum and NOTHING else.  Raw C-ABI calls on interior views, 16-byte aligned for the vector layouts."""
    from protoquant_amd import _lib as L
    cols = _cols(width, dtype)
    x, r, pw, w, spec = _case(dtype, cols)
    q_s, sc_s, s_s, h_s = spec
    xd, rd, pwd, wd = x[:rows].cuda(), r[:rows].cuda(), pw.cuda(), w.cuda()
    m = 4096          # margin in elements: a multiple of 16 bytes for every dtype
    for add_only in (False, True):
        sum_all = torch.full((rows * cols + 2 * m,), 7.0, dtype=dtype, device="cuda")
        h_all = torch.full((rows * cols + 2 * m,), 7.0, dtype=dtype, device="cuda")
        q_all = torch.full((rows * cols + 2 * m,), 77, dtype=torch.int8, device="cuda")
        sc_all = torch.full((rows + 2 * m,), 7.0, dtype=torch.float32, device="cuda")
        s_v, h_v, q_v, sc_v = sum_all[m:m + rows * cols], h_all[m:m + rows * cols], q_all[m:m + rows * cols], sc_all[m:m + rows]
        with torch.cuda.device(xd.device):
            if add_only:
                L.check(L.lib().pq_gemma_postnorm_add_rmsnorm_quant_rowwise(xd.data_ptr(), cols, pwd.data_ptr(), POST_EPS, rd.data_ptr(), cols, s_v.data_ptr(), cols, None, 0.0,
                                                                            L.dtype_code(dtype), rows, cols, None, cols, None, None, cols, L.stream_ptr(xd)), "raw K1pa")
            else:
                L.check(L.lib().pq_gemma_postnorm_add_rmsnorm_quant_rowwise(xd.data_ptr(), cols, pwd.data_ptr(), POST_EPS, rd.data_ptr(), cols, s_v.data_ptr(), cols, wd.data_ptr(),
                                                                            EPS, L.dtype_code(dtype), rows, cols, q_v.data_ptr(), cols, sc_v.data_ptr(), h_v.data_ptr(), cols,
                                                                            L.stream_ptr(xd)), "raw K1pang")
        torch.cuda.synchronize()
        _nan_class_equal(s_v.view(rows, cols), s_s[:rows], f"add_only={add_only}: sum")
        if add_only:
            assert bool((h_all == 7.0).all()) and bool((q_all == 77).all()) and bool((sc_all == 7.0).all()), "K1pa wrote something else than the sum"
        else:
            _nan_class_equal(h_v.view(rows, cols), h_s[:rows], "h")
            _nan_class_equal(sc_v, sc_s[:rows], "scales")
            assert np.array_equal(q_v.view(rows, cols).cpu().numpy(), q_s[:rows])
        for name, buf, n, fill in (("sum", sum_all, rows * cols, 7.0), ("h", h_all, rows * cols, 7.0), ("codes", q_all, rows * cols, 77), ("scales", sc_all, rows, 7.0)):
            assert bool((buf[:m] == fill).all()) and bool((buf[m + n:] == fill).all()), f"add_only={add_only}: the margin around {name} was written"
        assert torch.equal(xd.cpu().view(torch.uint8), x[:rows].contiguous().view(torch.uint8)) and torch.equal(rd.cpu().view(torch.uint8), r[:rows].contiguous().view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES[:2], ids=IDS[:2])
def test_the_storage_rounding_of_p_happens(pq, dtype):
    """33 x 2048 (one wave per row at 4 vectors per lane), the row whose p differs from its unrounded binary32 value in the most elements — the spec shows which.  The
    unrounded variant of the spec gives OTHER sum bits on that row (asserted: the case cannot go vacuous), so a kernel that adds the binary32 p fails here.  Also at
    2304 columns (256 threads per row) and 333 (generic), rows chosen the same way."""
    for cols in (2048, 2304, 333):
        x, r, pw, w, spec = _case(dtype, cols)
        p, pu = P.postnorm(x, pw, POST_EPS), torch.from_numpy(P.unrounded_p(x, pw, POST_EPS))
        finite = torch.isfinite(pu).all(dim=1)
        changed = ((p.float() != pu) & finite[:, None]).sum(dim=1)
        row = int(changed.argmax())
        assert int(changed[row]) > cols // 2, (cols, row, int(changed[row]))
        want = torch.from_numpy(spec[2][row:row + 1].view(np.int16).copy())
        wrong = P.unrounded_sum(x[row:row + 1], pw, r[row:row + 1], POST_EPS).view(torch.int16)
        n_wrong = int((wrong != want).sum())
        print(f"{dtype} cols {cols}: row {row}, p changed by its rounding in {int(changed[row])} elements, the unrounded sum differs in {n_wrong}")
        assert n_wrong > 0, "the unrounded variant stores the same sum: this case would show nothing"
        xd, rd = x[row:row + 1].cuda(), r[row:row + 1].cuda()
        qt, summed = pq.gemma_postnorm_add_rmsnorm_quantize(xd, pw.cuda(), rd, w.cuda(), EPS, POST_EPS)
        only = pq.gemma_postnorm_add(xd, pw.cuda(), rd, POST_EPS)
        assert torch.equal(summed.cpu().view(torch.int16), want) and torch.equal(only.cpu().view(torch.int16), want)
        assert not torch.equal(summed.cpu().view(torch.int16), wrong)
        assert np.array_equal(qt.int_data.cpu().numpy(), spec[0][row:row + 1])


def test_batch_shapes_module_and_empty_inputs(pq):
    """[batch, seq, hidden] inputs keep their shape; GemmaSandwichNormQuant is the function; empty inputs launch nothing"""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 7, 512, generator=g).to(torch.bfloat16).cuda()
    r = torch.randn(2, 7, 512, generator=g).to(torch.bfloat16).cuda()
    pw = (0.3 * torch.randn(512, generator=g)).to(torch.bfloat16).cuda()
    w = (0.3 * torch.randn(512, generator=g)).to(torch.bfloat16).cuda()
    mod, post = pq.GemmaSandwichNormQuant(w, EPS), pq.GemmaRMSNormQuant(pw, POST_EPS)
    assert list(mod.state_dict()) == ["weight"]
    qt, s = mod(x, residual=r, post_norm=post)
    assert s.shape == x.shape and qt.int_data.shape == x.shape and qt.scale.shape == (14,)
    q_s, sc_s, s_s, _ = P.postnorm_add_rmsnorm_quantize(x.reshape(14, 512), pw, r.reshape(14, 512), w, EPS, POST_EPS)
    _nan_class_equal(s.reshape(14, 512), s_s, "sum")
    assert np.array_equal(qt.int_data.reshape(14, 512).cpu().numpy(), q_s)
    _nan_class_equal(qt.scale, sc_s, "scales")
    assert torch.equal(pq.gemma_postnorm_add(x, pw, r, POST_EPS), s)
    # without post_norm it is GemmaRMSNormQuant
    plain = pq.GemmaRMSNormQuant(w, EPS)
    assert torch.equal(mod(x).int_data, plain(x).int_data) and torch.equal(mod(x, residual=r)[1], plain(x, residual=r)[1])
    e = torch.empty(0, 512, dtype=torch.bfloat16, device="cuda")
    qe, se = pq.gemma_postnorm_add_rmsnorm_quantize(e, pw, e, w)
    assert se.shape == (0, 512) and qe.int_data.shape == (0, 512) and qe.scale.shape == (0,)
    assert pq.gemma_postnorm_add(e, pw, e).shape == (0, 512)
    z = torch.empty(3, 0, dtype=torch.bfloat16, device="cuda")
    w0 = torch.empty(0, dtype=torch.bfloat16, device="cuda")
    qz, sz = pq.gemma_postnorm_add_rmsnorm_quantize(z, w0, z, w0)
    assert sz.shape == (3, 0) and qz.int_data.shape == (3, 0) and qz.scale.tolist() == [1.0, 1.0, 1.0]          # QSPEC Q3
