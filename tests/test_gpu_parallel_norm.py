"""-m gpu: K1pl / K1l2, pq_parallel_layernorm_quant_rowwise / add2_layernorm_quantize / layernorm_quantize2 — the three-way add of a parallel-residual block fused
into one or two LayerNorms + per-token int8 quantisation.  The stored sum and, per norm, codes, scales and h are compared bit for bit (NaNs as a class) with (a) the
two torch adds on the GPU in the association (a + b) + c followed by layernorm_quantize per norm and (b) the CPU specification (tests/add2lnorm_spec.py), over a grid
that launches every instantiation: one wave per row at 1 / 2 / 4 vectors (8 with PQ_RMS_WAVE_MAX=512), 256 threads per row at 1 .. 16 vectors (and on short rows
with PQ_RMS_WAVE_MAX=0), the generic kernel on ragged widths, unaligned bases and odd leading dimensions; one and two norms, with and without the add group, a bias
present or absent per group, a different eps per group, out = None / a / b / c, return_h on and off; guarded margins around every output.  There is no tolerance
anywhere in this file."""
import numpy as np
import pytest
import torch

from tests import add2lnorm_spec as A2
from tests.gpu_util import bits

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
EPV = {torch.bfloat16: 8, torch.float16: 8, torch.float32: 4}
EPS1, EPS2 = 1e-5, 1e-3
FORMS = ("add2", "add1", "dual")          # K1pl with two norms, K1pl with one, K1l2
OUTS = ("none", "a", "b", "c")


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


def _same_bytes(t_gpu, t_cpu):
    return torch.equal(t_gpu.cpu().contiguous().view(torch.uint8), t_cpu.contiguous().view(torch.uint8))


def _check(pq, ins, what, form="add2", out_mode="none", bias=(True, True), against_spec=True):
    """ins: the CPU tensors of add2lnorm_spec.inputs.  Runs the fused kernel on copies on the GPU (with and without h) and compares with the torch adds + K1l per group
    and with the CPU specification."""
    a, b, c, w1, b1, w2, b2 = ins
    groups_cpu = [(w1, b1 if bias[0] else None, EPS1)] + ([(w2, b2 if bias[1] else None, EPS2)] if form != "add1" else [])
    dev = lambda t: None if t is None else t.cuda()          # noqa: E731
    ad, bd, cd = a.cuda(), b.cuda(), c.cuda()
    groups = [(dev(w), dev(bi), e) for w, bi, e in groups_cpu]
    ng = len(groups)
    with torch.no_grad():
        s_ref = (ad + bd) + cd if form != "dual" else cd.clone()
        refs = [pq.layernorm_quantize(s_ref, w, bi, e, return_h=True) for w, bi, e in groups]
        g2 = dict(weight2=groups[1][0], bias2=groups[1][1], eps2=EPS2) if ng == 2 else {}
        if form == "dual":
            res = pq.layernorm_quantize2(cd, groups[0][0], groups[0][1], groups[1][0], groups[1][1], EPS1, EPS2, return_h=True)
            res0 = pq.layernorm_quantize2(cd, groups[0][0], groups[0][1], groups[1][0], groups[1][1], EPS1, EPS2)
            qts, hs, summed = res[:2], res[2:], cd
            qts0, summed0 = res0, cd
        else:
            out = {"none": None, "a": ad, "b": bd, "c": cd}[out_mode]
            res = pq.add2_layernorm_quantize(ad, bd, cd, groups[0][0], groups[0][1], EPS1, out=out, return_h=True, **g2)
            res0 = pq.add2_layernorm_quantize(a.cuda(), b.cuda(), c.cuda(), groups[0][0], groups[0][1], EPS1, **g2)          # the instantiation without h
            assert len(res) == 2 * ng + 1 and len(res0) == ng + 1
            qts, summed, hs = res[:ng], res[ng], res[ng + 1:]
            qts0, summed0 = res0[:ng], res0[ng]
            if out is not None:
                assert summed is out
    torch.cuda.synchronize()
    assert summed.shape == a.shape
    if not bool(torch.isnan(s_ref.float()).any()):          # the issue's own statement of the contract: torch.equal with the library's own three-launch form
        assert torch.equal(summed, s_ref), what + ": torch.equal(sum, the two torch adds)"
        for i in range(ng):
            assert torch.equal(hs[i], refs[i][1]) and torch.equal(qts[i].scale, refs[i][0].scale), f"{what}: torch.equal with K1l, group {i + 1}"
    _nan_class_equal(summed, s_ref, what + ": sum vs the torch adds")
    _nan_class_equal(summed0, s_ref, what + ": sum (no h)")
    for i in range(ng):
        assert qts[i].int_data.shape == a.shape and hs[i].shape == a.shape
        _nan_class_equal(hs[i], refs[i][1], f"{what}: h{i + 1} vs K1l")
        _nan_class_equal(qts[i].scale, refs[i][0].scale, f"{what}: scales {i + 1} vs K1l")
        assert torch.equal(qts[i].int_data, refs[i][0].int_data), f"{what}: codes {i + 1} vs K1l"
        _nan_class_equal(qts0[i].scale, refs[i][0].scale, f"{what}: scales {i + 1} (no h)")
        assert torch.equal(qts0[i].int_data, refs[i][0].int_data), f"{what}: codes {i + 1} (no h)"
    for name, t_gpu, t_cpu in (("a", ad, a), ("b", bd, b), ("c", cd, c)):          # untouched operands are unwritten
        if form == "dual" or out_mode != name:
            assert _same_bytes(t_gpu, t_cpu), f"{what}: {name} was written"
    for (w, bi, _), (wc, bc, _) in zip(groups, groups_cpu):
        assert _same_bytes(w, wc) and (bi is None or _same_bytes(bi, bc)), what + ": a weight or a bias was written"
    if against_spec:
        if form == "dual":
            s_s, gs = A2.to_bits(c), A2.layernorm_quantize_groups(c, groups_cpu)
        else:
            s_s, gs = A2.add2_layernorm_quantize(a, b, c, groups_cpu)
        _nan_class_equal(summed, s_s, what + ": sum vs spec")
        for i, (q_s, sc_s, h_s) in enumerate(gs):
            _nan_class_equal(hs[i], h_s, f"{what}: h{i + 1} vs spec")
            _nan_class_equal(qts[i].scale, sc_s, f"{what}: scales {i + 1} vs spec")
            assert np.array_equal(qts[i].int_data.cpu().numpy(), q_s), f"{what}: codes {i + 1} vs spec"


def _sweep(pq, dtype, cols, rows_list, seed, tag=""):
    """every form at every row count; the bias pattern and the destination of the sum rotate so that each combination is met at every width over the row counts"""
    k = 0
    for rows in rows_list:
        ins = A2.inputs(rows, cols, dtype, seed + rows)
        for form in FORMS:
            bias = ((True, True), (False, True), (True, False), (False, False))[k % 4]
            _check(pq, ins, f"{tag}{dtype} {rows}x{cols} {form} bias={bias}", form=form, out_mode=OUTS[(k // 2) % 4], bias=bias)
            k += 1


# vectors per row -> the layout it reaches by default: <= 64 / 128 / 256 one wave per row (1 / 2 / 4 vectors per lane); beyond, 256 threads x 1 / 2 / 4 / 8 / 16
VEC_COUNTS = [1, 40, 64, 65, 128, 200, 256, 257, 512, 700, 1024, 1500, 2048, 3000, 4096]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("nvec", VEC_COUNTS)
def test_every_vector_layout_matches_the_three_launch_form_and_the_spec(pq, dtype, nvec):
    _sweep(pq, dtype, nvec * EPV[dtype], (1, 3, 5, 9), 100 + nvec)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("wave_max,nvecs", [("512", [300, 512]), ("0", [1, 64, 100, 256])])
def test_wave_max_switch_changes_no_bit(pq, pq_opt, dtype, wave_max, nvecs):
    """PQ_RMS_WAVE_MAX=512: one wave per row at 8 vectors per lane; PQ_RMS_WAVE_MAX=0: the 256-thread layout on short rows.  Time only, never bits."""
    pq_opt("PQ_RMS_WAVE_MAX", wave_max)
    for nvec in nvecs:
        _sweep(pq, dtype, nvec * EPV[dtype], (1, 3, 5, 9), 900 + nvec, tag=f"PQ_RMS_WAVE_MAX={wave_max} ")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("cols", [1, 7, 333, 1001])
def test_ragged_widths_take_the_generic_kernel(pq, dtype, cols):
    _sweep(pq, dtype, cols, (1, 3, 5, 9), 300 + cols)


def test_many_rows_at_2560_columns(pq):
    ins = A2.inputs(300, 2560, torch.bfloat16, 2560)
    for form, out_mode in (("add2", "c"), ("add1", "none"), ("dual", "none")):
        _check(pq, ins, f"bf16 300x2560 {form}", form=form, out_mode=out_mode)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
def test_unaligned_and_strided_views(pq, dtype):
    """column slices at an odd element offset (a base off by one element), odd leading dimensions, and the sum written to a strided view — directly and over an addend"""
    rows, cols = 6, 512
    a, b, c, w1, b1, w2, b2 = (t.cuda() for t in A2.inputs(rows, cols + 37, dtype, 44))
    big_o = torch.zeros(rows, cols + 5, dtype=dtype, device="cuda")
    for off_a, off_b, off_c, off_o, off_w in ((1, 3, 5, 1, 1), (0, 0, 0, 0, 0), (8, 8, 8, 0, 8), (0, 0, 1, 0, 0)):
        av, bv, cv, ov = a[:, off_a:off_a + cols], b[:, off_b:off_b + cols], c[:, off_c:off_c + cols], big_o[:, off_o:off_o + cols]
        wv1, bv1, wv2, bv2 = (t[off_w:off_w + cols] for t in (w1, b1, w2, b2))
        big_o.zero_()
        with torch.no_grad():
            s_ref = (av + bv) + cv
            refs = [pq.layernorm_quantize(s_ref, wv1, bv1, EPS1, return_h=True), pq.layernorm_quantize(s_ref, wv2, None, EPS2, return_h=True)]
            q1, q2, summed, h1, h2 = pq.add2_layernorm_quantize(av, bv, cv, wv1, bv1, EPS1, wv2, None, EPS2, out=ov, return_h=True)
            d1, d2 = pq.layernorm_quantize2(cv, wv1, bv1, wv2, None, EPS1, EPS2)
            e1, e2 = pq.layernorm_quantize(cv.contiguous(), wv1, bv1, EPS1), pq.layernorm_quantize(cv.contiguous(), wv2, None, EPS2)
        assert summed is ov
        _nan_class_equal(ov, s_ref, f"{dtype} strided sum {off_a, off_b, off_c, off_o}")
        for (qt, h), (qr, hr) in zip(((q1, h1), (q2, h2)), refs):
            _nan_class_equal(h, hr, "strided h")
            assert torch.equal(qt.scale, qr.scale) and torch.equal(qt.int_data, qr.int_data)
        assert torch.equal(d1.int_data, e1.int_data) and torch.equal(d1.scale, e1.scale) and torch.equal(d2.int_data, e2.int_data) and torch.equal(d2.scale, e2.scale)
        mask = torch.ones_like(big_o, dtype=torch.bool)
        mask[:, off_o:off_o + cols] = False
        assert not bool(big_o[mask].float().abs().sum() > 0), "columns outside the output view were written"
        s_s, gs = A2.add2_layernorm_quantize(av.cpu().contiguous(), bv.cpu().contiguous(), cv.cpu().contiguous(), [(wv1.cpu(), bv1.cpu(), EPS1), (wv2.cpu(), None, EPS2)])
        _nan_class_equal(ov, s_s, "strided sum vs spec")
        assert np.array_equal(q1.int_data.cpu().numpy(), gs[0][0]) and np.array_equal(q2.int_data.cpu().numpy(), gs[1][0])
    # in place over each strided addend in turn: the other two, and the columns around the view, are untouched
    for target in range(3):
        big = [a.clone(), b.clone(), c.clone()]
        views = [big[0][:, 3:3 + cols], big[1][:, 1:1 + cols], big[2][:, 8:8 + cols]]
        with torch.no_grad():
            s_ref = (views[0] + views[1]) + views[2]
            q_ref = pq.layernorm_quantize(s_ref, w1[:cols], b1[:cols], EPS1)
            qt, summed = pq.add2_layernorm_quantize(views[0], views[1], views[2], w1[:cols], b1[:cols], EPS1, out=views[target])
        _nan_class_equal(summed, s_ref, f"{dtype} in place over strided addend {target}")
        assert torch.equal(qt.int_data, q_ref.int_data) and torch.equal(qt.scale, q_ref.scale)
        for i, (t, orig, off) in enumerate(zip(big, (a, b, c), (3, 1, 8))):
            if i != target:
                assert torch.equal(t, orig)
            else:
                assert torch.equal(t[:, :off], orig[:, :off]) and torch.equal(t[:, off + cols:], orig[:, off + cols:])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("cols", [256, 4096, 37])
def test_special_values(pq, dtype, cols):
    """rows holding NaN, +-Inf, Inf - Inf, all zeros, -0, a row whose sum cancels to zero everywhere, and a row whose A2 intermediate t = a + b overflows the storage
    format although the grouping a + (b + c) would not (fp16: 60000 + 60000 - 60000)"""
    ins = A2.inputs(11, cols, dtype, 555 + cols)
    a, b, c = ins[:3]
    big = {torch.bfloat16: 3.0e38, torch.float16: 60000.0, torch.float32: 3.0e38}[dtype]
    a[0, 3] = float("nan")
    c[1, 5] = float("nan")
    a[2, 1], b[2, 2], c[2, 0] = float("inf"), float("-inf"), float("inf")
    a[3, 7], c[3, 7] = float("inf"), float("-inf")                 # Inf - Inf in the SECOND add: a NaN made by the kernel
    a[4], b[4], c[4] = 0.0, 0.0, 0.0
    a[5], b[5], c[5] = -0.0, -0.0, -0.0
    a[6], b[6], c[6] = 0.0, -0.0, 0.0
    a[7, :], b[7, :], c[7, :] = big, big, -big                       # t overflows to +Inf in the storage dtype: s = Inf, where a + (b + c) = big
    a[8, 0], b[8, 0] = big, -big                                     # exact cancellation next to ordinary values
    for i in range(3):
        ins[i][9] = (ins[i][9].float() * 1e-30).to(dtype)            # tiny rows (fp16: zeros and subnormals)
    c[10] = -A2.add_a2(a[10:11], b[10:11], torch.zeros_like(a[10:11]))[0]      # the whole row cancels: mean 0, variance 0, h = bias
    k = 0
    for form in FORMS:
        for mode in (OUTS if form != "dual" else ("none",)):
            bias = ((True, True), (False, True), (True, False), (False, False))[k % 4]
            _check(pq, tuple(t.clone() for t in ins), f"{dtype} special values, {cols} columns, {form}, out={mode}, bias={bias}", form=form, out_mode=mode, bias=bias)
            k += 1
    qt, s = pq.add2_layernorm_quantize(a.cuda(), b.cuda(), c.cuda(), ins[3].cuda(), None, EPS1)
    assert not bool(s[10].float().abs().sum() > 0) and not bool(qt.int_data[10].any()) and not bool(qt.int_data[4].any())      # all-zero sums: zero codes
    assert bool(torch.isinf(s[7]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("rows,cols", [(5, 4096), (3, 520), (7, 37), (4, 32768 // 2), (1, 8192)])
@pytest.mark.parametrize("form", FORMS)
def test_guarded_margins_stay_untouched(pq, dtype, rows, cols, form):
    """every output buffer (sum, both code arrays, both scale arrays, both h) lies inside a larger allocation filled with a pattern: the kernel writes its rows and
    nothing around them.  Raw C-ABI call on interior views, 16-byte aligned for the vector layouts."""
    from protoquant_amd import _lib as L
    a, b, c, w1, b1, w2, b2 = (t.cuda() for t in A2.inputs(rows, cols, dtype, 70 + rows + cols))
    m, n = 4096, rows * cols          # margin in elements: a multiple of 16 bytes for every dtype
    full = lambda count, fill, dt: torch.full((count + 2 * m,), fill, dtype=dt, device="cuda")          # noqa: E731
    sum_all, h_all = full(n, 7.0, dtype), [full(n, 7.0, dtype), full(n, 7.0, dtype)]
    q_all, sc_all = [full(n, 77, torch.int8), full(n, 77, torch.int8)], [full(rows, 7.0, torch.float32), full(rows, 7.0, torch.float32)]
    s_v, h_v, q_v, sc_v = sum_all[m:m + n], [t[m:m + n] for t in h_all], [t[m:m + n] for t in q_all], [t[m:m + rows] for t in sc_all]
    add, two = form != "dual", form != "add1"
    p = lambda t, on=True: t.data_ptr() if on else None          # noqa: E731
    with torch.cuda.device(a.device):
        L.check(L.lib().pq_parallel_layernorm_quant_rowwise(
            p(a, add), cols, p(b, add), cols, c.data_ptr(), cols, p(s_v, add), cols, w1.data_ptr(), b1.data_ptr(), EPS1, p(w2, two), p(b2, two), EPS2,
            L.dtype_code(dtype), rows, cols, q_v[0].data_ptr(), cols, sc_v[0].data_ptr(), h_v[0].data_ptr(), cols, p(q_v[1], two), cols, p(sc_v[1], two), p(h_v[1], two), cols,
            L.stream_ptr(a)), "raw K1pl / K1l2")
    torch.cuda.synchronize()
    with torch.no_grad():
        s_ref = (a + b) + c if add else c
        refs = [pq.layernorm_quantize(s_ref, w1, b1, EPS1, return_h=True)] + ([pq.layernorm_quantize(s_ref, w2, b2, EPS2, return_h=True)] if two else [])
    if add:
        _nan_class_equal(s_v.view(rows, cols), s_ref, "sum")
    for i, (q_ref, h_ref) in enumerate(refs):
        _nan_class_equal(h_v[i].view(rows, cols), h_ref, f"h{i + 1}")
        assert torch.equal(q_v[i].view(rows, cols), q_ref.int_data) and torch.equal(sc_v[i], q_ref.scale)
    bufs = [("sum", sum_all, n if add else 0, 7.0)]
    for i in (0, 1):
        on = i == 0 or two
        bufs += [(f"h{i + 1}", h_all[i], n if on else 0, 7.0), (f"codes {i + 1}", q_all[i], n if on else 0, 77), (f"scales {i + 1}", sc_all[i], rows if on else 0, 7.0)]
    for name, buf, count, fill in bufs:          # (count 0: an output this form does not have — the whole buffer keeps its pattern)
        assert bool((buf[:m] == fill).all()) and bool((buf[m + count:] == fill).all()), f"the margin around {name} was written"


def test_batch_shapes_empty_problems_and_refusals(pq):
    from protoquant_amd import _lib
    a, b, c, w1, b1, w2, b2 = (t.cuda() for t in A2.inputs(14, 512, torch.bfloat16, 3))
    a3, b3, c3 = a.view(2, 7, 512), b.view(2, 7, 512), c.view(2, 7, 512)
    q1, q2, s = pq.add2_layernorm_quantize(a3, b3, c3, w1, b1, 1e-5, w2, None)          # eps2 defaults to eps
    r1, r2 = pq.layernorm_quantize((a3 + b3) + c3, w1, b1, 1e-5), pq.layernorm_quantize((a3 + b3) + c3, w2, None, 1e-5)
    assert s.shape == a3.shape and q1.int_data.shape == a3.shape and q1.scale.shape == (14,) and torch.equal(s, (a3 + b3) + c3)
    assert torch.equal(q1.int_data, r1.int_data) and torch.equal(q2.int_data, r2.int_data) and torch.equal(q1.scale, r1.scale) and torch.equal(q2.scale, r2.scale)
    qv, sv = pq.add2_layernorm_quantize(a[0], b[0], c[0], w1, b1)
    assert sv.shape == (512,) and torch.equal(qv.int_data, r1.int_data[0, 0]) and torch.equal(sv, s[0, 0])
    e = torch.empty(0, 512, dtype=torch.bfloat16, device="cuda")
    qe1, qe2, se, he1, he2 = pq.add2_layernorm_quantize(e, e, e, w1, b1, weight2=w2, return_h=True)
    assert se.shape == (0, 512) and qe1.int_data.shape == (0, 512) and he2.shape == (0, 512)
    e0, w0 = torch.empty(3, 0, dtype=torch.bfloat16, device="cuda"), torch.empty(0, dtype=torch.bfloat16, device="cuda")
    q0, s0 = pq.add2_layernorm_quantize(e0, e0, e0, w0, None)
    d0, d1 = pq.layernorm_quantize2(e0, w0, None, w0, None)
    assert s0.shape == (3, 0) and torch.equal(q0.scale, pq.layernorm_quantize(e0, w0, None).scale) and torch.equal(d1.scale, q0.scale) and d0.int_data.shape == (3, 0)
    buf = torch.zeros(15, 512, dtype=torch.bfloat16, device="cuda")
    buf[:14] = c
    with pytest.raises(_lib.PQError, match="sum_out overlaps c"):
        pq.add2_layernorm_quantize(a, b, buf[:14], w1, None, out=buf[1:15])              # shifted by one row: overlaps c without being c
    flat = torch.zeros(14 * 512, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_lib.PQError, match="sum_out overlaps bias2"):
        pq.add2_layernorm_quantize(a, b, c, w1, None, weight2=w2, bias2=flat[13 * 512:], out=flat.view(14, 512))
    with pytest.raises(ValueError):
        pq.add2_layernorm_quantize(a, b[:, :256], c, w1, None)
    with pytest.raises(ValueError):
        pq.add2_layernorm_quantize(a, b, c, w1, None, bias2=b2)
