"""GPU: pq_glu_quant_rowwise (glu_quantize) against the CPU restatement of QSPEC G1-G6 (tests/glu_spec.py), bit for bit — codes, scales and h_out, with guarded margins
around every output: both kinds x bf16 / fp16 / f32, every row layout (one wave per row, 256 threads, 512 threads, the widest block, the generic kernel), g / u as the
halves of one tensor and as separate tensors, rows far beyond +-limit, NaN / Inf / all-zero rows, every 16-bit pattern, and the division-free sequence against the
specified one over its whole domain."""
import numpy as np
import pytest
import torch

from oracle import qspec_numpy as Q
from tests import glu_spec as G
from tests.gpu_util import TD, bits, same, same_f, to_gpu

pytestmark = pytest.mark.gpu

KINDS = [("clamped_silu", G.CLAMPED_SILU, 7.0, None), ("alpha_sigmoid", G.ALPHA_SIGMOID, 7.0, 1.702)]
CANARY_Q, CANARY_S = 0x5A, 1234.5


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    return protoquant_amd


def _rows(rng, rows, cols, code, spread=4.0):
    x = (rng.standard_normal((rows, cols)) * spread).astype(np.float32)
    return x if code == 2 else Q.from_f32(x, code)


def _call_guarded(g_t, u_t, code, kname, limit, alpha, want_h=True, margin=64):
    """the C entry point writing into the middle of canary-filled buffers: returns (q, scale, h) and asserts that nothing outside [rows, cols] was written"""
    from protoquant_amd import _lib
    rows, cols = g_t.shape
    ldq = cols + 2 * margin
    qb = torch.full((rows + 2, ldq), CANARY_Q, dtype=torch.int8, device="cuda")
    sb = torch.full((rows + 2 * margin,), CANARY_S, dtype=torch.float32, device="cuda")
    hb = torch.full((rows + 2, ldq), 3.0, dtype=TD[code], device="cuda")
    esz = hb.element_size()
    st = _lib.lib().pq_glu_quant_rowwise(g_t.data_ptr(), _lib.ld(g_t), u_t.data_ptr(), _lib.ld(u_t), code, rows, cols, _lib.GLU_KINDS[kname], limit, alpha or 0.0,
                                         qb.data_ptr() + ldq + margin, ldq, sb.data_ptr() + 4 * margin, (hb.data_ptr() + (ldq + margin) * esz) if want_h else None, ldq,
                                         torch.cuda.current_stream().cuda_stream)
    _lib.check(st, "glu")
    torch.cuda.synchronize()
    q, s, h = qb[1:rows + 1, margin:margin + cols], sb[margin:margin + rows], hb[1:rows + 1, margin:margin + cols]
    qm, sm, hm = qb.clone(), sb.clone(), hb.clone()
    qm[1:rows + 1, margin:margin + cols] = CANARY_Q; sm[margin:margin + rows] = CANARY_S; hm[1:rows + 1, margin:margin + cols] = 3.0
    assert bool((qm == CANARY_Q).all()) and bool((sm == CANARY_S).all()) and bool((hm == 3.0).all()), "a write outside the output"
    if not want_h:
        assert bool((hb == 3.0).all())
    return q, s, h


# widths in elements: one wave per row (<= 256 vectors), 256 threads x 1 .. 16 vectors, 512 threads x 3 vectors (1025 .. 1536 vectors), the real widths 2880 (GPT-OSS) and
# 2048 k, the widest rows a block holds (4096 vectors); then every boundary of the family's ladder (rowmap_dispatch) in vectors: 65, 128, 257, 1024, 1025, 1536, 1537, 2048
WIDTHS_16 = [8, 64, 512, 1000, 2048, 2880, 4096, 6144, 11008, 14336, 32768, 520, 1024, 2056, 8192, 8200, 12288, 12296, 16384]


@pytest.mark.parametrize("kname,kind,limit,alpha", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("code", [0, 1, 2], ids=["bf16", "fp16", "f32"])
def test_every_row_layout_against_the_spec(pq, kname, kind, limit, alpha, code):
    rng = np.random.default_rng(100 + 10 * kind + code)
    for cols in WIDTHS_16:
        if code == 2:
            cols //= 2                                         # the same vector counts
        rows = 7 if cols <= 4096 else 3
        gu = _rows(rng, rows, 2 * cols, code)
        gu_t = to_gpu(gu, code)
        want_q, want_s, want_h = G.glu_quantize(gu[:, :cols], gu[:, cols:], code, kind, limit, alpha or 0.0)
        q, s, h = _call_guarded(gu_t[:, :cols], gu_t[:, cols:], code, kname, limit, alpha)             # the halves of one tensor: ld = 2 cols
        same(q, want_q, f"{kname} {cols}: q"); same(s, want_s, f"{kname} {cols}: scale"); same_f(h, want_h, code, f"{kname} {cols}: h")
        qt = pq.glu_quantize(gu_t[:, :cols].contiguous(), gu_t[:, cols:].contiguous(), kname, limit, alpha)       # separate tensors, no h_out
        same(qt.int_data, want_q, f"{kname} {cols}: q (separate, no h)"); same(qt.scale, want_s, f"{kname} {cols}: scale (separate, no h)")


@pytest.mark.parametrize("kname,kind,limit,alpha", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("code", [0, 1, 2], ids=["bf16", "fp16", "f32"])
def test_wide_rows_with_256_threads(pq, pq_opt, kname, kind, limit, alpha, code):
    """rows of 1025 .. 1536 vectors take 512 threads x 3 vectors; PQ_SILU_TPR=256 sends them to 256 threads x 8, as for K1s, K1u and K1gg.  Time only, never bits."""
    cols = 1300 * (4 if code == 2 else 8)
    gu = _rows(np.random.default_rng(400 + 10 * kind + code), 3, 2 * cols, code)
    gu_t = to_gpu(gu, code)
    g_t, u_t = gu_t[:, :cols], gu_t[:, cols:]
    want_q, want_s, want_h = G.glu_quantize(gu[:, :cols], gu[:, cols:], code, kind, limit, alpha or 0.0)
    d, hd = pq.glu_quantize(g_t, u_t, kname, limit, alpha, return_h=True)
    pq_opt("PQ_SILU_TPR", 256)
    qt, h = pq.glu_quantize(g_t, u_t, kname, limit, alpha, return_h=True)
    q2 = pq.glu_quantize(g_t, u_t, kname, limit, alpha)
    for t, tag in ((qt, ""), (q2, " (no h)")):
        same(t.int_data, want_q, f"{kname} PQ_SILU_TPR=256: q{tag}"); same(t.scale, want_s, f"{kname} PQ_SILU_TPR=256: scale{tag}")
        assert torch.equal(t.int_data, d.int_data) and torch.equal(t.scale.view(torch.int32), d.scale.view(torch.int32)), "the switch changed a bit"
    same_f(h, want_h, code, f"{kname} PQ_SILU_TPR=256: h")
    assert torch.equal(h.view(torch.uint8), hd.view(torch.uint8)), "the switch changed a bit of h"


@pytest.mark.parametrize("kname,kind,limit,alpha", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("code", [0, 1, 2], ids=["bf16", "fp16", "f32"])
def test_generic_kernel_odd_widths_and_unaligned_leading_dimensions(pq, kname, kind, limit, alpha, code):
    rng = np.random.default_rng(200 + 10 * kind + code)
    for cols, pad in ((1, 0), (7, 3), (129, 1), (1001, 5), (2881, 2), (640, 1), (50257, 2)):
        rows = 5
        ga, ua = _rows(rng, rows, cols + pad + 1, code), _rows(rng, rows, cols + pad + 1, code)
        g_t, u_t = to_gpu(ga, code)[:, 1:cols + 1], to_gpu(ua, code)[:, 1:cols + 1]                    # odd leading dimension, base off the 16-byte grid
        want_q, want_s, want_h = G.glu_quantize(ga[:, 1:cols + 1], ua[:, 1:cols + 1], code, kind, limit, alpha or 0.0)
        q, s, h = _call_guarded(g_t, u_t, code, kname, limit, alpha, margin=3)
        same(q, want_q, f"{kname} generic {cols}: q"); same(s, want_s, f"{kname} generic {cols}: scale"); same_f(h, want_h, code, f"{kname} generic {cols}: h")
        qt, h2 = pq.glu_quantize(g_t, u_t, kname, limit, alpha, return_h=True)
        same(qt.int_data, want_q, f"{kname} generic {cols}: q (python)"); same_f(h2, want_h, code, f"{kname} generic {cols}: h (python)")


@pytest.mark.parametrize("kname,kind,limit,alpha", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("code", [0, 1, 2], ids=["bf16", "fp16", "f32"])
def test_special_rows(pq, kname, kind, limit, alpha, code):
    """rows far beyond +-limit (the `/` path: |g| > 86), NaN and Inf rows, all-zero rows, one NaN in an otherwise ordinary row, -0 — in the vector and the generic kernel"""
    rng = np.random.default_rng(300 + 10 * kind + code)
    for cols in (512, 2880, 515):
        g = (rng.standard_normal((10, cols)) * 3).astype(np.float32)
        u = (rng.standard_normal((10, cols)) * 3).astype(np.float32)
        g[0] *= 1000; u[0] *= 1000                                    # far beyond the limit, both signs
        g[1, 5] = np.nan
        u[2, 9] = np.nan
        g[3, 3] = np.inf; g[3, 4] = -np.inf
        u[4, 7] = np.inf; u[4, 8] = -np.inf
        g[5] = 0.0; u[5] = 0.0
        g[6] = -0.0
        g[7] = 0.0                                                    # h = 0 everywhere: scale of an all-zero row
        g[8, :] = 100.0; u[8, :] = -100.0                             # every element clamped: h = f(L) * (-L [+ 1])
        g[9, ::2] = 86.5; g[9, 1::2] = -87.0
        if code != 2:
            g, u = Q.from_f32(g, code), Q.from_f32(u, code)
        want_q, want_s, want_h = G.glu_quantize(g, u, code, kind, limit, alpha or 0.0)
        qt, h = pq.glu_quantize(to_gpu(g, code), to_gpu(u, code), kname, limit, alpha, return_h=True)
        same_f(h, want_h, code, f"{kname} special {cols}: h")
        same(qt.int_data, want_q, f"{kname} special {cols}: q")
        ws, gs = want_s.view(np.uint32), bits(qt.scale)
        assert np.array_equal(np.isnan(want_s), np.isnan(qt.scale.cpu().numpy())) and np.array_equal(ws[~np.isnan(want_s)], gs[~np.isnan(want_s)]), f"{kname} special {cols}: scale"


@pytest.mark.parametrize("kname,kind,limit,alpha", KINDS + [("alpha_sigmoid", G.ALPHA_SIGMOID, 7.03, 1.702), ("clamped_silu", G.CLAMPED_SILU, 7.03, None),
                                                            ("alpha_sigmoid", G.ALPHA_SIGMOID, 3.0, -0.5)], ids=lambda v: str(v))
@pytest.mark.parametrize("code", [0, 1], ids=["bf16", "fp16"])
def test_every_16_bit_pattern_through_the_kernel(pq, kname, kind, limit, alpha, code):
    """all 65 536 patterns of the gate (rows of 4096: patterns of one exponent range share a wave, so both division paths run) x a few up values, and all patterns of up;
    a limit that is no value of the dtype (7.03 -> 7.03125) included"""
    pats = np.arange(65536, dtype=np.uint16).reshape(16, 4096)
    for uval in (1.0, -0.5, 9.0):
        other = np.broadcast_to(Q.from_f32(np.array([uval], np.float32), code), pats.shape)
        for what, g, u in (("gate", pats, other), ("up", other, pats)):
            want_q, want_s, want_h = G.glu_quantize(g, u, code, kind, limit, alpha or 0.0)
            qt, h = pq.glu_quantize(to_gpu(np.ascontiguousarray(g), code), to_gpu(np.ascontiguousarray(u), code), kname, limit, alpha, return_h=True)
            same_f(h, want_h, code, f"{kname} all {what} patterns, other = {uval}: h")
            same(qt.int_data, want_q, f"{kname} all {what} patterns, other = {uval}: q")


@pytest.mark.parametrize("kname,kind,limit,alpha", KINDS + [("alpha_sigmoid", G.ALPHA_SIGMOID, 7.03, 1.0), ("alpha_sigmoid", G.ALPHA_SIGMOID, 20.0, -3.5)], ids=lambda v: str(v))
@pytest.mark.parametrize("code", [0, 1], ids=["bf16", "fp16"])
def test_division_free_sequence_equals_the_specified_one_on_its_whole_domain(pq, kname, kind, limit, alpha, code):
    from protoquant_amd import _lib
    out = torch.zeros(2, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().pq_selftest_glu_short(code, _lib.GLU_KINDS[kname], limit, alpha or 0.0, out.data_ptr(), torch.cuda.current_stream().cuda_stream), "selftest")
    n, bad = out.cpu().tolist()
    print(f"\n  {kname} {'bf16' if code == 0 else 'fp16'} limit {limit} alpha {alpha}: {n} patterns on the division-free path, {bad} differ")
    assert n > 20000 and bad == 0


def test_f32_division_free_path_equals_true_division(pq):
    """binary32 rows cannot be enumerated: the vector kernel (division-free when the wave's gates allow it) against the generic kernel (`/` always) on the same values"""
    rng = np.random.default_rng(9)
    rows, cols = 256, 2048
    for kname, kind, limit, alpha in KINDS:
        g = (rng.standard_normal((rows, cols)) * 6).astype(np.float32)
        u = (rng.standard_normal((rows, cols)) * 6).astype(np.float32)
        g[:, :64] = np.exp(rng.uniform(-80, 4, (rows, 64))).astype(np.float32) * rng.choice([-1, 1], (rows, 64))     # tiny and moderate magnitudes
        gt, ut = torch.from_numpy(g).cuda(), torch.from_numpy(u).cuda()
        pad_g, pad_u = torch.zeros(rows, cols + 3, device="cuda"), torch.zeros(rows, cols + 3, device="cuda")
        pad_g[:, 1:cols + 1] = gt; pad_u[:, 1:cols + 1] = ut
        qa, ha = pq.glu_quantize(gt, ut, kname, limit, alpha, return_h=True)
        qb, hb = pq.glu_quantize(pad_g[:, 1:cols + 1], pad_u[:, 1:cols + 1], kname, limit, alpha, return_h=True)
        assert torch.equal(ha.view(torch.int32), hb.view(torch.int32)) and torch.equal(qa.int_data, qb.int_data) and torch.equal(qa.scale, qb.scale)
        want_q, want_s, want_h = G.glu_quantize(g[:32], u[:32], 2, kind, limit, alpha or 0.0)
        same(qa.int_data[:32], want_q, "f32 q"); same(ha[:32], want_h, "f32 h")


def test_python_surface_shapes_and_errors(pq):
    g = torch.randn(2, 5, 64, device="cuda").to(torch.bfloat16)
    u = torch.randn(2, 5, 64, device="cuda").to(torch.bfloat16)
    qt, h = pq.glu_quantize(g, u, "alpha_sigmoid", 7.0, 1.702, return_h=True)
    assert qt.int_data.shape == g.shape and qt.scale.shape == (10,) and h.shape == g.shape and h.dtype == g.dtype
    want_q, want_s, _ = G.glu_quantize(bits(g).reshape(10, 64), bits(u).reshape(10, 64), 0, G.ALPHA_SIGMOID, 7.0, 1.702)
    same(qt.int_data.reshape(10, 64), want_q, "3-D q"); same(qt.scale, want_s, "3-D scale")
    e = pq.glu_quantize(g[:0], u[:0], "clamped_silu", 7.0)
    assert e.int_data.numel() == 0
    for bad in (dict(kind="silu"), dict(limit=0.0), dict(limit=float("inf")), dict(limit=None), dict(kind="alpha_sigmoid", alpha=None), dict(alpha=float("nan"))):
        a = dict(kind="clamped_silu", limit=7.0, alpha=1.0); a.update(bad)
        with pytest.raises(ValueError):
            pq.glu_quantize(g, u, a["kind"], a["limit"], a["alpha"])
    with pytest.raises(ValueError):
        pq.glu_quantize(g, u[:, :, :32], "clamped_silu", 7.0)
