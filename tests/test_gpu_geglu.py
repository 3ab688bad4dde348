"""-m gpu: K1gg (pq_gelu_mul_quant_rowwise / gelu_mul_quantize) against the CPU specification (tests/gemma_spec.py: GG1-GG3), bit for bit — codes, scales and h;
NaNs as a class.  Every 16-bit pattern of g against 12 values of u: as two [12, 32768] tensors per dtype through the 256-thread x 16-vector layout and through the
generic kernel — both of which DIVIDE on every pattern (each wave of the wide layout also holds |g| > 9.5) — and as rows of 512 patterns sorted by magnitude, one
wave per row, where every pattern of 0 < |g| <= 9.5 runs the division-free quotient (the test counts those rows); random rows at widths that reach every row layout (one
wave per row at 1 / 2 / 4 vectors, 512 threads x 3 and the same rows with PQ_SILU_TPR=256, 256 threads x 1 .. 16, generic) for bf16, fp16 and f32; g and u as the
column halves of one tensor; and h equal to the product of K1u's stored tanh GELU with u, which holds the restated U2 sequence to act_kernels.hip's."""
import functools

import numpy as np
import pytest
import torch

from tests import gemma_spec as G
from tests.gemma_spec import nan_class_equal as _nan_class_equal

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
IDS = ["bf16", "fp16", "f32"]
U_VALUES = (1.0, -1.0, 0.5, -2.0, 3.140625, 0.333251953125, 1e-3, 300.0, -0.0751953125, 0.0, 1.0e4, float("inf"))
# one vector (f32: two); one wave x 2 vectors (f32: x 4); ragged in vectors (87 / 174); 256 threads x 2 (f32: x 4); 512 threads x 3 (16-bit 9216 = f32 4608 = 1152 vectors);
# 256 threads x 8 (f32: x 16, the vector limit); a ragged width (generic)
WIDTHS = (8, 640, 696, 2816, 9216, 16384, 333)
# then every boundary of the family's layout ladder (rowmap_dispatch) in 16-byte vectors, as widths of 16-bit rows (8 elements per vector) and of f32 rows (4)
WIDTHS += tuple(c for c in sorted({v * e for v in [1, 64, 65, 128, 256, 257, 512, 1024, 1025, 1536, 1537, 2048, 4096] for e in (8, 4)}) if c not in WIDTHS)


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    from protoquant_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return protoquant_amd


def _check(pq, gd, ud, spec, what):
    """gd, ud: GPU tensors (views allowed); spec: (q, scale, h) of the CPU specification"""
    q_s, sc_s, h_s = spec
    qt, h = pq.gelu_mul_quantize(gd, ud, return_h=True)
    qt2 = pq.gelu_mul_quantize(gd, ud)                                  # the instantiation without h_out
    a = pq.act_quantize(gd, "gelu_tanh", return_h=True)[1]             # K1u's stored tanh GELU
    torch.cuda.synchronize()
    _nan_class_equal(h, h_s, what + ": h")
    _nan_class_equal(h, (a.float() * ud.float()).to(gd.dtype), what + ": h vs act_quantize's gelu times u")
    for t, tag in ((qt, ""), (qt2, " (no h)")):
        _nan_class_equal(t.scale, sc_s, what + ": scales" + tag)
        assert np.array_equal(t.int_data.cpu().numpy(), q_s), what + ": codes" + tag


@functools.lru_cache(maxsize=None)
def _patterns(dtype, half):
    """[12, 32768]: row i holds the 16-bit patterns half * 32768 .. half * 32768 + 32767 of g against the constant u = U_VALUES[i]; with the specification"""
    pats = (torch.arange(32768, dtype=torch.int32) + half * 32768).to(torch.int16).view(dtype)
    g = pats.repeat(12, 1).contiguous()
    u = torch.tensor(U_VALUES).to(dtype).reshape(12, 1).repeat(1, 32768).contiguous()
    return g, u, G.gelu_mul_quantize_t(g, u)


@pytest.mark.parametrize("dtype", DTYPES[:2], ids=IDS[:2])
@pytest.mark.parametrize("half", [0, 1], ids=["positive", "negative"])
def test_every_pattern_of_g_against_twelve_values_of_u(pq, dtype, half):
    g, u, spec = _patterns(dtype, half)
    _check(pq, g.cuda(), u.cuda(), spec, f"{dtype} patterns {half}: 256 threads x 16 vectors")
    # the same through the generic kernel (an unaligned base): every pattern through `/`
    big_g, big_u = torch.zeros(12, 32768 + 8, dtype=dtype), torch.zeros(12, 32768 + 8, dtype=dtype)
    big_g[:, 1:32769], big_u[:, 3:32771] = g, u
    _check(pq, big_g.cuda()[:, 1:32769], big_u.cuda()[:, 3:32771], spec, f"{dtype} patterns {half}: generic")


@functools.lru_cache(maxsize=None)
def _short_rows(dtype, by_magnitude):
    """[12 * 128, 512]: all 65 536 patterns of g as rows of 512 (one wave per row, one vector per lane), once per value of u; by_magnitude: the patterns sorted by
    |g| (NaNs last), so that whole rows — whole waves — lie inside 0 < |g| <= 9.5 and run the division-free quotient; with the specification"""
    pats = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
    if by_magnitude:
        pats = pats[torch.argsort(pats.float().abs().nan_to_num(nan=float("inf")), stable=True)]
    g = pats.reshape(128, 512).repeat(12, 1).contiguous()
    u = torch.tensor(U_VALUES).to(dtype).reshape(12, 1, 1).expand(12, 128, 512).reshape(12 * 128, 512).contiguous()
    return g, u, G.gelu_mul_quantize_t(g, u)


@pytest.mark.parametrize("dtype", DTYPES[:2], ids=IDS[:2])
@pytest.mark.parametrize("by_magnitude", [False, True], ids=["in-order", "by-magnitude"])
def test_every_pattern_of_g_in_short_rows_reaches_the_division_free_quotient(pq, dtype, by_magnitude):
    """The [12, 32768] tensors above never take the division-free quotient: in the 256-thread x 16-vector layout every wave also holds patterns of the top of the
    range (|g| > 9.5) and divides.  Here a wave owns a row of 512 patterns; the test first counts the rows that hold nothing but 0 < |g| <= 9.5 — the condition of
    geglu_fast_ok — and, sorted by magnitude, those rows must cover EVERY pattern of that domain: each of them goes through the FASTDIV instantiation against each
    of the 12 values of u, and the rest through `/`."""
    g, u, spec = _short_rows(dtype, by_magnitude)
    mag = g[:128].float().abs()
    fast_rows = ((mag > 0) & (mag <= 9.5)).all(dim=1)                 # (a NaN fails both comparisons)
    in_domain = int(((mag > 0) & (mag <= 9.5)).sum())
    assert in_domain == {torch.bfloat16: 2 * (0x4118), torch.float16: 2 * (0x48C0)}[dtype]          # every non-zero pattern up to 9.5, both signs
    covered = int(fast_rows.sum()) * 512
    if by_magnitude:
        assert in_domain - covered < 2 * 512, (in_domain, covered)     # all of the domain but the two rows at its ends, which hold a zero or a |g| > 9.5
        edge = g[:128][~fast_rows].float().abs()
        assert int(((edge > 0) & (edge <= 9.5)).sum()) == in_domain - covered          # (those run in the next test)
    else:
        assert covered >= 32 * 512                                      # in pattern order: 512 consecutive patterns share sign and binade range
    _check(pq, g.cuda(), u.cuda(), spec, f"{dtype} all patterns as rows of 512, by_magnitude={by_magnitude}")


def test_the_patterns_left_at_the_ends_of_the_domain_in_rows_of_their_own(pq):
    """sorted by magnitude, the rows at the two ends of 0 < |g| <= 9.5 also hold a zero or a larger value and divide: the patterns of the domain in those two rows,
    padded to whole rows with a value of the domain, against every u — so that NO pattern of the domain is left without a run through the division-free quotient"""
    for dtype in DTYPES[:2]:
        pats = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
        pats = pats[torch.argsort(pats.float().abs().nan_to_num(nan=float("inf")), stable=True)].reshape(128, 512)
        mag = pats.float().abs()
        dom = (mag > 0) & (mag <= 9.5)
        left = pats[~dom.all(dim=1)][dom[~dom.all(dim=1)]]              # the patterns of the domain outside the all-fast rows
        assert 0 < left.numel() < 1024
        g1 = torch.full((1024,), 1.5, dtype=dtype)
        g1[:left.numel()] = left
        g = g1.reshape(2, 512).repeat(12, 1).contiguous()
        assert bool(((g.float().abs() > 0) & (g.float().abs() <= 9.5)).all())
        u = torch.tensor(U_VALUES).to(dtype).reshape(12, 1, 1).expand(12, 2, 512).reshape(24, 512).contiguous()
        _check(pq, g.cuda(), u.cuda(), G.gelu_mul_quantize_t(g, u), f"{dtype} the ends of the fast domain")


@functools.lru_cache(maxsize=None)
def _random(dtype, cols):
    """7 rows: gates of a few units (the fast quotient), row 1 with a zero and row 2 with a large gate (`/`), row 3 with a NaN, -Inf and +Inf; with the specification"""
    gen = torch.Generator().manual_seed(500 + cols)
    g = (torch.randn(7, cols, generator=gen) * 2.5).to(dtype)
    u = (torch.randn(7, cols, generator=gen) * 1.5).to(dtype)
    g[1, cols // 2] = 0.0
    g[2, cols // 3] = 40.0
    g[3, 0], g[3, cols // 2], g[3, cols - 1] = float("nan"), float("-inf"), float("inf")
    g[4] = (g[4].float() * 1e-3).to(dtype)
    return g, u, G.gelu_mul_quantize_t(g, u)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cols", WIDTHS)
def test_random_rows_at_every_layout(pq, dtype, cols):
    if dtype == torch.float32 and cols == 9216:
        cols = 4608                                                    # 1152 vectors of f32: the 512-thread layout
    g, u, spec = _random(dtype, cols)
    _check(pq, g.cuda(), u.cuda(), spec, f"{dtype} 7x{cols}")
    one = tuple(s[:1] for s in spec)
    _check(pq, g[:1].cuda(), u[:1].cuda(), one, f"{dtype} 1x{cols}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cols", [640, 9216, 333])
def test_column_halves_of_one_tensor(pq, dtype, cols):
    """g and u as the two column halves of one fused gate+up output (leading dimension 2 * cols) — what GatedMLP hands over"""
    if dtype == torch.float32 and cols == 9216:
        cols = 4608
    g, u, spec = _random(dtype, cols)
    gu = torch.cat((g, u), dim=-1).cuda()
    gv, uv = torch.split(gu, [cols, cols], dim=-1)
    assert gv.stride(0) == 2 * cols and uv.data_ptr() != gv.data_ptr()
    _check(pq, gv, uv, spec, f"{dtype} 7x{cols} column halves")
    assert torch.equal(gu.cpu().view(torch.uint8), torch.cat((g, u), dim=-1).view(torch.uint8)), "the inputs were written"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_silu_tpr_switch_changes_no_bit(pq, pq_opt, dtype):
    """rows of 1025 .. 1536 vectors take 512 threads x 3 vectors; PQ_SILU_TPR=256 sends them to 256 threads x 8.  Time only, never bits."""
    cols = 9216 if dtype != torch.float32 else 4608
    g, u, spec = _random(dtype, cols)
    pq_opt("PQ_SILU_TPR", 256)
    _check(pq, g.cuda(), u.cuda(), spec, f"{dtype} 7x{cols} PQ_SILU_TPR=256")


def test_guarded_margins_batch_shapes_and_refusals(pq):
    from protoquant_amd import _lib as L
    dtype, rows, cols = torch.bfloat16, 7, 696
    g, u, spec = _random(dtype, cols)
    gd, ud = g.cuda(), u.cuda()
    m = 4096
    h_all = torch.full((rows * cols + 2 * m,), 7.0, dtype=dtype, device="cuda")
    q_all = torch.full((rows * cols + 2 * m,), 77, dtype=torch.int8, device="cuda")
    sc_all = torch.full((rows + 2 * m,), 7.0, dtype=torch.float32, device="cuda")
    h_v, q_v, sc_v = h_all[m:m + rows * cols], q_all[m:m + rows * cols], sc_all[m:m + rows]
    with torch.cuda.device(gd.device):
        L.check(L.lib().pq_gelu_mul_quant_rowwise(gd.data_ptr(), cols, ud.data_ptr(), cols, 0, rows, cols, 1, q_v.data_ptr(), cols, sc_v.data_ptr(), h_v.data_ptr(), cols,
                                                  L.stream_ptr(gd)), "raw K1gg")
    torch.cuda.synchronize()
    _nan_class_equal(h_v.view(rows, cols), spec[2], "h")
    _nan_class_equal(sc_v, spec[1], "scales")
    assert np.array_equal(q_v.view(rows, cols).cpu().numpy(), spec[0])
    for name, buf, n, fill in (("h", h_all, rows * cols, 7.0), ("codes", q_all, rows * cols, 77), ("scales", sc_all, rows, 7.0)):
        assert bool((buf[:m] == fill).all()) and bool((buf[m + n:] == fill).all()), f"the margin around {name} was written"
    # [batch, seq, I] keeps its shape; an empty input launches nothing; another kind is refused
    qt = pq.gelu_mul_quantize(gd[:6].reshape(2, 3, cols), ud[:6].reshape(2, 3, cols))
    assert qt.int_data.shape == (2, 3, cols) and qt.scale.shape == (6,) and np.array_equal(qt.int_data.reshape(6, cols).cpu().numpy(), spec[0][:6])
    e = torch.empty(0, cols, dtype=dtype, device="cuda")
    assert pq.gelu_mul_quantize(e, e).int_data.shape == (0, cols)
    with pytest.raises(ValueError):
        pq.gelu_mul_quantize(gd, ud, kind="gelu_erf")
    with torch.cuda.device(gd.device):
        assert L.lib().pq_gelu_mul_quant_rowwise(gd.data_ptr(), cols, ud.data_ptr(), cols, 0, rows, cols, 2, q_v.data_ptr(), cols, sc_v.data_ptr(), None, 0, L.stream_ptr(gd)) == 1
    assert b"kind" in L.lib().pq_last_error()
    # GatedMLP(act="gelu_tanh") is down(quantised gelu_tanh(g) * u) over the fused gate+up GEMM
    lins = [torch.nn.Linear(i, o, bias=False, dtype=dtype, device="cuda") for (o, i) in ((384, 256), (384, 256), (256, 384))]
    gate, up, down = (pq.qlinear.from_linear(l) for l in lins)
    mlp = pq.GatedMLP(pq.FusedQLinear([gate, up]), down, act="gelu_tanh")
    x = torch.randn(9, 256, device="cuda").to(dtype)
    xq = pq.quantize(x)
    assert torch.equal(mlp(x), down(pq.gelu_mul_quantize(gate(xq), up(xq))))
    silu = pq.GatedMLP(pq.FusedQLinear([gate, up]), down)
    assert silu.act == "silu" and torch.equal(silu(x), down(pq.silu_mul_quantize(gate(xq), up(xq))))
