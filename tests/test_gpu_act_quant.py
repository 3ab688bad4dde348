"""-m gpu: K1u, pq_act_quant_rowwise / act_quantize — relu, the tanh GELU and the erf GELU fused into the per-token int8 quantisation.  Codes, scales and h are
compared bit for bit (NaNs as a class) with the CPU specification (tests/act_spec.py: QSPEC U1-U3, then Q1-Q6 by oracle.qspec_numpy), over a grid that launches
every instantiation: one wave per row at 1 / 2 / 4 vectors, 512 threads x 3 vectors (and the same rows with PQ_SILU_TPR=256), 256 threads per row at 1 .. 16
vectors, the generic kernel on ragged widths, unaligned bases and odd leading dimensions, column blocks of a wider tensor; EVERY 16-bit pattern through the vector
and the generic kernel; rows on and off the fast-division domain of the tanh GELU; guarded margins around every output.  Addressing past 2^31 elements and more than 4 x 65 535 rows: tests/test_gpu_row_addressing.py."""
import numpy as np
import pytest
import torch

from oracle import qspec_numpy as Q
from tests import act_spec as AS
from tests.gpu_util import bits

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
CODE = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}
EPV = {torch.bfloat16: 8, torch.float16: 8, torch.float32: 4}
KINDS = ["relu", "gelu_tanh", "gelu_erf"]
GUARD = 64


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    from protoquant_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return protoquant_amd


def _store(t: torch.Tensor) -> np.ndarray:
    t = t.detach().contiguous().cpu()
    return t.numpy().copy() if t.dtype == torch.float32 else t.view(torch.int16).numpy().view(np.uint16).copy()


def _same_h(got: torch.Tensor, want: np.ndarray, code, what):
    g = bits(got)
    w = want.view(np.uint32) if want.dtype == np.float32 else want
    wn = np.isnan(Q.to_f32(want, code))
    gn = torch.isnan(got.detach().float().cpu()).numpy()
    assert g.shape == w.shape and np.array_equal(gn, wn), f"{what}: NaN positions differ"
    bad = (g != w) & ~wn
    assert not bad.any(), f"{what}: {int(bad.sum())} of {g.size} values of h differ (first at {np.argwhere(bad)[:3].tolist()}: got {g[bad][:3]}, want {w[bad][:3]})"


def _check(pq, x, kind, what, xd=None):
    code = CODE[x.dtype]
    q_s, s_s, h_s = AS.act_quantize(_store(x), code, kind)
    xd = x.cuda() if xd is None else xd
    qt, h = pq.act_quantize(xd, kind, return_h=True)
    qt2 = pq.act_quantize(xd, kind)
    torch.cuda.synchronize()
    _same_h(h, h_s, code, what)
    assert np.array_equal(qt.scale.cpu().numpy().view(np.uint32), s_s.view(np.uint32)), f"{what}: scales differ"
    assert np.array_equal(qt.int_data.cpu().numpy(), q_s), f"{what}: {int((qt.int_data.cpu().numpy() != q_s).sum())} codes differ from the specification"
    assert torch.equal(qt2.int_data, qt.int_data) and torch.equal(qt2.scale.view(torch.int32), qt.scale.view(torch.int32)), f"{what}: with and without h_out differ"
    k1 = pq.quantize(h)          # K1u == the activation then K1
    assert torch.equal(k1.int_data, qt.int_data) and torch.equal(k1.scale.view(torch.int32), qt.scale.view(torch.int32)), f"{what}: K1 on the stored h differs"


def _x(rows, cols, dtype, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, cols, generator=g) * scale).to(dtype)


# wave x1 / x2 / x4 (<= 256 vectors), 256 x2 (<= 512), x4 (<= 1024), 512 x3 (1025 .. 1536), 256 x8 (<= 2048), x16 (<= 4096)
VEC_COUNTS = [1, 64, 65, 128, 200, 256, 257, 512, 1000, 1025, 1536, 1537, 2048, 4096]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("nvec", VEC_COUNTS)
def test_every_vector_layout_matches_the_spec(pq, kind, dtype, nvec):
    rows = 6 if nvec <= 1024 else 3
    x = _x(rows, nvec * EPV[dtype], dtype, nvec)
    x[0] = x[0].abs().clamp(0.01, 9.0) * torch.where(x[0] < 0, -1.0, 1.0).to(dtype)      # a row inside the fast-division domain of the tanh GELU
    x[1, 0] = 0.0                                                                         # a zero: the `/` path
    x[2, -1] = -40.0                                                                      # the deep negative tail
    _check(pq, x, kind, f"{kind} {dtype} nvec={nvec}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
def test_wide_rows_with_256_threads(pq, pq_opt, kind, dtype):
    pq_opt("PQ_SILU_TPR", 256)
    _check(pq, _x(3, 1300 * EPV[dtype], dtype, 3), kind, f"{kind} {dtype} PQ_SILU_TPR=256")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("cols", [1, 7, 100, 50257])
def test_generic_kernel_on_ragged_widths(pq, kind, dtype, cols):
    _check(pq, _x(3, cols, dtype, cols), kind, f"{kind} {dtype} cols={cols}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
def test_column_blocks_and_odd_views(pq, kind, dtype):
    e = EPV[dtype]
    x = _x(9, 64 * e, dtype, 5)
    wide = torch.zeros(9, 3 * 64 * e, dtype=dtype).cuda()
    wide[:, 64 * e:2 * 64 * e] = x.cuda()
    _check(pq, x, kind, f"{kind} {dtype} column block", xd=wide[:, 64 * e:2 * 64 * e])
    odd = torch.zeros(9, 64 * e + 3, dtype=dtype).cuda()
    odd[:, 1:1 + 64 * e] = x.cuda()
    _check(pq, x, kind, f"{kind} {dtype} odd leading dimension + unaligned base", xd=odd[:, 1:1 + 64 * e])
    qt = pq.act_quantize(x.cuda().reshape(3, 3, -1), kind)
    assert qt.int_data.shape == (3, 3, 64 * e) and qt.scale.shape == (9,)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_every_16_bit_pattern(pq, kind, dtype):
    """all 65 536 patterns, as rows of 512 (vector kernel; rows that hold only small values take the fast division of the tanh GELU) and as rows of 509 (generic)"""
    pats = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
    _check(pq, pats.reshape(128, 512), kind, f"{kind} {dtype} all patterns, vector kernel")
    # sorted by magnitude: whole rows inside 0 < |x| <= 9.5
    order = torch.argsort(pats.float().abs().nan_to_num(nan=float("inf")))
    _check(pq, pats[order].reshape(128, 512), kind, f"{kind} {dtype} all patterns by magnitude")
    _check(pq, pats[:509 * 128].reshape(128, 509), kind, f"{kind} {dtype} patterns, generic kernel")


@pytest.mark.parametrize("kind", KINDS)
def test_f32_sweep_and_random_patterns(pq, kind):
    x = torch.linspace(-12.5, 12.5, 256 * 1024).reshape(256, 1024)
    _check(pq, x, kind, f"{kind} f32 sweep")
    g = torch.Generator().manual_seed(9)
    r = torch.randint(-2 ** 31, 2 ** 31 - 1, (64, 1024), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    _check(pq, r, kind, f"{kind} f32 random patterns")


@pytest.mark.parametrize("kind", KINDS)
def test_special_values(pq, kind):
    for dtype in DTYPES:
        x = _x(6, 64, dtype, 2)
        x[0] = 0.0
        x[1] = -0.0
        x[2, 3] = float("nan")
        x[3, 5] = float("inf")
        x[4, 7] = float("-inf")
        x[5] = -50.0
        _check(pq, x, kind, f"{kind} {dtype} special values")
        qt, h = pq.act_quantize(x.cuda(), kind, return_h=True)
        h, s = h.cpu().float(), qt.scale.cpu()
        assert s[0] == 1.0 and s[1] == 1.0 and s[5] == 1.0 and torch.isnan(s[2]) and torch.isinf(s[3]) and torch.isnan(h[2, 3]) and h[3, 5] == float("inf")
        assert h[4, 7] == 0.0 and (h[5] == 0.0).all() and bool(torch.signbit(h[4, 7])) == (kind != "relu") and bool(torch.signbit(h[5]).all()) == (kind != "relu")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cols", [1024, 100])
def test_nothing_is_written_outside_the_outputs(pq, kind, cols):
    from protoquant_amd import _lib
    rows, dtype = 5, torch.bfloat16
    x = _x(rows, cols, dtype, 21)
    xd = x.cuda()
    qb = torch.full((rows * cols + 2 * GUARD,), 0x55, dtype=torch.int8).cuda()
    sb = torch.full((rows + 2 * GUARD,), -7.0, dtype=torch.float32).cuda()
    hb = torch.full((rows * cols + 2 * GUARD,), -3.0, dtype=dtype).cuda()
    _lib.check(_lib.lib().pq_act_quant_rowwise(xd.data_ptr(), cols, 0, rows, cols, _lib.ACT_KINDS[kind], qb.data_ptr() + GUARD, cols, sb.data_ptr() + 4 * GUARD,
                                               hb.data_ptr() + 2 * GUARD, cols, torch.cuda.current_stream().cuda_stream), "K1u")
    torch.cuda.synchronize()
    assert (qb[:GUARD] == 0x55).all() and (qb[-GUARD:] == 0x55).all() and (sb[:GUARD] == -7.0).all() and (sb[-GUARD:] == -7.0).all()
    assert (hb[:GUARD] == -3.0).all() and (hb[-GUARD:] == -3.0).all() and torch.equal(xd.cpu().view(torch.int16), x.view(torch.int16))
    q_s, s_s, h_s = AS.act_quantize(_store(x), 0, kind)
    assert np.array_equal(qb[GUARD:-GUARD].cpu().numpy().reshape(rows, cols), q_s) and np.array_equal(sb[GUARD:-GUARD].cpu().numpy(), s_s)
    _same_h(hb[GUARD:-GUARD].reshape(rows, cols), h_s, 0, "guarded h")


def test_module_and_refusals(pq):
    from protoquant_amd import _lib
    m = pq.ActQuant("gelu_erf")
    assert not m.state_dict()
    x = _x(4, 256, torch.float16, 1)
    qt = m(x.cuda().reshape(2, 2, 256))
    q_s, s_s, _ = AS.act_quantize(_store(x), 1, "gelu_erf")
    assert np.array_equal(qt.int_data.cpu().numpy().reshape(4, 256), q_s) and np.array_equal(qt.scale.cpu().numpy(), s_s)
    with pytest.raises(ValueError):
        pq.ActQuant("quick_gelu")
    with pytest.raises(ValueError):
        pq.act_quantize(x.cuda(), "silu")
    xd = x.cuda()
    st = _lib.lib().pq_act_quant_rowwise(xd.data_ptr(), 256, 1, 4, 256, 2, qt.int_data.data_ptr(), 256, qt.scale.data_ptr(), xd.data_ptr(), 256, None)
    assert st == 1 and b"h_out overlaps x" in _lib.lib().pq_last_error()
