"""-m gpu: K1l, pq_layernorm_quant_rowwise / layernorm_quantize — LayerNorm fused into the per-token int8 quantisation.  Codes, scales and h are compared bit for bit
(NaNs as a class) with the CPU specification (tests/lnorm_spec.py: QSPEC L1-L6, then Q1-Q6 by oracle.qspec_numpy), over a grid that launches every instantiation:
one wave per row at 1 / 2 / 4 vectors (8 with PQ_RMS_WAVE_MAX=512), 256 threads per row at 1 .. 16 vectors (and on short rows with PQ_RMS_WAVE_MAX=0), the generic
kernel on ragged widths, unaligned bases and odd leading dimensions; with and without bias; rows of zeros, constant rows, NaN / Inf rows; guarded margins around every
output.  Addressing past 2^31 elements and more than 4 x 65 535 rows: tests/test_gpu_row_addressing.py."""
import numpy as np
import pytest
import torch

from oracle import qspec_numpy as Q
from tests import lnorm_spec as LS
from tests.gpu_util import bits

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
CODE = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}
EPV = {torch.bfloat16: 8, torch.float16: 8, torch.float32: 4}
EPS = 1e-5
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
    assert not bad.any(), f"{what}: {int(bad.sum())} of {g.size} values of h differ (first at {np.argwhere(bad)[:3].tolist()})"


def _inputs(rows, cols, dtype, seed, bias=True, scale=1.0, shift=0.5):
    g = torch.Generator().manual_seed(seed)
    x = ((torch.randn(rows, cols, generator=g) + shift) * scale).to(dtype)
    w = (1.0 + 0.25 * torch.randn(cols, generator=g)).to(dtype)
    b = (0.3 * torch.randn(cols, generator=g)).to(dtype) if bias else None
    return x, w, b


def _check(pq, x, w, b, what, xd=None):
    """x, w, b: CPU tensors (b may be None); xd: the GPU operand when it is not simply x.cuda() (a view with a leading dimension or an odd base)"""
    code = CODE[x.dtype]
    q_s, s_s, h_s = LS.layernorm_quantize(_store(x), _store(w), None if b is None else _store(b), EPS, code)
    xd = x.cuda() if xd is None else xd
    wd, bd = w.cuda(), None if b is None else b.cuda()
    qt, h = pq.layernorm_quantize(xd, wd, bd, EPS, return_h=True)
    qt2 = pq.layernorm_quantize(xd, wd, bd, EPS)
    torch.cuda.synchronize()
    assert np.array_equal(qt.int_data.cpu().numpy(), q_s), f"{what}: {int((qt.int_data.cpu().numpy() != q_s).sum())} codes differ from the specification"
    sg = qt.scale.cpu().numpy()
    assert np.array_equal(sg.view(np.uint32), s_s.view(np.uint32)), f"{what}: scales differ"
    _same_h(h, h_s, code, what)
    assert torch.equal(qt2.int_data, qt.int_data) and torch.equal(qt2.scale.view(torch.int32), qt.scale.view(torch.int32)), f"{what}: with and without h_out differ"
    # K1l == LayerNorm then K1: the stored h through quantize() gives the same codes and scales
    k1 = pq.quantize(h)
    assert torch.equal(k1.int_data, qt.int_data) and torch.equal(k1.scale.view(torch.int32), qt.scale.view(torch.int32)), f"{what}: K1 on the stored h differs"


# nvec (16-byte vectors per row) -> layout: wave x1 (<= 64), x2 (<= 128), x4 (<= 256); 256 threads x1 (never by default: <= 256 is wave), x2 (<= 512), x4, x8, x16
VEC_COUNTS = [1, 5, 64, 65, 128, 200, 256, 257, 512, 513, 1024, 1500, 2048, 2049, 4096]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("nvec", VEC_COUNTS)
def test_every_vector_layout_matches_the_spec(pq, dtype, nvec):
    cols = nvec * EPV[dtype]
    rows = 7 if nvec <= 1024 else 3
    x, w, b = _inputs(rows, cols, dtype, nvec)
    _check(pq, x, w, b, f"{dtype} nvec={nvec}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("wave_max,nvec", [(512, 300), (512, 512), (0, 1), (0, 40), (0, 256)])
def test_switched_layouts_give_the_same_bits(pq, pq_opt, dtype, wave_max, nvec):
    """PQ_RMS_WAVE_MAX=512: one wave per row at 8 vectors per lane; PQ_RMS_WAVE_MAX=0: the 256-thread layout on short rows (1 vector per thread)"""
    pq_opt("PQ_RMS_WAVE_MAX", wave_max)
    x, w, b = _inputs(6, nvec * EPV[dtype], dtype, 100 + nvec)
    _check(pq, x, w, b, f"{dtype} PQ_RMS_WAVE_MAX={wave_max} nvec={nvec}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("cols", [1, 7, 100, 50257])
def test_generic_kernel_on_ragged_widths(pq, dtype, cols):
    x, w, b = _inputs(3, cols, dtype, cols)
    _check(pq, x, w, b, f"{dtype} cols={cols}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
def test_without_bias_and_views(pq, dtype):
    e = EPV[dtype]
    x, w, _ = _inputs(9, 64 * e, dtype, 5, bias=False)
    _check(pq, x, w, None, f"{dtype} no bias")
    # a column block of a wider tensor (aligned leading dimension: vector layout), an odd leading dimension and an unaligned base (generic)
    wide = torch.zeros(9, 64 * e + 2 * e, dtype=dtype).cuda()
    wide[:, e:e + 64 * e] = x.cuda()
    _check(pq, x, w, None, f"{dtype} column block", xd=wide[:, e:e + 64 * e])
    odd = torch.zeros(9, 64 * e + 3, dtype=dtype).cuda()
    odd[:, 1:1 + 64 * e] = x.cuda()
    x2, w2, b2 = _inputs(9, 64 * e, dtype, 6)
    odd[:, 1:1 + 64 * e] = x2.cuda()
    _check(pq, x2, w2, b2, f"{dtype} odd leading dimension + unaligned base", xd=odd[:, 1:1 + 64 * e])
    # 3-D input keeps its shape
    x3, w3, b3 = _inputs(8, 32 * e, dtype, 7)
    qt = pq.layernorm_quantize(x3.cuda().reshape(2, 4, -1), w3.cuda(), b3.cuda(), EPS)
    assert qt.int_data.shape == (2, 4, 32 * e) and qt.scale.shape == (8,)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("cols_vec", [16, 300, 1])
def test_special_rows(pq, dtype, cols_vec):
    """rows of zeros (h = bias; without bias h = 0 and the scale is 1), constant rows (var = 0), a NaN, +Inf, -Inf or both in a row: the whole row is NaN (scale NaN, codes 0)"""
    cols = cols_vec * EPV[dtype] + (3 if cols_vec == 1 else 0)
    x, w, b = _inputs(8, cols, dtype, 11)
    x[0] = 0
    x[1] = 3.0
    x[2, cols // 2] = float("nan")
    x[3, 0] = float("inf")
    x[4, cols - 1] = float("-inf")
    x[5, 0], x[5, cols - 1] = float("inf"), float("-inf")
    x[6] = -0.0
    _check(pq, x, w, b, f"{dtype} special rows, bias")
    _check(pq, x, w, None, f"{dtype} special rows, no bias")
    qt = pq.layernorm_quantize(x.cuda(), w.cuda(), None, EPS)
    s = qt.scale.cpu()
    assert s[0] == 1.0 and s[1] == 1.0 and s[6] == 1.0 and torch.isnan(s[2:6]).all() and (qt.int_data[2:6] == 0).all()
    assert s[2:6].view(torch.int32).tolist() == [0x7FC00000] * 4


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("cols", [1024, 100])
def test_nothing_is_written_outside_the_outputs(pq, dtype, cols):
    """the C entry on buffers with guarded margins: q, scale and h_out keep their margins, x / weight / bias are not written"""
    from protoquant_amd import _lib
    rows = 5
    x, w, b = _inputs(rows, cols, dtype, 21)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    qb = torch.full((rows * cols + 2 * GUARD,), 0x55, dtype=torch.int8).cuda()
    sb = torch.full((rows + 2 * GUARD,), -7.0, dtype=torch.float32).cuda()
    hb = torch.full((rows * cols + 2 * GUARD,), -3.0, dtype=dtype).cuda()
    L = _lib.lib()
    es = xd.element_size()
    _lib.check(L.pq_layernorm_quant_rowwise(xd.data_ptr(), cols, wd.data_ptr(), bd.data_ptr(), EPS, CODE[dtype], rows, cols, qb.data_ptr() + GUARD, cols,
                                            sb.data_ptr() + 4 * GUARD, hb.data_ptr() + es * GUARD, cols, torch.cuda.current_stream().cuda_stream), "K1l")
    torch.cuda.synchronize()
    assert (qb[:GUARD] == 0x55).all() and (qb[-GUARD:] == 0x55).all() and (sb[:GUARD] == -7.0).all() and (sb[-GUARD:] == -7.0).all()
    assert (hb[:GUARD] == -3.0).all() and (hb[-GUARD:] == -3.0).all()
    assert torch.equal(xd.cpu().view(torch.uint8), x.view(torch.uint8)) and torch.equal(wd.cpu().view(torch.uint8), w.view(torch.uint8)) and torch.equal(bd.cpu().view(torch.uint8), b.view(torch.uint8))
    q_s, s_s, h_s = LS.layernorm_quantize(_store(x), _store(w), _store(b), EPS, CODE[dtype])
    assert np.array_equal(qb[GUARD:-GUARD].cpu().numpy().reshape(rows, cols), q_s) and np.array_equal(sb[GUARD:-GUARD].cpu().numpy(), s_s)
    _same_h(hb[GUARD:-GUARD].reshape(rows, cols), h_s, CODE[dtype], "guarded h")


def test_module_and_refusals(pq):
    from protoquant_amd import _lib
    ln = torch.nn.LayerNorm(256, eps=1e-5).to(torch.bfloat16)
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5)
        ln.bias.uniform_(-0.5, 0.5)
    m = pq.LayerNormQuant(ln.weight, ln.bias, ln.eps).cuda()
    assert set(m.state_dict()) == {"weight", "bias"}
    m.load_state_dict(ln.state_dict())
    x = torch.randn(4, 10, 256).to(torch.bfloat16)
    qt = m(x.cuda())
    q_s, s_s, _ = LS.layernorm_quantize(_store(x.reshape(40, 256)), _store(ln.weight), _store(ln.bias), 1e-5, 0)
    assert np.array_equal(qt.int_data.cpu().numpy().reshape(40, 256), q_s) and np.array_equal(qt.scale.cpu().numpy(), s_s)
    with pytest.raises(ValueError):
        pq.layernorm_quantize(x.cuda(), None, None)
    with pytest.raises(ValueError):
        pq.layernorm_quantize(x.cuda(), ln.weight.cuda()[:128], None)
    xd = x.cuda().reshape(40, 256)
    st = _lib.lib().pq_layernorm_quant_rowwise(xd.data_ptr(), 256, m.weight.data_ptr(), None, 1e-5, 0, 40, 256, xd.data_ptr(), 256, qt.scale.data_ptr(), None, 0, None)
    assert st == 1 and b"q overlaps x" in _lib.lib().pq_last_error()
