"""-m gpu: K1hn, the per-head RMSNorm of q and k (pq_head_rmsnorm / pq.head_rmsnorm; QSPEC HN1: N1-N5 or NG1-NG5 on rows of head_dim), through the C-ABI and the
Python surface.

Every C-ABI call here runs on GUARDED operands: x lies in a flat buffer filled with NaN (its neighbours, the gaps between its rows and the columns behind it), the
weight between NaN margins (a read past its end poisons the result), out in a flat buffer filled with a finite sentinel.  After every call the WHOLE input buffer
and the weight buffer are compared with what they held before it, and the WHOLE output buffer outside the rows of out with the sentinel.

1. to the specification, bits (NaN as a class): both gains x bf16 / fp16 / f32 x every width class x heads in {1, 3, 8, 40} x tokens in {1, 2, 5, 33}, against
   oracle.qspec_numpy.rmsnorm_quantize(...)[2] / tests.gemma_spec.gemma_h on the rows reshaped [tokens * heads, D], and against the library's own row kernels;
2. layouts: the q and the k slice of a fused q/k/v buffer (v NaN, unchanged), Gemma-3's transposed view, batch 2, a view that does not collapse (the copy path), a
   base off by one element (the generic form): the same bits everywhere;
3. heads that share a wave do not see each other: NaN, +Inf, -Inf, the largest finite value, an all-zero row with eps = 0 and a subnormal row planted in every group
   slot of a wave, for every G;
4. dead lanes: NaN / Inf in the columns just behind a head's end change nothing;
5. far addressing: offsets on both sides of element 2^31 and byte 2^32, and 262 149 outer rows;
6. eager closeness to transformers' Qwen3RMSNorm and Gemma3RMSNorm on >= 10^7 bf16 elements at D = 128."""
import numpy as np
import pytest
import torch

from oracle import qspec_numpy as Q
from tests import gemma_spec as G
from tests.gpu_util import TD, bits, to_gpu

pytestmark = pytest.mark.gpu

EPS = 1e-6
KINDS = {"llama": 0, "gemma": 1}
NAMES = {0: "bf16", 1: "fp16", 2: "f32"}
SENT = {0: 0x5A5B, 1: 0x5A5B, 2: 0x5A5B5A5B}          # finite in every dtype
IVIEW = {0: torch.int16, 1: torch.int16, 2: torch.int32}
MARGIN = 64                                          # elements: a multiple of 16 bytes in every dtype, so a margin moves no alignment


@pytest.fixture(scope="module")
def L():
    from protoquant_amd import _lib
    assert torch.cuda.is_available()
    return _lib.lib()


def spec(rows_bits, w_bits, eps, code, kind):
    """the CPU specification of the normalised rows, as storage bits"""
    rows_bits = np.ascontiguousarray(rows_bits)
    return Q.rmsnorm_quantize(rows_bits, w_bits, eps, code)[2] if kind == "llama" else G.gemma_h(rows_bits, w_bits, eps, code)


def rand_rows(rng, n, D, code):
    """n seeded rows of D at three magnitudes, as storage bits"""
    a = rng.standard_normal((n, D)).astype(np.float32) * np.array([0.05, 1.0, 20.0], np.float32)[rng.integers(0, 3, n)][:, None]
    return Q.from_f32(a, code)


def rand_weight(rng, D, code, kind):
    return Q.from_f32(((1.0 if kind == "llama" else 0.0) + 0.3 * rng.standard_normal(D)).astype(np.float32), code)


class Guarded:
    """The operands of one pq_head_rmsnorm call.  x[n_outer, n_inner, D] with strides (ld_xo, ld_xi) in a NaN-filled buffer at element offset MARGIN + x_odd, the
    weight between NaN margins, out with strides (ld_oo, ld_oi) in a sentinel-filled buffer at MARGIN + o_odd."""

    def __init__(self, code, n_outer, n_inner, D, ld_xo, ld_xi, ld_oo=None, ld_oi=None, x_odd=0, o_odd=0):
        self.code, self.shape = code, (n_outer, n_inner, D)
        self.ld_x, self.ld_o = (ld_xo, ld_xi), (ld_oo if ld_oo is not None else n_inner * D, ld_oi if ld_oi is not None else D)
        span = lambda ld: (n_outer - 1) * ld[0] + (n_inner - 1) * ld[1] + D          # noqa: E731
        self.x_off, self.o_off = MARGIN + x_odd, MARGIN + o_odd
        self.xbuf = torch.full((self.x_off + span(self.ld_x) + MARGIN,), float("nan"), dtype=TD[code], device="cuda")
        self.obuf = torch.full((self.o_off + span(self.ld_o) + MARGIN,), SENT[code], dtype=IVIEW[code], device="cuda")
        self.wbuf = torch.full((2 * MARGIN + D,), float("nan"), dtype=TD[code], device="cuda")
        self.x = self.xbuf.as_strided(self.shape, self.ld_x + (1,), self.x_off)
        self.out = self.obuf.view(TD[code]).as_strided(self.shape, self.ld_o + (1,), self.o_off)
        self.w = self.wbuf[MARGIN:MARGIN + D]

    def set(self, rows_bits, w_bits):
        self.x.copy_(to_gpu(rows_bits, self.code).reshape(self.shape))
        self.w.copy_(to_gpu(w_bits, self.code))

    def call(self, L, kind, eps=EPS):
        """the call, then the whole-buffer checks; returns the rows of out as storage bits [n_outer * n_inner, D]"""
        from protoquant_amd import _lib
        n_outer, n_inner, D = self.shape
        xb, wb = self.xbuf.view(IVIEW[self.code]).clone(), self.wbuf.view(IVIEW[self.code]).clone()
        self.obuf.fill_(SENT[self.code])
        st = L.pq_head_rmsnorm(self.x.data_ptr(), self.ld_x[0], self.ld_x[1], self.w.data_ptr(), float(eps), KINDS[kind], self.code, n_outer, n_inner, D,
                               self.out.data_ptr(), self.ld_o[0], self.ld_o[1], torch.cuda.current_stream().cuda_stream)
        _lib.check(st, "pq_head_rmsnorm")
        torch.cuda.synchronize()
        got = bits(self.out).reshape(n_outer * n_inner, D)
        assert torch.equal(self.xbuf.view(IVIEW[self.code]), xb), "the input buffer was written"
        assert torch.equal(self.wbuf.view(IVIEW[self.code]), wb), "the weight buffer was written"
        rest = self.obuf.clone()
        rest.as_strided(self.shape, self.ld_o + (1,), self.o_off).fill_(SENT[self.code])
        assert bool((rest == SENT[self.code]).all()), f"stores outside the rows of out: {int((rest != SENT[self.code]).sum())} elements"
        return got


def store(t):
    """a tensor as the specification takes it: uint16 bit patterns for the half types, float32 values for f32"""
    b = bits(t)
    return b.view(np.float32) if b.dtype == np.uint32 else b


def as_bits(a, code):
    """storage bits as unsigned integers (f32 rows travel as float32 in the specification)"""
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _is_nan(b, code):
    if code == 2:
        return (b & 0x7FFFFFFF) > 0x7F800000
    return (b & 0x7FFF) > (0x7F80 if code == 0 else 0x7C00)


def same_bits(got, want, code, what):
    """storage bits against storage bits: NaN positions equal, everything else bit for bit"""
    got, want = as_bits(got, code), as_bits(want, code)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = _is_nan(got, code), _is_nan(want, code)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ ({int(gn.sum())} vs {int(wn.sum())})"
    bad = (got != want) & ~wn
    assert not bad.any(), f"{what}: {int(bad.sum())} of {got.size} elements differ (first at {np.argwhere(bad)[:3].tolist()})"


# ---------------------------------------------------------------------------------------------------------------- 1. to the specification
# D: 8 one vector; 72 nine of 16 lanes; 512 bf16 / fp16: 64 lanes, f32: the generic form; 100: no whole number of vectors (generic); 1024 (bf16): over 1024 bytes (generic)
WIDTHS = (8, 64, 72, 80, 96, 128, 256, 512, 100)
HEADS, TOKENS = (1, 3, 8, 40), (1, 2, 5, 33)
CASES_1 = [(code, kind, D) for code in (0, 1, 2) for kind in KINDS for D in WIDTHS + ((1024,) if code == 0 else ())]


@pytest.mark.parametrize("code,kind,D", CASES_1, ids=[f"{NAMES[c]}-{k}-{d}" for c, k, d in CASES_1])
def test_to_the_specification_bit_for_bit(L, code, kind, D):
    import protoquant_amd as pq
    rng = np.random.default_rng(1000 * code + D + 7 * KINDS[kind])
    nmax = max(HEADS) * max(TOKENS)
    rows, w = rand_rows(rng, nmax, D, code), rand_weight(rng, D, code, kind)
    want = as_bits(spec(rows, w, EPS, code, kind), code)          # once: every (heads, tokens) below takes the first tokens * heads rows
    row_kernel = pq.rmsnorm_quantize if kind == "llama" else pq.gemma_rmsnorm_quantize
    for heads in HEADS:
        for tokens in TOKENS:
            n = heads * tokens
            what = f"{NAMES[code]} {kind} D={D} heads={heads} tokens={tokens}"
            g = Guarded(code, tokens, heads, D, heads * D + 16, D, heads * D + 32, D)          # gaps between the tokens of x (NaN) and of out (sentinel)
            g.set(rows[:n], w)
            got = g.call(L, kind)
            same_bits(as_bits(got, code), want[:n], code, what)
            # the Python surface on the same strided view, and the library's own row kernel on the rows copied contiguous
            py = pq.head_rmsnorm(g.x, g.w, EPS, kind)
            lib_h = row_kernel(g.x.reshape(n, D).contiguous(), g.w.contiguous(), EPS, return_h=True)[1]
            assert py.shape == g.x.shape and py.is_contiguous() and torch.equal(py.reshape(n, D), lib_h), what
            assert np.array_equal(bits(py).reshape(n, D), got), what


# ---------------------------------------------------------------------------------------------------------------- 2. layouts
@pytest.mark.parametrize("code,kind,D", [(0, "llama", 128), (0, "gemma", 80), (1, "llama", 64), (2, "gemma", 64), (2, "llama", 40)])
def test_layouts_give_the_same_bits(L, code, kind, D):
    import protoquant_amd as pq
    from protoquant_amd.qtensor import _collapse_heads
    B, T, Hq, Hkv = 2, 5, 6, 3          # (three kv heads: the view that does not collapse keeps two of them)
    rng = np.random.default_rng(D + code)
    width = (Hq + 2 * Hkv) * D
    w_bits = rand_weight(rng, D, code, kind)
    w = to_gpu(w_bits, code)
    qkv = to_gpu(rand_rows(rng, B * T, width, code), code).reshape(B, T, width)
    qkv[..., (Hq + Hkv) * D:] = float("nan")                   # the v columns
    before = qkv.view(IVIEW[code]).clone()
    for name, lo, H in (("q", 0, Hq), ("k", Hq * D, Hkv)):
        sl = qkv[..., lo:lo + H * D]
        want = as_bits(spec(store(sl).reshape(B * T * H, D), w_bits, EPS, code, kind), code)
        # Qwen3: q_proj(x).view(B, T, H, D) on a column slice: no copy, (tokens, ld) x (heads, D)
        v4 = sl.view(B, T, H, D)
        assert _collapse_heads(v4.shape, v4.stride()) == (B * T, width, H, D)
        got = pq.head_rmsnorm(v4, w, EPS, kind)
        assert got.is_contiguous() and got.shape == v4.shape
        same_bits(bits(got).reshape(-1, D), want, code, f"{name} slice, [B, T, H, D]")
        # Gemma-3: the transposed view; the result is laid out in x's stride order, as eager's elementwise chain lays it out
        vt = v4.transpose(1, 2)
        assert _collapse_heads(vt.shape, vt.stride()) == (B * T, width, H, D)
        got_t = pq.head_rmsnorm(vt, w, EPS, kind)
        assert got_t.shape == vt.shape and got_t.stride() == (vt.float() * 1.0).stride() and got_t.transpose(1, 2).is_contiguous()
        assert torch.equal(got_t.transpose(1, 2).view(IVIEW[code]), got.view(IVIEW[code])), f"{name} slice, transposed view"
        # a view that does not collapse (three strided axes are left): one copy, the same bits
        nc = v4[:, :T - 1, :H - 1]
        assert _collapse_heads(nc.shape, nc.stride()) is None
        got_nc = pq.head_rmsnorm(nc, w, EPS, kind)
        assert got_nc.is_contiguous() and torch.equal(got_nc.view(IVIEW[code]), got[:, :T - 1, :H - 1].view(IVIEW[code])), f"{name} slice, the copy path"
        # through the C-ABI: the vector form where it lies, and the generic form by a base off by one element; both hold the same bits
        n = B * T * H
        for x_odd, o_odd in ((0, 0), (1, 0), (0, 1)):
            g = Guarded(code, B * T, H, D, width, D, H * D + 16, D, x_odd=x_odd, o_odd=o_odd)
            g.set(store(sl).reshape(n, D), w_bits)
            same_bits(as_bits(g.call(L, kind), code), want, code, f"{name} slice, C-ABI, x base +{x_odd}, out base +{o_odd}")
    assert torch.equal(qkv.view(IVIEW[code]), before), "the fused q/k/v buffer (its NaN v columns included) was written"
    # a plain contiguous tensor collapses to ONE axis
    c = to_gpu(rand_rows(rng, 3 * 4 * 5, D, code), code).reshape(3, 4, 5, D)
    assert _collapse_heads(c.shape, c.stride()) == (60, D, 1, D)
    same_bits(bits(pq.head_rmsnorm(c, w, EPS, kind)).reshape(60, D), as_bits(spec(store(c).reshape(60, D), w_bits, EPS, code, kind), code), code, "contiguous")
    # an empty x: an empty tensor, no launch; a CPU tensor raises
    assert pq.head_rmsnorm(c[:0], w, EPS, kind).shape == (0, 4, 5, D)
    from protoquant_amd._lib import PQError
    with pytest.raises(PQError):
        pq.head_rmsnorm(c.cpu(), w.cpu(), EPS, kind)


# ---------------------------------------------------------------------------------------------------------------- 3. heads that share a wave
def _plants(D, code):
    """name -> (row of D as f32 values, eps)"""
    big = {0: 3.3895313892515355e38, 1: 65504.0, 2: 3.4028234663852886e38}[code]
    tiny = {0: 2.0 ** -133, 1: 2.0 ** -24, 2: 2.0 ** -149}[code]          # the smallest subnormal of the dtype
    base = np.linspace(-1.0, 1.0, D, dtype=np.float32) + np.float32(0.25)

    def with_(v):
        r = base.copy()
        r[D // 2] = v
        return r
    return {"nan": (with_(np.nan), EPS), "+inf": (with_(np.inf), EPS), "-inf": (with_(-np.inf), EPS), "max finite": (np.full(D, big, np.float32), EPS),
            "all zero, eps 0": (np.zeros(D, np.float32), 0.0), "subnormal": (np.full(D, tiny, np.float32) * np.sign(base + np.float32(1e-3)), EPS)}


# (dtype, gain, D) -> G lanes per head: bf16 8 -> 4, 64 -> 8, 72 -> 16 (nine live), 256 -> 32, 512 -> 64;  f32 16 -> 4, 32 -> 8, 40 -> 16 (ten live), 128 -> 32, 256 -> 64
CASES_3 = [(0, "llama", 8, 4), (0, "gemma", 64, 8), (0, "llama", 72, 16), (0, "gemma", 256, 32), (0, "llama", 512, 64),
           (2, "gemma", 16, 4), (2, "llama", 32, 8), (2, "gemma", 40, 16), (2, "llama", 128, 32), (2, "gemma", 256, 64), (1, "llama", 128, 16)]


@pytest.mark.parametrize("code,kind,D,lanes", CASES_3, ids=[f"{NAMES[c]}-{k}-{d}-G{g}" for c, k, d, g in CASES_3])
def test_heads_that_share_a_wave_do_not_see_each_other(L, code, kind, D, lanes):
    nvec = D * (4 if code == 2 else 2) // 16
    assert lanes >= max(nvec, 4) and (lanes == 4 or lanes // 2 < nvec)
    hpw = 64 // lanes                                       # heads per wave
    heads = 3 * hpw + 1                                     # the planted wave is the second: full waves on either side of it, and a ragged last one
    rng = np.random.default_rng(D * 3 + code)
    rows, w = rand_rows(rng, heads, D, code), rand_weight(rng, D, code, kind)
    g = Guarded(code, 1, heads, D, heads * D, D)
    base = {}
    for eps in (EPS, 0.0):
        g.set(rows, w)
        base[eps] = g.call(L, kind, eps)
        same_bits(as_bits(base[eps], code), as_bits(spec(rows, w, eps, code, kind), code), code, f"no plant, eps={eps}")
    for name, (row, eps) in _plants(D, code).items():
        row_bits = Q.from_f32(row, code)
        want_row = as_bits(spec(row_bits[None, :], w, eps, code, kind), code)
        for slot in range(hpw):
            h = hpw + slot
            planted = rows.copy()
            planted[h] = row_bits
            g.set(planted, w)
            got = g.call(L, kind, eps)
            same_bits(as_bits(got[h:h + 1], code), want_row, code, f"{name} in slot {slot}: the planted head")
            others = np.arange(heads) != h
            assert np.array_equal(got[others], base[eps][others]), f"{name} in slot {slot}: another head of the wave changed"


# ---------------------------------------------------------------------------------------------------------------- 4. dead lanes
@pytest.mark.parametrize("code,D", [(0, 72), (0, 80), (2, 40)])
@pytest.mark.parametrize("kind", list(KINDS))
def test_dead_lanes_read_nothing_that_counts(L, code, D, kind):
    """D = 72 / 80 (bf16: 9 / 10 of 16 lanes) and 40 (f32: 10 of 16): heads laid end to end, so the columns just behind a head are the next head's first columns (the
    NaN margin behind the last head, and NaN behind the weight's end: Guarded).  Poisoning every second head changes nothing in the heads between them."""
    heads = 9
    rng = np.random.default_rng(D + code)
    rows, w = rand_rows(rng, heads, D, code), rand_weight(rng, D, code, kind)
    g = Guarded(code, 1, heads, D, heads * D, D)
    g.set(rows, w)
    base = g.call(L, kind)
    same_bits(as_bits(base, code), as_bits(spec(rows, w, EPS, code, kind), code), code, "no poison")
    for parity in (0, 1):
        for poison in (np.nan, np.inf, -np.inf):
            p = Q.to_f32(rows, code).copy()
            p[parity::2, :8] = poison
            g.set(Q.from_f32(p, code), w)
            got = g.call(L, kind)
            keep = np.arange(heads) % 2 != parity
            assert np.array_equal(got[keep], base[keep]), f"{poison} in the first columns of the heads of parity {parity} reached their neighbours"


# ---------------------------------------------------------------------------------------------------------------- 5. far addressing
FAR_LD = (1 << 31) + 64          # elements (bf16): o * FAR_LD lies on both sides of element 2^31, o * FAR_LD * 2 on both sides of byte 2^32
FAR_FRONT = 1 << 31              # elements in front of the base: an offset truncated to 32 bits (signed or unsigned, elements or bytes) stays inside the allocation


def _need(nbytes):
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + (2 << 30):
        pytest.skip(f"needs {nbytes >> 20} MiB of free device memory, {free >> 20} MiB are free")


def test_far_addressing_on_both_sides_of_2g_elements_and_4g_bytes(L):
    """bf16, ld_o = 2^31 + 64 elements, three outer rows of 8 heads of 128: once with x far (out dense), once with out far (x dense), in ONE uninitialised buffer of
    which only the windows around the rows are written and checked (a margin of 64 elements on either side of each row: NaN around x, the sentinel around out)."""
    from protoquant_amd import _lib
    code, kind, n_outer, H, D = 0, "llama", 3, 8, 128
    offs = [o * FAR_LD for o in range(n_outer)]
    assert offs[1] > (1 << 31) > offs[0] and offs[1] * 2 > (1 << 32) and offs[2] > (1 << 32)
    total = FAR_FRONT + offs[-1] + H * D + (1 << 16)
    assert total >= FAR_FRONT + (1 << 32) + H * D          # an unsigned 32-bit truncation of an element offset lands inside
    _need(total * 2)
    far = torch.empty(total, dtype=torch.bfloat16, device="cuda")
    rng = np.random.default_rng(5)
    rows, w_bits = rand_rows(rng, n_outer * H, D, code), rand_weight(rng, D, code, kind)
    want = spec(rows, w_bits, EPS, code, kind)
    w = to_gpu(w_bits, code)
    dense = to_gpu(rows, code).reshape(n_outer, H, D)
    windows = [far[FAR_FRONT + o - MARGIN:FAR_FRONT + o + H * D + MARGIN] for o in offs]
    st = torch.cuda.current_stream().cuda_stream
    # x far
    for o, win in enumerate(windows):
        win.fill_(float("nan"))
        win[MARGIN:MARGIN + H * D].copy_(dense[o].reshape(-1))
    out = torch.empty((n_outer, H, D), dtype=torch.bfloat16, device="cuda")
    _lib.check(L.pq_head_rmsnorm(far.data_ptr() + FAR_FRONT * 2, FAR_LD, D, w.data_ptr(), EPS, 0, code, n_outer, H, D, out.data_ptr(), H * D, D, st), "pq_head_rmsnorm")
    torch.cuda.synchronize()
    same_bits(bits(out).reshape(-1, D), want, code, "x far")
    for o, win in enumerate(windows):
        assert bool(torch.isnan(win[:MARGIN]).all()) and bool(torch.isnan(win[MARGIN + H * D:]).all()) and torch.equal(win[MARGIN:MARGIN + H * D], dense[o].reshape(-1))
    # out far
    for win in windows:
        win.view(torch.int16).fill_(SENT[code])
    _lib.check(L.pq_head_rmsnorm(dense.data_ptr(), H * D, D, w.data_ptr(), EPS, 0, code, n_outer, H, D, far.data_ptr() + FAR_FRONT * 2, FAR_LD, D, st), "pq_head_rmsnorm")
    torch.cuda.synchronize()
    got = torch.stack([win[MARGIN:MARGIN + H * D] for win in windows])
    same_bits(bits(got).reshape(-1, D), want, code, "out far")
    for win in windows:
        wi = win.view(torch.int16)
        assert bool((wi[:MARGIN] == SENT[code]).all()) and bool((wi[MARGIN + H * D:] == SENT[code]).all()), "a store outside a far row of out"
    del far, windows
    torch.cuda.empty_cache()


def test_more_than_4x65535_outer_rows(L):
    """262 149 outer rows x 1 head x 64 columns (bf16): every row against the library's own row kernel on the GPU, sampled rows against the specification"""
    import protoquant_amd as pq
    code, kind, rows_n, D = 0, "llama", 4 * 65535 + 9, 64
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(rows_n, D, generator=g) * 2).to(torch.bfloat16).cuda()
    rng = np.random.default_rng(3)
    w_bits = rand_weight(rng, D, code, kind)
    w = to_gpu(w_bits, code)
    got = pq.head_rmsnorm(x.view(rows_n, 1, D), w, EPS, kind).view(rows_n, D)
    assert torch.equal(got, pq.rmsnorm_quantize(x, w, EPS, return_h=True)[1])
    pick = np.array(sorted({0, 1, 2, 65535, 65536, *range(262136, rows_n)} | set(rng.choice(rows_n, 2048, replace=False).tolist())))
    idx = torch.from_numpy(pick).cuda()
    same_bits(bits(got[idx]), spec(bits(x[idx]), w_bits, EPS, code, kind), code, "sampled rows")


# ---------------------------------------------------------------------------------------------------------------- 6. eager closeness
# Measured by this test on an MI355X (the figures stand in the docstring of the test).  The bound on the differing share is four times the measured share (seed-to-seed spread);
# the reference is the eager module, never the kernel under test.
MEASURED_SHARE = {"qwen3": 4.0e-6, "gemma3": 5.7e-6}


@pytest.mark.parametrize("family", ["qwen3", "gemma3"])
def test_eager_closeness_at_head_dim_128(family):
    """K1hn against transformers' Qwen3RMSNorm / Gemma3RMSNorm run eagerly on the same GPU, >= 10^7 bf16 elements at D = 128 in the layout of the q slice of a fused
    q/k/v output (32 heads, 8 kv heads).  No element may differ by more than 2 ulp (the project's standing condition for its norms); the share of differing elements
    is held to four times what this test measured on an MI355X.
    Measured by this test on an MI355X (1.05e7 elements each): Qwen3RMSNorm 42 stored activations differ (4.0e-6), max 2 ulp; Gemma3RMSNorm 60 differ (5.7e-6), max
    1 ulp.  The bounds are therefore 1.6e-5 and 2.3e-5."""
    import protoquant_amd as pq
    tr = pytest.importorskip("transformers")
    if family == "qwen3":
        mod = pytest.importorskip("transformers.models.qwen3.modeling_qwen3")
        cls, kind, mean = mod.Qwen3RMSNorm, "llama", 1.0
    else:
        mod = pytest.importorskip("transformers.models.gemma3.modeling_gemma3")
        cls, kind, mean = mod.Gemma3RMSNorm, "gemma", 0.0
    del tr
    D, H, Hkv, eps = 128, 32, 8, 1e-6
    width = (H + 2 * Hkv) * D
    tokens_total = -(-10_500_000 // (H * D))
    g = torch.Generator().manual_seed(900 + D)
    norm = cls(D, eps=eps).to(torch.bfloat16).cuda()
    with torch.no_grad():
        norm.weight.copy_((mean + 0.3 * torch.randn(D, generator=g)).to(torch.bfloat16))
    w = norm.weight.detach()
    n = dh = max_ulp = done = 0
    while done < tokens_total:
        t = min(512, tokens_total - done)
        scale = torch.exp(torch.empty(t, 1).uniform_(float(np.log(0.05)), float(np.log(20.0)), generator=g))
        qkv = (torch.randn(t, width, generator=g) * scale).to(torch.bfloat16).cuda()
        x = qkv[:, :H * D].view(1, t, H, D)
        with torch.no_grad():
            h_t = norm(x)                                   # the eager chain on the GPU
        h = pq.head_rmsnorm(x, w, eps, kind)                # K1hn through the C-ABI
        hb, hb_t = h.view(torch.int16).to(torch.int32), h_t.contiguous().view(torch.int16).to(torch.int32)
        diff = hb != hb_t
        dh += int(diff.sum())
        if bool(diff.any()):          # same-sign neighbours of a 16-bit float format differ by 1 in the bit pattern per ulp
            max_ulp = max(max_ulp, int((hb[diff] - hb_t[diff]).abs().max()))
        n += t * H * D
        done += t
    assert n >= 10_000_000
    print(f"{family} D={D}: {n} elements, stored activations differing {dh} ({dh / n:.3e}), max {max_ulp} ulp")
    assert max_ulp <= 2
    assert dh / n <= 4 * MEASURED_SHARE[family], (dh, n, MEASURED_SHARE[family])
