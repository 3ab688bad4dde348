"""-m gpu: int4 weights (QSPEC W1-W4; w4_pack_kernels.hip, gemm_w4_stream.hip).  No tolerance anywhere: the packer and the expansion against tests/w4_spec.py byte for
byte, the int32 form of the streaming GEMM against an int64 matmul on the CPU by the spec's W8, the float forms against the library's own int8 path (qlinear_s8) on
w4_expand's output, the module against a qlinear that holds the expanded weight."""
import numpy as np
import pytest
import torch

from tests import w4_spec as S

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _designed(N, K):
    """group gi = n G + j of the padded weight has the maximum a = (gi + 77) % 128 and walks w = -a .. a from a start that moves with gi // 128: over 37 x 9 groups
    every a occurs, and every w under it"""
    G = S.round_k(K) // 128
    gi = np.arange(N * G).reshape(N, G, 1)
    a = (gi + 77) % 128
    w = (np.arange(128) + 128 * (gi // 128)) % (2 * a + 1) - a
    return w.reshape(N, G * 128)[:, :K].astype(np.int8)


@pytest.mark.parametrize("N", [1, 5, 37])
@pytest.mark.parametrize("K", [128, 200, 1152])
def test_pack_and_expand_are_the_spec(N, K):
    import protoquant_amd as pq
    wq = _designed(N, K)
    big = torch.full((N, K + 24), 55, dtype=torch.int8, device=DEV)          # a pitched wq: the packer may not read past K
    big[:, :K] = torch.from_numpy(wq).to(DEV)
    w4, gs = pq.w4_pack(big[:, :K])
    w4_want, gs_want = S.pack(wq)
    assert np.array_equal(w4.cpu().numpy(), w4_want), "w4 (the zero tail included)"
    assert np.array_equal(gs.cpu().numpy(), gs_want), "gs (the rows past N included)"
    assert np.array_equal(pq.w4_expand(w4, gs).cpu().numpy(), S.expand(w4_want, gs_want))
    assert np.array_equal(pq.w4_expand(w4, gs, K).cpu().numpy(), S.expand(w4_want, gs_want)[:, :K])


def _operands(pattern, M, N, G, seed):
    """(xq, wq) int8 on the CPU.  "random": seeded codes, every group of the weight under an amplitude of its own (so the multipliers differ).  "extreme": x = +-127 and
    w = +-126 (q = +-7, g = 18) in the even groups, +-7 (g = 1) in the odd ones, signs u[n] v[k] and t[m] v[k]: every product of a group has ONE sign, its sum reaches
    the bound 128 * 127 * 126 — a lost shift, a 24-bit overflow or swapped nibbles (v[k] against v[k + 64]) change it."""
    rng = np.random.default_rng(seed)
    Kp = G * 128
    if pattern == "random":
        amp = rng.integers(0, 128, (N, G, 1))
        wq = (rng.integers(-127, 128, (N, G, 128)) * amp // 127).reshape(N, Kp)
        return rng.integers(-128, 128, (M, Kp)).astype(np.int8), wq.astype(np.int8)
    u, t, v = (rng.integers(0, 2, n) * 2 - 1 for n in (N, M, Kp))
    mag = np.where((np.arange(Kp) // 128) % 2 == 0, 126, 7)
    return (127 * t[:, None] * v[None, :]).astype(np.int8), (u[:, None] * (mag * v)[None, :]).astype(np.int8)


# M x N x groups x PQ_SKINNY_KS, paired: every M, N, group count and split occurs; ks = 16 with 1 group and ks = 8 with 5 are more waves than groups
CASES = [(1, 37, 1, 16), (2, 272, 2, None), (16, 1, 3, 1), (17, 37, 5, 8), (33, 272, 9, 4), (64, 37, 43, 2), (1, 272, 43, None), (64, 272, 9, 16)]


@pytest.mark.parametrize("pattern", ["random", "extreme"])
@pytest.mark.parametrize("M,N,G,ks", CASES)
def test_streaming_gemm_is_the_int8_gemm_on_the_expanded_weight(pq_opt, pattern, M, N, G, ks):
    import protoquant_amd as pq
    Kp = G * 128
    xq_h, wq_h = _operands(pattern, M, N, G, seed=M * 1000 + N)
    w8_h = S.expand(*S.pack(wq_h))
    xbig = torch.full((M, Kp + 64), 99, dtype=torch.int8, device=DEV)          # xq and w4 as prefix views of wider buffers
    xbig[:, :Kp] = torch.from_numpy(xq_h).to(DEV)
    xq = xbig[:, :Kp]
    w4_c, gs = pq.w4_pack(torch.from_numpy(wq_h).to(DEV))
    wbig = torch.full((N, Kp // 2 + 32), 0x88, dtype=torch.uint8, device=DEV)
    wbig[:, :Kp // 2] = w4_c
    w4 = wbig[:, :Kp // 2]
    if ks is not None:
        pq_opt("PQ_SKINNY_KS", ks)
    acc = pq.int_mm_w4(xq, w4, gs)
    want = xq_h.astype(np.int64) @ w8_h.astype(np.int64).T
    assert np.abs(want).max() < 2 ** 31 and np.array_equal(acc.cpu().numpy().astype(np.int64), want), "int32 accumulator"
    w8 = pq.w4_expand(w4, gs)
    g = torch.Generator(device=DEV).manual_seed(M + N)
    xs, ws = torch.rand(M, device=DEV, generator=g) * 0.02 + 1e-3, torch.rand(N, device=DEV, generator=g) * 0.01 + 1e-4
    for kind in (torch.bfloat16, torch.float16, torch.float32):
        for bias in (None, torch.randn(N, device=DEV, generator=g).to(kind)):
            ybig = torch.full((M + 2, N + 5), 77, dtype=torch.float32, device=DEV).to(kind)      # y as an interior view: odd N, odd ldy, unaligned rows
            y = pq.qlinear_w4(xq, xs, w4, gs, ws, bias, kind, out=ybig[1:M + 1, :N])
            ref = pq.qlinear_s8(xq, xs, w8, ws, bias, kind)
            assert torch.equal(y.contiguous().view(torch.uint8), ref.view(torch.uint8)), (kind, bias is not None)
            ybig[1:M + 1, :N] = 77
            assert bool((ybig == 77).all()), "a store outside y"


@pytest.mark.parametrize("hidden", [320, 256])
def test_module(hidden):
    import protoquant_amd as pq
    from protoquant_amd.qlinear import is_code_fed
    torch.manual_seed(hidden)
    lin = torch.nn.Linear(hidden, 72, bias=True, dtype=torch.bfloat16).to(DEV)
    m = pq.QLinearW4.from_linear(lin)
    ref = pq.qlinear.from_linear(lin)
    assert torch.equal(m.ws, ref.ws) and not hasattr(m, "wq") and not is_code_fed(m)
    w4_want, gs_want = S.pack(ref.wq.cpu().numpy())
    assert np.array_equal(m.w4.cpu().numpy(), w4_want) and np.array_equal(m.gs.cpu().numpy(), gs_want), "from_linear: the level-1 codes of qlinear.from_linear, packed"
    ref.wq = pq.w4_expand(m.w4, m.gs, hidden).contiguous()          # the twin: a qlinear that holds the expanded weight
    for rows in (3, 80):                                             # the streaming kernel; expand + tiles
        x = torch.randn(2, rows, hidden, device=DEV).to(torch.bfloat16)[0]
        want = ref(x)
        assert torch.equal(m(x).view(torch.int16), want.view(torch.int16)), rows
        assert torch.equal(m(pq.quantize(x)).view(torch.int16), want.view(torch.int16)), (rows, "QTensor")
        m.stream_rows = 0
        assert torch.equal(m(x).view(torch.int16), want.view(torch.int16)), (rows, "stream_rows = 0")
        m.stream_rows = 64
    m2 = pq.QLinearW4(hidden, 72, bias=True, device=DEV)
    m2.load_state_dict(m.state_dict())
    assert sorted(m.state_dict()) == ["bias", "gs", "w4", "ws"] and torch.equal(m2(x).view(torch.int16), want.view(torch.int16)), "state_dict round trip"


def test_swap_linears_w4_counts_and_is_idempotent():
    import protoquant_amd as pq
    from protoquant_amd.qlinear import is_code_fed
    model = torch.nn.Sequential(torch.nn.Linear(128, 64, dtype=torch.bfloat16), torch.nn.SiLU(),
                                torch.nn.Sequential(torch.nn.Linear(64, 32, dtype=torch.bfloat16), torch.nn.Linear(32, 16, dtype=torch.bfloat16))).to(DEV)
    assert pq.swap_linears_w4(model, predicate=lambda name, mod: mod.in_features != 32) == 2 and pq.swap_linears_w4(model, predicate=lambda name, mod: mod.in_features != 32) == 0
    assert isinstance(model[0], pq.QLinearW4) and isinstance(model[2][0], pq.QLinearW4) and type(model[2][1]) is torch.nn.Linear and not is_code_fed(model[0])
    pq.swap_linears(model)
    assert type(model[2][1]) is pq.qlinear and isinstance(model[0], pq.QLinearW4)
    assert model(torch.randn(5, 128, device=DEV).to(torch.bfloat16)).shape == (5, 16)
