"""-m gpu: int4 expert weights at decode (gemm_w4_grouped_stream.hip, w4.py's grouped entries).  No tolerance anywhere: the int32 form against an int64 matmul per
expert on the spec's W8 (tests/w4_spec.py), the float forms against the library's own int8 grouped streaming kernel on the stacked w4_expand outputs, the modules
against twins that hold the expanded weights."""
import numpy as np
import pytest
import torch

from tests import w4_spec as S

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _operands(pattern, R, E, N, G, rng):
    """(xq [R, Kp], wq [E, N, Kp]) int8 on the CPU.  "random": every group of the weight under an amplitude of its own (so the multipliers differ).  "extreme": x = +-127,
    w = +-126 (q = +-7, g = 18) in the even groups and +-7 (g = 1) in the odd ones, signs u[e, n] v[k] and t[m] v[k]: every product of a group has ONE sign, its sum
    reaches the bound 128 * 127 * 126 — a lost shift, a 24-bit overflow or swapped nibbles change it."""
    Kp = G * 128
    if pattern == "random":
        amp = rng.integers(0, 128, (E, N, G, 1))
        wq = (rng.integers(-127, 128, (E, N, G, 128)) * amp // 127).reshape(E, N, Kp)
        return rng.integers(-128, 128, (R, Kp)).astype(np.int8), wq.astype(np.int8)
    u, t, v = rng.integers(0, 2, (E, N, 1)) * 2 - 1, rng.integers(0, 2, (R, 1)) * 2 - 1, rng.integers(0, 2, Kp) * 2 - 1
    mag = np.where((np.arange(Kp) // 128) % 2 == 0, 126, 7)
    return (127 * t * v).astype(np.int8), (u * (mag * v)).astype(np.int8)


def _sparse(E, live):
    c = [0] * E
    for e, n in live.items():
        c[e] = n
    return c


# (rows per expert, N, groups, PQ_GROUPED_STREAM_KS, gather).  M_total 64 / 36 / 52: MT = 4 with the bodies 1-direct, 1-staged, 2 / 3 / 4; 8: MT = 1; 21 and 22: MT = 2.
# E = 70 and 300: live experts beyond the 64- and 256-expert steps of the slot search.  ks = 16 with 1 group and ks = 8 with 5: more waves than groups.
CASES = [([0, 1, 0, 2, 16, 17, 0, 28], 37, 3, None, True), ([33, 3], 272, 5, 8, False), ([1, 49, 0, 2], 37, 9, 1, True), ([2, 0, 1, 5], 1, 1, 16, False),
         ([17, 1, 3], 272, 9, None, True), (_sparse(70, {3: 1, 66: 2, 69: 1}), 37, 1, None, False), (_sparse(300, {5: 1, 70: 3, 260: 17, 299: 1}), 1, 3, 16, True)]


@pytest.mark.parametrize("pattern", ["random", "extreme"])
@pytest.mark.parametrize("counts,N,G,ks,gather", CASES)
def test_grouped_streaming_gemm_is_the_int8_grouped_gemm_on_the_expanded_weights(pq_opt, pattern, counts, N, G, ks, gather):
    import protoquant_amd as pq
    E, M, Kp = len(counts), sum(counts), G * 128
    rng = np.random.default_rng(M * 1000 + N + E)
    R = M // 2 + 3 if gather else M                                             # gather: x_rows != M_total, and a source row read twice
    xq_h, wq_h = _operands(pattern, R, E, N, G, rng)
    packed = [S.pack(w) for w in wq_h]
    w8_h = np.stack([S.expand(*p) for p in packed])
    idx_h = rng.integers(0, R, M)
    idx_h[1] = idx_h[0]
    src = idx_h if gather else np.arange(M)
    off_h = np.concatenate([[0], np.cumsum(counts)])
    xq = torch.from_numpy(xq_h).to(DEV)
    w4, gs = (torch.from_numpy(np.stack(a)).to(DEV) for a in zip(*packed))
    offsets = torch.from_numpy(off_h.astype(np.int32)).to(DEV)
    row_index = torch.from_numpy(idx_h.astype(np.int32)).to(DEV) if gather else None
    if ks is not None:
        pq_opt("PQ_GROUPED_STREAM_KS", ks)
    acc = pq.int_mm_w4_grouped(xq, w4, gs, offsets, row_index).cpu().numpy().astype(np.int64)
    for e in np.nonzero(counts)[0]:
        lo, hi = off_h[e], off_h[e + 1]
        want = xq_h[src[lo:hi]].astype(np.int64) @ w8_h[e].astype(np.int64).T
        assert np.abs(want).max() < 2 ** 31 and np.array_equal(acc[lo:hi], want), ("int32 accumulator", e)
    w8 = torch.stack([pq.w4_expand(w4[e], gs[e]) for e in range(E)])
    assert np.array_equal(w8.cpu().numpy(), w8_h)
    g = torch.Generator(device=DEV).manual_seed(M + N)
    xs, ws = torch.rand(M, device=DEV, generator=g) * 0.02 + 1e-3, torch.rand((E, N), device=DEV, generator=g) * 0.01 + 1e-4
    short = offsets.clone()
    short[-1] -= 1                                                              # the last grouped row belongs to nobody: it is not written
    for kind in (torch.bfloat16, torch.float16, torch.float32):
        for bias in (None, torch.randn((E, N), device=DEV, generator=g).to(kind)):
            ybig = torch.full((M + 2, N + 5), 77, dtype=torch.float32, device=DEV).to(kind)      # y as an interior view: odd N, odd ldy, unaligned rows
            y = pq.qlinear_w4_grouped(xq, xs, w4, gs, ws, bias, short, kind, row_index=row_index, out=ybig[1:M + 1, :N])
            ref = pq.qlinear_s8_grouped_stream(xq, xs, w8, ws, bias, offsets, kind, row_index=row_index)
            assert torch.equal(y[:M - 1].contiguous().view(torch.uint8), ref[:M - 1].view(torch.uint8)), (kind, bias is not None)
            ybig[1:M, :N] = 77
            assert bool((ybig == 77).all()), "a store outside y, or into a row >= offsets[E]"


@pytest.mark.parametrize("hidden", [256, 320])
def test_modules_and_swap(hidden):
    import protoquant_amd as pq
    torch.manual_seed(hidden)
    E, inter = 4, 136
    gu, dn = (torch.randn(s, device=DEV).to(torch.bfloat16) for s in ((E, 2 * inter, hidden), (E, hidden, inter)))
    model, twin = (torch.nn.ModuleDict({"mlp": pq.MoEGatedMLP.from_stacked(gu, dn)}) for _ in range(2))
    src = model["mlp"].down
    assert pq.swap_moe_experts_w4(model, predicate=lambda name, mod: name != "mlp") == 0
    assert pq.swap_moe_experts_w4(model) == 1 and pq.swap_moe_experts_w4(model) == 0
    for name in ("gate_up", "down"):
        m, t = getattr(model["mlp"], name), getattr(twin["mlp"], name)
        assert isinstance(m, pq.GroupedQLinearW4) and not hasattr(m, "wq") and sorted(m.state_dict()) == ["gs", "w4", "ws"]
        for e in range(E):                                                      # per expert the spec's bytes, the gs rows past N (136 % 4 == 0, 272 and hidden too) and K padding included
            w4_want, gs_want = S.pack(t.wq[e].cpu().numpy())
            assert np.array_equal(m.w4[e].cpu().numpy(), w4_want) and np.array_equal(m.gs[e].cpu().numpy(), gs_want), (name, e)
        t.wq = torch.stack([pq.w4_expand(m.w4[e], m.gs[e], t.in_features) for e in range(E)]).contiguous()      # the twin holds the expanded weights
    odd = pq.GroupedQLinearW4.from_weight(dn[:, :37])                           # N % 4 != 0: the stacked rows' quads are re-laid per expert
    for e in range(E):
        assert np.array_equal(odd.gs[e].cpu().numpy(), S.pack(src.wq[e, :37].cpu().numpy())[1]), e
    m2 = pq.GroupedQLinearW4(E, inter, hidden, device=DEV)
    m2.load_state_dict(model["mlp"].down.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), model["mlp"].down.state_dict().values()))
    for T in (3, 40):                                                           # 6 grouped rows: the streaming kernel; 80: expand + tiles
        x = torch.randn(T, hidden, device=DEV).to(torch.bfloat16)
        ids = torch.rand(T, E, device=DEV).topk(2, dim=-1).indices
        w = torch.rand(T, 2, device=DEV).to(torch.bfloat16)
        want = twin["mlp"](x, ids, w)
        for rows in (64, 0):
            model["mlp"].gate_up.stream_rows = model["mlp"].down.stream_rows = rows
            assert torch.equal(model["mlp"](x, ids, w).view(torch.int16), want.view(torch.int16)), (T, rows)
