"""-m gpu: the grouped int8 qlinear (pq_qlinear_s8_grouped, one launch over all experts of a mixture-of-experts layer) — every comparison bit for bit, against the C oracle
per expert at small shapes and against the per-expert loop of pq.qlinear_s8 at real ones."""
import numpy as np
import pytest
import torch

from tests.gpu_util import TD, bits, same, same_f, to_gpu

pytestmark = pytest.mark.gpu
TILES = ("64x128", "64x64")


def _operands(rng, counts, N, K, code, bias, x_rows=None, gather=False, tail=0):
    """Seeded operands of one grouped problem: counts[e] rows per expert, `tail` rows past offsets[E]."""
    E = len(counts)
    M = int(sum(counts)) + tail
    T = x_rows if x_rows is not None else M
    xq = rng.integers(-128, 128, (T, K), dtype=np.int8)
    idx = rng.integers(0, T, M).astype(np.int32) if gather else None
    xs = (rng.random(M, dtype=np.float32) * 0.02 + 1e-3).astype(np.float32)
    wq = rng.integers(-128, 128, (E, N, K), dtype=np.int8)
    ws = (rng.random((E, N), dtype=np.float32) * 0.01 + 1e-4).astype(np.float32)
    b = None
    if bias and code is not None:
        b = rng.standard_normal((E, N)).astype(np.float32)
        if code != 2:
            b = bits(torch.from_numpy(b).to(TD[code]))          # (half types travel as their bit patterns: gpu_util.to_gpu)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return dict(xq=xq, idx=idx, xs=xs, wq=wq, ws=ws, bias=b, off=off, E=E, M=M, N=N, K=K, code=code)


def _launch(pq, p, out=None):
    """the grouped call on the GPU; code None = the int32 twin"""
    xq, wq, off = (torch.from_numpy(p[k]).cuda() for k in ("xq", "wq", "off"))
    idx = torch.from_numpy(p["idx"]).cuda() if p["idx"] is not None else None
    if p["code"] is None:
        return pq.int_mm_grouped(xq, wq, off, row_index=idx, out=out)
    bias = to_gpu(p["bias"], p["code"]) if p["bias"] is not None else None
    return pq.qlinear_s8_grouped(xq, torch.from_numpy(p["xs"]).cuda(), wq, torch.from_numpy(p["ws"]).cuda(), bias, off, TD[p["code"]], row_index=idx, out=out)


def _oracle(p):
    """per expert through oracle.c_oracle on the row slices; rows >= offsets[E] are not part of it"""
    from oracle import c_oracle as C
    rows = p["xq"][p["idx"]] if p["idx"] is not None else p["xq"]
    outs = []
    for e in range(p["E"]):
        lo, hi = int(p["off"][e]), int(p["off"][e + 1])
        if hi == lo:
            continue
        if p["code"] is None:
            outs.append(C.gemm_s8s8s32(rows[lo:hi], p["wq"][e]))
        else:
            outs.append(C.qlinear_s8(rows[lo:hi], p["xs"][lo:hi], p["wq"][e], p["ws"][e], p["bias"][e] if p["bias"] is not None else None, p["code"]))
    return np.concatenate(outs) if outs else np.zeros((0, p["N"]))


def _check_oracle(pq, p, what):
    got = _launch(pq, p)
    torch.cuda.synchronize()
    want = _oracle(p)
    n = int(p["off"][-1])
    if p["code"] is None:
        same(got[:n], want, what)
    else:
        same_f(got[:n], want, p["code"], what)


def test_smallest_case_against_oracle():
    """E = 1, one 64 x 64 tile, K = 128: the first thing to run on a new build"""
    import protoquant_amd as pq
    p = _operands(np.random.default_rng(1), [64], 64, 128, 0, False)
    _check_oracle(pq, p, "E=1 64x64x128")


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("E", (1, 3, 8))
def test_small_shapes_against_oracle(E, tile, pq_opt):
    import protoquant_amd as pq
    pq_opt("PQ_GROUPED_TILE", tile)
    rng = np.random.default_rng(100 + E)
    for K in (128, 384):
        for N in (64, 80, 200, 1000):
            for code in (0, 1, 2, None):
                for bias in ((False, True) if code is not None else (False,)):
                    counts = rng.integers(0, 150, E)
                    p = _operands(rng, counts, N, K, code, bias)
                    _check_oracle(pq, p, f"E={E} K={K} N={N} code={code} bias={bias} counts={counts.tolist()} tile={tile}")


def _per_expert_loop(pq, xq, xs, wq, ws, bias, off, dtype):
    outs = []
    for e in range(wq.shape[0]):
        lo, hi = int(off[e]), int(off[e + 1])
        if hi > lo:
            outs.append(pq.qlinear_s8(xq[lo:hi], xs[lo:hi], wq[e], ws[e], bias[e] if bias is not None else None, dtype))
    return torch.cat(outs)


def _routing_counts(rng, E, M, kind):
    if kind == "balanced":
        c = np.full(E, M // E)
        c[: M - c.sum()] += 1
        return c
    w = 1.0 / np.arange(1, E + 1) ** 1.2
    return np.bincount(rng.choice(E, size=M, p=w / w.sum()), minlength=E)


@pytest.mark.parametrize("E,M,N,K,kind", [(8, 8192, 28672, 4096, "skewed"), (8, 8192, 4096, 14336, "balanced"),
                                          (128, 32768, 1536, 2048, "skewed"), (128, 32768, 2048, 768, "balanced"), (4, 700, 50257, 256, "skewed")])
def test_real_sizes_against_per_expert_loop(E, M, N, K, kind):
    """Mixtral 8 x 7B (E = 8, k = 2, 4096 tokens), 128 small experts (k = 8) and a 50 257-wide output (odd leading dimension: element-aligned staged stores)"""
    import protoquant_amd as pq
    g = torch.Generator(device="cuda").manual_seed(E * 1000 + N)
    rng = np.random.default_rng(E + N)
    off = np.concatenate([[0], np.cumsum(_routing_counts(rng, E, M, kind))]).astype(np.int32)
    xq = torch.randint(-128, 128, (M, K), generator=g, device="cuda", dtype=torch.int8)
    wq = torch.randint(-128, 128, (E, N, K), generator=g, device="cuda", dtype=torch.int8)
    xs = torch.rand(M, generator=g, device="cuda") * 0.02 + 1e-3
    ws = torch.rand(E, N, generator=g, device="cuda") * 0.01 + 1e-4
    bias = torch.randn(E, N, generator=g, device="cuda").to(torch.bfloat16) if N == 50257 else None
    got = pq.qlinear_s8_grouped(xq, xs, wq, ws, bias, torch.from_numpy(off).cuda(), torch.bfloat16)
    want = _per_expert_loop(pq, xq, xs, wq, ws, bias, off, torch.bfloat16)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{int((got.view(torch.int16) != want.view(torch.int16)).sum())} elements differ"


SPLITS = {
    "one row each": [1] * 8,
    "63/64/65/127/129": [63, 64, 65, 127, 129],
    "empty at start, middle, end": [0, 0, 70, 0, 3, 130, 0, 0],
    "one expert owns every row": [0, 0, 300, 0],
    "tail rows past offsets[E]": [40, 90, 5],
}


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", sorted(SPLITS))
def test_row_bounds_and_untouched_output(name, tile, pq_opt):
    """y pre-filled with a sentinel: rows >= offsets[E] and the padding columns up to ldy must still hold it"""
    import protoquant_amd as pq
    pq_opt("PQ_GROUPED_TILE", tile)
    rng = np.random.default_rng(7)
    for code, N, pad in ((0, 200, 8), (2, 72, 5), (None, 129, 3), (1, 64, 0)):
        tail = 37 if name.startswith("tail") else 0
        p = _operands(rng, SPLITS[name], N, 256, code, code == 0, tail=tail)
        dt = torch.int32 if code is None else TD[code]
        full = torch.full((p["M"], N + pad), 12345 if code is None else -777.0, dtype=dt, device="cuda")
        sentinel = full.clone()
        _launch(pq, p, out=full[:, :N])
        torch.cuda.synchronize()
        n = int(p["off"][-1])
        want = _oracle(p)
        (same if code is None else (lambda a, b, w: same_f(a, b, code, w)))(full[:n, :N], want, f"{name} code={code}")
        assert torch.equal(full[n:], sentinel[n:]), f"{name}: rows past offsets[E] were written"
        assert torch.equal(full[:, N:], sentinel[:, N:]), f"{name}: padding columns were written"


@pytest.mark.parametrize("tile", TILES)
def test_one_expert_equals_qlinear_s8(tile, pq_opt):
    import protoquant_amd as pq
    pq_opt("PQ_GROUPED_TILE", tile)
    g = torch.Generator(device="cuda").manual_seed(3)
    for (M, N, K) in ((300, 520, 512), (64, 4096, 1024), (1000, 136, 128)):
        xq = torch.randint(-128, 128, (M, K), generator=g, device="cuda", dtype=torch.int8)
        wq = torch.randint(-128, 128, (1, N, K), generator=g, device="cuda", dtype=torch.int8)
        xs, ws = torch.rand(M, generator=g, device="cuda") * 0.02, torch.rand(1, N, generator=g, device="cuda") * 0.01
        bias = torch.randn(1, N, generator=g, device="cuda").to(torch.float16)
        off = torch.tensor([0, M], dtype=torch.int32, device="cuda")
        got = pq.qlinear_s8_grouped(xq, xs, wq, ws, bias, off, torch.float16)
        want = pq.qlinear_s8(xq, xs, wq[0], ws[0], bias[0], torch.float16)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (M, N, K, tile)
        assert torch.equal(pq.int_mm_grouped(xq, wq, off), pq.int_mm(xq, wq[0])), (M, N, K, tile)


@pytest.mark.parametrize("tile", TILES)
def test_row_index_equals_pregathered_codes(tile, pq_opt):
    import protoquant_amd as pq
    pq_opt("PQ_GROUPED_TILE", tile)
    rng = np.random.default_rng(11)
    for code in (0, 2, None):
        p = _operands(rng, [100, 0, 37, 200, 1], 264, 384, code, True, x_rows=90, gather=True)      # 338 grouped rows over 90 source rows: many repeats
        got = _launch(pq, p)
        q = dict(p, xq=p["xq"][p["idx"]], idx=None)
        want = _launch(pq, q)
        assert torch.equal(got.view(torch.int32) if got.element_size() == 4 else got.view(torch.int16),
                           want.view(torch.int32) if want.element_size() == 4 else want.view(torch.int16)), code
        _check_oracle(pq, p, f"row_index code={code}")


def test_graph_replays_follow_the_offsets_in_device_memory():
    """a hipGraph captured ONCE, after another graph, and replayed alongside it for three routings written into the SAME offsets / row_index buffers"""
    import protoquant_amd as pq
    E, T, k, N, K = 8, 96, 2, 200, 256
    M = T * k
    g = torch.Generator(device="cuda").manual_seed(5)
    xq = torch.randint(-128, 128, (T, K), generator=g, device="cuda", dtype=torch.int8)
    wq = torch.randint(-128, 128, (E, N, K), generator=g, device="cuda", dtype=torch.int8)
    xs, ws = torch.rand(M, generator=g, device="cuda") * 0.02, torch.rand(E, N, generator=g, device="cuda") * 0.01
    off = torch.zeros(E + 1, dtype=torch.int32, device="cuda")
    idx = torch.zeros(M, dtype=torch.int32, device="cuda")
    y = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
    a = torch.randint(-128, 128, (256, 256), generator=g, device="cuda", dtype=torch.int8)
    acc = torch.zeros(256, 256, dtype=torch.int32, device="cuda")

    def routing(seed):
        rng = np.random.default_rng(seed)
        counts = np.bincount(rng.integers(0, E, M), minlength=E) if seed != 2 else np.array([0, M, 0, 0, 0, 0, 0, 0])
        return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), rng.integers(0, T, M).astype(np.int32)

    o0, i0 = routing(0)
    off.copy_(torch.from_numpy(o0)); idx.copy_(torch.from_numpy(i0))
    pq.qlinear_s8_grouped(xq, xs, wq, ws, None, off, torch.bfloat16, row_index=idx, out=y)      # warm-up outside capture
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    other, graph = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(other, stream=s):
            acc.copy_(pq.int_mm(a, a))
        with torch.cuda.graph(graph, stream=s):
            pq.qlinear_s8_grouped(xq, xs, wq, ws, None, off, torch.bfloat16, row_index=idx, out=y)
    want_acc = pq.int_mm(a, a)
    for seed in (1, 2, 3):
        o, i = routing(seed)
        off.copy_(torch.from_numpy(o)); idx.copy_(torch.from_numpy(i))
        y.zero_()
        torch.cuda.synchronize()
        other.replay(); graph.replay(); other.replay()
        torch.cuda.synchronize()
        want = _per_expert_loop(pq, xq[idx.long()], xs, wq, ws, None, o, torch.bfloat16)
        assert torch.equal(y.view(torch.int16), want.view(torch.int16)), f"replay for routing {seed} differs"
        assert torch.equal(acc, want_acc)


def test_seeded_fuzz():
    """200 random (E, split, N, K, dtype, bias, index, tile) draws in one process"""
    import protoquant_amd as pq
    from protoquant_amd import _lib
    rng = np.random.default_rng(2024)
    try:
        for it in range(200):
            E = int(rng.choice([1, 2, 5, 8, 17, 64, 130]))
            style = int(rng.integers(0, 3))
            counts = rng.integers(0, 90, E) if style == 0 else (rng.integers(0, 3, E) if style == 1 else rng.integers(0, 2, E) * rng.integers(1, 260, E))
            N, K = int(rng.integers(1, 400)), int(rng.choice([128, 256, 640]))
            code = [0, 1, 2, None][int(rng.integers(0, 4))]
            gather = bool(rng.integers(0, 2))
            _lib.set_option("PQ_GROUPED_TILE", ["", "64x128", "64x64"][int(rng.integers(0, 3))])
            p = _operands(rng, counts, N, K, code, bool(rng.integers(0, 2)), x_rows=int(rng.integers(1, 300)) if gather else None, gather=gather, tail=int(rng.integers(0, 2)) * 9)
            if p["M"] == 0:
                continue
            _check_oracle(pq, p, f"fuzz draw {it}: E={E} counts={counts.tolist()} N={N} K={K} code={code} gather={gather}")
    finally:
        _lib.set_option("PQ_GROUPED_TILE", "")


def test_nan_and_inf_rows_stay_in_their_expert():
    """QSPEC: a NaN (Inf) row scale gives a NaN output row — that row only"""
    import protoquant_amd as pq
    rng = np.random.default_rng(9)
    p = _operands(rng, [70, 30, 64], 136, 128, 2, True)
    p["xs"][75] = np.float32("nan")
    p["xs"][140] = np.float32("inf")
    p["xq"][140] = 0
    got = _launch(pq, p)
    torch.cuda.synchronize()
    same_f(got, _oracle(p), 2, "NaN / Inf rows")
    nan_rows = torch.isnan(got).all(dim=1).cpu().numpy()
    assert nan_rows[75] and nan_rows[140] and nan_rows.sum() == 2, np.flatnonzero(nan_rows)
