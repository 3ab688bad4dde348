"""-m gpu: the promises of the grouped int8 qlinear (gemm_s8_grouped.hip, pq_qlinear_s8_grouped) that tests/test_gpu_grouped.py does not hold it to: the K rotation
between the m-tiles of one expert (PQ_GROUPED_ROT=1), strided operands (ldx, ldw, w_expert_stride, ldy), the clamps on untrusted `offsets` and `row_index`, operands
past 2^31, and decode-sized routing up to the documented maximum of 1024 experts.  Every comparison is bit for bit against the C oracle per expert.

The out-of-range test checks a clamp BY ITS RESULT and is built so that no outcome can leave the allocations: every operand the bad values could steer an access
into is an interior view of a larger buffer whose margins are wider than the largest excursion used."""
import numpy as np
import pytest
import torch

from tests.gpu_util import TD, bits, same, same_f, to_gpu
from tests.test_gpu_grouped import TILES, _launch, _operands, _oracle

pytestmark = pytest.mark.gpu
KINDS = (0, 1, 2, None)                  # bf16, fp16, f32, the int32 twin


def _check(got, want, code, what):
    if code is None:
        same(got, want, what)
    else:
        same_f(got, want, code, what)


# ---------------------------------------------------------------- PQ_GROUPED_ROT=1
# The rotation acts between the m-tiles of ONE expert (rot_div = min(its m-tiles, 8)): an expert needs at least 65 rows.  The launcher sizes the chunk for the average
# expert — here 1543 rows over 7 experts = 4 m-tiles -> rot_chunk_ktiles(4, TN) = 16 K-tiles on both tiles — so K = 128 x 5 is one short chunk rotated as a whole, 128 x 17
# leaves a last chunk of one K-tile and 128 x 37 one of five.
ROT_COUNTS = [0, 1, 64, 65, 200, 513, 700]


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("gather", (False, True))
@pytest.mark.parametrize("NT", (5, 17, 37))
def test_rotation_between_the_m_tiles_of_an_expert(pq_opt, tile, gather, NT):
    import protoquant_amd as pq
    pq_opt("PQ_GROUPED_TILE", tile)
    N, K = 200, 128 * NT
    assert max(ROT_COUNTS) > 8 * 64 and sorted(ROT_COUNTS)[3] == 65
    for code in KINDS:
        for bias in ((False, True) if code is not None else (False,)):
            rng = np.random.default_rng(NT * 100 + (code or 7) * 10 + bias)
            p = _operands(rng, ROT_COUNTS, N, K, code, bias, x_rows=900 if gather else None, gather=gather)
            want = _oracle(p)
            pq_opt("PQ_GROUPED_ROT", "")
            off = _launch(pq, p)
            pq_opt("PQ_GROUPED_ROT", "1")
            on = _launch(pq, p)
            what = f"tile {tile} gather {gather} K-tiles {NT} code {code} bias {bias}"
            _check(off, want, code, what + " (rotation off)")
            _check(on, want, code, what + " (PQ_GROUPED_ROT=1)")
            assert torch.equal(on.view(torch.uint8), off.view(torch.uint8)), what


def test_rotation_with_k_tile_indexed_codes(pq_opt):
    """activation codes that grow with the K-tile index against positive weights (as in test_gpu_k_rotation.py): a K-tile taken twice for one left out moves every sum"""
    import protoquant_amd as pq
    pq_opt("PQ_GROUPED_ROT", "1")
    N, K = 136, 128 * 37
    for tile in TILES:
        pq_opt("PQ_GROUPED_TILE", tile)
        p = _operands(np.random.default_rng(3), ROT_COUNTS, N, K, None, False)
        k = np.arange(K)
        p["xq"] = ((k // 128) % 120 + 1 + (np.arange(p["M"]) % 7)[:, None]).astype(np.int8)
        p["wq"] = np.broadcast_to((1 + (np.arange(N)[:, None] + k) % 5).astype(np.int8), (p["E"], N, K)).copy()
        same(_launch(pq, p), _oracle(p), f"K-tile pattern, tile {tile}")


# ---------------------------------------------------------------- strided operands
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("gather", (False, True))
def test_strided_operands_through_the_wrapper_without_a_copy(pq_opt, monkeypatch, tile, gather):
    """xq with ldx > K, wq as a slice of a larger [E, N + 3, K + 128] buffer (ldw and w_expert_stride both padded), out with a padded ldy: the bits of the contiguous call,
    the padding of out untouched — and the C-ABI really received the views' pointers and strides (a wrapper that quietly made contiguous copies would pass everything else)."""
    import protoquant_amd as pq
    from protoquant_amd import _lib
    pq_opt("PQ_GROUPED_TILE", tile)
    L = _lib.lib()
    counts, N, K = [70, 0, 129, 5, 300], 200, 384
    for code in KINDS:
        rng = np.random.default_rng(11 + (code or 5))
        p = _operands(rng, counts, N, K, code, code in (0, 2), x_rows=400 if gather else None, gather=gather)
        want = _oracle(p)
        dense = _launch(pq, p)
        _check(dense, want, code, f"contiguous operands, code {code}")
        E, M, T = p["E"], p["M"], p["xq"].shape[0]
        x_big = torch.full((T, K + 64), 99, dtype=torch.int8, device="cuda")
        x_big[:, :K] = torch.from_numpy(p["xq"]).cuda()
        w_big = torch.full((E, N + 3, K + 128), -99, dtype=torch.int8, device="cuda")
        w_big[:, :N, :K] = torch.from_numpy(p["wq"]).cuda()
        xv, wv = x_big[:, :K], w_big[:, :N, :K]
        odt = torch.int32 if code is None else TD[code]
        y_big = torch.full((M, N + 24), 77, dtype=torch.int32, device="cuda").to(odt)
        sentinel = y_big.clone()
        yv = y_big[:, :N]
        seen = {}
        name = "pq_gemm_s8s8s32_grouped" if code is None else "pq_qlinear_s8_grouped"
        real = getattr(L, name)

        def spy(*a, _real=real):
            seen["a"] = a
            return _real(*a)
        monkeypatch.setattr(L, name, spy)
        off_t = torch.from_numpy(p["off"]).cuda()
        idx_t = torch.from_numpy(p["idx"]).cuda() if gather else None
        if code is None:
            got = pq.int_mm_grouped(xv, wv, off_t, row_index=idx_t, out=yv)
            a = seen["a"]
            xq_ptr, ldx, wq_ptr, ldw, wstride, y_ptr, ldy = a[0], a[1], a[4], a[5], a[6], a[12], a[13]
        else:
            got = pq.qlinear_s8_grouped(xv, torch.from_numpy(p["xs"]).cuda(), wv, torch.from_numpy(p["ws"]).cuda(), to_gpu(p["bias"], code) if p["bias"] is not None else None,
                                        off_t, odt, row_index=idx_t, out=yv)
            a = seen["a"]
            xq_ptr, ldx, wq_ptr, ldw, wstride, y_ptr, ldy = a[0], a[1], a[5], a[6], a[7], a[15], a[16]
        monkeypatch.setattr(L, name, real)
        assert (xq_ptr, ldx) == (x_big.data_ptr(), K + 64), "xq was copied"
        assert (wq_ptr, ldw, wstride) == (w_big.data_ptr(), K + 128, (N + 3) * (K + 128)), "wq was copied"
        assert (y_ptr, ldy) == (y_big.data_ptr(), N + 24)
        assert got.data_ptr() == y_big.data_ptr()
        n = int(p["off"][-1])
        assert torch.equal(yv[:n].contiguous().view(torch.uint8), dense[:n].contiguous().view(torch.uint8)), f"strided operands differ from the contiguous call, code {code}"
        assert torch.equal(y_big[:, N:], sentinel[:, N:]), "the padding of out was written"


# ---------------------------------------------------------------- out-of-range device data
MARGIN = 128          # rows of margin on both sides of every operand a bad value could reach; the largest excursion below is 40 rows (offsets) / 100 rows (row_index)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("gather", (False, True))
def test_out_of_range_offsets_and_row_index_are_clamped(pq_opt, tile, gather):
    """What the header states: offsets outside [0, M_total] are clamped into it, indices into [0, x_rows) — "wrong results, never a wild access".  offsets carries a first
    entry of -5, a last entry 40 rows past M_total and a repeated value (an empty expert); row_index carries values in [x_rows, x_rows + 100).  No two experts claim a row.
    Expected: the oracle under the clamped values; every margin still holds its sentinel.
    Construction: xq, xs, row_index and y are interior views, MARGIN = 128 rows inside their allocations on both sides, so an access steered by the UNclamped values (rows
    -5 .. M_total + 39 of the grouped list, source rows up to x_rows + 99) would still land inside the allocation — and show in the result or in a margin of y."""
    import protoquant_amd as pq
    pq_opt("PQ_GROUPED_TILE", tile)
    M, N, K, E = 600, 200, 384, 6
    T = 300 if gather else M
    bad_off = np.array([-5, 70, 199, 199, 330, 520, M + 40], np.int32)
    good_off = np.clip(bad_off, 0, M)
    assert np.all(np.diff(good_off) >= 0) and bad_off.min() > -MARGIN and bad_off.max() < M + MARGIN
    for code in KINDS:
        rng = np.random.default_rng(40 + (code or 9))
        x_all = rng.integers(-128, 128, (T + 2 * MARGIN, K), dtype=np.int8)
        xs_all = (rng.random(M + 2 * MARGIN, dtype=np.float32) * 0.02 + 1e-3).astype(np.float32)
        wq = rng.integers(-128, 128, (E, N, K), dtype=np.int8)
        ws = (rng.random((E, N), dtype=np.float32) * 0.01 + 1e-4).astype(np.float32)
        bias = None
        if code is not None:
            bias = rng.standard_normal((E, N)).astype(np.float32)
            bias = bias if code == 2 else bits(torch.from_numpy(bias).to(TD[code]))
        idx_all = None
        if gather:
            idx_all = rng.integers(0, T, M + 2 * MARGIN).astype(np.int32)            # (the margins of the index hold VALID rows)
            bad = rng.choice(M, 60, replace=False) + MARGIN
            idx_all[bad] = T + rng.integers(0, 100, 60)                               # [x_rows, x_rows + 100): inside the back margin of xq
            assert idx_all.max() < T + MARGIN and idx_all.min() >= 0
        xg, xsg = torch.from_numpy(x_all).cuda(), torch.from_numpy(xs_all).cuda()
        idxg = torch.from_numpy(idx_all).cuda() if gather else None
        odt = torch.int32 if code is None else TD[code]
        y_all = torch.full((M + 2 * MARGIN, N), 23130, dtype=torch.int32, device="cuda").to(odt)
        sentinel = y_all.clone()
        xv, xsv, yv = xg[MARGIN:MARGIN + T], xsg[MARGIN:MARGIN + M], y_all[MARGIN:MARGIN + M]
        iv = idxg[MARGIN:MARGIN + M] if gather else None
        off_t = torch.from_numpy(bad_off).cuda()
        if code is None:
            pq.int_mm_grouped(xv, torch.from_numpy(wq).cuda(), off_t, row_index=iv, out=yv)
        else:
            pq.qlinear_s8_grouped(xv, xsv, torch.from_numpy(wq).cuda(), torch.from_numpy(ws).cuda(), to_gpu(bias, code), off_t, odt, row_index=iv, out=yv)
        torch.cuda.synchronize()
        # the oracle under the clamped values
        x_in = x_all[MARGIN:MARGIN + T]
        idx = np.minimum(idx_all[MARGIN:MARGIN + M], T - 1) if gather else None
        p = dict(xq=x_in, idx=idx, xs=xs_all[MARGIN:MARGIN + M], wq=wq, ws=ws, bias=bias, off=good_off, E=E, M=M, N=N, K=K, code=code)
        _check(yv, _oracle(p), code, f"clamped offsets / indices, tile {tile} gather {gather} code {code}")
        assert torch.equal(y_all[:MARGIN], sentinel[:MARGIN]), "rows in front of y were written"
        assert torch.equal(y_all[MARGIN + M:], sentinel[MARGIN + M:]), "rows behind y were written"


# ---------------------------------------------------------------- past 2^31
def _need(nbytes):
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + (2 << 30):
        pytest.skip(f"needs {nbytes >> 20} MiB of free device memory, {free >> 20} MiB are free")


def test_weight_expert_stride_past_2g_bytes(pq_opt):
    """a weight view whose expert stride puts the last expert beyond byte 2^31 of its allocation"""
    import protoquant_amd as pq
    E, N, K = 3, 200, 512
    S = (1 << 30) + 4096
    _need(2 * S + N * K)
    buf = torch.empty(2 * S + N * K, dtype=torch.int8, device="cuda")
    wv = buf.as_strided((E, N, K), (S, K, 1))
    rng = np.random.default_rng(31)
    p = _operands(rng, [100, 37, 130], N, K, 0, True)
    for e in range(E):
        wv[e] = torch.from_numpy(p["wq"][e]).cuda()
    assert wv[E - 1].data_ptr() - buf.data_ptr() > (1 << 31)
    want = _oracle(p)
    for tile in TILES:
        pq_opt("PQ_GROUPED_TILE", tile)
        got = pq.qlinear_s8_grouped(torch.from_numpy(p["xq"]).cuda(), torch.from_numpy(p["xs"]).cuda(), wv, torch.from_numpy(p["ws"]).cuda(), to_gpu(p["bias"], 0),
                                    torch.from_numpy(p["off"]).cuda(), torch.bfloat16)
        same_f(got, want, 0, f"expert stride 2^30 + 4096, tile {tile}")


def test_output_rows_past_2g_elements(pq_opt):
    """an output whose last rows lie beyond element 2^31 of its allocation, through a large ldy (staged and direct epilogue: full and ragged wave blocks)"""
    import protoquant_amd as pq
    M, N, K, LDY = 320, 200, 256, 7_200_000
    _need(M * LDY * 2)
    y_big = torch.empty((M, LDY), dtype=torch.bfloat16, device="cuda")
    rng = np.random.default_rng(32)
    p = _operands(rng, [150, 0, 130, 40], N, K, 0, True)
    assert p["M"] == M and (M - 20) * LDY > (1 << 31)
    want = _oracle(p)
    for tile in TILES:
        pq_opt("PQ_GROUPED_TILE", tile)
        yv = y_big[:, 8:8 + N]
        yv.zero_()
        got = _launch(pq, p, out=yv)
        assert got.data_ptr() == yv.data_ptr() and yv.stride(0) == LDY
        same_f(yv.contiguous(), want, 0, f"ldy = {LDY}, tile {tile}")


def test_row_index_into_the_last_rows_of_a_4g_code_matrix(pq_opt):
    """x_rows * ldx just below 2^32 (the limit the C-ABI states for a_row_index: the loader's per-lane source offset is 32 bits) with indices that pick the last source rows,
    rows on both sides of byte 2^31, and the first ones"""
    import protoquant_amd as pq
    K = 1024
    T = (1 << 22) - 1
    assert T * K < (1 << 32) and (T + 1) * K >= (1 << 32)
    _need(T * K)
    xq = torch.empty((T, K), dtype=torch.int8, device="cuda")
    half = (1 << 31) // K
    picks = np.array([T - 1, T - 2, T - 64, half - 1, half, half + 1, 0, 1, T - 1, half + 77] * 25, np.int32)
    g = torch.Generator(device="cuda"); g.manual_seed(33)
    uniq = torch.from_numpy(np.unique(picks)).cuda().long()
    xq[uniq] = torch.randint(-128, 128, (uniq.numel(), K), dtype=torch.int8, device="cuda", generator=g)
    rng = np.random.default_rng(33)
    p = _operands(rng, [100, 65, 85], 136, K, 0, False, x_rows=8, gather=True)
    assert p["M"] == picks.size
    p["idx"] = picks
    want_p = dict(p, xq=xq[torch.from_numpy(picks).cuda().long()].cpu().numpy(), idx=None)
    want = _oracle(want_p)
    for tile in TILES:
        pq_opt("PQ_GROUPED_TILE", tile)
        got = pq.qlinear_s8_grouped(xq, torch.from_numpy(p["xs"]).cuda(), torch.from_numpy(p["wq"]).cuda(), torch.from_numpy(p["ws"]).cuda(), None,
                                    torch.from_numpy(p["off"]).cuda(), torch.bfloat16, row_index=torch.from_numpy(picks).cuda())
        same_f(got, want, 0, f"x_rows * ldx = 2^32 - 1024, tile {tile}")


# ---------------------------------------------------------------- decode-sized routing
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("E", (128, 1024))
def test_decode_sized_routing(pq_opt, tile, E):
    """M_total = 256 over 128 and 1024 experts (the documented maximum: sixteen steps of the kernel's 64-lane prefix sum): most experts empty, forty with 1 to 4 rows"""
    import protoquant_amd as pq
    pq_opt("PQ_GROUPED_TILE", tile)
    M, N, K = 256, 136, 384
    for code in KINDS:
        rng = np.random.default_rng(E + KINDS.index(code))
        counts = np.zeros(E, np.int64)
        chosen = rng.choice(E, 43, replace=False)
        counts[chosen[:40]] = rng.integers(1, 5, 40)                 # forty experts with 1 to 4 rows ...
        rest = M - int(counts.sum())
        counts[chosen[40:]] = [rest // 3, rest // 3, rest - 2 * (rest // 3)]          # ... and three that share what is left
        assert counts.sum() == M and (counts == 0).sum() > E // 2 and ((counts >= 1) & (counts <= 4)).sum() == 40
        p = _operands(rng, counts, N, K, code, code in (0, 1), x_rows=64, gather=True)
        _check(_launch(pq, p), _oracle(p), code, f"E = {E}, tile {tile}, code {code}")
        p = _operands(rng, counts, N, K, code, False)
        _check(_launch(pq, p), _oracle(p), code, f"E = {E}, tile {tile}, code {code}, codes in grouped order")
