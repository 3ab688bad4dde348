"""-m gpu: the grouped weight-streaming qlinear for decode (gemm_s8_grouped_stream.hip; pq_qlinear_s8_grouped_stream / pq_gemm_s8s8s32_grouped_stream, at most 64 grouped
rows).  Every result is compared, as bit patterns, against qlinear_s8_grouped (the 64-row tiles) on the same operands AND against qlinear_s8 / int_mm run per expert on
that expert's row slice.  The output is always an interior view of a larger sentinel-filled buffer: rows above and below it, the columns right of it and the rows
>= offsets[E] must still hold the sentinel afterwards.

The tests of untrusted device data check a clamp BY ITS RESULT and are built so that no outcome can leave the allocations: xq, xs, the row index and y are interior
views with margins wider than the largest excursion used."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
KINDS = (torch.bfloat16, torch.float16, torch.float32, None)          # None = the int32 twin
GUARD = 8                                                              # sentinel rows above and below y
PLAN = re.compile(rb"^gstream_mt([124])_rb([12])_ks(\d+)_16x16x64$")


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    bad = (_bits(a) != _bits(b))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} bytes differ"


def _operands(seed, counts, N, K, kind, bias=False, gather=False, x_rows=None, tail=0, ldx=None, ldw=None, n_pad=0):
    """Seeded operands on the GPU.  counts[e] rows per expert, `tail` rows past offsets[E]; ldx / ldw / n_pad make xq and wq views of larger buffers."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    E, M = len(counts), int(sum(counts)) + tail
    T = x_rows if x_rows is not None else M
    x_big = torch.randint(-128, 128, (T, ldx or K), dtype=torch.int8, device="cuda", generator=g)
    w_big = torch.randint(-128, 128, (E, N + n_pad, ldw or K), dtype=torch.int8, device="cuda", generator=g)
    p = dict(xq=x_big[:, :K], wq=w_big[:, :N, :K], E=E, M=M, N=N, K=K, kind=kind, counts=list(counts), T=T)
    p["idx"] = torch.randint(0, T, (M,), dtype=torch.int32, device="cuda", generator=g) if gather else None
    p["xs"] = torch.rand(M, device="cuda", generator=g) * 0.02 + 1e-3
    p["ws"] = torch.rand((E, N), device="cuda", generator=g) * 0.01 + 1e-4
    p["bias"] = torch.randn((E, N), device="cuda", generator=g).to(kind) if (bias and kind is not None) else None
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    p["off_host"] = off
    p["off"] = torch.tensor(off, dtype=torch.int32, device="cuda")
    return p


def _guarded(p, ldy=None):
    """y as an interior view of a sentinel-filled buffer: (buffer, view)"""
    dt = torch.int32 if p["kind"] is None else p["kind"]
    big = torch.full((p["M"] + 2 * GUARD, ldy or p["N"] + 8), 77, dtype=torch.int32, device="cuda").to(dt)
    return big, big[GUARD:GUARD + p["M"], :p["N"]]


def _stream(pq, p, out=None):
    if p["kind"] is None:
        return pq.int_mm_grouped_stream(p["xq"], p["wq"], p["off"], row_index=p["idx"], out=out)
    return pq.qlinear_s8_grouped_stream(p["xq"], p["xs"], p["wq"], p["ws"], p["bias"], p["off"], p["kind"], row_index=p["idx"], out=out)


def _tiles(pq, p):
    if p["kind"] is None:
        return pq.int_mm_grouped(p["xq"], p["wq"], p["off"], row_index=p["idx"])
    return pq.qlinear_s8_grouped(p["xq"], p["xs"], p["wq"], p["ws"], p["bias"], p["off"], p["kind"], row_index=p["idx"])


def _per_expert(pq, p, off=None, idx=None):
    """pq.qlinear_s8 / pq.int_mm once per expert on its row slice (off: host list of the offsets to go by; idx: host-clamped row index)"""
    off = off or p["off_host"]
    idx = idx if idx is not None else p["idx"]
    rows = p["xq"].index_select(0, idx.long()) if idx is not None else p["xq"]
    outs = []
    for e in range(p["E"]):
        lo, hi = off[e], off[e + 1]
        if hi <= lo:
            continue
        x, w = rows[lo:hi].contiguous(), p["wq"][e].contiguous()
        if p["kind"] is None:
            outs.append((lo, hi, pq.int_mm(x, w)))
        else:
            outs.append((lo, hi, pq.qlinear_s8(x, p["xs"][lo:hi].contiguous(), w, p["ws"][e].contiguous(), p["bias"][e].contiguous() if p["bias"] is not None else None, p["kind"])))
    return outs


def _check(pq, p, what, ldy=None, against_tiles=True):
    big, view = _guarded(p, ldy)
    sentinel = big.clone()
    got = _stream(pq, p, out=view)
    assert got.data_ptr() == view.data_ptr()
    n = p["off_host"][-1]
    for lo, hi, want in _per_expert(pq, p):
        _same(view[lo:hi], want, f"{what}: rows {lo}..{hi} against qlinear_s8 per expert")
    if against_tiles:
        _same(view[:n], _tiles(pq, p)[:n], f"{what}: against qlinear_s8_grouped")
    check = big.clone()
    check[GUARD:GUARD + n, :p["N"]] = sentinel[GUARD:GUARD + n, :p["N"]]
    assert torch.equal(_bits(check), _bits(sentinel)), f"{what}: something outside rows 0..{n} x columns 0..{p['N']} of y was written"
    return view


# ---------------------------------------------------------------- the first thing to run on a new build
def test_smallest_case():
    import protoquant_amd as pq
    for kind in KINDS:
        _check(pq, _operands(1, [1], 16, 128, kind), f"E = 1, one row, {kind}")


# ---------------------------------------------------------------- output kinds x row index x bias, over every row count that moves a tile edge
@pytest.mark.parametrize("M_total", (1, 2, 15, 16, 17, 33, 48, 49, 64))
@pytest.mark.parametrize("gather", (False, True))
def test_row_counts_kinds_bias_and_row_index(M_total, gather):
    import protoquant_amd as pq
    E = 8
    g = torch.Generator().manual_seed(M_total)
    owner = torch.randint(0, E, (M_total,), generator=g)
    counts = torch.bincount(owner, minlength=E).tolist()
    for kind in KINDS:
        for bias in ((False, True) if kind is not None else (False,)):
            p = _operands(100 + M_total, counts, 200, 256, kind, bias=bias, gather=gather, x_rows=40 if gather else None)
            _check(pq, p, f"M_total {M_total} gather {gather} {kind} bias {bias}")


ROUTINGS = {
    "one row per expert": [1] * 64,
    "one expert owns all 64 rows": [0, 0, 64, 0],
    "empty experts first": [0, 0, 0, 5, 20, 1],
    "empty experts last": [7, 30, 2, 0, 0, 0, 0],
    "empty experts in between": [3, 0, 0, 17, 0, 1, 0, 33],
    "rows straddle a 16-row tile edge": [10, 12, 19, 23],              # rows 10..21 and 22..40 and 41..63 cross rows 16, 32 and 48
    "three token tiles": [40, 1, 2],
}


@pytest.mark.parametrize("name", list(ROUTINGS))
def test_routings(name):
    import protoquant_amd as pq
    for kind, gather in ((torch.bfloat16, True), (torch.float32, False), (None, True)):
        p = _operands(7, ROUTINGS[name], 136, 384, kind, bias=kind is torch.bfloat16, gather=gather, x_rows=50 if gather else None)
        _check(pq, p, f"{name}, {kind}")


def test_rows_behind_the_last_offset_stay_untouched():
    """offsets[E] < M_total: the rows behind belong to nobody"""
    import protoquant_amd as pq
    for kind in KINDS:
        for tail in (1, 30):
            p = _operands(9, [4, 0, 13, 17], 200, 256, kind, bias=True, gather=True, x_rows=20, tail=tail)
            assert p["M"] == 34 + tail and p["off_host"][-1] == 34
            _check(pq, p, f"tail {tail}, {kind}")


@pytest.mark.parametrize("E", (1, 8, 128, 1024))
def test_expert_counts(E):
    """up to the documented maximum of 1024 experts: the slot search walks 16 steps of 64 experts; the live experts are spread over all of them"""
    import protoquant_amd as pq
    for M_total in (1, 17, 64):
        g = torch.Generator().manual_seed(E + M_total)
        spread = M_total - 2 if (E >= 128 and M_total > 2) else M_total
        counts = torch.bincount(torch.randint(0, E, (spread,), generator=g), minlength=E).tolist()
        if spread != M_total:
            counts[E - 1] += 1; counts[0] += 1                           # the first and the last expert are live
        assert sum(counts) == M_total
        for kind in (torch.bfloat16, None):
            p = _operands(E, counts, 48, 128, kind, bias=kind is not None, gather=True, x_rows=16)
            _check(pq, p, f"E {E} M_total {M_total} {kind}")


@pytest.mark.parametrize("N", (16, 200, 1537, 4096))
def test_widths(N):
    """N below one block, N that is no multiple of 16, an odd N (element-wise stores, rows of y that are not 8-byte aligned)"""
    import protoquant_amd as pq
    for kind in KINDS:
        p = _operands(N, [2, 0, 1, 14], N, 256, kind, bias=True)
        _check(pq, p, f"N {N} {kind}")


def test_odd_width_with_a_padded_leading_dimension():
    import protoquant_amd as pq
    for kind in KINDS:
        for ldy in (1537 + 24, 1537 + 7):
            p = _operands(3, [1, 20, 0, 2], 1537, 128, kind, bias=True, gather=True, x_rows=9)
            _check(pq, p, f"N 1537 ldy {ldy} {kind}", ldy=ldy)


@pytest.mark.parametrize("K", (128, 256, 2048, 14336))
def test_depths(pq_opt, K):
    import protoquant_amd as pq
    for kind in (torch.bfloat16, None):
        p = _operands(K, [1, 0, 18, 3], 72, K, kind, bias=True)
        _check(pq, p, f"K {K} {kind}")
    if K == 128:                                                         # two k-steps under 16 waves: fourteen waves add zeros
        pq_opt("PQ_GROUPED_STREAM_KS", 16)
        for counts in ([1], [3, 40, 2]):
            _check(pq, _operands(K + 1, counts, 72, K, torch.float16, bias=True), f"K 128, 16 waves, counts {counts}")


def test_strided_operands_reach_the_library_without_a_copy(monkeypatch):
    """ldx > K, wq a slice of a larger [E, N + 3, K + 128] buffer (ldw and w_expert_stride padded): the bits of the contiguous call, and the C-ABI received the views'
    own pointers and strides"""
    import protoquant_amd as pq
    from protoquant_amd import _lib
    L = _lib.lib()
    N, K = 200, 384
    for kind in KINDS:
        for gather in (False, True):
            p = _operands(21, [5, 0, 30, 1], N, K, kind, bias=True, gather=gather, x_rows=50 if gather else None, ldx=K + 64, ldw=K + 128, n_pad=3)
            assert p["xq"].stride(0) == K + 64 and p["wq"].stride() == ((N + 3) * (K + 128), K + 128, 1)
            name = "pq_gemm_s8s8s32_grouped_stream" if kind is None else "pq_qlinear_s8_grouped_stream"
            real, seen = getattr(L, name), {}

            def spy(*a, _real=real):
                seen["a"] = a
                return _real(*a)
            monkeypatch.setattr(L, name, spy)
            view = _check(pq, p, f"strided, {kind}, gather {gather}")
            monkeypatch.setattr(L, name, real)
            a = seen["a"]
            wi = 4 if kind is None else 5
            assert (a[0], a[1]) == (p["xq"].data_ptr(), K + 64), "xq was copied"
            assert (a[wi], a[wi + 1], a[wi + 2]) == (p["wq"].data_ptr(), K + 128, (N + 3) * (K + 128)), "wq was copied"
            q = dict(p, xq=p["xq"].contiguous(), wq=p["wq"].contiguous())
            _same(view, _stream(pq, q), "strided against contiguous operands")


@pytest.mark.parametrize("live,N,K,E", ((2, 28672, 4096, 2), (2, 4096, 14336, 2), (8, 1536, 2048, 128), (8, 2048, 768, 128)))
def test_real_layer_shapes(live, N, K, E):
    """gate+up and down of Mixtral 8x7B (two experts of its eight, to keep the operands small) and of a 128-small-expert layer, at a decode step's row counts"""
    import protoquant_amd as pq
    counts = [0] * E
    for i, e in enumerate(torch.randperm(E, generator=torch.Generator().manual_seed(N))[:live].tolist()):
        counts[e] = 1 + (i % 3 == 0)
    p = _operands(N, counts, N, K, torch.bfloat16, gather=True, x_rows=4)
    _check(pq, p, f"{K} -> {N}, E {E}")
    assert PLAN.match(_lib_name(E, p["M"], N, K))


def _lib_name(E, M, N, K):
    from protoquant_amd import _lib
    return _lib.lib().pq_grouped_stream_plan_name(E, M, N, K)


# ---------------------------------------------------------------- untrusted device data
MARGIN = 128      # rows of margin around every operand a bad value could reach: the largest excursion below is 40 rows (offsets) / 100 rows (row index)


@pytest.mark.parametrize("gather", (False, True))
def test_out_of_range_offsets_and_row_index_are_clamped(gather):
    """Negative, too large and descending offsets; row indices outside [0, x_rows).  Expected: the result under the clamped values (hi into [0, M_total], lo into [0, hi],
    indices into [0, x_rows)) — and nothing outside the rows those clamped ranges name changes.  xq, xs, the row index and y are interior views MARGIN rows inside their
    allocations, so an access steered by the unclamped values would still land in memory this test owns."""
    import protoquant_amd as pq
    M, N, K = 60, 136, 256
    T = 30 if gather else M
    for kind in KINDS:
        g = torch.Generator(device="cuda").manual_seed(5)
        x_all = torch.randint(-128, 128, (T + 2 * MARGIN, K), dtype=torch.int8, device="cuda", generator=g)
        xs_all = torch.rand(M + 2 * MARGIN, device="cuda", generator=g) * 0.02 + 1e-3
        p = _operands(6, [10] * 6, N, K, kind, bias=True)
        p.update(xq=x_all[MARGIN:MARGIN + T], xs=xs_all[MARGIN:MARGIN + M], T=T, M=M)
        # experts:      0: lo -5 -> 0       1        2: descending (hi < lo: empty)   3         4: hi 40 rows past M_total -> M       5: both past M: empty
        raw = [-5, 8, 20, 12, 30, M + 40, M + 40]
        p["off"] = torch.tensor(raw, dtype=torch.int32, device="cuda")
        clamped = []
        for e in range(6):
            hi = min(max(raw[e + 1], 0), M)
            clamped.append((min(max(raw[e], 0), hi), hi))
        assert clamped == [(0, 8), (8, 20), (12, 12), (12, 30), (30, M), (M, M)]
        idx_host = None
        if gather:
            idx_all = torch.zeros(M + 2 * MARGIN, dtype=torch.int32, device="cuda")
            idx = idx_all[MARGIN:MARGIN + M]
            idx.copy_(torch.randint(0, T, (M,), generator=torch.Generator().manual_seed(1)).to(torch.int32))
            idx[::7] = torch.arange(T, T + 100, 12, dtype=torch.int32, device="cuda")[:len(idx[::7])]       # too large
            idx[3::11] = -4                                                                                # negative (read as unsigned: too large)
            p["idx"] = idx
            idx_host = idx.clone()
            idx_host[(idx_host < 0) | (idx_host >= T)] = T - 1
        dt = torch.int32 if kind is None else kind
        big = torch.full((M + 2 * MARGIN, N + 8), 77, dtype=torch.int32, device="cuda").to(dt)
        view = big[MARGIN:MARGIN + M, :N]
        sentinel = big.clone()
        _stream(pq, p, out=view)
        torch.cuda.synchronize()
        # overlapping claims: experts 1 (rows 8..19) and 3 (rows 12..29) both write rows 12..19 — either may win; everything else is exact
        written = torch.zeros(M, dtype=torch.bool)
        for e, (lo, hi) in enumerate(clamped):
            if hi <= lo:
                continue
            q = dict(p, off_host=[lo, hi], E=1, wq=p["wq"][e:e + 1], ws=p["ws"][e:e + 1], bias=p["bias"][e:e + 1] if p["bias"] is not None else None)
            rows = p["xq"].index_select(0, idx_host.long()) if gather else p["xq"]
            if kind is None:
                want = pq.int_mm(rows[lo:hi].contiguous(), q["wq"][0].contiguous())
            else:
                want = pq.qlinear_s8(rows[lo:hi].contiguous(), p["xs"][lo:hi].contiguous(), q["wq"][0].contiguous(), q["ws"][0].contiguous(),
                                     q["bias"][0].contiguous() if q["bias"] is not None else None, kind)
            sole = [r for r in range(lo, hi) if not (12 <= r < 20)]
            _same(view[sole], want[[r - lo for r in sole]], f"clamped expert {e}, {kind}, gather {gather}")
            written[lo:hi] = True
        assert bool(written.all())
        check = big.clone()
        check[MARGIN:MARGIN + M, :N] = sentinel[MARGIN:MARGIN + M, :N]
        assert torch.equal(_bits(check), _bits(sentinel)), "something outside y was written"


# ---------------------------------------------------------------- the two forcing switches: time only, never bits
@pytest.mark.parametrize("counts", ([1], [0, 2, 1, 9], [20, 12], [1, 50, 13]), ids=lambda c: "-".join(map(str, c)))
def test_forced_plans_give_the_same_bits(pq_opt, counts):
    """PQ_GROUPED_STREAM_KS in (1, 4, 16) x PQ_GROUPED_STREAM_RB in (1, 2): the plan name reports what was forced, the bits do not move"""
    import protoquant_amd as pq
    N, K = 1000, 1152                                                    # 18 k-steps: uneven slices under 4 and 16 waves, a tail behind the batches
    M = sum(counts)
    for kind in KINDS:
        p = _operands(31, counts, N, K, kind, bias=True, gather=True, x_rows=11)
        pq_opt("PQ_GROUPED_STREAM_KS", ""); pq_opt("PQ_GROUPED_STREAM_RB", "")
        base = _check(pq, p, f"planned, {kind}").clone()
        for ks in (1, 4, 16):
            for rb in (1, 2):
                pq_opt("PQ_GROUPED_STREAM_KS", ks); pq_opt("PQ_GROUPED_STREAM_RB", rb)
                m = PLAN.match(_lib_name(len(counts), M, N, K))
                assert m and int(m.group(3)) == ks and int(m.group(2)) == (rb if M <= 32 else 1), (ks, rb, m and m.groups())
                assert int(m.group(1)) == (1 if M <= 16 else 2 if M <= 32 else 4)
                _same(_stream(pq, p), base, f"KS {ks} RB {rb} {kind} counts {counts}")


# ---------------------------------------------------------------- one captured launch, replayed over other routings
def test_one_graph_replayed_over_three_routings():
    """a torch.cuda.graph capture of ONE streaming launch (a single chain: no side stream); between replays only the CONTENTS of offsets, row index, xs and the codes change"""
    import protoquant_amd as pq
    E, N, K, M, T = 128, 200, 512, 48, 6
    routings = []
    for seed in (1, 2, 3):
        g = torch.Generator().manual_seed(seed)
        owner = torch.randint(0, E, (M,), generator=g) if seed != 2 else torch.full((M,), 77)         # the second routing: one expert owns every row
        routings.append(torch.bincount(owner, minlength=E).tolist())
    ps = [_operands(40 + i, c, N, K, torch.bfloat16, bias=True, gather=True, x_rows=T) for i, c in enumerate(routings)]
    live = dict(ps[0])
    for k in ("xq", "xs", "idx", "off"):
        live[k] = ps[0][k].clone()
    big, view = _guarded(live)
    sentinel = big.clone()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        _stream(pq, live, out=view)                                    # warm-up outside the capture
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            _stream(pq, live, out=view)
    for i, p in enumerate(ps):
        for k in ("xq", "xs", "idx", "off"):
            live[k].copy_(p[k])
        big.copy_(sentinel)
        graph.replay()
        torch.cuda.synchronize()
        q = dict(p, wq=live["wq"], ws=live["ws"], bias=live["bias"])           # (the weights are those of the capture)
        for lo, hi, want in _per_expert(pq, q):
            _same(view[lo:hi], want, f"replay {i}: rows {lo}..{hi}")
        _same(view, _tiles(pq, q), f"replay {i} against qlinear_s8_grouped")
        check = big.clone()
        check[GUARD:GUARD + M, :N] = sentinel[GUARD:GUARD + M, :N]
        assert torch.equal(_bits(check), _bits(sentinel)), f"replay {i}: something outside y was written"


def test_more_than_64_rows_is_refused():
    import protoquant_amd as pq
    p = _operands(2, [30, 35], 64, 128, torch.bfloat16)
    with pytest.raises(ValueError, match="at most 64 grouped rows"):
        _stream(pq, p)
    p["kind"] = None
    with pytest.raises(ValueError, match="at most 64 grouped rows"):
        _stream(pq, p)
