"""-m gpu: the EDGE SWEEP of the dense int8 GEMM kernels — every forced tile over its ragged edges, half-tile boundaries, K-tile counts 1 .. 9 and 13 and element-aligned
scales / bias (Part 1), the two-pass and the fused split-K over the 256-tile's edges (Part 2), and the weight-streaming kernel over its K split, batch parities, tails,
token tiles and store edges (Part 3).  The tables, the window reference and the buffer comparison are tests/gemm_edges.py (held on the CPU by
tests/test_gemm_edges_host.py); this file places one problem per tile geometry on the device and launches its prefix views.

Every launch writes into a window of a poisoned buffer and the WHOLE buffer is compared on the device (torch.equal's statement, kept as a device verdict) with an
expected buffer built there (poison fill + one slice copy of the full expected output); the verdicts of a batch are read back in one synchronisation.  On a mismatch the
first failing launch is run again alone, its buffer fetched, and the first bad (variant, kind, M, N, K, element) named against a host-built expected buffer.

Operands, scales, biases and the output buffer of a test live in ONE arena whose every other byte is 0x5B: an overrun of a few bytes reads or writes the test's own memory
and shows as a failed comparison.

Reach: for every tile launch pq_gemm_variant_name(M, N, K, lda, ldb) — for the transposed entry: of the swapped problem — is the forced variant's name and
pq_qlinear_workspace_bytes is 0 (K < 2048: single pass); for the split-K forms the workspace query is > 0 (the int32 twin has no split-K form: it runs the planner's
single-pass tile on the same shapes); for the weight-streaming kernel the name is skinny_16x16x64."""
import collections

import numpy as np
import pytest
import torch

from tests import gemm_edges as E
from tests.gpu_util import TD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    from protoquant_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    yield protoquant_amd
    E.problem.cache_clear()
    torch.cuda.empty_cache()


def _idt(code):
    return torch.int16 if E.ITEM[code] == 2 else torch.int32


def _window(flat, lay):
    return flat.as_strided((lay.rows, lay.cols), (lay.ld, 1), flat.storage_offset() + lay.offset)


class Arena:
    """one allocation per test, poisoned; take() hands out 256-byte aligned pieces with at least 256 poisoned bytes between them"""

    def __init__(self, nbytes):
        self.buf = torch.full((nbytes,), E.OPERAND_POISON, dtype=torch.uint8, device="cuda")
        self.top = 0

    def take(self, nbytes):
        off = -(-(self.top + 256) // 256) * 256
        self.top = off + nbytes
        assert self.top + 256 <= self.buf.numel(), "arena too small"
        return self.buf[off:off + nbytes]


def _arena_bytes(problems, out_bytes):
    n = out_bytes + 4096
    for p in problems:
        n += (p.Mmax + p.Nmax) * p.Kmax + 2 * 4 * (p.Mmax + p.Nmax + 2) + 2 * 12 * (p.Nmax + 1) + 16 * 512
    return n


def _out_bytes(rows, cols):
    return max(E.layout(rows, cols, m).total for m in E.MODES) * 4


class Placed:
    """a Problem in the arena: the operands, the scales and biases at 256-byte aligned bases ("") and as views from element 1 of a longer buffer ("s")"""

    def __init__(self, arena, p):
        self.p = p
        self.a = arena.take(p.Mmax * p.Kmax).view(torch.int8).view(p.Mmax, p.Kmax)
        self.a.copy_(torch.from_numpy(p.a))
        self.b = arena.take(p.Nmax * p.Kmax).view(torch.int8).view(p.Nmax, p.Kmax)
        self.b.copy_(torch.from_numpy(p.b))

        def vec(host, dtype, item):
            t = torch.from_numpy(host.view(np.int16) if item == 2 else host).view(dtype)
            n = t.numel()
            al, sh = arena.take(n * item).view(dtype), arena.take((n + 1) * item).view(dtype)[1:]
            al.copy_(t)
            sh.copy_(t)
            assert al.data_ptr() % 256 == 0 and sh.data_ptr() % 256 == item
            return {"": al, "s": sh}
        self.xs, self.ws = vec(p.xs, torch.float32, 4), vec(p.ws, torch.float32, 4)
        self.bias = {c: vec(np.ascontiguousarray(p.bias[c]), TD[c], E.ITEM[c]) for c in (0, 1, 2)}
        self._want = {}

    def want(self, kind, K):
        if (kind, K) not in self._want:
            w = self.p.want(kind, K)
            self._want[(kind, K)] = torch.from_numpy(w.view(np.int16 if w.itemsize == 2 else np.int32)).cuda()
        return self._want[(kind, K)]


Case = collections.namedtuple("Case", "dp kind M N K mode shift")


class Runner:
    """places problems, launches prefix views, keeps the verdicts on the device; reach = "tile" (display name + single pass), "split" (workspace > 0), "skinny" """

    def __init__(self, pq, what, reach, display, problems, out_rows, out_cols):
        from protoquant_amd import _lib
        self.pq, self.what, self.reach, self.display, self.L, self._ld = pq, what, reach, display, _lib.lib(), _lib.ld
        nb = _out_bytes(out_rows, out_cols)
        self.arena = Arena(_arena_bytes(problems, nb))
        self.placed = [Placed(self.arena, p) for p in problems]
        self.out = self.arena.take(nb)
        self.exp = torch.empty((nb,), dtype=torch.uint8, device="cuda")
        self.cases, self.verdicts, self.launches = [], [], 0

    def _reach(self, c, K, lda, ldb):
        M, N, L = c.M, c.N, self.L
        if self.reach == "split":
            if c.kind.entry != "acc":
                assert (L.pq_qlinear_t_workspace_bytes if c.kind.entry == "yt" else L.pq_qlinear_workspace_bytes)(M, N, K) > 0, (self.what, M, N, K)
            return
        name = L.pq_gemm_variant_name(N, M, K, ldb, lda) if (c.kind.entry == "yt" and self.reach == "tile") else L.pq_gemm_variant_name(M, N, K, lda, ldb)
        assert name == self.display, (self.what, c.kind.name, M, N, K, name)
        assert L.pq_qlinear_workspace_bytes(M, N, K) == 0 and L.pq_qlinear_t_workspace_bytes(M, N, K) == 0, "single pass"

    def _enqueue(self, c):
        dp, kind, M, N = c.dp, c.kind, c.M, c.N
        K = c.K or dp.p.Kmax
        rows, cols = (N, M) if kind.entry == "yt" else (M, N)
        lay = E.layout(rows, cols, c.mode)
        nb = lay.total * E.ITEM[kind.code]
        got, exp = self.out[:nb].view(_idt(kind.code)), self.exp[:nb].view(_idt(kind.code))
        got.fill_(E.POISON[kind.code])
        exp.fill_(E.POISON[kind.code])
        _window(exp, lay).copy_(dp.want(kind, K)[:rows, :cols])
        a, b = dp.a[:M, :K], dp.b[:N, :K]
        lda, ldb = self._ld(a), self._ld(b)
        self._reach(c, K, lda, ldb)
        if kind.entry == "acc":
            rc = self.L.pq_gemm_s8s8s32(a.data_ptr(), lda, b.data_ptr(), ldb, got.data_ptr() + 4 * lay.offset, lay.ld, M, N, K, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, self.L.pq_last_error()
        else:
            win = _window(got.view(TD[kind.code]), lay)
            xs, ws = dp.xs["s" if c.shift == "x" else ""][:M], dp.ws["s" if c.shift == "w" else ""][:N]
            bias = dp.bias[kind.code]["s" if c.shift == "w" else ""][:N] if kind.bias else None
            fn = self.pq.qlinear_s8_t if kind.entry == "yt" else self.pq.qlinear_s8
            y = fn(a, xs, b, ws, bias, TD[kind.code], out=win)
            assert y.data_ptr() == win.data_ptr() == got.data_ptr() + E.ITEM[kind.code] * lay.offset
        self.launches += 1
        return got, exp, lay, K

    def launch(self, dp, kind, M, N, K=None, mode="contig", shift=""):
        c = Case(dp, kind, M, N, K, mode, shift)
        got, exp, _, _ = self._enqueue(c)
        self.cases.append(c)
        self.verdicts.append((got == exp).all())

    def flush(self, switches=""):
        """one synchronisation for everything launched since the last flush (under the switches still in force: the failing launch is run again under them)"""
        if not self.cases:
            return
        ok = torch.stack(self.verdicts).cpu().numpy()
        cases, self.cases, self.verdicts = self.cases, [], []
        if ok.all():
            return
        c = cases[int(np.flatnonzero(~ok)[0])]
        got, _, lay, K = self._enqueue(c)
        host = got.cpu().numpy().view(E.bits_dtype(c.kind.code))
        want = E.expected_buffer(c.dp.p.window(c.kind, c.M, c.N, K), lay, c.kind.code)
        bad = E.first_bad(host, want, lay)
        extra = f"{c.dp.p.pattern} {c.mode} shift={c.shift!r} {switches} ({int((~ok).sum())} of {ok.size} launches of the batch differ)"
        if bad is None:
            pytest.fail(f"{self.what} {c.kind.name} M={c.M} N={c.N} K={K} {extra}: differed inside the batch but not when launched again alone")
        pytest.fail(E.describe(bad, self.what, c.kind, c.M, c.N, K, extra))


FORM_IDS = [f.id for f in E.FORMS]


def _force(pq_opt, form):
    if form.variant:
        pq_opt("PQ_FORCE_VARIANT", form.variant)
    for name, value in form.switches:
        pq_opt(name, value)


# ---------------------------------------------------------------- the device verdict can fail (the kernels here are the real ones: the EXPECTED side is bent)
@pytest.mark.parametrize("kind", [E.BF16_B, E.I32, E.BF16_BT], ids=lambda k: k.name)
def test_a_wrong_element_is_found_and_named(pq, pq_opt, kind):
    """one bit of one element of the expected output flipped on the device, in the middle of a batch of good launches: flush() must fail, on that launch, and name
    that element; the same batch without the flip passes"""
    pq_opt("PQ_FORCE_VARIANT", "ring64x64")
    p = E.Problem(130, 130, E.K_EDGE, "full")           # (a problem of this test's own: nothing bent here is shared)
    r = Runner(pq, "ring64x64", "tile", E.DISPLAY["ring64x64"], [p], 130, 130)
    dp = r.placed[0]

    def batch():
        for M, N in ((20, 130), (64, 64), (65, 69)):
            r.launch(dp, kind, M, N, mode="ld8")
    batch()
    r.flush()
    # [40, 7] lies outside the first launch's window (20 rows; transposed entry: 20 columns, but 130 rows — there it is inside) and inside the other two
    row, col = 40, 7
    p.want(kind)[row, col] ^= 1                        # the host's expected output and the device's copy of it, bent alike
    dp.want(kind, E.K_EDGE)[row, col] ^= 1
    batch()
    with pytest.raises(pytest.fail.Exception) as info:
        r.flush("bent")
    text = str(info.value)
    first, failing = ("M=20 N=130", 3) if kind.entry == "yt" else ("M=64 N=64", 2)
    assert first in text and f"first at element [{row}, {col}]" in text and "1 elements of the buffer differ" in text and kind.name in text, text
    assert f"{failing} of 3 launches" in text and f"want 0x{int(p.want(kind)[row, col]):X}" in text, text
    p.want(kind)[row, col] ^= 1
    dp.want(kind, E.K_EDGE)[row, col] ^= 1
    batch()
    r.flush()


# ---------------------------------------------------------------- Part 1
@pytest.mark.parametrize("form", E.FORMS, ids=FORM_IDS)
def test_every_edge_of_every_tile(pq, pq_opt, form):
    """K = 640; the required pairs x five kinds x (contiguous rows, 16-byte aligned rows, contiguous rows under PQ_EPI_ANY_ALIGN=0)"""
    TM, TN = E.TILE[form.variant]
    _force(pq_opt, form)
    Mx, Nx = E.edge_extent(TM, TN)
    p = E.problem(Mx, Nx, E.K_EDGE, "full")
    r = Runner(pq, form.id, "tile", E.DISPLAY[form.variant], [p], max(Mx, Nx), max(Mx, Nx))
    dp = r.placed[0]
    for mode, any_align in E.OUT_MODES:
        pq_opt("PQ_EPI_ANY_ALIGN", any_align)
        for M, N in E.edge_pairs(TM, TN):
            for kind in E.KINDS:
                r.launch(dp, kind, M, N, mode=mode)
        r.flush(f"PQ_EPI_ANY_ALIGN={any_align!r}")
    print(f"[gemm-edges] part 1 edges {form.id}: {r.launches} launches")


@pytest.mark.parametrize("form", E.FORMS, ids=FORM_IDS)
def test_k_tile_counts_and_element_aligned_scales(pq, pq_opt, form):
    """K = 128 n, n = 1 .. 9 and 13, as K-prefix views (lda = ldb = 1664) of both operand patterns at a fully staged and at a ragged shape; then, at K = 640 of the same
    views, ws and bias from element 1 of a longer buffer (4 and 2 / 4 bytes past a 256-byte boundary) and, separately, xs: the staged epilogue must refuse them, the
    bits stay"""
    TM, TN = E.TILE[form.variant]
    _force(pq_opt, form)
    ps = [E.problem(2 * TM, 2 * TN, E.KT_LD, pattern) for pattern in ("full", "ktile")]
    r = Runner(pq, form.id, "tile", E.DISPLAY[form.variant], ps, 2 * max(TM, TN), 2 * max(TM, TN))
    for dp in r.placed:
        for M, N in E.kt_shapes(TM, TN):
            for n in E.KT_COUNTS:
                for kind in E.KINDS:
                    for mode in E.MODES:
                        r.launch(dp, kind, M, N, K=128 * n, mode=mode)
    r.flush("K-tile counts")
    counts = r.launches
    for M, N in E.kt_shapes(TM, TN):
        for shift in ("w", "x"):
            for kind in E.KINDS:
                if kind.code is not None:
                    for mode in E.MODES:
                        r.launch(r.placed[0], kind, M, N, K=E.K_EDGE, mode=mode, shift=shift)
    r.flush("scales / bias from element 1")
    print(f"[gemm-edges] part 1 K-tile counts {form.id}: {counts} launches, element-aligned scales / bias: {r.launches - counts}")


# ---------------------------------------------------------------- Part 2
@pytest.mark.parametrize("form", E.SPLIT_FORMS, ids=[f.id for f in E.SPLIT_FORMS])
def test_split_k_forms_at_the_edges(pq, pq_opt, form):
    """K = 2560 (twenty K-tiles), the planner's own tile under a forced slice count; the workspace comes from the library's query through pq.qlinear_s8 / pq.qlinear_s8_t"""
    _force(pq_opt, form)
    p = E.problem(513, 513, E.K_SPLIT, "full")
    r = Runner(pq, form.id, "split", None, [p], 513, 513)
    for mode in E.SPLIT_MODES:
        for M, N in E.split_pairs():
            for kind in E.KINDS:
                r.launch(r.placed[0], kind, M, N, mode=mode)
        r.flush(mode)
    print(f"[gemm-edges] part 2 {form.id}: {r.launches} launches")


# ---------------------------------------------------------------- Part 3
def _skinny_runner(pq, pq_opt, what, mt, problems):
    if mt > 1:          # (M <= 16 is the planner's own choice; beyond, the kernel is forced as test_skinny_gemm_exact forces it)
        pq_opt("PQ_FORCE_VARIANT", "skinny")
    return Runner(pq, what, "skinny", E.DISPLAY["skinny"], problems, 64, 64)


@pytest.mark.parametrize("stage", E.SK_STAGE, ids=["staged", "unstaged"])
@pytest.mark.parametrize("rb", E.SK_RB, ids=["rb-plan", "rb-1", "rb-2"])
@pytest.mark.parametrize("mt", [1, 2, 3, 4])
def test_streaming_kernel_k_split(pq, pq_opt, mt, rb, stage):
    """K / 128 in 1 .. 20, 43, 86 as K-prefix views (lda = ldb = 11008), N = 37, every PQ_SKINNY_KS; int32 and bf16 with bias; both operand patterns, the "ktile" one
    indexed by the 64-byte k-step"""
    ps = [E.problem(64, E.SK_N, E.SK_KMAX, pattern, 64) for pattern in ("full", "ktile")]
    r = _skinny_runner(pq, pq_opt, f"skinny mt={mt} rb={rb!r} stage={stage!r}", mt, ps)
    pq_opt("PQ_SKINNY_RB", rb)
    pq_opt("PQ_SKINNY_STAGE", stage)
    for ks in E.SK_KS:
        pq_opt("PQ_SKINNY_KS", ks)
        for M in (m for m in E.SK_M if E.token_tiles(m) == mt):
            for n in E.SK_KT:
                for dp in r.placed:
                    for kind in E.SK_KINDS:
                        r.launch(dp, kind, M, E.SK_N, K=128 * n)
        r.flush(f"PQ_SKINNY_KS={ks!r}")
    print(f"[gemm-edges] part 3 K split mt={mt} rb={rb!r} stage={stage!r}: {r.launches} launches")


@pytest.mark.parametrize("rb", E.SK_EDGE_RB, ids=["rb-plan", "rb-2"])
@pytest.mark.parametrize("mt", [1, 2, 3, 4])
def test_streaming_kernel_store_edges(pq, pq_opt, mt, rb):
    """K = 640; N mod 4 (the vector store), mod 16 (the block), mod 32 (two blocks per wave); the five kinds (the transposed entry is the EPI_STORE_T branch) and bf16
    once more with ws / bias from element 1"""
    p = E.problem(64, E.SK_N, E.K_EDGE, "full", 64)
    r = _skinny_runner(pq, pq_opt, f"skinny edges mt={mt} rb={rb!r}", mt, [p])
    pq_opt("PQ_SKINNY_RB", rb)
    dp = r.placed[0]
    for mode in E.MODES:
        for M in (m for m in E.SK_EDGE_M if E.token_tiles(m) == mt):
            for N in E.SK_EDGE_N:
                for kind in E.KINDS:
                    r.launch(dp, kind, M, N, mode=mode)
                r.launch(dp, E.BF16_B, M, N, mode=mode, shift="w")
        r.flush(mode)
    print(f"[gemm-edges] part 3 store edges mt={mt} rb={rb!r}: {r.launches} launches")
