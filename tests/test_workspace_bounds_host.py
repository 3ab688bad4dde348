"""CPU: what tests/test_gpu_workspace_bounds.py rests on, before any kernel runs — the guard itself (a stray byte on either side of a Guarded workspace is seen and
named), the coverage of its FORMS table against the two C headers (every exported function with a workspace_bytes parameter has a row, every query a row names is
exported), every row's proof that it reaches its form, asked of the loaded library with PQ_FAKE_CUS=256 (no device is asked), and the algebra of the workspace queries
over a grid of shapes and every forced option of the table."""
import itertools
import os
import re

import pytest
import torch

from tests import test_gpu_workspace_bounds as W
from tests.guarded_workspace import ALIGN, MARGIN, SLAB_BYTES, Guarded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the helper tests itself
@pytest.mark.parametrize("nbytes", (0, 1, 255, 256, 257, 2 ** 20 + 3))
def test_interior_is_aligned_and_exactly_as_long_as_asked(nbytes):
    g = Guarded(nbytes, 0x11, "cpu")
    assert g.ptr % ALIGN == 0 and g.nbytes == nbytes and g.interior.numel() == nbytes and (nbytes == 0 or g.interior.data_ptr() == g.ptr)
    assert g.front >= MARGIN and g.back >= MARGIN and MARGIN >= 2 * SLAB_BYTES + 4096 == 512 * 1024 + 4096
    assert g.buf.numel() == g.front + nbytes + g.back and bool((g.interior == 0x11).all())
    g.assert_margins("fresh")
    assert g.touched() == {}


@pytest.mark.parametrize("nbytes", (1, 257, 4096))
def test_a_stray_byte_is_reported_with_its_side_and_offset(nbytes):
    g = Guarded(nbytes, 0, "cpu")
    end = g.front + nbytes
    places = {"interior end + 0": (end, "back", 0), "interior start - 1": (g.front - 1, "front", -nbytes - 1),
              "far end of the back margin": (g.buf.numel() - 1, "back", g.back - 1), "far end of the front margin": (0, "front", -nbytes - g.front)}
    for what, (index, side, offset) in places.items():
        old = int(g.buf[index])
        g.buf[index] = old ^ 0x80
        assert not bool(g.margins_intact()), what
        assert g.touched() == {side: (offset, offset)}, (what, g.touched())
        with pytest.raises(AssertionError, match=f"{side} margin written at bytes {offset} .. {offset} from the interior's end"):
            g.assert_margins(what)
        g.buf[index] = old
        g.assert_margins(what + ", restored")
    g.interior[-1] = 0xEE                                            # the last byte of the interior is the workspace's own
    g.interior[0] = 0xEE
    g.assert_margins("a write to the interior")
    g.buf[0], g.buf[end + 5], g.buf[end + 9] = 0xFF, 0xFF, 0xFF         # both sides at once: first and last touched byte of each
    assert g.touched() == {"front": (-nbytes - g.front, -nbytes - g.front), "back": (5, 9)}


def test_sentinel_differs_from_every_fill_and_refill_repeats_the_leftovers():
    g = Guarded(1000, 0xFF, "cpu")
    for fill in (0, 0xFF, 0xCD, 0x5A):
        assert not bool((g.buf[:g.front] == fill).all()) and int((g.buf[:64] == fill).sum()) <= 1, "no fill byte reproduces the margin"
    small = Guarded(300, 0, "cpu")
    small.interior.copy_(torch.arange(300, dtype=torch.int64).to(torch.uint8))
    g.refill_from(small)
    assert torch.equal(g.interior, torch.arange(300, dtype=torch.int64).to(torch.uint8).repeat(4)[:1000])
    g.assert_margins("refill_from")
    assert bool((g.refill(7).interior == 7).all())


def test_the_deferred_checks_of_the_gpu_file_report_what_they_saw():
    """W.Checks leaves its flags where the tensors live and reads them once: a margin touched BETWEEN two launches is still reported at the read"""
    g, checks = Guarded(64, 0, "cpu"), W.Checks()
    checks.margins(g, "first launch")
    checks.interior(g, 0, "first launch")
    checks.read()
    g.buf[g.front + 64 + 3] ^= 0xFF
    checks.margins(g, "second launch")
    g.interior[5] = 1
    checks.interior(g, 0, "third launch")
    checks.margins(g, "third launch")
    with pytest.raises(AssertionError, match=r"second launch: a workspace of 64 bytes was overrun: back margin written at bytes 3 \.\. 3(.|\n)*third launch: 1 bytes of the workspace were written"):
        checks.read()
    checks.read()                                                    # (read and gone)


# ---------------------------------------------------------------- the table against the headers
def _exported(header):
    """{function name: parameter text} of every prototype of a C header"""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(pq_\w+)\s*\(([^;{}()]*)\)\s*;", text)}


HEADERS = {**_exported("pq_hip.h"), **_exported("pq_rccl.h")}


def test_every_entry_that_takes_a_workspace_has_a_row():
    takers = sorted(name for name, params in HEADERS.items() if re.search(r"\bworkspace_bytes\b", params))
    assert {"pq_qlinear_s8", "pq_qlinear_s8_t", "pq_qlinear_s8_kslabs", "pq_qlinear_dyn", "pq_moe_route", "pq_allgather_cols", "pq_allgather_cols_v",
            "pq_allgather_cols_rows_async", "pq_reduce_scatter_rows", "pq_kslabs_way_name"} <= set(takers), "the parser lost a prototype"
    rows = {f.entry for f in W.FORMS}
    for name in takers:
        if name in W.HELD_ELSEWHERE:
            path, needle = W.HELD_ELSEWHERE[name]
            assert needle in open(os.path.join(ROOT, path)).read(), f"{name} is listed as held by {path}, which no longer checks the workspace's margins"
        elif name in W.OBSERVABLES:
            assert any(name in f.observable for f in W.FORMS), f"{name} only names a way: a row must use it as its observable"
        else:
            assert name in rows, f"{name} takes a workspace_bytes and has no row in FORMS of tests/test_gpu_workspace_bounds.py"
    assert rows <= set(takers), f"rows for entries that take no workspace: {sorted(rows - set(takers))}"


def test_every_row_names_exported_symbols_and_two_to_four_shapes():
    ids = [f.id for f in W.FORMS]
    assert len(set(ids)) == len(ids)
    for f in W.FORMS:
        assert f.entry in HEADERS and f.query in HEADERS, f"{f.id}: {f.entry} / {f.query} is not exported by include/pq_hip.h or include/pq_rccl.h"
        assert re.search(r"workspace_bytes", f.query) and f.observable, f.id
        assert 2 <= len(f.shapes) <= 4, f.id
        for name, _ in f.options + tuple(o for opts, _ in f.shapes for o in opts):
            assert name.startswith("PQ_") and name in open(os.path.join(ROOT, "include", "pq_hip.h")).read(), (f.id, name)
    assert {f.id for f in W.FORMS if not f.contents} == {"s8-fsk-symmetric-2", "s8-fsk-symmetric-4"}, "step 3 is left out for the symmetric forms only"


# ---------------------------------------------------------------- the library's own answers (no launch)
@pytest.fixture
def L(pq_opt):
    from protoquant_amd import _lib
    pq_opt("PQ_FAKE_CUS", "256")
    return _lib.lib()


@pytest.mark.parametrize("form", [f for f in W.FORMS if f.kind in ("gemm", "gemm_t", "planned", "kslabs", "dyn")], ids=lambda f: f.id)
def test_every_gemm_row_reaches_its_form_on_256_cus(form, L, pq_opt):
    branches = set()
    for opts, args in form.shapes:
        for name, value in form.options + tuple(opts):
            pq_opt(name, value)
        c = W.make_case(form, args)
        need = c.need()
        assert need > 0 or form.id == "dyn-no-split", c.what
        c.assert_reached(need)
        if form.kind == "planned":
            assert W.planned_branch(c.M, c.N, 256) == c.inner[1], c.what
            branches.add(c.inner[1])
        if form.kind == "kslabs" and not c.short:
            smaller = c.way_at(need - 1)
            assert smaller == ("in place: ring128" if c.way.startswith("in place: fused") else "layout pass"), (c.what, smaller)
    assert form.kind != "planned" or branches == {128, 256}, "both tile heights of splitk_plan"


def test_exchange_rows_report_the_closed_forms_of_the_header():
    from protoquant_amd import _rccl
    for form in W.FORMS:
        if form.kind in ("allgather_cols", "allgather_cols_v", "rows_async", "reduce_scatter"):
            for _, args in form.shapes:
                c = W.make_case(form, args)
                c.assert_reached(c.need())
    R = _rccl.lib()
    for q in (R.pq_allgather_cols_workspace_bytes, R.pq_allgather_cols_v_workspace_bytes, R.pq_reduce_scatter_rows_workspace_bytes):
        for nr, m, n in ((1, 0, 5), (1, 5, 0), (1, -1, 5), (1, 5, -2), (0, 5, 5), (-1, 5, 5)):
            assert q(nr, m, n, 0) == 0, (nr, m, n)
    assert sum(R.pq_allgather_cols_v_workspace_bytes(1, m1 - m0, 517, 0) for m0, m1 in W.ROW_BLOCKS) == R.pq_allgather_cols_v_workspace_bytes(1, 37, 517, 0), \
        "the row blocks' slices tile the one workspace"
    assert sorted(W.ROW_BLOCKS) != list(W.ROW_BLOCKS) and len({m1 - m0 for m0, m1 in W.ROW_BLOCKS}) == 3, "three unequal blocks, issued out of order"


def test_the_never_tiled_shape_asks_for_no_workspace(L, pq_opt):
    for M, N, S, NT in W.NEVER_TILED:
        K = W.kt(S * NT)
        for name, value in (("PQ_FORCE_SPLITK", str(S)), ("PQ_FORCE_SPLITK", ""), ("PQ_FSK", str(S))):
            pq_opt(name, value)
            assert L.pq_gemm_variant_name(M, N, K, K, K) == b"generic64"
            assert L.pq_qlinear_workspace_bytes(M, N, K) == 0 and L.pq_qlinear_t_workspace_bytes(N, M, K) == 0
            assert L.pq_qlinear_dyn_workspace_bytes(M, N, K) == W.align256(M * K) + W.align256(4 * M)


OPTION_SETS = sorted({f.options + tuple(opts) for f in W.FORMS for opts, _ in f.shapes if f.kind in ("gemm", "gemm_t", "planned", "kslabs", "dyn")})
# (the edges of the 64-token and 128^2 thresholds and of the 128- / 256-row tiles +- 1; K around the 2048, 8192, 10240, 12288 and 24576 thresholds of the planners, K that is no
# multiple of 128, 256 or 512, K whose K-tiles no slice count of the table divides)
GRID_M = (-5, 0, 1, 63, 64, 65, 127, 128, 129, 130, 255, 256, 257, 300, 511, 512, 513, 1021, 1024, 1025, 2048, 4095, 4096)
GRID_N = (-300, -1000, 0, 1, 63, 127, 128, 130, 255, 256, 257, 259, 517, 1023, 1024, 1025, 2048, 4096)
GRID_K = (-128, 0, 100, 128, 640, 1000, 1408, 1920, 2048, 2560, 4096, 8064, 8192, 8320, 10240, 11008, 12288, 14336, 24576, 28672)
POSITIVE = sum(m > 0 for m in GRID_M) * sum(n > 0 for n in GRID_N) * sum(k > 0 for k in GRID_K)


def _closed_forms(M, N):
    return {S * M * N * 4 for S in range(2, 9)} | {W.fsk_bytes(M, N, S) for S in range(2, 9)}


@pytest.mark.parametrize("options", OPTION_SETS, ids=lambda o: ",".join(f"{n}={v}" for n, v in o) or "defaults")
def test_query_algebra(options, L, pq_opt):
    """gemm_s8_fast.hip: fsk_workspace_bytes(M, N, S) = fsk_counter_bytes(ntiles, S) + ntiles (S - 1) 256 x 256 x 4 with fsk_counter_bytes = align256(ntiles 4 (S == 4 ? 4 : 2))
    — the words launch_gemm_fsk zeroes and the offset at which launcher and kernel both put the first slab: W.fsk_bytes is derived from there."""
    for name, value in options:
        pq_opt(name, value)
    fake = 1 << 20
    assert POSITIVE >= 5000, "some thousands of positive shapes reach the identities below"
    for M, N, K in itertools.product(GRID_M, GRID_N, GRID_K):
        q = L.pq_qlinear_workspace_bytes(M, N, K)
        assert L.pq_qlinear_t_workspace_bytes(N, M, K) == q, (M, N, K)
        if M <= 0 or N <= 0 or K <= 0:
            assert q == 0, f"a split-K workspace of {q} bytes for the non-positive size {(M, N, K)}"
            assert L.pq_qlinear_kslabs_workspace_bytes(M, N, K, 128) == 0 and L.pq_qlinear_kslabs_workspace_bytes_for(fake, 128, max(M, 0) * 128, 128, fake, K, M, N, K) == 0
            # (K == 0 with M, N > 0 is a call that still quantises M empty rows: their scales go to the workspace)
            assert L.pq_qlinear_dyn_workspace_bytes(M, N, K) == (W.align256(4 * M) if K == 0 and M > 0 and N > 0 else 0), (M, N, K)
            continue
        assert q == 0 or q in _closed_forms(M, N), f"{q} bytes for {(M, N, K)} is neither S M N 4 nor the fused closed form"
        assert L.pq_qlinear_dyn_workspace_bytes(M, N, K) == W.align256(M * K) + W.align256(4 * M) + q, (M, N, K)
        for G in (2, 8):
            if K % (G * 16) == 0:
                kps = K // G
                always = L.pq_qlinear_kslabs_workspace_bytes(M, N, K, kps)
                exact = L.pq_qlinear_kslabs_workspace_bytes_for(fake, kps, M * kps, kps, fake, K, M, N, K)
                assert always == W.align256(M * K) + q and always >= exact and exact in ({0, always} | _closed_forms(M, N)), (M, N, K, G, always, exact)
