"""-m gpu: every entry of the C-ABI that takes a caller-owned workspace, launched in a workspace of EXACTLY the bytes its query reports — tests/guarded_workspace.py:
the interior between two sentinel margins of 516 KiB each — through the raw C-ABI, one row of FORMS per entry x form.  Every other GPU test reaches these paths through
protoquant_amd.qlinear._workspace (one buffer per stream that only grows) or sharded.py's allocators: a slab store past S M N 4, a ticket past fsk_counter_bytes, a hand-over
one tile too far or a layout pass into the pad would land in slack nobody reads.  Per row and shape, in this order:

  1. BOUNDS.  The interior zero-filled, the output a window of a poisoned buffer (tests/gemm_edges.py): status PQ_OK, the whole output buffer equals the reference bit for
     bit (Q.epilogue of the exact int32 product; C.quant_rowwise + that for pq_qlinear_dyn; the plain concatenation / the cast f32 sum for the exchanges), both margins intact.
  2. ONE BYTE LESS.  The same buffer with workspace_bytes - 1: status 5 (PQ_ERR_WORKSPACE) and an error string that names the workspace, output poison and margins
     untouched — the query is the tight bound the check enforces.  pq_qlinear_s8_kslabs may instead take a smaller way (pq_kslabs_way_name says which): same output.
  3. CONTENTS.  Only after step 1 of the whole row has passed: the interior pre-filled with 0xFF, then with the bytes ANOTHER launch left behind (a five-slice ticket launch
     over six tiles: other tickets, ready words and slabs wherever this launch looks): same output, margins intact.  Not for the symmetric forms, which wait on their flags.

The counters (read before step 3 was written).  launch_gemm_fsk zeroes fsk_counter_bytes(ntiles, S) / 4 words with fsk_zero_counters; fsk_counter_bytes = align256(ntiles * 4 *
(4 if S == 4 else 2)).  gemm_s8_sp256<FSK = 1> (the ticket form) indexes ctr[t] and ctr[ntiles + t], t < ntiles: 2 ntiles words; FSK = 2 / 4 (symmetric) index flags[FSK t ..
FSK t + FSK): 2 / 4 words per tile; the slabs start at fsk_counter_bytes of the same (ntiles, S) in launcher, kernel and query.  They agree: every word the kernels poll is
one the launcher zeroed, whatever the workspace held.

Each test synchronises twice: once behind step 1 of all its shapes (step 3 must not start on a row that failed step 1), once at its end; every check in between is a flag
left on the device.  Measured wall time of the file on one MI355X: 7.7 s for its 29 tests — tests/test_gpu_gemm_edges.py takes minutes.

A shape the planner never splits: M N < 128^2 (300 x 1) goes to the generic kernel, which has no split form, whatever slice count is forced.  The query is 0 wherever
qlinear_core would not look at a workspace, and a call that is handed one anyway leaves it alone (NEVER_TILED); the N = 1 tail of the reduction pass is covered by (16384, 1).
pq_qlinear_dyn_workspace_bytes is 0 for M = 0 or N = 0, where the call returns before it looks at its workspace.

The second half re-runs Python-level flows under guarded_workspace.patched_allocators (exactly the requested bytes, pre-filled with garbage) against the same call under the
stock allocators, bit for bit: a wrapper that asks the query under one option snapshot or device and launches under another would overrun or be refused there."""
import collections
import functools
import os

import numpy as np
import pytest
import torch

from oracle import qspec_numpy as Q
from tests import gemm_edges as E
from tests.guarded_workspace import Guarded, patched_allocators

pytestmark = pytest.mark.gpu

MEASURED = "29 tests in 7.7 s (pytest's own figure, one MI355X, the file run alone; the slowest, 3.7 s, is the first exchange row: it creates the RCCL communicator)"
PQ_OK, PQ_ERR_WORKSPACE = 0, 5
SLAB = 256 * 256 * 4
TILED = (b"sp256_16x16x64", b"sp128x256_16x16x64", b"ring128_16x16x64")      # qlinear_core's `tiled`: the dispatches that may split K


def kt(n):
    return 128 * n


def align256(v):
    return (v + 255) // 256 * 256


def fsk_bytes(M, N, S):
    """gemm_s8_fast.hip: fsk_workspace_bytes = fsk_counter_bytes(ntiles, S) + ntiles (S - 1) slabs of 256 x 256 int32"""
    ntiles = -(-M // 256) * -(-N // 256)
    return align256(ntiles * 4 * (4 if S == 4 else 2)) + ntiles * (S - 1) * SLAB


# ---------------------------------------------------------------- the table
# kind: which Case below launches the row;  entry / query: the C symbols;  options: pq_set_option switches of the whole row;  observable: how the row proves that it reached
# its form;  shapes: (per-shape switches, arguments of the Case);  contents: step 3 applies
Form = collections.namedtuple("Form", "id kind entry query options observable shapes contents")
BF16, FP16, F32 = 0, 1, 2


def _forced(M, N, S, NT, code, bias):
    return ((("PQ_FORCE_SPLITK", str(S)),), (M, N, kt(S * NT), code, bias, ("twopass", S)))


def _ticket(M, N, S, tiles, code, bias):
    return ((), (M, N, kt(tiles), code, bias, ("fsk", S)))


def _ticket_rows(S):
    return (_ticket(257, 259, S, 5 * S, BF16, True), _ticket(257, 259, S, 5 * S + 1, F32, False), _ticket(512, 300, S, 5 * S + 1, FP16, True), _ticket(130, 130, S, 5 * S, BF16, False))


FORMS = (
    # (K = S NT 128; NT >= 5: launch_gemm_splitk_i32<256> runs the split-ring tile with the asm K-loop, NT = 4 the HIP ring.  Odd M N: slab bases 4- / 8-byte aligned only;
    # N = 1 and N = 3 mod 4: the vector tail of splitk_reduce_epilogue.  (16384, 1): see NEVER_TILED below)
    Form("s8-twopass-forced", "gemm", "pq_qlinear_s8", "pq_qlinear_workspace_bytes", (), "pq_gemm_variant_name in TILED and the query == S M N 4",
         (_forced(257, 259, 3, 5, BF16, True), _forced(130, 517, 2, 4, F32, True), _forced(16384, 1, 2, 5, BF16, False), _forced(65, 255, 5, 5, FP16, False)), True),
    # splitk_plan: tm = (t256 <= cus 5 / 8 && t128 > t256 && t128 <= cus) ? 128 : 256, tiles <= cus / 4, K >= 8192.  The candidates of each branch, in order; the first
    # whose branch condition holds at the CU count of this device runs (planned_branch restates the condition: bookkeeping only)
    Form("s8-twopass-planned", "planned", "pq_qlinear_s8", "pq_qlinear_workspace_bytes", (("PQ_NO_MIDM", "1"),), "pq_gemm_variant_name in TILED and the query == S M N 4, S in 2 .. 8",
         (((), (1021, 1019, kt(64), BF16, True, ("planned", 128))), ((), (300, 260, kt(64), FP16, False, ("planned", 128))),
          ((), (127, 1021, kt(64), F32, True, ("planned", 256))), ((), (100, 517, kt(64), BF16, False, ("planned", 256)))), True),
) + tuple(
    # fsk_plan, forced: f slices wherever K % 128 == 0 && (K / 128) / f >= 5; 5 S + 1 K-tiles: uneven slices.  4, 4 and 1 tiles, edge tiles through the direct epilogue
    Form(f"s8-fsk-ticket-{S}", "gemm", "pq_qlinear_s8", "pq_qlinear_workspace_bytes", (("PQ_FSK", str(S)),), "pq_gemm_variant_name in TILED and the query == the fused closed form",
         _ticket_rows(S), True) for S in (2, 3, 4, 8)
) + tuple(
    # launch_gemm_fsk: `kslices == 2 && sym` / `kslices == 4 && sym` pick gemm_s8_sp256<FSK = 2 / 4>; fsk_plan admits them when K % (128 f) == 0 and f tiles <= the CUs
    Form(f"s8-fsk-symmetric-{S}", "gemm", "pq_qlinear_s8", "pq_qlinear_workspace_bytes", (("PQ_FSK", str(S)), ("PQ_FSK_SYMMETRIC", "1")),
         "the query == the fused closed form; launch_gemm_fsk's `kslices == S && opt().fsk_symmetric`",
         (_ticket(300, 520, S, 5 * S, BF16, True), _ticket(512, 512, S, 5 * S, F32, False)), False) for S in (2, 4)
) + (
    Form("s8t-twopass-forced", "gemm_t", "pq_qlinear_s8_t", "pq_qlinear_t_workspace_bytes", (), "pq_gemm_variant_name(N, M) in TILED and the query == S M N 4",
         (_forced(259, 257, 3, 5, BF16, True), _forced(517, 130, 2, 4, F32, False)), True),
    Form("s8t-fsk-ticket-3", "gemm_t", "pq_qlinear_s8_t", "pq_qlinear_t_workspace_bytes", (("PQ_FSK", "3"),), "pq_gemm_variant_name(N, M) in TILED and the query == the fused closed form of (N, M)",
         (_ticket(259, 257, 3, 16, FP16, True), _ticket(300, 512, 3, 15, BF16, False)), True),
    # kslabs shapes: (M, N, G slabs, k_per_slab, lda, dtype, bias, expected way, inner form)
    Form("kslabs-fused-in-place", "kslabs", "pq_qlinear_s8_kslabs", "pq_qlinear_kslabs_workspace_bytes_for", (("PQ_FSK", "2"),), "pq_kslabs_way_name",
         (((), (257, 259, 2, kt(5), kt(5), BF16, True, "in place: fused split-K x2", ("fsk", 2))), ((), (65, 255, 4, kt(9), kt(9), F32, False, "in place: fused split-K x2", ("fsk", 2))),
          ((), (130, 300, 8, kt(4), kt(4), FP16, True, "in place: fused split-K x2", ("fsk", 2)))), True),
    # ("short": a workspace ONE BYTE smaller than the way above needs: not an error — the ring tile walks the slabs in place and nothing is written anywhere)
    Form("kslabs-ring-one-byte-short", "kslabs", "pq_qlinear_s8_kslabs", "pq_qlinear_kslabs_workspace_bytes_for", (("PQ_FSK", "2"),), "pq_kslabs_way_name",
         (((), (257, 259, 2, kt(5), kt(5), BF16, True, "in place: ring128", "short")), ((), (65, 255, 4, kt(9), kt(9), F32, False, "in place: ring128", "short")),
          ((), (130, 300, 8, kt(4), kt(4), FP16, True, "in place: ring128", "short"))), True),
    # unstack_kslabs_kernel<v4u_> (k_per_slab, lda, slab stride all multiples of 16) and <uint8_t> (k_per_slab = 600; lda = 152): M K = 76960, 616800, 74880, none a
    # multiple of 256 — the pad behind the flat codes is 96 .. 160 bytes
    Form("kslabs-layout-pass", "kslabs", "pq_qlinear_s8_kslabs", "pq_qlinear_kslabs_workspace_bytes_for", (), "pq_kslabs_way_name",
         (((), (65, 255, 2, 592, 592, BF16, True, "layout pass", ("none", 0))), ((), (257, 130, 4, 600, 600, F32, False, "layout pass", ("none", 0))),
          ((), (65, 130, 8, 144, 152, FP16, True, "layout pass", ("none", 0)))), True),
    # (slabs that are no whole K-tiles take the layout pass; K = 11, 11 and 13 K-tiles: M K = 128 mod 256, and the ticket form's counters start in "the rest", behind the pad)
    Form("kslabs-layout-then-ticket", "kslabs", "pq_qlinear_s8_kslabs", "pq_qlinear_kslabs_workspace_bytes_for", (("PQ_FSK", "2"),), "pq_kslabs_way_name; the rest == the fused closed form",
         (((), (65, 255, 2, 704, 704, BF16, True, "layout pass", ("fsk", 2))), ((), (257, 130, 4, 352, 352, F32, False, "layout pass", ("fsk", 2))),
          ((), (257, 259, 8, 208, 208, FP16, True, "layout pass", ("fsk", 2)))), True),
    # (K = 1920 = 3 slices of five K-tiles in slabs of 7.5, 3.75 and 1.875 K-tiles: M K = 128 mod 256, the two-pass slabs start behind a 128-byte pad)
    Form("kslabs-layout-then-twopass", "kslabs", "pq_qlinear_s8_kslabs", "pq_qlinear_kslabs_workspace_bytes_for", (("PQ_FORCE_SPLITK", "3"),),
         "pq_kslabs_way_name; the rest == S M N 4",
         (((), (65, 255, 2, 960, 960, BF16, True, "layout pass", ("twopass", 3))), ((), (257, 130, 4, 480, 480, F32, False, "layout pass", ("twopass", 3))),
          ((), (257, 259, 8, 240, 240, FP16, True, "layout pass", ("twopass", 3)))), True),
    # dyn shapes: (M, N, K, dtype, bias, inner form); K an odd number of K-tiles: M K and 4 M both fall short of 256-byte multiples
    Form("dyn-no-split", "dyn", "pq_qlinear_dyn", "pq_qlinear_dyn_workspace_bytes", (), "the query == align256(M K) + align256(4 M)",
         (((), (65, 255, kt(11), BF16, True, ("none", 0))), ((), (257, 259, kt(17), FP16, False, ("none", 0))), ((), (257, 130, kt(13), F32, True, ("none", 0)))), True),
    Form("dyn-twopass", "dyn", "pq_qlinear_dyn", "pq_qlinear_dyn_workspace_bytes", (("PQ_FORCE_SPLITK", "3"),), "the query == align256(M K) + align256(4 M) + S M N 4",
         (((), (65, 255, kt(15), BF16, True, ("twopass", 3))), ((), (257, 259, kt(15), F32, False, ("twopass", 3))), ((), (257, 130, kt(15), FP16, True, ("twopass", 3)))), True),
    Form("dyn-fsk-ticket", "dyn", "pq_qlinear_dyn", "pq_qlinear_dyn_workspace_bytes", (("PQ_FSK", "2"),), "the query == align256(M K) + align256(4 M) + the fused closed form",
         (((), (65, 255, kt(11), FP16, True, ("fsk", 2))), ((), (257, 259, kt(19), BF16, False, ("fsk", 2))), ((), (257, 130, kt(11), F32, True, ("fsk", 2)))), True),
    # exchange shapes: (M, n, dtype, leading dimension of the shard)
    Form("allgather-cols", "allgather_cols", "pq_allgather_cols", "pq_allgather_cols_workspace_bytes", (), "the query == nranks M n_shard sizeof(dtype)",
         (((), (37, 517, BF16, 517)), ((), (37, 517, F32, 517)), ((), (5, 7, BF16, 7))), True),
    Form("allgather-cols-v", "allgather_cols_v", "pq_allgather_cols_v", "pq_allgather_cols_v_workspace_bytes", (), "the query == (nranks + 1) M ceil(n_total / nranks) sizeof(dtype)",
         (((), (37, 517, BF16, 517)), ((), (37, 517, F32, 520)), ((), (37, 70, BF16, 77))), True),
    # (three row blocks of unequal length, issued out of order: each owns the slice of the ONE workspace at gather_ws_bytes(nranks, m0, ...))
    Form("allgather-cols-rows-async", "rows_async", "pq_allgather_cols_rows_async", "pq_allgather_cols_v_workspace_bytes", (), "the query == (nranks + 1) M ceil(n_total / nranks) sizeof(dtype)",
         (((), (37, 517, BF16, 517)), ((), (37, 517, F32, 523))), True),
    Form("reduce-scatter-rows", "reduce_scatter", "pq_reduce_scatter_rows", "pq_reduce_scatter_rows_workspace_bytes", (), "the query == m_shard N 4 for a 16-bit output, 0 for f32",
         (((), (37, 517, BF16, 517)), ((), (37, 517, F32, 517)), ((), (48, 200, FP16, 200))), True),
)
# entries with a workspace_bytes parameter that another file holds to the queried size, or that only NAME a form: tests/test_workspace_bounds_host.py reads these
HELD_ELSEWHERE = {"pq_moe_route": ("tests/test_gpu_moe_route.py", "a margin of the workspace was written")}
OBSERVABLES = ("pq_kslabs_way_name",)
ROW_BLOCKS = ((23, 37), (0, 5), (5, 23))
# M N < 128^2: pick_variant answers generic64 for any K — a 256 x 256 tile would be mostly padding — so NO K split is ever launched for it, whatever is forced; the
# two-pass reduce at N = 1 is reached by (16384, 1) above instead.  What holds here: the query is 0, and a call that is handed a workspace anyway leaves it alone.
NEVER_TILED = ((300, 1, 2, 5),)


def planned_branch(M, N, cus):
    """splitk_plan's tile height for (M, N) on `cus` CUs — BOOKKEEPING ONLY (which branch a candidate covers), never a source of an expected value"""
    t256, t128 = -(-M // 256) * -(-N // 256), -(-M // 128) * -(-N // 256)
    return 128 if (t256 <= cus * 5 // 8 and t128 > t256 and t128 <= cus) else 256


# ---------------------------------------------------------------- operands and references (computed once per shape)
def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _as_bits(y, code):
    return y.view(np.uint32) if code == 2 else y


@functools.lru_cache(maxsize=None)
def gemm_problem(M, N, K, code, bias):
    rng = np.random.default_rng([M, N, K, code, int(bias)])
    a = rng.integers(-128, 128, (M, K), dtype=np.int8)
    b = rng.integers(-128, 128, (N, K), dtype=np.int8)
    xs = (rng.random(M, dtype=np.float32) * 0.1 + 1e-3).astype(np.float32)
    ws = (rng.random(N, dtype=np.float32) * 0.01 + 1e-4).astype(np.float32)
    bv = Q.from_f32(rng.standard_normal(N).astype(np.float32), code) if bias else None
    want = _as_bits(Q.epilogue(Q.gemm_s8s8s32(a, b), xs, ws, bv, code), code)
    return dict(a=a, b=b, xs=xs, ws=ws, bias=bv, want=want)


@functools.lru_cache(maxsize=None)
def dyn_problem(M, N, K, code, bias):
    from oracle import c_oracle as C
    rng = np.random.default_rng([M, N, K, code, int(bias), 7])
    x = Q.from_f32((rng.standard_normal((M, K)) * 1.5).astype(np.float32), code)
    b = rng.integers(-128, 128, (N, K), dtype=np.int8)
    ws = (rng.random(N, dtype=np.float32) * 0.01 + 1e-4).astype(np.float32)
    bv = Q.from_f32(rng.standard_normal(N).astype(np.float32), code) if bias else None
    xq, xs = C.quant_rowwise(x, code)
    want = _as_bits(Q.epilogue(Q.gemm_s8s8s32(xq, b), xs, ws, bv, code), code)
    return dict(x=x, b=b, ws=ws, bias=bv, want=want)


class Output:
    """a window [rows, cols] of a poisoned flat buffer (tests/gemm_edges.py) and the whole buffer a correct launch leaves"""

    def __init__(self, window, code, mode="contig"):
        rows, cols = window.shape
        self.code, self.lay = code, E.layout(rows, cols, mode)
        self.want = _dev(E.expected_buffer(window, self.lay, code))
        self.poison = _dev(np.full(self.lay.total, E.POISON[code], E.bits_dtype(code)))
        self.buf = self.poison.clone()
        self.ptr = self.buf.data_ptr() + self.lay.offset * E.ITEM[code]
        self.ld = self.lay.ld

    def reset(self):
        self.buf.copy_(self.poison)

    def explain(self, snap, want):
        bad = E.first_bad(snap.cpu().numpy(), want.cpu().numpy(), self.lay)
        where = "element" if bad.inside else "MARGIN element"
        return f"{bad.count} elements of the output buffer differ, first at {where} [{bad.row}, {bad.col}] (got 0x{bad.got & 0xFFFFFFFF:X}, want 0x{bad.want & 0xFFFFFFFF:X})"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _hip():
    from protoquant_amd import _lib
    return _lib.lib()


def _rccl_error():
    from protoquant_amd import _rccl
    return _rccl.lib().pq_rccl_last_error()


class AlignedNowhere:
    """an operand the planners only look at the alignment of"""
    data_ptr = staticmethod(lambda: 1 << 20)


class Case:
    """one shape of a row: operands on the device, the guarded output, the query, the proof that the form is reached, and the launch"""
    lib_error = staticmethod(lambda: _hip().pq_last_error())
    less_refuses = True

    def variant(self, M, N, K):
        return _hip().pq_gemm_variant_name(M, N, K, K, K)

    def inner_bytes(self, M, N, inner):
        form, S = inner
        return {"twopass": S * M * N * 4, "fsk": fsk_bytes(M, N, S), "none": 0}[form]

    def assert_tiled(self, M, N, K, inner):
        if inner[0] != "none":
            name = self.variant(M, N, K)
            assert name.startswith(TILED), f"{self.what}: dispatched to {name}: no K split is launched for it — the row would run single-pass"


class GemmCase(Case):
    def __init__(self, form, args, transposed=False, plan_only=False):
        self.M, self.N, self.K, self.code, self.has_bias, self.inner = args
        self.t, self.what = transposed, f"{form.id} M={args[0]} N={args[1]} K={args[2]} dtype={args[3]} bias={args[4]}"
        if plan_only:
            return
        p = gemm_problem(*args[:5])
        self.a, self.b, self.xs, self.ws = _dev(p["a"]), _dev(p["b"]), _dev(p["xs"]), _dev(p["ws"])
        self.bias = _dev(p["bias"]) if self.has_bias else None
        self.out = Output(np.ascontiguousarray(p["want"].T) if transposed else p["want"], self.code)

    def need(self):
        L = _hip()
        return (L.pq_qlinear_t_workspace_bytes if self.t else L.pq_qlinear_workspace_bytes)(self.M, self.N, self.K)

    def assert_reached(self, need):
        gm, gn = (self.N, self.M) if self.t else (self.M, self.N)          # (the transposed entry runs the GEMM with the weight rows as its rows)
        self.assert_tiled(gm, gn, self.K, self.inner)
        if self.inner[0] == "planned":
            S = need // (self.M * self.N * 4)
            assert need == S * self.M * self.N * 4 and 2 <= S <= 8, f"{self.what}: {need} bytes is not S M N 4 for an S in 2 .. 8"
        else:
            assert need == self.inner_bytes(gm, gn, self.inner) > 0, f"{self.what}: the query reports {need} bytes, the form needs {self.inner_bytes(gm, gn, self.inner)}"

    def launch(self, ptr, nbytes):
        fn = _hip().pq_qlinear_s8_t if self.t else _hip().pq_qlinear_s8
        return fn(self.a.data_ptr(), self.K, self.xs.data_ptr(), self.b.data_ptr(), self.K, self.ws.data_ptr(), self.bias.data_ptr() if self.has_bias else None,
                  self.out.ptr, self.out.ld, self.code, self.M, self.N, self.K, ptr, nbytes, _stream())


class PlannedCase(GemmCase):
    def assert_tiled(self, M, N, K, inner):
        assert self.variant(M, N, K).startswith(TILED), self.what


class KslabsCase(Case):
    less_refuses = False          # (a smaller workspace may select a smaller way)

    def __init__(self, form, args, plan_only=False):
        self.M, self.N, self.G, self.kps, self.lda, self.code, self.has_bias, self.way, self.inner = args
        self.K = self.G * self.kps
        self.what = f"{form.id} M={self.M} N={self.N} G={self.G} k_per_slab={self.kps} lda={self.lda} dtype={self.code}"
        self.stride, self.short = self.M * self.lda, self.inner == "short"
        if plan_only:
            self.a = self.b = AlignedNowhere()
            return
        p = gemm_problem(self.M, self.N, self.K, self.code, self.has_bias)
        stacked = np.full((self.G, self.M, self.lda), E.OPERAND_POISON, np.int8)
        stacked[:, :, :self.kps] = p["a"].reshape(self.M, self.G, self.kps).transpose(1, 0, 2)
        self.a, self.b, self.xs, self.ws = _dev(stacked), _dev(p["b"]), _dev(p["xs"]), _dev(p["ws"])
        self.bias = _dev(p["bias"]) if self.has_bias else None
        self.out = Output(p["want"], self.code)

    def _operands(self):
        return (self.a.data_ptr(), self.lda, self.stride, self.kps, self.b.data_ptr(), self.K, self.M, self.N, self.K)

    def way_at(self, nbytes):
        return _hip().pq_kslabs_way_name(*self._operands(), nbytes).decode()

    def need(self):
        return _hip().pq_qlinear_kslabs_workspace_bytes_for(*self._operands()) - (1 if self.short else 0)

    def assert_reached(self, need):
        L = _hip()
        assert self.way_at(need) == self.way, f"{self.what}: takes the way {self.way_at(need)!r} with {need} bytes, the row is about {self.way!r}"
        if self.short:
            assert need + 1 == fsk_bytes(self.M, self.N, 2) and self.way_at(need + 1) == "in place: fused split-K x2", self.what
            return
        self.assert_tiled(self.M, self.N, self.K, self.inner)
        flat = align256(self.M * self.K) if self.way == "layout pass" else 0
        assert need == flat + self.inner_bytes(self.M, self.N, self.inner), f"{self.what}: the query reports {need} bytes"
        assert L.pq_qlinear_kslabs_workspace_bytes(self.M, self.N, self.K, self.kps) >= need, f"{self.what}: the short query is not always enough"

    def launch(self, ptr, nbytes):
        return _hip().pq_qlinear_s8_kslabs(self.a.data_ptr(), self.lda, self.stride, self.kps, self.xs.data_ptr(), self.b.data_ptr(), self.K, self.ws.data_ptr(),
                                           self.bias.data_ptr() if self.has_bias else None, self.out.ptr, self.out.ld, self.code, self.M, self.N, self.K, ptr, nbytes, _stream())


class DynCase(Case):
    def __init__(self, form, args, plan_only=False):
        self.M, self.N, self.K, self.code, self.has_bias, self.inner = args
        self.what = f"{form.id} M={self.M} N={self.N} K={self.K} dtype={self.code}"
        if plan_only:
            return
        p = dyn_problem(*args[:5])
        self.x, self.b, self.ws = _dev(p["x"]), _dev(p["b"]), _dev(p["ws"])
        self.bias = _dev(p["bias"]) if self.has_bias else None
        self.out = Output(p["want"], self.code)

    def need(self):
        return _hip().pq_qlinear_dyn_workspace_bytes(self.M, self.N, self.K)

    def assert_reached(self, need):
        self.assert_tiled(self.M, self.N, self.K, self.inner)
        inner = self.inner_bytes(self.M, self.N, self.inner)
        assert _hip().pq_qlinear_workspace_bytes(self.M, self.N, self.K) == inner, f"{self.what}: the GEMM inside plans {_hip().pq_qlinear_workspace_bytes(self.M, self.N, self.K)} bytes"
        assert (self.M * self.K) % 256 != 0 and (4 * self.M) % 256 != 0, "both carved regions end in a pad"
        assert need == align256(self.M * self.K) + align256(4 * self.M) + inner, f"{self.what}: the query reports {need} bytes"

    def launch(self, ptr, nbytes):
        return _hip().pq_qlinear_dyn(self.x.data_ptr(), self.code, self.K, self.b.data_ptr(), self.K, self.ws.data_ptr(), self.bias.data_ptr() if self.has_bias else None,
                                     self.out.ptr, self.out.ld, self.M, self.N, self.K, ptr, nbytes, _stream())


class ExchangeCase(Case):
    """world 1: the gather of one shard is the shard, the reduce-scatter of one partial is its cast"""
    lib_error = staticmethod(lambda: _rccl_error())

    def __init__(self, form, args, gather, plan_only=False):
        from protoquant_amd import _rccl
        self.R, self.kind = _rccl.lib(), form.kind
        self.M, self.n, self.code, self.ld = args
        self.what = f"{form.id} M={self.M} n={self.n} dtype={self.code} ld_shard={self.ld}"
        if plan_only:
            return
        self.comm = gather._comm
        rng = np.random.default_rng([self.M, self.n, self.code, self.ld])
        eb = E.ITEM[self.code]
        if self.kind == "reduce_scatter":
            part = rng.standard_normal((self.M, self.n)).astype(np.float32)
            self.src = _dev(part)
            window = _as_bits(Q.from_f32(part, self.code), self.code)
        else:
            wide = rng.integers(1, 0x7000 if eb == 2 else 0x70000000, (self.M, self.ld)).astype(E.bits_dtype(self.code))      # (bit patterns of finite positive numbers)
            self.src = _dev(wide)
            window = np.ascontiguousarray(wide[:, :self.n])
        self.out = Output(window, self.code, "contig" if self.kind in ("allgather_cols", "reduce_scatter") else "ld8")

    def need(self):
        R = self.R
        return {"allgather_cols": R.pq_allgather_cols_workspace_bytes, "allgather_cols_v": R.pq_allgather_cols_v_workspace_bytes,
                "rows_async": R.pq_allgather_cols_v_workspace_bytes, "reduce_scatter": R.pq_reduce_scatter_rows_workspace_bytes}[self.kind](1, self.M, self.n, self.code)

    def assert_reached(self, need):
        eb = E.ITEM[self.code]
        want = {"allgather_cols": self.M * self.n * eb, "allgather_cols_v": 2 * self.M * self.n * eb, "rows_async": 2 * self.M * self.n * eb,
                "reduce_scatter": 0 if self.code == 2 else self.M * self.n * 4}[self.kind]
        assert need == want, f"{self.what}: the query reports {need} bytes, pq_rccl.h says {want}"

    def launch(self, ptr, nbytes):
        R, st = self.R, _stream()
        if self.kind == "allgather_cols":
            return R.pq_allgather_cols(self.comm, 1, self.src.data_ptr(), self.out.ptr, self.M, self.n, self.code, ptr, nbytes, st)
        if self.kind == "allgather_cols_v":
            return R.pq_allgather_cols_v(self.comm, self.src.data_ptr(), self.ld, self.out.ptr, self.out.ld, self.M, self.n, self.code, ptr, nbytes, st)
        if self.kind == "reduce_scatter":
            return R.pq_reduce_scatter_rows(self.comm, 1, self.src.data_ptr(), self.out.ptr, self.M, self.n, self.code, ptr, nbytes, st)
        for m0, m1 in ROW_BLOCKS:
            rc = R.pq_allgather_cols_rows_async(self.comm, self.src.data_ptr(), self.ld, self.out.ptr, self.out.ld, self.M, m0, m1, self.n, self.code, ptr, nbytes, st)
            if rc != PQ_OK:
                return rc
        return R.pq_comm_join(self.comm, st)


def make_case(form, args, request=None):
    """request = None: the PLAN of the case only (queries and names: no device, no operands) — tests/test_workspace_bounds_host.py"""
    plan_only = request is None
    if form.kind in ("gemm", "gemm_t"):
        return GemmCase(form, args, transposed=form.kind == "gemm_t", plan_only=plan_only)
    if form.kind == "planned":
        return PlannedCase(form, args, plan_only=plan_only)
    if form.kind == "kslabs":
        return KslabsCase(form, args, plan_only=plan_only)
    if form.kind == "dyn":
        return DynCase(form, args, plan_only=plan_only)
    return ExchangeCase(form, args, None if plan_only else request.getfixturevalue("gather"), plan_only=plan_only)


# ---------------------------------------------------------------- checks left on the device, read once
class Checks:
    def __init__(self):
        self.items = []

    def output(self, case, want, what):
        snap = case.out.buf.clone()
        self.items.append(((snap == want).all(), lambda: f"{what}: " + case.out.explain(snap, want)))

    def margins(self, g, what):
        self.items.append((g.margins_intact(), lambda: g.describe(what)))

    def interior(self, g, fill, what):
        self.items.append(((g.interior == fill).all(), lambda: f"{what}: {int((g.interior != fill).sum())} bytes of the workspace were written"))

    def read(self):
        """ONE synchronisation: every flag queued so far"""
        if not self.items:
            return
        flags = torch.stack([f for f, _ in self.items]).cpu().tolist()
        bad = [explain for ok, (_, explain) in zip(flags, self.items) if not ok]
        self.items = []
        assert not bad, "\n".join(e() for e in bad)


# ---------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def donor():
    """what ANOTHER launch leaves in its workspace: the ticket form with five slices over the six tiles of 300 x 520 — other tile and slice counts than any row's"""
    from protoquant_amd import _lib
    M, N, S = 300, 520, 5
    form = Form("donor", "gemm", "pq_qlinear_s8", "pq_qlinear_workspace_bytes", (), "", (), False)
    _lib.set_option("PQ_FSK", str(S))
    try:
        c = GemmCase(form, (M, N, kt(5 * S), BF16, True, ("fsk", S)))
        need = c.need()
        c.assert_reached(need)
        g = Guarded(need, 0, "cuda")
        assert c.launch(g.ptr, need) == PQ_OK, _lib.lib().pq_last_error()
    finally:
        _lib.set_option("PQ_FSK", "")
    checks = Checks()
    checks.output(c, c.out.want, "donor")
    checks.margins(g, "donor")
    checks.read()
    assert bool(g.interior[:256].any()) and bool(g.interior[256:].any()), "the donor left counters and slabs behind"
    return g


@pytest.fixture(scope="module")
def gather():
    """a world-1 RCCL communicator, made the way tests/test_gpu_parity.py::test_native_rccl_gather makes its own"""
    import torch.distributed as dist
    import protoquant_amd as pq
    from protoquant_amd import _rccl
    if not os.path.exists(_rccl.LIB_PATH):
        pytest.skip("libpq_rccl.so is not built")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29547")
    created = False
    if not dist.is_initialized():
        dist.init_process_group("gloo", rank=0, world_size=1)
        created = True
    g = pq.RcclColumnGather()
    assert g.comm_ranks() == 1
    yield g
    torch.cuda.synchronize()
    g.close()
    if created:
        dist.destroy_process_group()


# ---------------------------------------------------------------- the rows
def _apply(pq_opt, form, opts):
    for name, value in form.options + tuple(opts):
        pq_opt(name, value)


def _select(form, cases):
    """the planned row: the first candidate of each branch of splitk_plan that the branch condition admits at this device's CU count"""
    if form.kind != "planned":
        return cases, None
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    picked, missing = [], []
    for tm in (128, 256):
        mine = [(o, c) for o, c in cases if c.inner[1] == tm and planned_branch(c.M, c.N, cus) == tm]      # (a candidate of a reached branch that plans no split FAILS in assert_reached)
        picked += mine[:1]
        if not mine:
            missing.append(f"no candidate under 1024 x 1024 x 8192 reaches splitk_plan's tm = {tm} branch on {cus} CUs")
    return picked, "; ".join(missing) or None


@pytest.mark.parametrize("form", FORMS, ids=[f.id for f in FORMS])
def test_exact_workspace(form, pq_opt, donor, request):
    _apply(pq_opt, form, ())
    cases = []
    for opts, args in form.shapes:
        _apply(pq_opt, form, opts)
        cases.append((opts, make_case(form, args, request)))
    cases, unreached = _select(form, cases)
    checks, live = Checks(), []
    # ---- step 1: bounds
    for opts, c in cases:
        _apply(pq_opt, form, opts)
        need = c.need()
        c.assert_reached(need)
        g = Guarded(need, 0, "cuda")
        rc = c.launch(g.ptr, need)
        assert rc == PQ_OK, f"{c.what}: status {rc} with the queried {need} bytes: {c.lib_error()}"
        checks.output(c, c.out.want, f"{c.what}: step 1")
        checks.margins(g, f"{c.what}: step 1")
        if getattr(c, "short", False):
            checks.interior(g, 0, f"{c.what}: step 1 (the ring tile needs no workspace)")
        live.append((opts, c, g, need))
    checks.read()
    for opts, c, g, need in live:
        _apply(pq_opt, form, opts)
        # ---- step 2: one byte less
        if need > 0 and not getattr(c, "short", False):
            c.out.reset()
            smaller_way = not c.less_refuses and c.way_at(need - 1) != c.way_at(need)
            rc = c.launch(g.ptr, need - 1)
            if smaller_way:
                assert rc == PQ_OK, f"{c.what}: {need - 1} bytes select the way {c.way_at(need - 1)!r}, yet status {rc}: {c.lib_error()}"
                checks.output(c, c.out.want, f"{c.what}: step 2, the way {c.way_at(need - 1)!r}")
            else:
                assert rc == PQ_ERR_WORKSPACE, f"{c.what}: status {rc} instead of 5 with one byte less than the queried {need}"
                assert b"workspace" in c.lib_error(), c.lib_error()
                checks.output(c, c.out.poison, f"{c.what}: step 2, a refused call wrote its output")
            checks.margins(g, f"{c.what}: step 2")
        # ---- step 3: the previous contents of the workspace
        if form.contents:
            for name in ("0xFF", "another launch's leftovers"):
                g.refill(0xFF) if name == "0xFF" else g.refill_from(donor)
                fill = None if not getattr(c, "short", False) else g.interior.clone()
                c.out.reset()
                rc = c.launch(g.ptr, need)
                assert rc == PQ_OK, f"{c.what}: status {rc} on a workspace that held {name}: {c.lib_error()}"
                checks.output(c, c.out.want, f"{c.what}: step 3, workspace pre-filled with {name}")
                checks.margins(g, f"{c.what}: step 3 ({name})")
                if fill is not None:
                    checks.interior(g, fill, f"{c.what}: step 3 ({name})")
    checks.read()
    if unreached:
        pytest.skip(unreached)


@pytest.mark.parametrize("M,N,S,NT", NEVER_TILED)
def test_a_shape_the_planner_never_splits_leaves_a_workspace_alone(M, N, S, NT, pq_opt):
    pq_opt("PQ_FORCE_SPLITK", str(S))
    form = Form("never-tiled", "gemm", "pq_qlinear_s8", "pq_qlinear_workspace_bytes", (), "", (), False)
    c = GemmCase(form, (M, N, kt(S * NT), BF16, True, ("none", 0)))
    assert c.variant(M, N, c.K) == b"generic64" and c.need() == 0, "no split is launched: the query must not ask for a workspace the call would not check"
    g = Guarded(S * M * N * 4, 0xFF, "cuda")
    checks = Checks()
    for nbytes in (g.nbytes, 1):
        c.out.reset()
        assert c.launch(g.ptr, nbytes) == PQ_OK, c.lib_error()
        checks.output(c, c.out.want, f"{c.what} with {nbytes} bytes")
        checks.margins(g, c.what)
        checks.interior(g, 0xFF, c.what)
    checks.read()


# ---------------------------------------------------------------- the Python-level flows under exact allocators
def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _stock_then_guarded(monkeypatch, run, what, expect_workspace=True):
    import protoquant_amd as pq
    want = run()
    torch.cuda.synchronize()
    pq.clear_workspaces()
    with monkeypatch.context() as mp:
        handed = patched_allocators(mp)
        got = run()
        torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want)), f"{what}: the result under exact-size workspaces differs from the stock allocators'"
    assert handed or not expect_workspace, f"{what}: no workspace was asked for — the flow does not reach what it is here for"
    for g in handed:
        g.assert_margins(f"{what} ({g.nbytes} bytes)")
    return handed


def test_flow_qlinear_module_that_plans_a_split(monkeypatch, pq_opt):
    import protoquant_amd as pq
    M, N, K = 300, 260, 8192                                   # (tests/test_gpu_parity.py::test_splitk_bit_identical)
    pq_opt("PQ_NO_MIDM", "1")
    assert _hip().pq_qlinear_workspace_bytes(M, N, K) == 4 * M * N * 4
    torch.manual_seed(1)
    m = pq.qlinear.from_linear(torch.nn.Linear(K, N, bias=True, device="cuda", dtype=torch.bfloat16))
    x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
    handed = _stock_then_guarded(monkeypatch, lambda: m(x), "qlinear module")
    assert [g.nbytes for g in handed] == [_hip().pq_qlinear_dyn_workspace_bytes(M, N, K)]
    xq = pq.quantize(x)
    handed = _stock_then_guarded(monkeypatch, lambda: m(xq), "qlinear module on a QTensor")
    assert [g.nbytes for g in handed] == [4 * M * N * 4]


def test_flow_qlinear_dyn(monkeypatch):
    import protoquant_amd as pq
    torch.manual_seed(2)
    w = pq.quantize(torch.randn(640, 512, device="cuda", dtype=torch.float16))
    x = torch.randn(3, 32, 512, device="cuda", dtype=torch.float16)
    _stock_then_guarded(monkeypatch, lambda: pq.qlinear_dyn(x, w.int_data, w.scale), "qlinear_dyn")


def test_flow_gated_mlp(monkeypatch, pq_opt):
    import protoquant_amd as pq
    torch.manual_seed(5)
    H, I, M = 256, 1408, 96                                    # (tests/test_gpu_parity.py::test_swap_linears_on_mlp, with an intermediate of eleven K-tiles)
    mlp = pq.GatedMLP.from_linears(*(torch.nn.Linear(i, o, bias=False, device="cuda", dtype=torch.bfloat16) for i, o in ((H, I), (H, I), (I, H))))
    x = torch.randn(M, H, device="cuda", dtype=torch.bfloat16)
    _stock_then_guarded(monkeypatch, lambda: mlp(x), "GatedMLP", expect_workspace=False)        # (shapes this small plan no split: whatever is asked for is held)
    pq_opt("PQ_FSK", "2")                                      # ... and with two forced ticket slices on `down` (96 x 256 x 1408: 6 + 5 K-tiles; gate+up has two K-tiles: single pass)
    handed = _stock_then_guarded(monkeypatch, lambda: mlp(x), "GatedMLP under PQ_FSK=2")
    assert [g.nbytes for g in handed] == [fsk_bytes(M, H, 2)]


def test_flow_kslabs_with_forced_fused_split_k(monkeypatch, pq_opt):
    import protoquant_amd as pq
    M, N, K, G = 300, 300, 4096, 2                             # (tests/test_gpu_int8_exchange.py::test_forced_fused_split_k_walks_stacked_blocks_in_place)
    g = torch.Generator().manual_seed(M + N + K)
    xq = torch.randint(-128, 128, (M, K), generator=g, dtype=torch.int8).cuda()
    wq = torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int8).cuda()
    xs, ws = (torch.rand(M, generator=g) * 0.01 + 1e-4).cuda(), (torch.rand(N, generator=g) * 0.01 + 1e-4).cuda()
    stacked = xq.reshape(M, G, K // G).permute(1, 0, 2).contiguous()
    pq_opt("PQ_FSK", "2")
    handed = _stock_then_guarded(monkeypatch, lambda: pq.qlinear_s8_kslabs(stacked, xs, wq, ws, None, torch.bfloat16), "qlinear_s8_kslabs")
    assert [h.nbytes for h in handed] == [fsk_bytes(M, N, 2)]


def test_flow_moe_forward_with_the_three_launch_route(monkeypatch):
    import protoquant_amd as pq
    E_, k, T, H, I = 8, 2, 2100, 200, 136                      # T k = 4200 > 4096 pairs (tests/test_gpu_moe_fused_path.py's experts)
    torch.manual_seed(E_ + k)
    mlps = [pq.GatedMLP.from_linears(*(torch.nn.Linear(i, o, bias=False, dtype=torch.bfloat16, device="cuda") for i, o in ((H, I), (H, I), (I, H)))) for _ in range(E_)]
    moe = pq.MoEGatedMLP.from_experts(mlps)
    x = (torch.randn(T, H, device="cuda") * 1.5).to(torch.bfloat16)
    wts, ids = torch.topk(torch.softmax(torch.randn(T, E_, device="cuda"), dim=1), k, dim=-1)
    w = (wts / wts.sum(dim=-1, keepdim=True)).to(torch.bfloat16)
    handed = _stock_then_guarded(monkeypatch, lambda: moe(x, ids, w), "MoEGatedMLP.forward")
    assert _hip().pq_moe_route_workspace_bytes(T, k, E_) in [g.nbytes for g in handed]


def test_flow_sharded_linears_at_world_1(monkeypatch, gather):
    import protoquant_amd as pq
    torch.manual_seed(4)
    lin = torch.nn.Linear(256, 384, bias=True, device="cuda", dtype=torch.bfloat16)       # (tests/test_gpu_sharded_forms.py::test_native_gather_forms_world1)
    x = torch.randn(700, 256, device="cuda", dtype=torch.bfloat16)
    for kw in ({}, {"overlap_chunks": 3}):
        m = pq.ColumnShardedQLinear.from_linear(lin, native_gather=gather, **kw)
        _stock_then_guarded(monkeypatch, lambda: m(x), f"ColumnShardedQLinear {kw}")
    rs = pq.RcclRowReduceScatter(gather)
    row = pq.RowShardedQLinear.from_linear(lin, native=rs)                                # (tests/test_gpu_parity.py::test_native_reduce_scatter_world1)
    x64 = x[:64].contiguous()
    handed = _stock_then_guarded(monkeypatch, lambda: row(x64), "RowShardedQLinear")
    assert 64 * 384 * 4 in [g.nbytes for g in handed]
