"""CPU: the grouped int8 qlinear's host side — exported symbols, argument validation before any HIP call, the tile planner, the routing sort / offsets / combine logic of
MoEGatedMLP against a brute-force loop, and the built code object of the grouped kernels (no scratch, no spill, the hand-written tile's instructions)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch
from tests.code_objects import kernels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("pq_qlinear_s8_grouped", "pq_gemm_s8s8s32_grouped", "pq_grouped_variant_name")
NAMES = (b"grouped64x128_16x16x64", b"grouped64x64_16x16x64")


def test_symbols_declared_exported_and_bound():
    from protoquant_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pq_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, hdr), f"pq_hip.h does not declare {s}"
        assert hasattr(L, s), f"libpq_hip.so does not export {s}"
        assert s in _lib.EXPORTS
    assert L.pq_version() == 1


def _call(L, **kw):
    """pq_qlinear_s8_grouped with plausible (never dereferenced) operands, one argument overridden"""
    a = dict(xq=0x1000, ldx=256, idx=None, x_rows=512, xs=0x2000, wq=0x3000, ldw=256, stride=64 * 256, ws=0x4000, bias=None, off=0x5000, E=4, M=512, N=64, K=256,
             y=0x6000, ldy=64, dt=0)
    a.update(kw)
    return L.pq_qlinear_s8_grouped(a["xq"], a["ldx"], a["idx"], a["x_rows"], a["xs"], a["wq"], a["ldw"], a["stride"], a["ws"], a["bias"], a["off"], a["E"], a["M"], a["N"],
                                   a["K"], a["y"], a["ldy"], a["dt"], None)


@pytest.mark.parametrize("kw,named", [
    (dict(xq=None), b"xq"), (dict(wq=None), b"wq"), (dict(y=None), b"y"), (dict(xs=None), b"xs"), (dict(ws=None), b"ws"), (dict(off=None), b"offsets"),
    (dict(E=0), b"E"), (dict(E=1025), b"E"), (dict(M=-1), b"M_total"), (dict(N=-3), b"N"), (dict(K=-128), b"K"), (dict(K=200), b"K"), (dict(ldx=264, K=256), b"ldx"),
    (dict(ldw=264), b"ldw"), (dict(ldx=128), b"ldx"), (dict(ldw=128), b"ldw"), (dict(ldy=63), b"ldy"), (dict(dt=3), b"dtype"), (dict(stride=100), b"w_expert_stride"),
    (dict(idx=0x7000, x_rows=1 << 24, ldx=256), b"2^32"), (dict(x_rows=100), b"x_rows"), (dict(xq=0x1008), b"xq"),
])
def test_bad_arguments_are_named_without_a_gpu(kw, named):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _call(L, **kw) == 1, kw
    assert named in L.pq_last_error(), (kw, L.pq_last_error())


def test_int32_twin_validates_too_and_empty_is_a_noop():
    from protoquant_amd import _lib
    L = _lib.lib()
    assert L.pq_gemm_s8s8s32_grouped(0x1000, 256, None, 512, 0x3000, 256, 64 * 256, 0x5000, 0, 512, 64, 256, 0x6000, 64, None) == 1
    assert b"E" in L.pq_last_error()
    assert L.pq_gemm_s8s8s32_grouped(0x1000, 256, None, 512, 0x3000, 256, 64 * 256, 0x5000, 4, 512, 64, 256, None, 64, None) == 1
    assert L.pq_gemm_s8s8s32_grouped(None, 256, None, 0, None, 256, 64 * 256, 0x5000, 4, 0, 64, 256, None, 64, None) == 0       # M_total = 0: no-op
    assert _call(L, M=0, x_rows=0) == 0


def test_variant_name_is_one_of_two_and_monotone():
    from protoquant_amd import _lib
    L = _lib.lib()
    for K in (128, 4096):
        for E in (1, 8, 128, 1024):
            for N in (64, 768, 4096, 28672):
                prev = None
                for M in (0, 1, 64, 256, 1024, 4096, 32768, 1 << 20):
                    name = L.pq_grouped_variant_name(E, M, N, K)
                    assert name in NAMES
                    if prev == NAMES[0]:
                        assert name == NAMES[0], f"more rows moved E={E} N={N} from 64x128 back to 64x64 at M={M}"
                    prev = name
            for M in (64, 4096):
                prev = None
                for N in (1, 64, 200, 1024, 8192, 65536):
                    name = L.pq_grouped_variant_name(E, M, N, K)
                    if prev == NAMES[0]:
                        assert name == NAMES[0]
                    prev = name
    assert L.pq_grouped_variant_name(1, 64, 64, 128) == NAMES[1] and L.pq_grouped_variant_name(128, 32768, 1536, 2048) == NAMES[0]
    _lib.set_option("PQ_GROUPED_TILE", "64x64")
    try:
        assert L.pq_grouped_variant_name(128, 32768, 1536, 2048) == NAMES[1]
    finally:
        _lib.set_option("PQ_GROUPED_TILE", "")


def _brute_force(ids, w, y_of):
    """the eager loop: for e ascending, for the tokens routed to e, final[t] += out_e[t] * w"""
    T, k = ids.shape
    E = int(ids.max()) + 1 if ids.numel() else 1
    final = torch.zeros(T, y_of(0, 0).shape[0], dtype=w.dtype)
    for e in range(E):
        for t in range(T):
            for j in range(k):
                if int(ids[t, j]) == e:
                    final[t] = final[t] + y_of(t, e) * w[t, j]
    return final


@pytest.mark.parametrize("T,k,E,seed", [(1, 1, 1, 0), (7, 1, 4, 1), (33, 2, 8, 2), (20, 8, 128, 3), (50, 4, 6, 4), (64, 2, 40, 5)])
def test_route_plan_and_combine_against_brute_force(T, k, E, seed):
    from protoquant_amd.moe import combine, route_plan
    g = torch.Generator().manual_seed(seed)
    ids = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)])       # distinct experts per token, many experts empty
    if seed == 4:
        ids = ids % 3 + 3 * (torch.arange(k)[None, :] // 3)                            # experts 0 .. 2 hot, the rest empty, still distinct per token
        ids = torch.stack([torch.randperm(6, generator=g)[:k] for _ in range(T)])
    w = torch.rand(T, k, generator=g).to(torch.bfloat16)
    row_index, offsets, rows_of, slot_of = route_plan(ids, E)
    assert row_index.dtype == torch.int32 and offsets.dtype == torch.int32 and offsets.shape == (E + 1,)
    counts = [int((ids == e).sum()) for e in range(E)]
    assert offsets.tolist() == [sum(counts[:e]) for e in range(E + 1)]
    flat = ids.reshape(-1)
    for e in range(E):                                                                 # rows of expert e: its (token, slot) pairs in their original order
        want = [p // k for p in range(T * k) if int(flat[p]) == e]
        assert row_index[offsets[e]:offsets[e + 1]].tolist() == want
    for t in range(T):
        experts = [int(ids[t, j]) for j in slot_of[t].tolist()]
        assert experts == sorted(experts)
        for s in range(k):
            r = int(rows_of[t, s])
            assert int(row_index[r]) == t and offsets[experts[s]] <= r < offsets[experts[s] + 1]
    H = 5
    table = torch.randn(T, E, H, generator=g).to(torch.bfloat16)                       # "expert e's output for token t"
    expert_of_row = torch.bucketize(torch.arange(T * k), offsets[1:].long(), right=True)
    y = table[row_index.long(), expert_of_row]
    got = combine(y, rows_of, slot_of, w)
    want = _brute_force(ids, w, lambda t, e: table[t, e])
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_grouped_code_object_is_the_hand_written_tile():
    """as `make spillcheck` reads it: no scratch, no VGPR spill in any gemm_s8_grouped instantiation; and the tile's own instructions are there"""
    kernels, dis = kernels_of("gemm_s8_grouped", disassembly=True)
    grouped = {k: v for k, v in kernels.items() if "gemm_s8_grouped" in k}
    assert len(grouped) == 16, sorted(grouped)            # 4 output kinds x 2 tiles x with / without the row index
    for k, v in grouped.items():
        assert v.get("private_segment_fixed_size", 1) == 0 and v.get("vgpr_spill_count", 1) == 0, (k, v)
    assert "global_load_lds_dwordx4" in dis and "v_mfma_i32_16x16x64_i8" in dis
