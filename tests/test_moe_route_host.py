"""CPU: the host side of the mixture-of-experts plumbing kernels (pq_moe_route, pq_moe_combine) — the symbols are declared, exported and bound; every bad argument is
rejected AND named before any HIP call (so all of this runs without a GPU); the workspace size is monotone; the built code object of moe_kernels.hip has no scratch and
no spill; and the Python entry points refuse CPU tensors."""
import os
import re
import subprocess

import pytest
import torch
from tests.code_objects import kernels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("pq_moe_route", "pq_moe_route_workspace_bytes", "pq_moe_combine")
OK, BAD_ARG, BAD_ALIGN, LAUNCH, WORKSPACE = 0, 1, 2, 3, 5


def test_symbols_declared_exported_and_bound():
    from protoquant_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pq_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, hdr), f"pq_hip.h does not declare {s}"
        assert hasattr(L, s), f"libpq_hip.so does not export {s}"
        assert s in _lib.EXPORTS
        assert getattr(L, s).argtypes, f"{s} has no ctypes signature"
    assert L.pq_version() == 1                                          # additions only


def _route(L, **kw):
    """pq_moe_route with plausible (never dereferenced) operands, one argument overridden.  T * k = 32768 pairs: the three-launch form, which needs a workspace."""
    a = dict(ids=0x1000, i64=1, ld=8, T=4096, k=8, E=128, off=0x2000, ridx=0x3000, rows=0x4000, slots=0x5000, xs=None, xss=None, ws=0x10000, wsb=1 << 20)
    a.update(kw)
    return L.pq_moe_route(a["ids"], a["i64"], a["ld"], a["T"], a["k"], a["E"], a["off"], a["ridx"], a["rows"], a["slots"], a["xs"], a["xss"], a["ws"], a["wsb"], None)


@pytest.mark.parametrize("kw,status,named", [
    (dict(ids=None), BAD_ARG, b"topk_ids"), (dict(off=None), BAD_ARG, b"offsets"), (dict(ridx=None), BAD_ARG, b"row_index"), (dict(rows=None), BAD_ARG, b"rows_of"),
    (dict(slots=None), BAD_ARG, b"slot_of"), (dict(E=0), BAD_ARG, b"E"), (dict(E=1025), BAD_ARG, b"E"), (dict(E=-3), BAD_ARG, b"E"), (dict(k=0, ld=8), BAD_ARG, b"k"),
    (dict(k=65, ld=65), BAD_ARG, b"k"), (dict(T=-1), BAD_ARG, b"T"), (dict(T=1 << 28), BAD_ARG, b"2^31"), (dict(T=1 << 31, k=1), BAD_ARG, b"2^31"),
    (dict(ld=7), BAD_ARG, b"ld_ids"), (dict(i64=2), BAD_ARG, b"ids_are_int64"), (dict(xs=0x6000), BAD_ARG, b"xs without xs_sorted"),
    (dict(xss=0x7000), BAD_ARG, b"xs_sorted without xs"), (dict(ws=None), BAD_ARG, b"workspace"), (dict(ws=0x10004), BAD_ALIGN, b"workspace"),
    (dict(wsb=100), WORKSPACE, b"workspace"), (dict(ws=None, wsb=0), BAD_ARG, b"workspace"), (dict(ids=0x1004), BAD_ALIGN, b"topk_ids"),
    (dict(ids=0x1002, i64=0), BAD_ALIGN, b"topk_ids"),
])
def test_route_bad_arguments_are_named_without_a_gpu(kw, status, named):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _route(L, **kw) == status, (kw, L.pq_last_error())
    assert named in L.pq_last_error(), (kw, L.pq_last_error())
    assert b"pq_moe_route" in L.pq_last_error()


def _combine(L, **kw):
    a = dict(y=0x1000, ldy=2048, dt=0, M=32768, rows=0x2000, slots=0x3000, w=0x4000, ldw=8, T=4096, k=8, H=2048, out=0x5000, ldo=2048)
    a.update(kw)
    return L.pq_moe_combine(a["y"], a["ldy"], a["dt"], a["M"], a["rows"], a["slots"], a["w"], a["ldw"], a["T"], a["k"], a["H"], a["out"], a["ldo"], None)


@pytest.mark.parametrize("kw,status,named", [
    (dict(y=None), BAD_ARG, b"y is null"), (dict(rows=None), BAD_ARG, b"rows_of"), (dict(slots=None), BAD_ARG, b"slot_of"), (dict(w=None), BAD_ARG, b"topk_w"),
    (dict(out=None), BAD_ARG, b"out"), (dict(dt=3), BAD_ARG, b"dtype"), (dict(dt=-1), BAD_ARG, b"dtype"), (dict(k=0), BAD_ARG, b"k"), (dict(k=65, ldw=65), BAD_ARG, b"k"),
    (dict(T=-2), BAD_ARG, b"T"), (dict(T=1 << 28), BAD_ARG, b"2^31"), (dict(ldw=7), BAD_ARG, b"ld_w"), (dict(ldy=2047), BAD_ARG, b"ldy"), (dict(ldo=2047), BAD_ARG, b"ld_out"),
    (dict(H=-1), BAD_ARG, b"H"), (dict(M=-1), BAD_ARG, b"M_total"), (dict(M=0), BAD_ARG, b"M_total"), (dict(y=0x1001), BAD_ALIGN, b"aligned"),
    (dict(out=0x5002, dt=2), BAD_ALIGN, b"aligned"),
])
def test_combine_bad_arguments_are_named_without_a_gpu(kw, status, named):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _combine(L, **kw) == status, (kw, L.pq_last_error())
    assert named in L.pq_last_error(), (kw, L.pq_last_error())
    assert b"pq_moe_combine" in L.pq_last_error()


def test_empty_problems():
    """A combine over no tokens (or no columns) is a no-op: OK without any pointer and without a GPU.  A routing of no tokens still has work to do — offsets = zeros is
    written by a launch — so its arguments pass the checks and the status is OK on a GPU and the launch error, never a bad argument, on a machine without one."""
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _combine(L, T=0, y=None, rows=None, slots=None, w=None, out=None, M=0) == OK
    assert _combine(L, H=0, ldy=0, ldo=0, y=None, out=None) == OK
    st = _route(L, T=0, ids=None, ridx=None, rows=None, slots=None, ws=None, wsb=0)
    if torch.cuda.is_available():
        assert st == OK
    else:
        assert st == LAUNCH and b"pq_moe_route" in L.pq_last_error(), (st, L.pq_last_error())


def test_route_workspace_bytes_is_monotone_and_zero_for_one_launch():
    from protoquant_amd import _lib
    L = _lib.lib()
    for k in (1, 2, 8, 64):
        for E in (1, 8, 128, 1024):
            prev = 0
            for T in (0, 1, 2, 31, 64, 257, 512, 513, 4096, 4097, 40000, 65536, 65537, 70000, 1 << 20, (1 << 24) + 5):
                if T * k >= 1 << 31:
                    continue
                b = L.pq_moe_route_workspace_bytes(T, k, E)
                assert b >= prev, f"workspace shrank at T={T} k={k} E={E}: {b} < {prev}"
                assert b % 256 == 0
                if T * k <= 4096:
                    assert b == 0, "a routing of at most 4096 pairs is one launch in LDS: no workspace"
                else:
                    assert b >= 2 * E * 4
                prev = b
            assert prev <= 257 * 4 * 1024 + 256               # bounded: the blocks grow instead of the table
    assert L.pq_moe_route_workspace_bytes(-1, 8, 128) == 0 and L.pq_moe_route_workspace_bytes(4096, 0, 128) == 0 and L.pq_moe_route_workspace_bytes(4096, 8, 0) == 0


def test_python_entry_points_have_no_cpu_fallback():
    import protoquant_amd as pq
    from protoquant_amd import _lib
    ids = torch.randint(0, 4, (5, 2))
    with pytest.raises(_lib.PQError):
        pq.moe_route(ids, 4)
    with pytest.raises(_lib.PQError):
        pq.moe_combine(torch.zeros(10, 8, dtype=torch.bfloat16), torch.zeros(5, 2, dtype=torch.int32), torch.zeros(5, 2, dtype=torch.int32),
                       torch.ones(5, 2, dtype=torch.bfloat16))
    assert pq.MoEGatedMLP.torch_plumbing is False


def test_moe_code_object_has_no_scratch_and_the_expected_kernels():
    """as `make spillcheck` reads the GEMM objects: no scratch, no VGPR spill in any kernel of moe_kernels.o; both forms of the routing and every layout of the combine are
    there; and no single-rounding mixed-precision instruction stands in for the two roundings of the combine"""
    kernels, dis = kernels_of("moe_kernels", disassembly=True)
    assert len([k for k in kernels if "moe_route_rank" in k]) == 4          # int32 / int64 ids x one-launch / three-launch form
    assert len([k for k in kernels if "moe_route_count" in k]) == 2
    assert len([k for k in kernels if "moe_route_scan" in k]) == 1
    assert len([k for k in kernels if "moe_combine_kernel" in k]) == 12     # 3 dtypes x (wave | workgroup per token) x (16-byte | element-wise rows)
    for k, v in kernels.items():
        assert v.get("private_segment_fixed_size", 1) == 0 and v.get("vgpr_spill_count", 1) == 0 and v.get("sgpr_spill_count", 1) == 0, (k, v)
    assert "global_load_dwordx4" in dis and "global_store_dwordx4" in dis
    body, cur = {}, None                                                   # disassembly per kernel
    for ln in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", ln)
        if m:
            cur = m.group(1)
        elif cur:
            body.setdefault(cur, []).append(ln)
    combine = {k: "\n".join(v) for k, v in body.items() if "moe_combine_kernel" in k}
    assert len(combine) == 12
    for k, text in combine.items():
        assert "v_mul_f32" in text or "v_pk_mul_f32" in text, k
        for bad in ("v_fma", "v_mad_mix", "v_fmac", "v_pk_fma", "v_mad_f32", "v_mac_f32", "v_pk_mul_f16", "v_pk_add_f16", "v_dot"):
            assert bad not in text, f"{bad} in {k}: the combine is one binary32 multiply and one binary32 add, each rounded on its own"
