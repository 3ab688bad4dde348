"""CPU: the host side of int4 expert weights at decode (pq_qlinear_w4_grouped_stream, gemm_w4_grouped_stream.hip) — the exported symbols, the Python names, argument
refusals before any HIP call, and the code object: exactly the instantiations the launcher dispatches to, none with scratch, a spill or more than 128 VGPRs."""
import re

import pytest
import torch

from tests.code_objects import kernels_of
from tests.test_abi import declared_prototypes

ENTRIES = ("pq_qlinear_w4_grouped_stream", "pq_gemm_s8w4s32_grouped_stream")
A16 = 4096      # a non-null, 16-byte aligned address: every refusal below comes before anything is read


def test_symbols_and_names():
    import protoquant_amd as pq
    from protoquant_amd import _lib
    protos = declared_prototypes()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and len(_lib.SIGNATURES[name][1]) == len(protos[name][1]), name
        assert hasattr(_lib.lib(), name), name
    for name in ("qlinear_w4_grouped", "int_mm_w4_grouped", "GroupedQLinearW4", "swap_moe_experts_w4"):
        assert name in pq.__all__ and callable(getattr(pq, name)), name


def _call(L, E=2, M=1, N=16, Kp=128, ldx=None, ldw4=None, w4s=None, gss=None, ldy=None, xq=A16, xs=A16, w4=A16, gs=A16, ws=A16, offsets=A16, y=A16, dtype=0):
    ldw4 = Kp // 2 if ldw4 is None else ldw4
    return L.pq_qlinear_w4_grouped_stream(xq, Kp if ldx is None else ldx, None, M, xs, w4, ldw4, N * ldw4 if w4s is None else w4s, gs,
                                          (N + 3) // 4 * (Kp // 128) * 4 if gss is None else gss, ws, None, offsets, E, M, N, Kp, y, N if ldy is None else ldy, dtype, None)


@pytest.mark.parametrize("kw,named", [(dict(M=65), b"M_total = 65"), (dict(Kp=192), b"Kp = 192"), (dict(Kp=0), b"Kp = 0"), (dict(ldw4=48), b"ldw4"), (dict(ldw4=72), b"ldw4"),
                                      (dict(w4s=15 * 64 + 48), b"w4_expert_stride"), (dict(w4s=16 * 64 + 8), b"w4_expert_stride"), (dict(gss=12), b"gs_expert_stride"),
                                      (dict(gss=18), b"gs_expert_stride"), (dict(w4=None), b"w4 is null"), (dict(gs=None), b"gs is null"),
                                      (dict(offsets=None), b"offsets is null"), (dict(y=None), b"y is null"), (dict(xq=None), b"xq is null"), (dict(xs=None), b"xs is null"),
                                      (dict(w4=A16 + 8), b"w4 must be 16-byte aligned"), (dict(gs=A16 + 2), b"gs must be 4-byte aligned"),
                                      (dict(xq=A16 + 4), b"xq must be 16-byte aligned"), (dict(dtype=3), b"dtype"), (dict(E=0), b"E = 0"), (dict(ldx=64), b"ldx")])
def test_bad_arguments_are_refused_by_name(kw, named):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _call(L, **kw) == 1 and named in L.pq_last_error(), (kw, L.pq_last_error())


def test_the_int32_entry_refuses_and_empty_is_a_no_op():
    from protoquant_amd import _lib
    L = _lib.lib()
    assert L.pq_gemm_s8w4s32_grouped_stream(A16, 128, None, 65, A16, 64, 16 * 64, A16, 16, A16, 2, 65, 16, 128, A16, 16, None) == 1 and b"M_total = 65" in L.pq_last_error()
    assert L.pq_gemm_s8w4s32_grouped_stream(A16, 128, None, 1, A16, 64, 16 * 64, A16, 16, None, 2, 1, 16, 128, A16, 16, None) == 1 and b"offsets is null" in L.pq_last_error()
    assert _call(L, M=0, xq=None, y=None, xs=None) == 0 and _call(L, N=0, w4=None, gs=None, ws=None, y=None, ldy=0) == 0
    assert L.pq_gemm_s8w4s32_grouped_stream(None, 128, None, 0, A16, 64, 16 * 64, A16, 16, A16, 2, 0, 16, 128, None, 16, None) == 0


def test_cpu_tensors_are_refused():
    import protoquant_amd as pq
    from protoquant_amd import _lib
    w4, gs = torch.zeros((2, 4, 64), dtype=torch.uint8), torch.ones((2, 1, 1, 4), dtype=torch.uint8)
    xq, offsets = torch.zeros((1, 128), dtype=torch.int8), torch.tensor([0, 1, 1], dtype=torch.int32)
    for call in (lambda: pq.int_mm_w4_grouped(xq, w4, gs, offsets), lambda: pq.qlinear_w4_grouped(xq, torch.ones(1), w4, gs, torch.ones(2, 4), None, offsets, torch.bfloat16),
                 lambda: pq.GroupedQLinearW4.from_weight(torch.zeros(2, 4, 128, dtype=torch.bfloat16))):
        with pytest.raises(_lib.PQError):
            call()


def test_code_object_holds_the_dispatched_instantiations_without_scratch():
    """launch_gemm_w4_grouped_stream dispatches OUT = bf16 / fp16 / f32 / int32 x MT = 1 / 2 / 4; every one carries bodies of up to MT token tiles and is launched with
    up to 16 waves per workgroup: at most 128 VGPRs, no scratch, no spills"""
    kernels = {k: v for k, v in kernels_of("gemm_w4_grouped_stream", must_be_built=True).items() if "gemm_w4_grouped_stream" in k}
    got = sorted(tuple(map(int, re.search(r"gemm_w4_grouped_streamILi(\d)ELi(\d)EEE", k).groups())) for k in kernels)
    assert got == [(o, mt) for o in range(4) for mt in (1, 2, 4)], got
    for k, v in kernels.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["vgpr_count"] <= 128, (k, v)
