"""CPU: the int4 weight format's host side — the exported symbols, the Python names, argument refusals before any HIP call, and the spec's own bounds (tests/w4_spec.py)
over its whole domain."""
import numpy as np
import pytest
import torch

from tests import w4_spec as S
from tests.test_abi import declared_prototypes

ENTRIES = ("pq_w4_pack", "pq_w4_expand", "pq_qlinear_w4", "pq_gemm_s8w4s32")
A16 = 4096      # a non-null, 16-byte aligned address: every refusal below comes before anything is read


def test_symbols_and_names():
    import protoquant_amd as pq
    from protoquant_amd import _lib
    protos = declared_prototypes()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and len(_lib.SIGNATURES[name][1]) == len(protos[name][1]), name
        assert hasattr(_lib.lib(), name), name
    for name in ("w4_pack", "w4_expand", "qlinear_w4", "int_mm_w4", "QLinearW4", "swap_linears_w4"):
        assert name in pq.__all__ and callable(getattr(pq, name)), name


def _qlinear_w4(L, M=1, N=16, Kp=128, ldx=None, ldw4=None, ldy=None, xq=A16, xs=A16, w4=A16, gs=A16, ws=A16, y=A16, dtype=0):
    return L.pq_qlinear_w4(xq, Kp if ldx is None else ldx, xs, w4, Kp // 2 if ldw4 is None else ldw4, gs, ws, None, y, N if ldy is None else ldy, dtype, M, N, Kp, None)


@pytest.mark.parametrize("kw,named", [(dict(M=65), b"M = 65"), (dict(Kp=192), b"Kp = 192"), (dict(Kp=0), b"Kp = 0"), (dict(ldw4=48), b"ldw4"), (dict(ldw4=72), b"ldw4"),
                                      (dict(ldx=64), b"ldx"), (dict(ldy=15), b"ldy"), (dict(w4=None), b"w4 is null"), (dict(gs=None), b"gs is null"),
                                      (dict(xq=None), b"xq is null"), (dict(y=None), b"y is null"), (dict(xs=None), b"xs is null"), (dict(ws=None), b"ws is null"),
                                      (dict(w4=A16 + 8), b"w4 must be 16-byte aligned"), (dict(gs=A16 + 2), b"gs must be 4-byte aligned"),
                                      (dict(xq=A16 + 4), b"xq must be 16-byte aligned"), (dict(dtype=3), b"dtype")])
def test_bad_arguments_are_refused_by_name(kw, named):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _qlinear_w4(L, **kw) == 1 and named in L.pq_last_error(), (kw, L.pq_last_error())


def test_the_other_entries_refuse_and_empty_is_a_no_op():
    from protoquant_amd import _lib
    L = _lib.lib()
    assert L.pq_gemm_s8w4s32(A16, 128, A16, 64, A16, A16, 16, 65, 16, 128, None) == 1 and b"M = 65" in L.pq_last_error()
    assert L.pq_w4_pack(A16, 100, 4, 200, A16, 128, A16, None) == 1 and b"ldw = 100" in L.pq_last_error()
    assert L.pq_w4_pack(None, 200, 4, 200, A16, 128, A16, None) == 1 and b"wq is null" in L.pq_last_error()
    assert L.pq_w4_pack(A16, 200, 4, 200, A16, 64, A16, None) == 1 and b"ldw4" in L.pq_last_error()      # Kp = 256: 128 bytes per packed row
    assert L.pq_w4_expand(A16, 64, A16, 4, 192, A16, 192, None) == 1 and b"Kp = 192" in L.pq_last_error()
    assert L.pq_w4_expand(A16, 64, A16, 4, 128, A16, 120, None) == 1 and b"ldw8" in L.pq_last_error()
    assert L.pq_w4_expand(A16, 64, A16, 4, 128, None, 128, None) == 1 and b"w8 is null" in L.pq_last_error()
    assert _qlinear_w4(L, M=0, xq=None, y=None) == 0 and _qlinear_w4(L, N=0, w4=None, gs=None, ldy=0) == 0
    assert L.pq_w4_pack(None, 128, 0, 128, None, 64, None, None) == 0 and L.pq_w4_expand(None, 64, None, 0, 128, None, 128, None) == 0


def test_cpu_tensors_are_refused():
    import protoquant_amd as pq
    from protoquant_amd import _lib
    w4, gs = (torch.from_numpy(a) for a in S.pack(np.zeros((4, 128), np.int8)))
    xq, one = torch.zeros((1, 128), dtype=torch.int8), torch.ones(4)
    for call in (lambda: pq.w4_pack(torch.zeros((4, 128), dtype=torch.int8)), lambda: pq.w4_expand(w4, gs), lambda: pq.int_mm_w4(xq, w4, gs),
                 lambda: pq.qlinear_w4(xq, one[:1], w4, gs, one, None, torch.bfloat16), lambda: pq.QLinearW4(128, 4)(torch.zeros(1, 128, dtype=torch.bfloat16)),
                 lambda: pq.QLinearW4.from_linear(torch.nn.Linear(128, 4, dtype=torch.bfloat16))):
        with pytest.raises(_lib.PQError):
            call()


def test_the_rule_holds_its_bounds_over_the_whole_domain():
    """every group maximum a = 0 .. 127 and every code w = -a .. a under it: |q g| <= 126 and |q g - w| <= g div 2; and pack / expand are inverse on the levels"""
    a = np.repeat(np.arange(128), 255)
    w = np.tile(np.arange(-127, 128), 128)
    keep = np.abs(w) <= a
    a, w = a[keep], w[keep]
    g = S.group_mult(a)
    q = S.code(w, g)
    assert g.min() == 1 and g.max() == 18 and np.abs(q).max() == 7
    assert np.abs(q * g).max() <= 126 and np.all(np.abs(q * g - w) <= g // 2)
    wq = np.random.default_rng(0).integers(-127, 128, (5, 200)).astype(np.int8)
    lv, gm = S.levels(wq)
    assert np.array_equal(S.expand(*S.pack(wq)), (lv * np.repeat(gm, 128, axis=1)).astype(np.int8))
