"""CPU: the host side of the grouped weight-streaming qlinear for decode (gemm_s8_grouped_stream.hip, pq_qlinear_s8_grouped_stream): exported symbols, argument validation
before any HIP call, the (token tiles, RB, KS) planner and its two forcing switches, the Python wrappers' row limit, GroupedQLinear.stream_rows, and the built code object:
every instantiation the launcher can reach is there, without scratch and without spills."""
import os
import re
import subprocess

import pytest
import torch
from tests.code_objects import kernels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("pq_qlinear_s8_grouped_stream", "pq_gemm_s8s8s32_grouped_stream", "pq_grouped_stream_plan_name")
TILE_NAMES = (b"grouped64x128_16x16x64", b"grouped64x64_16x16x64")
# (N, K) of the two GEMMs of Mixtral 8x7B's experts and of a 128-small-expert layer
LAYERS = ((28672, 4096), (4096, 14336), (1536, 2048), (2048, 768))
PLAN_RE = re.compile(rb"^gstream_mt([124])_rb([12])_ks(1|2|4|8|16)_16x16x64$")


def _lib():
    from protoquant_amd import _lib
    return _lib, _lib.lib()


def test_symbols_declared_exported_and_bound():
    _l, L = _lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pq_hip.h")).read(), flags=re.S)
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, hdr), f"pq_hip.h does not declare {s}"
        assert hasattr(L, s), f"libpq_hip.so does not export {s}"
        assert s in _l.EXPORTS
    import protoquant_amd as pq
    assert callable(pq.qlinear_s8_grouped_stream) and callable(pq.int_mm_grouped_stream)


def _call(L, **kw):
    """pq_qlinear_s8_grouped_stream with plausible (never dereferenced) operands, one argument overridden"""
    a = dict(xq=0x1000, ldx=256, idx=None, x_rows=64, xs=0x2000, wq=0x3000, ldw=256, stride=64 * 256, ws=0x4000, bias=None, off=0x5000, E=4, M=64, N=64, K=256,
             y=0x6000, ldy=64, dt=0)
    a.update(kw)
    return L.pq_qlinear_s8_grouped_stream(a["xq"], a["ldx"], a["idx"], a["x_rows"], a["xs"], a["wq"], a["ldw"], a["stride"], a["ws"], a["bias"], a["off"], a["E"], a["M"],
                                          a["N"], a["K"], a["y"], a["ldy"], a["dt"], None)


@pytest.mark.parametrize("kw,named", [
    (dict(M=65, x_rows=65), b"M_total = 65"), (dict(M=4096, x_rows=4096), b"M_total"), (dict(E=0), b"E"), (dict(E=1025), b"E"), (dict(K=64), b"K"), (dict(K=200), b"K"),
    (dict(off=None), b"offsets"), (dict(xq=0x1008), b"xq"), (dict(wq=0x3004), b"wq"), (dict(idx=0x7000, x_rows=1 << 24, ldx=256), b"2^32"), (dict(xs=None), b"xs"),
    (dict(ws=None), b"ws"), (dict(y=None), b"y"), (dict(dt=3), b"dtype"), (dict(ldy=63), b"ldy"), (dict(ldw=128), b"ldw"), (dict(stride=100), b"w_expert_stride"),
    (dict(x_rows=10), b"x_rows"), (dict(M=-1), b"M_total"),
])
def test_bad_arguments_are_named_without_a_gpu(kw, named):
    """(this process has no GPU: a HIP call before the answer would fail differently, or crash on the made-up pointers)"""
    _l, L = _lib()
    assert _call(L, **kw) == 1, kw
    assert named in L.pq_last_error(), (kw, L.pq_last_error())
    assert b"pq_qlinear_s8_grouped_stream" in L.pq_last_error()


def test_int32_twin_validates_too_and_empty_is_a_noop():
    _l, L = _lib()
    twin = L.pq_gemm_s8s8s32_grouped_stream
    assert twin(0x1000, 256, None, 64, 0x3000, 256, 64 * 256, 0x5000, 4, 65, 64, 256, 0x6000, 64, None) == 1
    assert b"M_total = 65" in L.pq_last_error() and b"pq_gemm_s8s8s32_grouped_stream" in L.pq_last_error()
    assert twin(0x1000, 256, None, 64, 0x3000, 256, 64 * 256, 0x5000, 0, 64, 64, 256, 0x6000, 64, None) == 1
    assert b"E" in L.pq_last_error()
    assert twin(0x1000, 256, None, 64, 0x3000, 256, 64 * 256, None, 4, 64, 64, 256, 0x6000, 64, None) == 1
    assert b"offsets" in L.pq_last_error()
    assert twin(0x1000, 256, None, 64, 0x3000, 256, 64 * 256, 0x5000, 4, 64, 64, 256, None, 64, None) == 1
    assert twin(None, 256, None, 0, None, 256, 64 * 256, 0x5000, 4, 0, 64, 256, None, 64, None) == 0          # M_total = 0: no-op
    assert _call(L, M=0, x_rows=0) == 0
    assert _call(L, N=0, ldy=0, stride=0) == 0                                                                # N = 0: no-op


def _plan(L, E, M, N, K):
    name = L.pq_grouped_stream_plan_name(E, M, N, K)
    m = PLAN_RE.match(name or b"")
    assert m, f"plan name {name!r} for E={E} M_total={M} N={N} K={K}"
    return tuple(int(g) for g in m.groups())


def test_plan_name_is_static_names_the_plan_and_leaves_the_tile_planner_alone():
    _l, L = _lib()
    seen = {}
    for E in (1, 8, 128, 1024):
        for M in (1, 16, 17, 64):
            for N, K in LAYERS:
                mt, rb, ks = _plan(L, E, M, N, K)
                assert mt == (1 if M <= 16 else 2 if M <= 32 else 4), (E, M, N, K, mt)
                assert rb == 1 or mt <= 2, "two weight blocks per wave exist for at most two token tiles"
                a, b = L.pq_grouped_stream_plan_name(E, M, N, K), L.pq_grouped_stream_plan_name(E, M, N, K)
                assert a == b
                seen.setdefault(a, []).append((E, M, N, K))
                assert L.pq_grouped_variant_name(E, M, N, K) in TILE_NAMES             # the tile planner still answers for pq_qlinear_s8_grouped
    assert len(seen) > 3, f"the plan does not depend on its arguments: {list(seen)}"
    # the static string: the same address for the same plan, call after call (ctypes: read the raw pointer)
    import ctypes
    raw = ctypes.CDLL(_l.LIB_PATH)
    raw.pq_grouped_stream_plan_name.restype = ctypes.c_void_p
    raw.pq_grouped_stream_plan_name.argtypes = [ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]
    assert raw.pq_grouped_stream_plan_name(8, 2, 4096, 14336) == raw.pq_grouped_stream_plan_name(8, 2, 4096, 14336) != 0
    # one token per expert: at least four waves split K, as for the dense kernel's single token
    for N, K in LAYERS[:3]:
        assert _plan(L, 8, 2, N, K)[2] >= 4


def test_plan_follows_the_two_forcing_switches():
    _l, L = _lib()
    try:
        for ks in (1, 4, 16):
            _l.set_option("PQ_GROUPED_STREAM_KS", ks)
            for E, M in ((8, 1), (128, 17), (1024, 64)):
                for N, K in LAYERS + ((200, 128),):                 # (K = 128: two k-steps, the forced split holds all the same)
                    assert _plan(L, E, M, N, K)[2] == ks, (ks, E, M, N, K)
        _l.set_option("PQ_GROUPED_STREAM_KS", None)
        for rb in (1, 2):
            _l.set_option("PQ_GROUPED_STREAM_RB", rb)
            for N, K in LAYERS:
                assert _plan(L, 8, 2, N, K)[1] == rb and _plan(L, 128, 32, N, K)[1] == rb
                assert _plan(L, 8, 64, N, K)[1] == 1                # three or four token tiles: one block per wave whatever is forced
                assert L.pq_grouped_variant_name(8, 2, N, K) in TILE_NAMES
    finally:
        _l.set_option("PQ_GROUPED_STREAM_KS", None)
        _l.set_option("PQ_GROUPED_STREAM_RB", None)
    assert _plan(L, 8, 2, 4096, 14336) == _plan(L, 8, 2, 4096, 14336)


def test_wrappers_refuse_more_than_64_rows_before_the_library(monkeypatch):
    """the Python entry points check the row limit themselves (CPU tensors: require_gpu answers first, so the limit is checked through the shared helper)"""
    import importlib
    Q = importlib.import_module("protoquant_amd.qlinear")           # (the package exports the CLASS qlinear under the module's name)
    assert Q.STREAM_ROWS_MAX == 64
    calls = []
    monkeypatch.setattr(Q, "_grouped_operands", lambda what, xq, wq, offsets, row_index: (calls.append(what), (xq, wq, 4, 8, 128, xq.shape[0]))[1])
    xq, wq = torch.zeros((65, 128), dtype=torch.int8), torch.zeros((4, 8, 128), dtype=torch.int8)
    with pytest.raises(ValueError, match="at most 64 grouped rows"):
        Q.qlinear_s8_grouped_stream(xq, None, wq, None, None, None, torch.bfloat16)
    with pytest.raises(ValueError, match="at most 64 grouped rows"):
        Q.int_mm_grouped_stream(xq, wq, None)
    assert calls == ["qlinear_s8_grouped_stream", "int_mm_grouped_stream"]


def test_grouped_qlinear_picks_its_entry_from_the_row_count(monkeypatch):
    """GroupedQLinear.forward: 0 < M_total <= stream_rows -> the streaming entry, anything else -> the tile entry; stream_rows is a class default, settable per instance"""
    from protoquant_amd import moe as M
    from protoquant_amd.qtensor import QTensor
    assert M.GroupedQLinear.stream_rows in (0, 16, 32, 64)
    taken = []
    monkeypatch.setattr(M, "qlinear_s8_grouped", lambda *a, **k: taken.append("tile"))
    monkeypatch.setattr(M, "qlinear_s8_grouped_stream", lambda *a, **k: taken.append("stream"))
    g = M.GroupedQLinear(4, 128, 16)
    assert f"stream_rows={g.stream_rows}" in g.extra_repr()
    off = torch.zeros(5, dtype=torch.int32)

    def run(rows, gathered=None):
        x = QTensor(torch.zeros((rows, 128), dtype=torch.int8), torch.ones(rows), 1, torch.bfloat16, torch.Size((rows, 128)))
        idx = torch.zeros(gathered, dtype=torch.int32) if gathered is not None else None
        g(x, off, idx, torch.ones(gathered if gathered is not None else rows))
        return taken.pop()

    g.stream_rows = 64
    assert [run(1), run(64), run(65), run(0)] == ["stream", "stream", "tile", "tile"]
    assert [run(4, gathered=64), run(4, gathered=65), run(200, gathered=8)] == ["stream", "tile", "stream"]      # M_total is the length of the row index
    g.stream_rows = 16
    assert [run(16), run(17)] == ["stream", "tile"]
    g.stream_rows = 0
    assert [run(1), run(64)] == ["tile", "tile"]
    assert M.GroupedQLinear(4, 128, 16).stream_rows == M.GroupedQLinear.stream_rows                                # the instance setting did not leak


def _kernel_notes():
    return {k: v for k, v in kernels_of("gemm_s8_grouped_stream").items() if "gemm_s8_grouped_stream" in k}


def test_code_object_holds_every_reachable_instantiation_without_scratch_or_spills():
    """OUT in (bf16, fp16, f32, int32) x (MT, RB) in ((1, 1), (1, 2), (2, 1), (2, 2), (4, 1)): what launch_gemm_grouped_stream dispatches to.  Up to 16 waves per
    workgroup: at most 128 VGPRs."""
    kernels = _kernel_notes()
    want = {f"Li{o}ELi{mt}ELi{rb}E" for o in range(4) for mt, rb in ((1, 1), (1, 2), (2, 1), (2, 2), (4, 1))}
    got = {re.search(r"gemm_s8_grouped_streamI((?:Li\d+E){3})E", k).group(1) for k in kernels}           # the mangled template arguments <OUT, MT, RB>
    assert got == want, f"missing {sorted(want - got)}, unexpected {sorted(got - want)}"
    for k, v in kernels.items():
        assert v.get("private_segment_fixed_size") == 0 and v.get("vgpr_spill_count") == 0 and v.get("sgpr_spill_count") == 0, (k, v)
        assert 0 < v.get("vgpr_count") <= 128, (k, v)
