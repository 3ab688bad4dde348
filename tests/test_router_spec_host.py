"""CPU: QSPEC RT (tests/router_spec.py) against the torch recipes it restates, the designed rows held to their own conditions on the reference alone, the argument
checks of pq_moe_topk (every bad argument refused and named before any HIP call, so none of this needs a GPU), and the built code object of moe_topk_kernels.hip: no
scratch and no spill in any instantiation.

Eager-close on the CPU, on rows whose f32 probabilities are pairwise distinct (asserted on torch's output alone): ids equal; f32 weights within 4 x eager's own largest
relative error against a binary64 evaluation of the recipe; bf16 / fp16 weights within 1 ulp of eager's (two binary32 values that agree to ~2^-20 round to the same or to
neighbouring 16-bit values)."""
import os
import re

import numpy as np
import pytest
import torch

from oracle.qspec_numpy import from_f32, to_f32
from tests import code_objects, router_spec as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "pq_moe_topk"
ARGS = ["logits", "dtype", "ld_logits", "T", "E", "k", "kind", "renormalise", "weights", "w_dtype", "ld_w", "ids", "ids_are_int64", "ld_ids", "stream"]
TORCH_DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}


def stored_to_torch(a, dtype):
    return torch.from_numpy(a.copy()) if dtype == "f32" else torch.from_numpy(a.view(np.int16).copy()).view(TORCH_DT[dtype])


def torch_to_stored(t, dtype):
    return t.numpy().copy() if dtype == "f32" else t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def torch_recipe(l: torch.Tensor, k, kind, renorm, dt=torch.float32):
    """the eager chains the kernel replaces, evaluated in `dt` (float32: the model's; float64: the yardstick of both)"""
    if kind == "softmax_topk":
        p = torch.softmax(l.to(dt), dim=1)
        w, ids = torch.topk(p, k, dim=-1)
        if renorm:
            w = w / w.sum(dim=-1, keepdim=True)
        return w, ids, p
    v, ids = torch.topk(l, k, dim=-1)
    return torch.softmax(v.to(dt), dim=1), ids, torch.softmax(l.to(dt), dim=1)


def distinct_logits(T, E, dtype, seed):
    """rows of E DISTINCT logits each, other values in every row: drawn per row without replacement from the multiples of 1/32 in [-8, 8] (513 values, exact in bf16) or,
    for fp16 and f32, of 1/128 (2049 values, exact in fp16); f32 rows moved element by element by less than a quarter step.  Logits a step apart have pairwise distinct
    f32 probabilities, which the test asserts on torch's output."""
    g = torch.Generator().manual_seed(seed)
    step, n = (1.0 / 32, 513) if dtype == "bf16" else (1.0 / 128, 2049)
    grid = (torch.arange(n, dtype=torch.float32) - n // 2) * step
    rows = grid[torch.rand(T, n, generator=g).argsort(dim=1)[:, :E]]
    if dtype == "f32":
        return (rows + (torch.rand(T, E, generator=g) - 0.5) * (step / 2)).numpy()
    out = rows.to(TORCH_DT[dtype])
    assert torch.equal(out.float(), rows)
    return torch_to_stored(out, dtype)


def assert_distinct_probabilities(p: torch.Tensor):
    s = torch.sort(p, dim=1).values
    assert bool((s[:, 1:] != s[:, :-1]).all()), "the rows were meant to have pairwise distinct f32 probabilities"


@pytest.mark.parametrize("kind,renorm", [("softmax_topk", False), ("softmax_topk", True), ("topk_softmax", False)])
@pytest.mark.parametrize("E,k,dtype", [(8, 2, "f32"), (64, 8, "f32"), (128, 8, "f32"), (32, 4, "f32"), (60, 4, "bf16"), (128, 8, "fp16"), (8, 2, "bf16"), (384, 8, "fp16")])
def test_reference_against_the_torch_recipe(E, k, dtype, kind, renorm):
    T = 256
    stored = distinct_logits(T, E, dtype, seed=E * 7 + k)
    l = stored_to_torch(stored, dtype)
    w32, ids_t, p = torch_recipe(l, k, kind, renorm)
    assert_distinct_probabilities(p)
    w64, ids64, _ = torch_recipe(l, k, kind, renorm, torch.float64)
    _, ids, wf = RS.moe_topk(stored, dtype, k, kind, renorm, "f32")
    assert np.array_equal(ids, ids_t.numpy()) and np.array_equal(ids, ids64.numpy())
    err_spec = float(((torch.from_numpy(wf).double() - w64).abs() / w64).max())
    err_eager = float(((w32.double() - w64).abs() / w64).max())
    print(f"E={E} k={k} {dtype} {kind} renorm={renorm}: largest relative error vs binary64: spec {err_spec:.3e}, eager {err_eager:.3e}")
    assert err_spec <= 4 * err_eager
    for wd in ("bf16", "fp16"):
        got = RS.moe_topk(stored, dtype, k, kind, renorm, wd)[0].astype(np.int64)
        want = torch_to_stored(w32.to(TORCH_DT[wd]), wd).astype(np.int64)
        assert int(np.abs(got - want).max()) <= 1, (wd, int(np.abs(got - want).max()))
        assert len({r.tobytes() for r in want}) > T // 4, "the rows were meant to differ from each other in their weights"


CASES = [(1, 1), (2, 1), (2, 2), (3, 2), (8, 2), (8, 8), (31, 4), (32, 4), (33, 8), (60, 4), (64, 8), (64, 64), (65, 8), (128, 8), (160, 64), (384, 8), (1000, 8), (1024, 64)]


@pytest.mark.parametrize("E,k", CASES)
def test_designed_rows_hold_their_own_conditions(E, k):
    G, S = RS.layout(E)
    assert G in (4, 8, 16, 32, 64) and G * S >= E and (G == 64 or S == 1) and S <= 16
    for dtype in ("bf16", "f32"):
        names, stored = RS.designed_matrix(E, k, dtype)
        l = to_f32(stored, dtype)
        seen = set()
        for kind in RS.KINDS:
            for renorm in (False, True):
                w, ids, wf = RS.moe_topk(stored, dtype, k, kind, renorm, "f32")
                assert ids.shape == (len(names), k) and ids.min() >= 0 and ids.max() < E
                assert all(len(set(r)) == k for r in ids.tolist()), "ids of a row are distinct, whatever it holds"
                for name, row, rid, rw in zip(names, l, ids, wf):
                    tag = name.split(":")[0].split("@")[0]
                    seen.add(tag)
                    sel = row[rid]
                    key = RS.order_keys(sel[None])[0].astype(np.int64)
                    assert np.all(key[:-1] >= key[1:]), (name, "slot 0 is the largest")
                    rest = np.delete(np.arange(E), rid)
                    if rest.size:
                        assert RS.order_keys(row[rest][None])[0].astype(np.int64).max() <= key[-1], (name, "nothing left out is larger than the last one taken")
                    if tag == "equal" or name == "zeros":
                        assert rid.tolist() == list(range(k)), name
                        assert np.all(rw == rw[0]), name
                    elif tag == "max":
                        p = int(name.split("@")[1].split(":")[0])
                        assert rid[0] == p, name
                        if name.endswith(":flat"):
                            assert rid[1:].tolist() == [e for e in range(E) if e != p][:k - 1], name
                    elif tag == "ties":
                        n, j = int(name.split(":")[1]), int(name.split(":")[2])
                        group = np.flatnonzero(row == np.float32(3.25))
                        assert group.size == n and j < k < j + n, name
                        assert np.all(row[rid[:j]] > 3.25) and rid[j:].tolist() == group[:k - j].tolist(), (name, "the tie group straddles k: its lowest ids are taken")
                    elif tag in ("nan", "nan2", "+inf", "allinf", "mixed"):
                        assert np.all(np.isnan(rw)) and np.all(rw.view(np.uint32) == 0x7FC00000), name
                        if tag in ("nan", "nan2", "mixed"):
                            assert rid[0] == np.flatnonzero(np.isnan(row))[0], (name, "NaN sorts first, the lower id among NaNs")
                    elif tag == "spread" and kind == "softmax_topk" and not renorm:
                        assert rid[0] == int(np.argmax(row)) and 1 - 1e-9 <= float(rw[0]) <= 1.0, name       # the clamp adds at most (E - 1) * exp_spec(-30) < 1e-10
                        if k > 1:
                            assert np.all(rw[1:] == rw[1]) and 9.0e-14 < float(rw[1]) < 9.7e-14, name
                    if tag in ("-inf", "maxfinite", "subnormal", "spread", "ties", "max", "equal"):
                        assert np.all(np.isfinite(rw)), name
                        if kind == "topk_softmax" or renorm:
                            assert abs(float(rw.astype(np.float64).sum()) - 1.0) < 1e-5, name
        assert {"equal", "max", "nan", "+inf", "spread", "subnormal", "maxfinite", "mixed"} <= seen and ("-inf" in seen or E == 1)
        if E >= 3 and k < E:
            assert "ties" in seen


def test_pinned_sum_depends_on_the_dealing():
    """the order of RT3 is the pinned one: on a row built so that orders differ, the reference gives the bits of lanes-then-butterfly, not of a left-to-right sum"""
    x = np.zeros((1, 128), np.float32)
    x[0, 0], x[0, 1:] = np.float32(2.0 ** 24), np.float32(1.0)
    lr = np.float32(0)
    for v in x[0]:
        lr = np.float32(lr + v)
    assert lr == np.float32(2.0 ** 24)                       # left to right every 1 is lost
    assert RS.pinned_sum(x)[0] == np.float32(2.0 ** 24 + 126)          # lane 0 loses its second slot's 1; the butterfly adds 63 pairs of 1 exactly
    assert np.array_equal(RS.pinned_sum(np.repeat(x, 5, axis=0)), np.full(5, 2.0 ** 24 + 126, np.float32))          # a row's sum does not depend on its neighbours


def test_symbol_declared_exported_and_bound():
    import ctypes

    from protoquant_amd import _lib
    src = open(os.path.join(ROOT, "include", "pq_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % SYM, hdr)
    assert m, f"pq_hip.h does not declare {SYM}"
    assert [re.split(r"[\s*]+", a.strip())[-1] for a in m.group(1).split(",")] == ARGS
    assert re.search(r"#define\s+PQ_ROUTER_SOFTMAX_TOPK\s+0\b", src) and re.search(r"#define\s+PQ_ROUTER_TOPK_SOFTMAX\s+1\b", src)
    L = _lib.lib()
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert hasattr(L, SYM) and SYM in _lib.EXPORTS
    assert list(getattr(L, SYM).argtypes) == [vp, i32, i64, i64, i32, i32, i32, i32, vp, i32, i64, vp, i32, i64, vp] and getattr(L, SYM).restype is i32
    assert _lib.ROUTER_KINDS == {"softmax_topk": 0, "topk_softmax": 1}
    assert not re.search(r"pq_\w+_rowwise(_amax)?$|pq_\w+_rowamax$|pq_quant_\w+$|pq_dequant$|pq_moe_combine$", SYM)      # no row entry: no row of tests/row_forms.py
    assert SYM in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    import protoquant_amd as pq
    for name in ("moe_topk", "fuse_moe_routers"):
        assert name in pq.__all__ and callable(getattr(pq, name)), name
    assert pq.MoEBlock.hip_routing is False


def _call(L, **kw):
    """64 tokens x 128 bf16 logits, k = 8, bf16 weights, int64 ids; addresses that are never dereferenced"""
    a = dict(logits=0x100000, dtype=0, ldl=128, T=64, E=128, k=8, kind=0, renorm=1, w=0x200000, wdt=0, ldw=8, ids=0x300000, i64=1, ldi=8)
    a.update(kw)
    return getattr(L, SYM)(a["logits"], a["dtype"], a["ldl"], a["T"], a["E"], a["k"], a["kind"], a["renorm"], a["w"], a["wdt"], a["ldw"], a["ids"], a["i64"], a["ldi"], None)


BAD = [
    (dict(logits=None), 1, b"logits is null"), (dict(w=None), 1, b"weights is null"), (dict(ids=None), 1, b"ids is null"),
    (dict(E=0), 1, b"E = 0"), (dict(E=1025, ldl=1025), 1, b"E = 1025"), (dict(k=0), 1, b"k = 0"), (dict(E=4, k=5, ldl=4), 1, b"k = 5 > E = 4"),
    (dict(k=65, ldw=65, ldi=65), 1, b"k = 65"), (dict(dtype=3), 1, b"dtype"), (dict(dtype=-1), 1, b"dtype"), (dict(wdt=3), 1, b"w_dtype"), (dict(wdt=-1), 1, b"w_dtype"),
    (dict(kind=2), 1, b"kind"), (dict(kind=-1), 1, b"kind"), (dict(renorm=2), 1, b"renormalise"), (dict(i64=2), 1, b"ids_are_int64"),
    (dict(ldl=127), 1, b"ld_logits"), (dict(ldw=7), 1, b"ld_w"), (dict(ldi=7), 1, b"ld_ids"), (dict(T=-1), 1, b"T = -1"), (dict(T=1 << 31), 1, b"2^31"),
    (dict(logits=0x100001), 2, b"logits"), (dict(w=0x200002, wdt=2), 2, b"weights"), (dict(ids=0x300004), 2, b"ids"),
    (dict(w=0x100000), 1, b"weights overlaps logits"), (dict(ids=0x100000 + 64), 1, b"ids overlaps logits"), (dict(ids=0x200000 + 8), 1, b"overlaps"),
]


@pytest.mark.parametrize("kw,status,named", BAD, ids=[f"{i}-{n.decode().replace(' ', '_')}" for i, (_, _, n) in enumerate(BAD)])
def test_bad_arguments_are_named_before_any_hip_call(kw, status, named):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _call(L, **kw) == status, (kw, L.pq_last_error())          # a call that reached the launch answers 3 on a machine without a GPU
    err = L.pq_last_error()
    assert SYM.encode() in err and named in err, (kw, err)


def test_no_tokens_is_a_no_op_and_there_is_no_cpu_path():
    import protoquant_amd as pq
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _call(L, T=0, logits=None, w=None, ids=None) == 0
    assert _call(L, T=0, ldl=127) == 1                                # the checks of the shape still run
    with pytest.raises(_lib.PQError):
        pq.moe_topk(torch.zeros(4, 8), 2)
    with pytest.raises(ValueError):
        pq.moe_topk(torch.zeros(4, 8), 2, kind="sigmoid")


def test_code_object_has_no_scratch_and_the_expected_kernels():
    kernels = code_objects.kernels_of("moe_topk_kernels", must_be_built=True)
    assert len(kernels) == 3 * 9 and all("moe_topk_kernel" in k for k in kernels), sorted(kernels)          # 3 logits dtypes x (G = 4 .. 64 with one slot, 64 lanes x 2 / 4 / 8 / 16 slots)
    for name, notes in kernels.items():
        assert notes["private_segment_fixed_size"] == 0 and notes["vgpr_spill_count"] == 0 and notes["sgpr_spill_count"] == 0, (name, notes)
        assert notes["vgpr_count"] <= (80 if "ELi16E" in name else 64), (name, notes)          # eight waves per SIMD; six for the 16-slot layout (E > 512)
