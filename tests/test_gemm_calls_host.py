"""CPU: the contract between the GEMM wrappers (protoquant_amd/qlinear.py, w4.py, moe.GroupedQLinear) and libpq_hip.so, pinned call by call, the way
tests/test_qtensor_calls_host.py pins qtensor.py.  Every wrapper, module forward, constructor and tree walker is driven on CPU tensors with the library replaced by a
recording fake, and what it does is compared with tests/golden/gemm_calls.json: every symbol called, every argument (a pointer as the operand it points into plus the byte
offset, `workspace+<offset>` for the cached workspace, `copy(x)` / `cast(x)` for a dense copy or a dtype cast of an input, `new[shape]dtype` for a buffer the wrapper
allocated, `gather(xs,row_index)` for scales gathered into grouped order; every number verbatim), what is handed to require_gpu / check, the sizes of the cached workspaces, what is returned (structure, shapes, dtypes, strides; for a
module its buffers, attributes and state_dict keys) and which results ARE inputs; for a refused call the exception's type and message.  The patches are those of the
qtensor test plus torch.cuda.current_stream -> stream 0, is_current_stream_capturing -> False, clear_workspaces() before each case, and `*_workspace_bytes*` queries that
answer a fixed value per case (0: the null-pointer arm; 4096: the pointer-and-size arm).

    python -m tests.test_gemm_calls_host --record        rewrites the golden file from the code as it stands

A trace that changes is a change of behaviour: understand it before recording it."""
import contextlib
import ctypes
import importlib
import json
import os
import sys
import types

import pytest
import torch
from torch import nn

from protoquant_amd import _lib
from protoquant_amd import moe as MOE
from protoquant_amd import qtensor as Q
from protoquant_amd import w4 as W4
from tests.test_qtensor_calls_host import BF, F32, F64, HF, I8, I32, _extent, _resolve, mk

QL = importlib.import_module("protoquant_amd.qlinear")          # (the package attribute of that name is the qlinear CLASS)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_calls.json")
U8 = torch.uint8
W4_FUNCS = ("w4_pack", "w4_expand", "int_mm_w4", "qlinear_w4", "int_mm_w4_grouped", "qlinear_w4_grouped", "swap_linears_w4", "swap_moe_experts_w4")


class Plain:
    """a result recorded verbatim (JSON-able)"""

    def __init__(self, value):
        self.value = value


class FakeCuda(torch.Tensor):
    """a CPU tensor that answers is_cuda = True: gemm_operands passes CPU stand-ins through"""
    is_cuda = property(lambda self: True)


def _fn(fname):
    return getattr(W4 if fname in W4_FUNCS else QL, fname)


def call(fname, make, **change):
    """a case: <fname>(**make()) with `change` applied (a callable value is called with the keyword arguments made so far)"""
    def build():
        kw = make()
        for k, v in change.items():
            kw[k] = v(kw) if callable(v) else v
        return kw, lambda: _fn(fname)(**kw)
    return build


# ------------------------------------------------------------------------------------------------------------------------------------------------- operands
def dense(M=4, N=8, K=128, t=False):
    return lambda: dict(xq=mk((M, K), I8, 0), xs=mk((M,), F32, 1), wq=mk((N, K), I8, 2), ws=mk((N,), F32, 3), bias=mk((N,), BF, 4), out_dtype=BF)


def kslabs(M=4, N=8, G=2, kps=64):
    return lambda: dict(xq_stacked=mk((G, M, kps), I8, 0), xs=mk((M,), F32, 1), wq=mk((N, G * kps), I8, 2), ws=mk((N,), F32, 3), bias=mk((N,), BF, 4), out_dtype=BF)


def dyn(M=4, N=8, K=128, lead=None):
    return lambda: dict(x=mk(lead + (K,) if lead else (M, K), BF, 0), wq=mk((N, K), I8, 2), ws=mk((N,), F32, 3), bias=mk((N,), BF, 4))


def imm(M=4, N=8, K=128):
    return lambda: dict(xq=mk((M, K), I8, 0), wq=mk((N, K), I8, 2))


def _offsets(E):
    return mk((E + 1,), I32, 5)          # (never read on the host)


def grouped(M=4, E=3, N=8, K=128, R=None, epi=True):
    """R: rows of xq when a row_index of M entries reads them"""
    def make():
        kw = dict(xq=mk((R or M, K), I8, 0))
        if epi:
            kw["xs"] = mk((M,), F32, 1)
        kw["wq"] = mk((E, N, K), I8, 2)
        if epi:
            kw.update(ws=mk((E, N), F32, 3), bias=mk((E, N), BF, 4))
        kw["offsets"] = _offsets(E)
        if epi:
            kw["out_dtype"] = BF
        if R:
            kw["row_index"] = mk((M,), I32, 6)
        return kw
    return make


def packed(N=8, kp=128, seed=2):
    return mk((N, kp // 2), U8, seed), mk(((N + 3) // 4, kp // 128, 4), U8, seed + 1)


def w4dense(M=4, N=8, kp=128, epi=True):
    def make():
        w4, gs = packed(N, kp)
        if not epi:
            return dict(xq=mk((M, kp), I8, 0), w4=w4, gs=gs)
        return dict(xq=mk((M, kp), I8, 0), xs=mk((M,), F32, 1), w4=w4, gs=gs, ws=mk((N,), F32, 5), bias=mk((N,), BF, 4), out_dtype=BF)
    return make


def w4grouped(M=4, E=3, N=8, kp=128, R=None, epi=True):
    def make():
        kw = dict(xq=mk((R or M, kp), I8, 0))
        if epi:
            kw["xs"] = mk((M,), F32, 1)
        kw.update(w4=mk((E, N, kp // 2), U8, 2), gs=mk((E, (N + 3) // 4, kp // 128, 4), U8, 3))
        if epi:
            kw.update(ws=mk((E, N), F32, 7), bias=mk((E, N), BF, 4))
        kw["offsets"] = _offsets(E)
        if epi:
            kw["out_dtype"] = BF
        if R:
            kw["row_index"] = mk((M,), I32, 6)
        return kw
    return make


# ------------------------------------------------------------------------------------------------------------------------------------------------- modules
def _qt(shape, axis=1, seed=9):
    lead = 1
    for d in shape[:-1]:
        lead *= d
    return Q.QTensor(mk(shape, I8, seed), mk((lead,) if axis == 1 else (shape[-1],), F32, seed + 1), axis, BF, torch.Size(shape))


def qlin(K=128, N=8, bias=BF, seed=0):
    return QL.qlinear.from_qtensor(Q.QTensor(mk((N, K), I8, seed + 2), mk((N,), F32, seed + 3), 1, BF, torch.Size((N, K))), None if bias is None else mk((N,), bias, seed + 4))


def linear(K=128, N=8, bias=True, seed=0, cls=nn.Linear):
    lin = cls(K, N, bias=bias, dtype=BF)
    with torch.no_grad():
        lin.weight.copy_(mk((N, K), BF, seed))
        if bias:
            lin.bias.copy_(mk((N,), BF, seed + 1))
    return lin


def fusedq(K=128):
    return QL.FusedQLinear([qlin(K, 8, seed=0), qlin(K, 4, seed=5)])


def groupedq(E=3, K=128, N=8, bias=True):
    return MOE.GroupedQLinear.from_linears([qlin(K, N, BF if bias else None, seed=5 * e) for e in range(E)])


def _fill(m):
    with torch.no_grad():
        for i, (_, b) in enumerate(m.named_buffers()):
            b.copy_(mk(tuple(b.shape), b.dtype, i + 2))
    return m


def qlin_w4(K=128, N=8, bias=True):
    return _fill(W4.QLinearW4(K, N, bias=bias))


def groupedq_w4(E=3, K=128, N=8, bias=True):
    return _fill(W4.GroupedQLinearW4(E, K, N, bias=bias))


MODULES = {"qlinear": qlin, "FusedQLinear": fusedq, "GroupedQLinear": groupedq, "QLinearW4": qlin_w4, "GroupedQLinearW4": groupedq_w4}


def forward(kind, K, x, **attrs):
    """a case: <module of `kind` with in_features K>.forward(*x()) (x() gives the positional arguments as a dict name -> value)"""
    def build():
        m = MODULES[kind](K=K)
        for a, v in attrs.items():
            setattr(m, a, v)
        args = x(K)
        return dict(m=m, **args), lambda: m(*args.values())
    return build


def made(f):
    """a case that makes something of inputs: f() -> (inputs, thunk)"""
    return f


# trees for the walkers
class OddLinear(nn.Linear):
    def forward(self, x):
        return super().forward(x), None


class Conv1D(nn.Module):
    def __init__(self, nf, nx):
        super().__init__()
        self.nf = nf
        self.weight, self.bias = nn.Parameter(mk((nx, nf), BF, 5)), nn.Parameter(mk((nf,), BF, 6))


def _tree(moe=False):
    root, blk, mlp = nn.Module(), nn.Module(), nn.Module()
    root.a, root.q, root.blk = linear(seed=1), qlin(seed=2), blk
    blk.b, blk.skip, blk.odd, blk.c1d, blk.mlp = linear(200, 4, False, seed=3), linear(seed=4), linear(seed=5, cls=OddLinear), Conv1D(8, 128), mlp
    mlp.gate_proj, mlp.up_proj, mlp.down_proj, mlp.act_fn = linear(128, 256, False, 6), linear(128, 256, False, 7), linear(256, 128, False, 8), nn.SiLU()
    if moe:
        for name, parent in (("moe", root), ("moe2", blk), ("skip_moe", blk)):
            setattr(parent, name, MOE.MoEGatedMLP(groupedq(2, 128, 16, False), groupedq(2, 8, 128, False)))
    return root


def _classes(model):
    return {n: type(m).__name__ for n, m in model.named_modules() if n}


def walk(fname, moe=False, **kw):
    def build():
        model = _tree(moe)

        def run():
            before = _classes(model)
            first = _fn(fname)(model, **kw)
            after = _classes(model)
            second = _fn(fname)(model, **kw)
            say = lambda r: "the model" if r is model else r          # noqa: E731
            return Plain({"replaced": {n: c for n, c in after.items() if before.get(n) != c}, "returned": say(first), "second call": say(second),
                          "after the second": {n: c for n, c in _classes(model).items() if after.get(n) != c}})
        return dict(model=model), run
    return build


def skip_pred(name, mod):
    return not name.startswith("skip")


# ------------------------------------------------------------------------------------------------------------------------------------------------- the cases
def cases():
    """id -> (build, the answer of the workspace queries); build() -> (named inputs, thunk)"""
    out = {}

    def add(cid, build, wsq=0):
        assert cid not in out, cid
        out[cid] = (build, wsq)

    def epilogue_and_out(fname, base, oshape, add_as=None, N=8, M=4, vec=True):
        """the variations every fused entry shares: bias, out, xs / ws"""
        a = lambda tag, wsq=0, **ch: add(f"{add_as or fname}/{tag}", call(fname, base, **ch), wsq)          # noqa: E731
        bshape = (N,) if vec else (3, N)
        a("bias=None", bias=None)
        a("bias f32 (cast)", bias=mk(bshape, F32, 4))
        a("bias f16 (cast),out_dtype f32", bias=mk(bshape, HF, 4), out_dtype=F32)
        a("bias:length", bias=mk((N + 1,) if vec else (3, N + 1), BF, 4))
        a("out_dtype f64", out_dtype=F64)
        a("out=valid", out=mk(oshape, BF, 12))
        a("out=valid,ws=4096", 4096, out=mk(oshape, BF, 12))
        a("out=row slice of a wider buffer", out=mk((oshape[0], 3 * oshape[1]), BF, 12)[:, oshape[1]:2 * oshape[1]])
        a("out:shape", out=mk((oshape[0] + 1, oshape[1]), BF, 12))
        a("out:3d", out=mk((1,) + oshape, BF, 12))
        a("out:dtype", out=mk(oshape, HF, 12))
        a("out:column stride", out=mk((oshape[1], oshape[0]), BF, 12).t())
        a("xs:dtype", xs=mk((M,), BF, 1))
        a("xs:length", xs=mk((M + 1,), F32, 1))
        a("xs:strided", xs=mk((2 * M,), F32, 1)[::2])
        a("ws:dtype", ws=mk(bshape, BF, 3))
        a("ws:length", ws=mk((N + 1,) if vec else (3, N + 1), F32, 3))

    # ---- the dense fused entries
    for fname, base, xname, osh in (("qlinear_s8", dense, "xq", lambda M, N: (M, N)), ("qlinear_s8_t", dense, "xq", lambda M, N: (N, M)),
                                    ("qlinear_s8_kslabs", kslabs, "xq_stacked", lambda M, N: (M, N))):
        a = lambda tag, make=None, wsq=0, **ch: add(f"{fname}/{tag}", call(fname, make or base(), **ch), wsq)          # noqa: E731
        a("plain")
        a("plain,ws=4096", wsq=4096)
        a("M=0", base(M=0))
        a("N=0", base(N=0))
        a("M=1,N=1", base(M=1, N=1))
        a("wq a column slice", wq=mk((8, 384), I8, 2)[:, 128:256])
        a("wq:last stride (copied)", wq=mk((128, 8), I8, 2).t())
        a("wq:dtype", wq=mk((8, 128), U8, 2))
        a("wq:K mismatch", wq=mk((8, 256), I8, 2))
        a("wq:3d", wq=mk((1, 8, 128), I8, 2))
        a(f"{xname}:dtype", **{xname: lambda kw, xname=xname: kw[xname].to(U8)})
        if fname != "qlinear_s8_kslabs":
            a("xq a column slice", xq=mk((4, 384), I8, 0)[:, 128:256])
            a("xq:last stride (copied)", xq=mk((128, 4), I8, 0).t())
            a("xq:1d", xq=mk((128,), I8, 0))
            a("K=200", base(K=200))
            a("K=200,ws=4096", base(K=200), wsq=4096)
            a("K=0", base(K=0))
            a("M N K = 2^31 - 2^20 (no pad)", base(1024, 1024, 2047), bias=None)
            a("M N K = 2^31 + 2^20 (padded)", base(1024, 1024, 2049), bias=None)
            a("M N K = 2^31 + 2^20 (padded),ws=4096", base(1024, 1024, 2049), wsq=4096, bias=None)
        else:
            a("G=1", base(G=1, kps=128))
            a("k_per_slab=100", base(G=2, kps=100))
            a("xq:not contiguous", xq_stacked=mk((2, 4, 128), I8, 0)[:, :, :64])
            a("xq:2d", xq_stacked=mk((4, 128), I8, 0))
        epilogue_and_out(fname, base(), osh(4, 8))
    for args in ((4, 8, 128), (4, 8, 0), (4, 8, 200), (1 << 15, 1 << 15, 2), (1 << 15, 1 << 15, 1), (1024, 1024, 2047), (1024, 1024, 2048), (1024, 1024, 2049), (0, 8, 200)):
        add(f"_pad_pays/{args!r}", made(lambda args=args: ({}, lambda: Plain(QL._pad_pays(*args)))))

    a = lambda tag, make=None, wsq=0, **ch: add(f"int_mm/{tag}", call("int_mm", make or imm(), **ch), wsq)          # noqa: E731
    a("plain")
    a("M=0", imm(M=0))
    a("N=0", imm(N=0))
    a("column slices", xq=mk((4, 384), I8, 0)[:, 128:256], wq=mk((8, 384), I8, 2)[:, 128:256])
    a("last strides (copied)", xq=mk((128, 4), I8, 0).t(), wq=mk((128, 8), I8, 2).t())
    a("xq:dtype", xq=mk((4, 128), U8, 0))
    a("wq:dtype", wq=mk((8, 128), I32, 2))
    a("K mismatch", wq=mk((8, 256), I8, 2))
    a("K=200", imm(K=200))
    a("M N K = 2^31 - 2^20 (no pad)", imm(1024, 1024, 2047))
    a("M N K = 2^31 + 2^20 (padded)", imm(1024, 1024, 2049))

    a = lambda tag, make=None, wsq=0, **ch: add(f"qlinear_dyn/{tag}", call("qlinear_dyn", make or dyn(), **ch), wsq)          # noqa: E731
    a("plain")
    a("plain,ws=4096", wsq=4096)
    a("3d", dyn(lead=(2, 3)))
    a("1d", dyn(lead=()))
    a("M=0", dyn(M=0))
    a("N=0", dyn(N=0))
    a("K=200", dyn(K=200))
    a("f16", x=mk((4, 128), HF, 0))
    a("f64", x=mk((4, 128), F64, 0))
    a("column slices", x=mk((4, 384), BF, 0)[:, 128:256], wq=mk((8, 384), I8, 2)[:, 128:256])
    a("last strides (copied)", x=mk((128, 4), BF, 0).t(), wq=mk((128, 8), I8, 2).t())
    a("bias=None", bias=None)
    a("bias f32 (cast)", bias=mk((8,), F32, 4))
    a("bias:length", bias=mk((9,), BF, 4))
    a("wq:dtype", wq=mk((8, 128), U8, 2))
    a("wq:K mismatch", wq=mk((8, 256), I8, 2))
    a("ws:dtype", ws=mk((8,), BF, 3))
    a("ws:length", ws=mk((9,), F32, 3))
    a("M N K = 2^31 + 2^20 (quantize, then padded qlinear_s8)", dyn(1024, 1024, 2049), wsq=4096)

    # ---- the grouped int8 entries
    for fname, epi in (("qlinear_s8_grouped", True), ("qlinear_s8_grouped_stream", True), ("int_mm_grouped", False), ("int_mm_grouped_stream", False)):
        g = lambda **k: grouped(epi=epi, **k)          # noqa: E731
        a = lambda tag, make=None, **ch: add(f"{fname}/{tag}", call(fname, make or g(), **ch))          # noqa: E731
        a("E=3")
        a("E=1", g(E=1))
        a("E=3,row_index", g(R=3))
        a("E=1,row_index", g(E=1, R=2))
        a("N=1", g(N=1))
        a("N=1,E=1", g(N=1, E=1))
        a("N=0", g(N=0))
        a("M=0", g(M=0))
        a("64 rows", g(M=64))
        a("65 rows", g(M=65))
        a("65 rows through a row_index over 3", g(M=65, R=3))
        a("K=192", g(K=192))
        a("K=0", g(K=0))
        a("K=256,xq a column slice", g(K=256), xq=mk((4, 512), I8, 0)[:, 256:])
        a("xq:last stride (copied)", xq=mk((128, 4), I8, 0).t())
        a("xq:dtype", xq=mk((4, 128), U8, 0))
        a("wq:padded row pitch", wq=mk((3, 8, 256), I8, 2)[:, :, :128])
        a("wq:padded expert stride", wq=mk((3, 10, 128), I8, 2)[:, :8])
        a("wq:padded both,E=1", g(E=1), wq=mk((1, 10, 256), I8, 2)[:, :8, :128])
        a("wq:last stride (copied)", wq=mk((3, 128, 8), I8, 2).transpose(1, 2))
        a("wq:experts overlap (copied)", wq=mk((1, 8, 128), I8, 2).expand(3, 8, 128))
        a("wq:dtype", wq=mk((3, 8, 128), U8, 2))
        a("wq:2d", wq=mk((8, 128), I8, 2))
        a("wq:K mismatch", wq=mk((3, 8, 256), I8, 2))
        a("offsets:dtype", offsets=mk((4,), torch.int64, 5))
        a("offsets:length", offsets=mk((3,), I32, 5))
        a("row_index:dtype", g(R=3), row_index=mk((4,), torch.int64, 6))
        a("row_index:2d", g(R=3), row_index=mk((2, 2), I32, 6))
        a("row_index:strided", g(R=3), row_index=mk((8,), I32, 6)[::2])
        odt = BF if epi else I32
        a("out=valid", out=mk((4, 8), odt, 12))
        a("out=row slice of a wider buffer,row_index", g(R=3), out=mk((4, 24), odt, 12)[:, 8:16])
        a("out:shape", out=mk((5, 8), odt, 12))
        a("out:3d", out=mk((1, 4, 8), odt, 12))
        a("out:dtype", out=mk((4, 8), HF, 12))
        a("out:column stride", out=mk((8, 4), odt, 12).t())
        if epi:
            a("bias=None", bias=None)
            a("bias f32 (cast)", bias=mk((3, 8), F32, 4))
            a("bias:shape", bias=mk((8,), BF, 4))
            a("bias:not contiguous", bias=mk((3, 16), BF, 4)[:, :8])
            a("out_dtype f64", out_dtype=F64)
            a("xs:dtype", xs=mk((4,), BF, 1))
            a("xs:length", xs=mk((5,), F32, 1))
            a("xs:length of xq under a row_index", g(M=4, R=3), xs=mk((3,), F32, 1))
            a("ws:dtype", ws=mk((3, 8), BF, 3))
            a("ws:shape", ws=mk((24,), F32, 3))
            a("ws:not contiguous", ws=mk((3, 16), F32, 3)[:, :8])

    # ---- W4: the dense entries
    a = lambda tag, **ch: add(f"w4_pack/{tag}", call("w4_pack", lambda: dict(wq=mk((8, 128), I8, 2)), **ch))          # noqa: E731
    a("plain")
    for tag, t in (("K=200", mk((8, 200), I8, 2)), ("K=0", mk((8, 0), I8, 2)), ("N=0", mk((0, 128), I8, 2)), ("N=6,K=300", mk((6, 300), I8, 2)), ("a column slice", mk((8, 384), I8, 2)[:, 128:256]),
                   ("last stride (copied)", mk((128, 8), I8, 2).t()), ("dtype", mk((8, 128), U8, 2)), ("3d", mk((1, 8, 128), I8, 2))):
        a(tag, wq=t)

    def pk(N=8, kp=256, **kw):
        return lambda: dict(zip(("w4", "gs"), packed(N, kp)), **kw)
    a = lambda tag, make=None, **ch: add(f"w4_expand/{tag}", call("w4_expand", make or pk(), **ch))          # noqa: E731
    a("K=None")
    a("K=Kp", K=256)
    a("K in range", K=200)
    a("K=Kp-127", K=129)
    a("K=Kp-128 (out of range)", K=128)
    a("K=Kp+1 (out of range)", K=257)
    a("N=0", pk(N=0))
    a("N=6", pk(N=6))
    a("w4:dtype", w4=mk((8, 128), I8, 2))
    a("w4:width", w4=mk((8, 96), U8, 2))
    a("w4:3d", w4=mk((1, 8, 128), U8, 2))
    a("gs:dtype", gs=mk((2, 2, 4), I8, 3))
    a("gs:shape", gs=mk((2, 1, 4), U8, 3))
    a("gs:not contiguous", gs=mk((2, 2, 8), U8, 3)[:, :, :4])
    a("w4:padded row pitch", w4=mk((8, 256), U8, 2)[:, :128])
    a("w4:misaligned by one column (copied)", w4=mk((8, 129), U8, 2)[:, 1:])
    a("w4:last stride (copied)", w4=mk((128, 8), U8, 2).t())

    a = lambda tag, make=None, **ch: add(f"int_mm_w4/{tag}", call("int_mm_w4", make or w4dense(epi=False), **ch))          # noqa: E731
    a("plain")
    a("64 rows", w4dense(M=64, epi=False))
    a("65 rows", w4dense(M=65, epi=False))
    a("M=0", w4dense(M=0, epi=False))
    a("N=0", w4dense(N=0, epi=False))
    a("Kp=256,N=6", w4dense(N=6, kp=256, epi=False))
    a("xq:K mismatch", xq=mk((4, 256), I8, 0))
    a("xq:dtype", xq=mk((4, 128), U8, 0))
    a("xq:misaligned by one column (copied)", xq=mk((4, 129), I8, 0)[:, 1:])
    a("xq an aligned column slice", xq=mk((4, 384), I8, 0)[:, 128:256])
    a("gs:shape", gs=mk((2, 2, 4), U8, 3))

    a = lambda tag, make=None, wsq=0, **ch: add(f"qlinear_w4/{tag}", call("qlinear_w4", make or w4dense(), **ch), wsq)          # noqa: E731
    a("plain")
    for rows, ms in ((64, (64, 65)), (8, (8, 9)), (0, (0, 1)), (100, (64, 65))):
        for M in ms:
            a(f"stream_rows={rows},M={M}", w4dense(M=M), stream_rows=rows)
    a("expand,ws=4096", w4dense(M=65), wsq=4096)
    a("expand,ws=4000 (front rounds up)", w4dense(M=65), wsq=4000)
    a("expand,Kp=256,N=6,ws=4096", w4dense(M=3, N=6, kp=256), wsq=4096, stream_rows=0)
    a("expand,N=0", w4dense(M=65, N=0))
    a("expand,out=valid", w4dense(M=65), out=mk((65, 8), BF, 12))
    a("expand,bias f32 (cast)", w4dense(M=65), bias=mk((8,), F32, 4))
    a("expand,w4:misaligned by one column (copied)", w4dense(M=65), w4=mk((8, 65), U8, 2)[:, 1:])
    a("N=0", w4dense(N=0))
    a("M=0", w4dense(M=0))
    a("xq:K mismatch", xq=mk((4, 256), I8, 0))
    a("xq:dtype", xq=mk((4, 128), U8, 0))
    a("xq:misaligned by one column (copied)", xq=mk((4, 129), I8, 0)[:, 1:])
    a("w4:dtype", w4=mk((8, 64), I8, 2))
    a("w4:misaligned by one column (copied)", w4=mk((8, 65), U8, 2)[:, 1:])
    a("gs:dtype", gs=mk((2, 1, 4), I8, 3))
    a("gs:shape", gs=mk((2, 2, 4), U8, 3))
    epilogue_and_out("qlinear_w4", w4dense(), (4, 8))

    # ---- W4: the grouped entries
    for fname, epi in (("qlinear_w4_grouped", True), ("int_mm_w4_grouped", False)):
        g = lambda **k: w4grouped(epi=epi, **k)          # noqa: E731
        a = lambda tag, make=None, wsq=0, **ch: add(f"{fname}/{tag}", call(fname, make or g(), **ch), wsq)          # noqa: E731
        a("stream,E=3")
        a("stream,E=1", g(E=1))
        a("stream,row_index", g(R=3))
        a("stream,N=1", g(N=1))
        a("stream,N=6,Kp=256", g(N=6, kp=256))
        a("N=0", g(N=0))
        a("M=0", g(M=0))
        a("64 rows", g(M=64))
        a("65 rows", g(M=65))
        a("65 rows through a row_index over 3", g(M=65, R=3))
        a("w4:padded expert stride", w4=mk((3, 10, 64), U8, 2)[:, :8])
        a("w4:padded row pitch", w4=mk((3, 8, 128), U8, 2)[:, :, :64])
        a("w4:misaligned by one column (copied)", w4=mk((3, 8, 65), U8, 2)[:, :, 1:])
        a("w4:dtype", w4=mk((3, 8, 64), I8, 2))
        a("w4:2d", w4=mk((8, 64), U8, 2))
        a("w4:E=0", w4=mk((0, 8, 64), U8, 2))
        a("w4:width", w4=mk((3, 8, 96), U8, 2))
        a("gs:dtype", gs=mk((3, 2, 1, 4), I8, 3))
        a("gs:shape", gs=mk((3, 2, 2, 4), U8, 3))
        a("xq:K mismatch", xq=mk((4, 256), I8, 0))
        a("xq:dtype", xq=mk((4, 128), U8, 0))
        a("xq:misaligned by one column (copied)", xq=mk((4, 129), I8, 0)[:, 1:])
        a("offsets:dtype", offsets=mk((4,), torch.int64, 5))
        a("offsets:length", offsets=mk((3,), I32, 5))
        a("row_index:dtype", g(R=3), row_index=mk((4,), torch.int64, 6))
        a("row_index:2d", g(R=3), row_index=mk((2, 2), I32, 6))
        if epi:
            for tag, ch in (("N=8 (one expand)", {}), ("N=8,E=1", None), ("N=6 (per expert)", None), ("w4 with a padded expert stride (per expert)", dict(w4=mk((3, 10, 64), U8, 2)[:, :8])),
                            ("w4 with a padded row pitch (one expand)", dict(w4=mk((3, 8, 128), U8, 2)[:, :, :64])),
                            ("w4 misaligned by one column (copied, one expand)", dict(w4=mk((3, 8, 65), U8, 2)[:, :, 1:])), ("row_index", None), ("out=valid", dict(out=mk((65, 8), BF, 12))),
                            ("bias=None", dict(bias=None))):
                make = {"N=8,E=1": g(M=65, E=1), "N=6 (per expert)": g(M=65, N=6, kp=256), "row_index": g(M=65, R=3)}.get(tag, g(M=65))
                a("expand," + tag, make, **(ch or {}))
                a("expand," + tag + ",ws=4096", make, wsq=4096, **(ch or {}))
            a("expand,stream_rows=0,M=1", g(M=1), stream_rows=0)
            a("expand,stream_rows=2,M=3", g(M=3), stream_rows=2)
            a("stream,stream_rows=100,M=64", g(M=64), stream_rows=100)
            a("expand,N=0", g(M=65, N=0))
            epilogue_and_out(fname, g(), (4, 8), vec=False)
            a("ws:not contiguous", ws=mk((3, 16), F32, 7)[:, :8])
            a("bias:not contiguous", bias=mk((3, 16), BF, 4)[:, :8])

    # ---- the operands of a module's GEMM
    for K in (128, 200):
        add(f"gemm_operands/K={K}", made(lambda K=K: (lambda m, c: (dict(local=m, codes=c), lambda: QL.gemm_operands(m, c)))(qlin(K), mk((4, K), I8, 9).as_subclass(FakeCuda))))
        add(f"gemm_operands/K={K},a CPU stand-in passes through", made(lambda K=K: (lambda m, c: (dict(local=m, codes=c), lambda: QL.gemm_operands(m, c)))(qlin(K), mk((4, K), I8, 9))))
        add(f"gemm_operands/K={K},twice (the padded weight is cached)", made(lambda K=K: (lambda m, c: (dict(local=m, codes=c), lambda: QL.gemm_operands(m, c) + QL.gemm_operands(m, c)))(
            qlin(K), mk((4, K), I8, 9).as_subclass(FakeCuda))))
        for kind in ("GroupedQLinear", "GroupedQLinearW4"):
            add(f"{kind}.codes_for_gemm/K={K}", made(lambda K=K, kind=kind: (lambda m, c: (dict(m=m, codes=c), lambda: m.codes_for_gemm(c)))(MODULES[kind](K=K), mk((4, K), I8, 9))))
            add(f"{kind}.codes_for_gemm/K={K},a column slice", made(lambda K=K, kind=kind: (lambda m, c: (dict(m=m, codes=c), lambda: m.codes_for_gemm(c)))(MODULES[kind](K=K), mk((4, 3 * K), I8, 9)[:, K:2 * K])))

    # ---- forward
    for kind in ("qlinear", "FusedQLinear", "QLinearW4"):
        for K in (128, 200):
            a = lambda tag, x, wsq=0, **attrs: add(f"{kind}.forward/K={K},{tag}", forward(kind, K, x, **attrs), wsq)          # noqa: E731
            a("float", lambda K: dict(x=mk((4, K), BF, 9)))
            a("float,ws=4096", lambda K: dict(x=mk((4, K), BF, 9)), 4096)
            a("float f16,3d", lambda K: dict(x=mk((2, 3, K), HF, 9)))
            a("float,a column slice", lambda K: dict(x=mk((4, 3 * K), BF, 9)[:, K:2 * K]))
            a("float,last stride (copied)", lambda K: dict(x=mk((K, 4), BF, 9).t()))
            a("float,M=0", lambda K: dict(x=mk((0, K), BF, 9)))
            a("float f64", lambda K: dict(x=mk((4, K), F64, 9)))
            a("QTensor", lambda K: dict(x=_qt((4, K))))
            a("QTensor,ws=4096", lambda K: dict(x=_qt((4, K))), 4096)
            a("QTensor,3d", lambda K: dict(x=_qt((2, 3, K))))
            a("QTensor per channel", lambda K: dict(x=_qt((4, K), axis=0)))
            a("float,wrong last dim", lambda K: dict(x=mk((4, K + 1), BF, 9)))
            a("QTensor,wrong last dim", lambda K: dict(x=_qt((4, K + 1))))
            if kind == "QLinearW4":
                a("float,stream_rows=0", lambda K: dict(x=mk((4, K), BF, 9)), 4096, stream_rows=0)
                a("QTensor,stream_rows=3", lambda K: dict(x=_qt((4, K))), stream_rows=3)
                a("QTensor,stream_rows=4", lambda K: dict(x=_qt((4, K))), stream_rows=4)
    for kind in ("GroupedQLinear", "GroupedQLinearW4"):
        for K in (128, 200):
            a = lambda tag, x, wsq=0, **attrs: add(f"{kind}.forward/K={K},{tag}", forward(kind, K, x, **attrs), wsq)          # noqa: E731
            a("float", lambda K: dict(xq=mk((4, K), BF, 9), offsets=_offsets(3)))
            a("QTensor", lambda K: dict(xq=_qt((4, K)), offsets=_offsets(3)))
            a("QTensor,3d", lambda K: dict(xq=_qt((2, 3, K)), offsets=_offsets(3)))
            a("QTensor per channel", lambda K: dict(xq=_qt((4, K), axis=0), offsets=_offsets(3)))
            a("QTensor,wrong last dim", lambda K: dict(xq=_qt((4, K + 1)), offsets=_offsets(3)))
            a("QTensor,M=0", lambda K: dict(xq=_qt((0, K)), offsets=_offsets(3)))
            a("row_index,xs defaulted", lambda K: dict(xq=_qt((3, K)), offsets=_offsets(3), row_index=mk((4,), I32, 6) % 3))
            a("row_index,xs given", lambda K: dict(xq=_qt((3, K)), offsets=_offsets(3), row_index=mk((4,), I32, 6) % 3, xs=mk((4,), F32, 1)))
            a("xs given", lambda K: dict(xq=_qt((4, K)), offsets=_offsets(3), row_index=None, xs=mk((4,), F32, 1)))
            for rows in (3, 4, 0):
                a(f"stream_rows={rows},M=4", lambda K: dict(xq=_qt((4, K)), offsets=_offsets(3)), 4096, stream_rows=rows)
                a(f"stream_rows={rows},M=4 through a row_index over 3", lambda K: dict(xq=_qt((3, K)), offsets=_offsets(3), row_index=mk((4,), I32, 6) % 3), stream_rows=rows)
            a("65 rows", lambda K: dict(xq=_qt((65, K)), offsets=_offsets(3)), 4096)

    # ---- constructors
    def ctor(cid, f):
        add(cid, made(f))

    for kw in (dict(in_features=128, out_features=8), dict(in_features=200, out_features=6, bias=False), dict(in_features=128, out_features=8, dtype=HF), dict(in_features=0, out_features=0)):
        ctor(f"qlinear.__init__/{kw!r}", lambda kw=kw: ({}, lambda: QL.qlinear(**kw)))
        ctor(f"QLinearW4.__init__/{kw!r}", lambda kw=kw: ({}, lambda: W4.QLinearW4(**kw)))
    for kw in (dict(num_experts=3, in_features=128, out_features=8), dict(num_experts=2, in_features=200, out_features=6, bias=True), dict(num_experts=1, in_features=128, out_features=8, bias=True, dtype=HF)):
        ctor(f"GroupedQLinear.__init__/{kw!r}", lambda kw=kw: ({}, lambda: MOE.GroupedQLinear(**kw)))
        ctor(f"GroupedQLinearW4.__init__/{kw!r}", lambda kw=kw: ({}, lambda: W4.GroupedQLinearW4(**kw)))
    for cls in ("qlinear", "QLinearW4"):
        C = lambda cls=cls: getattr(W4 if cls == "QLinearW4" else QL, cls)          # noqa: E731
        for tag, mkl in (("bias", lambda: linear()), ("no bias,K=200", lambda: linear(200, 6, False)), ("f16", lambda: linear().to(HF))):
            ctor(f"{cls}.from_linear/{tag}", lambda C=C, mkl=mkl: (lambda lin: (dict(lin=lin), lambda: C().from_linear(lin)))(mkl()))
    ctor("qlinear.from_kn_weight/bias", lambda: (lambda w, b: (dict(weight_kn=w, bias=b), lambda: QL.qlinear.from_kn_weight(w, b)))(mk((128, 8), BF, 5), mk((8,), BF, 6)))
    ctor("qlinear.from_kn_weight/no bias", lambda: (lambda w: (dict(weight_kn=w), lambda: QL.qlinear.from_kn_weight(w)))(mk((200, 6), HF, 5)))
    ctor("qlinear.from_kn_weight/3d", lambda: (lambda w: (dict(weight_kn=w), lambda: QL.qlinear.from_kn_weight(w)))(mk((1, 128, 8), BF, 5)))
    ctor("qlinear.from_qtensor/bias", lambda: (lambda q, b: (dict(qw=q, bias=b), lambda: QL.qlinear.from_qtensor(q, b)))(_qt((8, 128)), mk((8,), BF, 4)))
    ctor("qlinear.from_qtensor/no bias", lambda: (lambda q: (dict(qw=q), lambda: QL.qlinear.from_qtensor(q)))(_qt((8, 128))))
    ctor("qlinear.from_qtensor/per input channel", lambda: (lambda q: (dict(qw=q), lambda: QL.qlinear.from_qtensor(q)))(_qt((8, 128), axis=0)))
    ctor("qlinear.from_qtensor/3d", lambda: (lambda q: (dict(qw=q), lambda: QL.qlinear.from_qtensor(q)))(_qt((1, 8, 128))))
    for tag, parts in (("bias", lambda: [qlin(seed=0), qlin(N=4, seed=5)]), ("no bias", lambda: [qlin(200, 6, None), qlin(200, 2, None, 5)]), ("one with a bias", lambda: [qlin(), qlin(bias=None)]),
                       ("in_features differ", lambda: [qlin(), qlin(200)]), ("none", lambda: [])):
        ctor(f"FusedQLinear.__init__/{tag}", lambda parts=parts: (lambda ps: ({f"p{i}": p for i, p in enumerate(ps)}, lambda: QL.FusedQLinear(ps)))(parts()))
    ctor("FusedQLinear.from_linears/bias", lambda: (lambda a, b: (dict(a=a, b=b), lambda: QL.FusedQLinear.from_linears(a, b)))(linear(seed=1), linear(128, 4, seed=2)))
    for cls in ("GroupedQLinear", "GroupedQLinearW4"):
        C = lambda cls=cls: getattr(W4 if cls == "GroupedQLinearW4" else MOE, cls)          # noqa: E731
        for tag, parts in (("qlinears", lambda: [qlin(seed=0), qlin(seed=5)]), ("qlinears,no bias,K=200,N=6", lambda: [qlin(200, 6, None, 0), qlin(200, 6, None, 5)]),
                           ("nn.Linear", lambda: [linear(seed=1), linear(seed=2)]), ("shapes differ", lambda: [qlin(), qlin(N=4)]), ("none", lambda: [])):
            ctor(f"{cls}.from_linears/{tag}", lambda parts=parts, C=C: (lambda ps: ({f"p{i}": p for i, p in enumerate(ps)}, lambda: C().from_linears(ps)))(parts()))
        ctor(f"{cls}.from_weight/bias", lambda C=C: (lambda w, b: (dict(weight=w, bias=b), lambda: C().from_weight(w, b)))(mk((3, 8, 128), BF, 1), mk((3, 8), BF, 2)))
        ctor(f"{cls}.from_weight/no bias,K=200,N=6", lambda C=C: (lambda w: (dict(weight=w), lambda: C().from_weight(w)))(mk((2, 6, 200), HF, 1)))
        ctor(f"{cls}.from_weight/2d", lambda C=C: (lambda w: (dict(weight=w), lambda: C().from_weight(w)))(mk((8, 128), BF, 1)))
    for tag, src in (("bias", lambda: qlin()), ("no bias,K=200,N=6", lambda: qlin(200, 6, None)), ("a QLinearW4", lambda: qlin_w4()), ("an nn.Linear", lambda: linear()), ("a FusedQLinear", lambda: fusedq())):
        ctor(f"QLinearW4.from_qlinear/{tag}", lambda src=src: (lambda m: (dict(m=m), lambda: W4.QLinearW4.from_qlinear(m)))(src()))
    for tag, src in (("bias", lambda: groupedq()), ("no bias,K=200,N=6", lambda: groupedq(2, 200, 6, False)), ("E=1,N=1", lambda: groupedq(1, 128, 1)), ("a qlinear", lambda: qlin())):
        ctor(f"GroupedQLinearW4.from_grouped/{tag}", lambda src=src: (lambda m: (dict(m=m), lambda: W4.GroupedQLinearW4.from_grouped(m)))(src()))

    # ---- the walkers
    add("swap_linears/all", walk("swap_linears"))
    add("swap_linears/predicate", walk("swap_linears", predicate=skip_pred))
    add("swap_linears/fuse_gated_mlp", walk("swap_linears", predicate=skip_pred, fuse_gated_mlp=True))
    add("swap_linears_w4/all", walk("swap_linears_w4"))
    add("swap_linears_w4/predicate", walk("swap_linears_w4", predicate=skip_pred))
    add("swap_moe_experts_w4/all", walk("swap_moe_experts_w4", moe=True))
    add("swap_moe_experts_w4/predicate", walk("swap_moe_experts_w4", moe=True, predicate=skip_pred))
    add("swap_moe_experts_w4/no MoE", walk("swap_moe_experts_w4"))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------------- the recorder
def _named(value, prefix):
    """(name, tensor) for every tensor in an argument or a result"""
    if isinstance(value, Q.QTensor):
        yield prefix + ".q", value.int_data
        yield prefix + ".s", value.scale
    elif isinstance(value, torch.Tensor):
        yield prefix, value
    elif isinstance(value, nn.Module):
        for n, t in list(value.named_parameters()) + list(value.named_buffers()):
            yield f"{prefix}.{n}", t
    elif isinstance(value, (tuple, list)):
        for i, v in enumerate(value):
            yield from _named(v, f"{prefix}{i}")


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b""


def _copy_or_cast_of(p, named):
    """the input whose dense copy, or whose cast to another float type, lies at p (read while it is alive: 8 bytes first, the rest once they agree)"""
    for n, t in named:
        if t.device.type != "cpu" or t.numel() * t.element_size() < 8:
            continue
        forms = [(f"copy({n})", t)] if not t.is_contiguous() else []
        if t.is_floating_point() and t.numel() <= 64:
            forms += [(f"cast({n},{str(dt)[6:]})", t.to(dt)) for dt in (BF, HF, F32) if dt != t.dtype]
        for name, form in forms:
            want = _bytes(form)
            if ctypes.string_at(p, 8) == want[:8] and ctypes.string_at(p, len(want)) == want:
                return name
    vecs = [(n, t) for n, t in named if t.dim() == 1 and t.dtype == F32 and t.numel()]
    for ni, idx in named:
        if idx.dim() == 1 and idx.dtype == I32 and idx.numel():
            for n, t in vecs:
                if int(idx.min()) >= 0 and int(idx.max()) < t.numel() and ctypes.string_at(p, 4 * idx.numel()) == _bytes(t.index_select(0, idx)):
                    return f"gather({n},{ni})"
    return None


class _Recorder:
    def __init__(self, real, wsq):
        self.real, self.wsq, self.log, self.inputs, self.modules, self.fresh = real, wsq, [], [], [], []

    def live(self):
        """the named inputs and, of the modules among them, the lazily padded weight"""
        pads = [(f"{n}._wq_pad", m.__dict__["_wq_pad"][1]) for n, m in self.modules if m.__dict__.get("_wq_pad") is not None]
        return self.inputs + pads

    def workspace(self, p):
        for buf, _ in QL._WORKSPACES.values():
            if buf.data_ptr() <= p < buf.data_ptr() + max(buf.numel(), 1):
                return f"workspace+{p - buf.data_ptr()}"
        return None

    def fresh_name(self, p):
        for t in self.fresh:
            if t.numel() and t.data_ptr() <= p < t.data_ptr() + _extent(t):
                return f"new{list(t.shape)}{str(t.dtype)[6:]}" + (f"+{p - t.data_ptr()}" if p != t.data_ptr() else "")
        return None

    def __getattr__(self, sym):
        argtypes = getattr(self.real, sym).argtypes

        def call(*args):
            assert len(args) == len(argtypes), (sym, len(args), len(argtypes))
            rec = []
            for i, (a, ty) in enumerate(zip(args, argtypes)):
                if ty is not ctypes.c_void_p or a is None:
                    assert a is None or type(a) in (int, float), (sym, i, type(a))
                    rec.append(a)
                elif i == len(args) - 1:
                    assert a == 0, "the stream of the patched stream_ptr"
                    rec.append("stream")
                elif a == 0:
                    rec.append("empty")          # the pointer of a tensor without storage
                else:
                    live = self.live()
                    rec.append(_resolve(a, live) or self.workspace(a) or _copy_or_cast_of(a, live) or a)
            self.log.append([sym, rec])
            return self.wsq if "workspace_bytes" in sym else 0
        return call


def _describe(v):
    if isinstance(v, Plain):
        return v.value
    if isinstance(v, Q.QTensor):
        return {"QTensor": [_describe(v.int_data), _describe(v.scale), v.axis, str(v.orig_dtype)[6:], list(v.shape)]}
    if isinstance(v, torch.Tensor):
        d = [list(v.shape), str(v.dtype)[6:]] if v.is_contiguous() else [list(v.shape), list(v.stride()), str(v.dtype)[6:]]
        if v.dtype == F32 and v.device.type == "cpu" and 0 < v.numel() <= 8 and bool((v != 0).any()):
            d.append(v.tolist())          # written on the host (torch.empty gives zeros here)
        return d
    if isinstance(v, nn.Module):
        attrs = {a: getattr(v, a) for a in ("in_features", "out_features", "num_experts", "stream_rows", "splits", "code_fed") if hasattr(v, a)}
        return {"module": type(v).__name__, "attrs": attrs, "buffers": {n: _describe(b) for n, b in v.named_buffers()}, "parameters": [n for n, _ in v.named_parameters()],
                "bias is None": v.bias is None, "state_dict": list(v.state_dict()), "extra_repr": v.extra_repr(), "children": [n for n, _ in v.named_children()]}
    if isinstance(v, tuple):
        return {"tuple": [_describe(e) for e in v]}
    assert v is None or type(v) in (int, float, str, bool), type(v)
    return v


def trace(build, wsq, mp):
    """one case under the patches -> its JSON-able trace"""
    rec = _Recorder(_lib.lib(), wsq)
    real_empty, real_strided, real_check = torch.empty, torch.empty_strided, _lib.check

    def fresh(t):
        rec.fresh.append(t)
        return t.zero_()
    mp.setattr(_lib, "lib", lambda: rec)
    mp.setattr(_lib, "require_gpu", lambda t, name: rec.log.append(name))
    mp.setattr(_lib, "check", lambda status, what: (rec.log.append("check " + what), real_check(status, what))[1])
    mp.setattr(_lib, "stream_ptr", lambda t: 0)
    mp.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    mp.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    mp.setattr(torch, "empty", lambda *a, **k: fresh(real_empty(*a, **k)))
    mp.setattr(torch, "empty_strided", lambda *a, **k: fresh(real_strided(*a, **k)))
    out = {}
    try:
        inputs, run = build()
        rec.inputs = [nt for n, v in inputs.items() for nt in _named(v, n)]
        rec.modules = [(n, v) for n, v in inputs.items() if isinstance(v, nn.Module)]
        del rec.log[:], rec.fresh[:]
        QL.clear_workspaces()
        try:
            ret = run()
        except Exception as e:          # noqa: BLE001  (whatever it raises is the behaviour recorded)
            ret = None
            out["raises"] = [type(e).__name__, str(e)]
        sizes = [buf.numel() for buf, _ in QL._WORKSPACES.values()]
    finally:
        mp.undo()
        QL.clear_workspaces()
    results = list(_named(ret, "r"))
    for entry in rec.log:
        if isinstance(entry, list):
            for i, a in enumerate(entry[1]):
                if type(a) is int and getattr(rec.real, entry[0]).argtypes[i] is ctypes.c_void_p:
                    entry[1][i] = _resolve(a, results) or rec.fresh_name(a) or "made by a torch op"
    out["log"] = rec.log if any(isinstance(e, list) for e in rec.log) else rec.log + ["no call"]
    if sizes:
        out["workspaces"] = sizes
    if "raises" not in out:
        out["ret"] = _describe(ret)
        same = [f"{rn} is {n}" for rn, r in results for n, t in rec.inputs if r is t]
        if same:
            out["same"] = same
    return json.loads(json.dumps(out))


def record():
    with pytest.MonkeyPatch.context() as mp:
        return {cid: trace(build, wsq, mp) for cid, (build, wsq) in cases().items()}


CASES = cases()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return {f"{fn}/{tag}": t for fn, by_tag in json.load(f).items() for tag, t in by_tag.items()}


@pytest.mark.parametrize("cid", list(CASES))
def test_call_is_the_recorded_one(cid, golden, monkeypatch):
    build, wsq = CASES[cid]
    assert trace(build, wsq, monkeypatch) == golden[cid]


def test_golden_file_holds_these_cases_and_no_others(golden):
    assert sorted(golden) == sorted(CASES)
    called = {e[0] for t in golden.values() for e in t["log"] if isinstance(e, list)}
    assert called <= set(_lib.EXPORTS)
    for fn in ("int_mm", "qlinear_s8", "qlinear_s8_t", "qlinear_s8_kslabs", "qlinear_dyn", "qlinear_s8_grouped", "int_mm_grouped", "qlinear_s8_grouped_stream", "int_mm_grouped_stream",
               "w4_pack", "w4_expand", "int_mm_w4", "qlinear_w4", "int_mm_w4_grouped", "qlinear_w4_grouped"):
        assert any(isinstance(e, list) and e[0].startswith("pq_") for c, t in golden.items() if c.startswith(fn + "/") for e in t["log"]), f"{fn} reaches the library"


NO_CPU = {
    "int_mm": imm(), "qlinear_s8": dense(), "qlinear_s8_t": dense(), "qlinear_s8_kslabs": kslabs(), "qlinear_dyn": dyn(), "qlinear_s8_grouped": grouped(),
    "qlinear_s8_grouped_stream": grouped(), "int_mm_grouped": grouped(epi=False), "int_mm_grouped_stream": grouped(epi=False), "w4_pack": lambda: dict(wq=mk((8, 128), I8, 2)),
    "w4_expand": lambda: dict(zip(("w4", "gs"), packed())), "int_mm_w4": w4dense(epi=False), "qlinear_w4": w4dense(), "int_mm_w4_grouped": w4grouped(epi=False),
    "qlinear_w4_grouped": w4grouped(),
}


@pytest.mark.parametrize("fname", list(NO_CPU))
def test_no_cpu_path(fname):
    """with the real require_gpu an operand on the CPU is refused, before the library is looked at"""
    with pytest.raises(_lib.PQError) as e:
        _fn(fname)(**NO_CPU[fname]())
    assert " is on cpu" in str(e.value) and fname.replace("qlinear_dyn", "qlinear") in str(e.value)


@pytest.mark.parametrize("kind", list(MODULES))
def test_no_cpu_path_of_the_modules(kind):
    m = MODULES[kind]()
    args = (_qt((4, 128)), _offsets(3)) if kind.startswith("Grouped") else (mk((4, 128), BF, 9),)
    with pytest.raises(_lib.PQError) as e:
        m(*args)
    assert " is on cpu" in str(e.value)


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python -m tests.test_gemm_calls_host --record"
    with open(GOLDEN, "w") as f:
        by_fn = {}
        for c, t in record().items():
            by_fn.setdefault(c.partition("/")[0], []).append(f" {json.dumps(c.partition('/')[2])}:{json.dumps(t, separators=(',', ':'))}")
        f.write("{\n" + ",\n".join(f"{json.dumps(fn)}:{{\n" + ",\n".join(lines) + "}" for fn, lines in by_fn.items()) + "\n}\n")
