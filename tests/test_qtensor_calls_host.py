"""CPU: the contract between protoquant_amd/qtensor.py and libpq_hip.so, pinned call by call.  Every public callable of qtensor.py is driven on CPU tensors with the
library replaced by a recording fake, and what it does is compared with tests/golden/qtensor_calls.json: the symbol it calls, every argument (a pointer as the operand
it points into, with the byte offset where there is one; every number verbatim), the `what` it hands to _lib.check and the operands it hands to require_gpu, in order
(the function's own name left out of both), what it returns (structure, shapes, dtypes, the strides of what is not contiguous, the contents the host itself wrote)
and which returned tensors ARE inputs; for a refused call the exception's type and message (without the function's name in front).  The patches: _lib.lib -> the
fake, _lib.require_gpu / _lib.check -> recorders, _lib.stream_ptr -> 0, torch.cuda.device -> a null context, and torch.empty / empty_strided -> zeros, so that fresh
memory never looks like a copy of an input and a scale the wrapper filled with ones (an entry that returns before launching) is told from one it left to the kernel.

    python -m tests.test_qtensor_calls_host --record        rewrites the golden file from the code as it stands

A trace that changes is a change of behaviour: understand it before recording it."""
import contextlib
import ctypes
import inspect
import json
import os
import sys

import pytest
import torch

from protoquant_amd import _lib
from protoquant_amd import qtensor as Q

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qtensor_calls.json")
BF, HF, F32, F64, I8, I32 = torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.int8, torch.int32
ROW_NAMES = ("g", "u", "x", "residual", "a", "b", "c")
VEC_NAMES = ("weight", "bias", "post_weight", "weight2", "bias2")


def mk(shape, dtype, seed=0, device="cpu"):
    """small whole numbers 1 .. 13, element 0 == seed % 13 + 1: operands made with different seeds differ in their first bytes (how a copy is told from another)"""
    n = 1
    for d in shape:
        n *= d
    return ((torch.arange(n, device=device) + seed) % 13 + 1).reshape(shape).to(dtype)


def _dense(shape, dtype):
    return lambda: (lambda k: mk(shape, dtype, k))


def _memo(f):
    seen = {}
    return lambda k: seen[k] if k in seen else seen.setdefault(k, f(k))


def _halves():
    wide = mk((4, 256), BF, 0)
    return lambda k: (wide[:, :128], wide[:, 128:])[k] if k < 2 else mk((4, 128), BF, k)


# the k-th row operand of a call, per layout (a fresh factory per case; within a case operand k is one tensor)
LAYOUTS = {
    "2d": _dense((4, 64), BF), "3d": _dense((2, 3, 64), HF), "row": _dense((1, 64), F32), "rows0": _dense((0, 64), BF), "cols0": _dense((4, 0), BF),
    "slice": lambda: (lambda k: mk((4, 256), BF, k)[:, 64:128]),          # every row operand a column block of a wider buffer of its own
    "halves": _halves,                                                     # g, u: the halves of ONE 4 x 256 buffer
    "tstride": lambda: (lambda k: mk((64, 4), BF, k).t() if k == 0 else mk((4, 64), BF, k)),     # operand 0 has last stride 4: it must be copied
    "0d": _dense((), BF), "f64": _dense((4, 64), F64),
}
BASE = ("2d", "3d", "row", "rows0", "cols0")


def _lead(t):
    n = 1
    for d in t.shape[:-1]:
        n *= d
    return n


def _qt(X):
    x = X(0)
    return Q.QTensor(mk(tuple(x.shape), I8, 3), mk((_lead(x),), F32, 4), 1, x.dtype, x.shape)


# fname -> the keyword arguments of a plain call; X(k): row operand k, W(k): a [cols] vector of X(0)'s dtype
CALLS = {
    "quantize": lambda X, W: dict(x=X(0)),
    "dequantize": lambda X, W: dict(q=_qt(X)),
    "silu_mul_quantize": lambda X, W: dict(g=X(0), u=X(1)),
    "glu_quantize": lambda X, W: dict(g=X(0), u=X(1), kind="clamped_silu", limit=7.0),
    "gelu_mul_quantize": lambda X, W: dict(g=X(0), u=X(1)),
    "silu_mul_rowamax": lambda X, W: dict(g=X(0), u=X(1)),
    "silu_mul_quantize_with_amax": lambda X, W: dict(g=X(0), u=X(1), amax_bits=mk((_lead(X(0)),), I32, 5)),
    "rowamax": lambda X, W: dict(x=X(0)),
    "quantize_with_amax": lambda X, W: dict(x=X(0), amax_bits=mk((_lead(X(0)),), I32, 5)),
    "rmsnorm_quantize": lambda X, W: dict(x=X(0), weight=W(0), eps=1e-5),
    "add_rmsnorm_quantize": lambda X, W: dict(x=X(0), residual=X(1), weight=W(0), eps=1e-5),
    "scaled_add_rmsnorm_quantize": lambda X, W: dict(x=X(0), residual=X(1), multiplier=0.22, weight=W(0)),
    "scaled_add": lambda X, W: dict(x=X(0), residual=X(1), multiplier=3),
    "layernorm_quantize": lambda X, W: dict(x=X(0), weight=W(0), bias=W(1)),
    "add_layernorm_quantize": lambda X, W: dict(x=X(0), residual=X(1), weight=W(0), bias=W(1), eps=1e-6),
    "add2_layernorm_quantize": lambda X, W: dict(a=X(0), b=X(1), c=X(2), weight=W(0), bias=W(1), eps=1e-5, weight2=W(2), bias2=W(3), eps2=1e-6),
    "layernorm_quantize2": lambda X, W: dict(x=X(0), weight=W(0), bias=W(1), weight2=W(2), bias2=None),
    "act_quantize": lambda X, W: dict(x=X(0), kind="gelu_tanh"),
    "gemma_rmsnorm_quantize": lambda X, W: dict(x=X(0), weight=W(0)),
    "add_gemma_rmsnorm_quantize": lambda X, W: dict(x=X(0), residual=X(1), weight=W(0)),
    "gemma_postnorm_add_rmsnorm_quantize": lambda X, W: dict(x=X(0), post_weight=W(0), residual=X(1), weight=W(1), eps=1e-6, post_eps=1e-5),
    "gemma_postnorm_add": lambda X, W: dict(x=X(0), post_weight=W(0), residual=X(1), post_eps=1e-5),
    "olmo_postnorm_add_quantize": lambda X, W: dict(x=X(0), post_weight=W(0), residual=X(1), post_eps=1e-5),
    "olmo_postnorm_add": lambda X, W: dict(x=X(0), post_weight=W(0), residual=X(1)),
    "olmo_rmsnorm": lambda X, W: dict(x=X(0), weight=W(0)),
    "head_rmsnorm": lambda X, W: dict(x=X(0), weight=W(0)),
}
NO_TENSOR = ("glu_params", "QTensor")          # traced by cases of their own below
AMAX = ("silu_mul_quantize_with_amax", "quantize_with_amax")


def _kwargs(fname, layout):
    X = _memo(LAYOUTS[layout]())
    x = X(0)
    cols = x.shape[-1] if x.dim() else 1
    return CALLS[fname](X, _memo(lambda k: mk((cols,), x.dtype, 6 + k)))


def _params(fname):
    return inspect.signature(getattr(Q, fname)).parameters


def cases():
    """id -> (fname, keyword arguments), in a fixed order"""
    out = {}

    def add(cid, fname, kw):
        assert cid not in out, cid
        out[cid] = (fname, kw)

    def vary(fname, tag, layout="2d", **change):
        kw = _kwargs(fname, layout)
        kw.update({k: (v(kw) if callable(v) else v) for k, v in change.items()})
        add(f"{fname}/{tag}", fname, kw)

    for fname in CALLS:
        P = _params(fname)
        rows_of = [n for n in P if n in ROW_NAMES]
        vecs_of = [n for n in P if n in VEC_NAMES]
        # 1, 3: the five plain shapes, return_h both ways
        for layout in BASE:
            for rh in (((False, True) if layout in ("2d", "cols0") else (False,)) if "return_h" in P else (None,)):
                vary(fname, layout + ("" if rh is None else f",h={int(rh)}"), layout, **({} if rh is None else {"return_h": rh}))
        # 2: views stay views, a last stride that is not 1 is copied
        vary(fname, "halves" if rows_of[:2] == ["g", "u"] else "slice", "halves" if rows_of[:2] == ["g", "u"] else "slice")
        vary(fname, "tstride", "tstride")
        # 6: a 0-d input, an unsupported dtype
        vary(fname, "0d", "0d")
        vary(fname, "f64", "f64")
        if fname == "dequantize":
            continue
        # 6: row operands that disagree in shape, dtype, device (a meta tensor stands for another device)
        for n in rows_of[1:]:
            vary(fname, f"{n}:shape", **{n: mk((4, 32), BF, 1)})
            vary(fname, f"{n}:device", **{n: mk((4, 64), BF, 1, "meta")})
        # 5, 6: the norm parameters
        for n in vecs_of:
            vary(fname, f"{n}:length", **{n: mk((65,), BF, 9)})
            vary(fname, f"{n}:dtype", **{n: mk((64,), F32, 9)})
        if vecs_of:
            vary(fname, "strided params", **{n: (lambda kw, n=n, i=i: None if kw[n] is None else mk((128,), BF, 9 + i)[::2]) for i, n in enumerate(vecs_of)})
        if "bias" in P:
            vary(fname, "bias=None", bias=None)
            vary(fname, "weight=None", weight=None)
        # 4: out
        if "out" in P and fname not in AMAX:
            for n in rows_of:
                vary(fname, f"out={n}", out=lambda kw, n=n: kw[n])
            vary(fname, "out=fresh", out=mk((4, 64), BF, 12))
            vary(fname, "out=slice", out=mk((4, 256), BF, 12)[:, 128:192])
            vary(fname, "out=tstride", out=mk((64, 4), BF, 12).t())
            if fname in ("add_rmsnorm_quantize", "add2_layernorm_quantize", "olmo_rmsnorm"):          # .view() itself refuses: one shared function, before and after
                vary(fname, "out=no view,3d", "3d", out=mk((3, 2, 64), HF, 12).transpose(0, 1))
            vary(fname, "out:shape", out=mk((4, 32), BF, 12))
            if "return_h" not in P:
                vary(fname, f"out={rows_of[-1]},cols0", "cols0", out=lambda kw: kw[rows_of[-1]])
            else:
                vary(fname, f"out={rows_of[0]},cols0,h=1", "cols0", out=lambda kw: kw[rows_of[0]], return_h=True)
        if "multiplier" in P:
            for tag, m in (("bool", True), ("tensor", torch.tensor(0.5)), ("nan", float("nan")), ("inf", float("inf")), ("int", 2)):
                vary(fname, f"multiplier:{tag}", multiplier=m)
            vary(fname, "multiplier:bool before operands", multiplier=False, residual=mk((4, 32), BF, 1))
        if fname in AMAX:
            vary(fname, "amax:dtype", amax_bits=mk((4,), F32, 5))
            vary(fname, "amax:shape", amax_bits=mk((5,), I32, 5))
            vary(fname, "amax:strided", amax_bits=mk((8,), I32, 5)[::2])
            vary(fname, "out=fresh", out=mk((4, 64), I8, 12))
            vary(fname, "out=slice", out=mk((4, 256), I8, 12)[:, 64:128])
            vary(fname, "out=wide,row", "row", out=mk((1, 256), I8, 12)[:, :64])
            vary(fname, "out=fresh,cols0", "cols0", out=mk((4, 0), I8, 12))
            vary(fname, "out:dtype", out=mk((4, 64), BF, 12))
            vary(fname, "out:shape", out=mk((64, 4), I8, 12))
            vary(fname, "out:tstride", out=mk((64, 4), I8, 12).t())
    # 6: the kinds
    for k in ("relu", "gelu_tanh", "gelu_erf", "gelu", None):
        vary("act_quantize", f"kind={k}", kind=k)
    vary("glu_quantize", "kind=alpha_sigmoid", kind="alpha_sigmoid", alpha=1.702, return_h=True)
    vary("glu_quantize", "kind=alpha_sigmoid without alpha", kind="alpha_sigmoid")
    vary("glu_quantize", "kind=silu", kind="silu")
    vary("glu_quantize", "limit=0", limit=0.0)
    vary("glu_quantize", "limit=int", limit=7)
    vary("gelu_mul_quantize", "kind=gelu_erf", kind="gelu_erf")
    vary("gelu_mul_quantize", "kind=gelu_tanh", kind="gelu_tanh", return_h=True)
    for args in (("clamped_silu", 7.0), ("clamped_silu", 7, 0.5), ("alpha_sigmoid", 7.0, 1.702), ("alpha_sigmoid", 7.0), ("swish", 7.0), ("clamped_silu", None), ("clamped_silu", 0.0),
                 ("clamped_silu", -1.0), ("clamped_silu", float("inf")), ("clamped_silu", float("nan")), ("clamped_silu", 7.0, float("inf")), ("clamped_silu", 7.0, float("-inf")),
                 ("alpha_sigmoid", 7.0, float("nan")), ("alpha_sigmoid", "7", "2")):
        add(f"glu_params/{args!r}", "glu_params", dict(zip(("kind", "limit", "alpha"), args)))
    # 5: the second norm of add2_layernorm_quantize, the eps2 default of both dual forms
    vary("add2_layernorm_quantize", "one norm", weight2=None, bias2=None, eps2=None)
    vary("add2_layernorm_quantize", "one norm,h=1", weight2=None, bias2=None, eps2=None, return_h=True)
    vary("add2_layernorm_quantize", "one norm,cols0,h=1", "cols0", weight2=None, bias2=None, eps2=None, return_h=True)
    vary("add2_layernorm_quantize", "eps2 defaulted", eps2=None)
    vary("add2_layernorm_quantize", "eps2 defaulted,cols0", "cols0", eps2=None)
    vary("add2_layernorm_quantize", "bias2=None", bias2=None)
    vary("add2_layernorm_quantize", "bias2 without weight2", weight2=None, eps2=None)
    vary("add2_layernorm_quantize", "eps2 without weight2", weight2=None, bias2=None)
    vary("add2_layernorm_quantize", "weight2=None,bias=None", weight2=None, bias2=None, eps2=None, bias=None)
    vary("layernorm_quantize2", "eps2 given", eps2=1e-6, bias2=lambda kw: mk((64,), BF, 11), return_h=True)
    vary("layernorm_quantize2", "eps2 given,rows0", "rows0", eps2=1e-6)
    vary("layernorm_quantize2", "weight2=None", weight2=None)
    # 7: head_rmsnorm
    fused = mk((2, 5, 3 * 4 * 16), BF, 0)          # [B, T, q | k | v] with 4 heads of 16
    qv = fused[..., 64:128].view(2, 5, 4, 16)
    for kind in ("llama", "gemma"):
        w = mk((16,), BF, 7)
        add(f"head_rmsnorm/contiguous,{kind}", "head_rmsnorm", dict(x=mk((2, 5, 4, 16), BF, 1), weight=w, eps=1e-5, kind=kind))
        add(f"head_rmsnorm/qkv view,{kind}", "head_rmsnorm", dict(x=qv, weight=w, kind=kind))
        add(f"head_rmsnorm/qkv view transposed,{kind}", "head_rmsnorm", dict(x=qv.transpose(1, 2), weight=w, kind=kind))
        add(f"head_rmsnorm/expanded,{kind}", "head_rmsnorm", dict(x=mk((2, 1, 16), BF, 1).expand(2, 3, 16), weight=w, kind=kind))
        add(f"head_rmsnorm/three strides,{kind}", "head_rmsnorm", dict(x=mk((2, 3, 5, 32), BF, 1)[:, :2, :4:2, :16], weight=w, kind=kind))
        add(f"head_rmsnorm/empty,{kind}", "head_rmsnorm", dict(x=mk((2, 0, 4, 16), BF, 1), weight=w, kind=kind))
        add(f"head_rmsnorm/empty transposed,{kind}", "head_rmsnorm", dict(x=mk((2, 0, 4, 16), BF, 1).transpose(1, 2), weight=w, kind=kind))
        add(f"head_rmsnorm/1d,{kind}", "head_rmsnorm", dict(x=mk((16,), BF, 1), weight=mk((32,), BF, 7)[::2], kind=kind))
    vary("head_rmsnorm", "kind=olmo", kind="olmo")
    # 8: quantize's axes, dequantize's
    for tag, kw in (("axis=-1", dict(x=mk((4, 64), BF), axis=-1)), ("axis=1", dict(x=mk((4, 64), BF), axis=1)), ("axis=0", dict(x=mk((4, 64), BF), axis=0)),
                    ("axis=-2", dict(x=mk((4, 64), BF), axis=-2)), ("axis=0,tstride", dict(x=mk((64, 4), HF).t(), axis=0)), ("axis=0,slice", dict(x=mk((4, 256), F32)[:, 64:128], axis=0)),
                    ("axis=0,3d", dict(x=mk((2, 3, 64), BF), axis=0)), ("axis=1,3d", dict(x=mk((2, 3, 64), BF), axis=1)), ("axis=2,3d", dict(x=mk((2, 3, 64), BF), axis=2)),
                    ("axis=0,1d", dict(x=mk((64,), BF), axis=0)), ("axis=0,cols0", dict(x=mk((4, 0), BF), axis=0)), ("axis=0,rows0", dict(x=mk((0, 64), BF), axis=0))):
        add(f"quantize/{tag}", "quantize", kw)
    qd = mk((4, 64), I8, 3)
    for tag, kw in (("axis=0", dict(q=Q.QTensor(qd, mk((64,), F32, 4), 0, BF, qd.shape))), ("axis=0,dtype", dict(q=Q.QTensor(qd, mk((64,), F32, 4), 0, BF, qd.shape), dtype=F32)),
                    ("axis=1,dtype", dict(q=Q.QTensor(qd, mk((4,), F32, 4), 1, BF, qd.shape), dtype=HF)), ("axis=1,dtype f64", dict(q=Q.QTensor(qd, mk((4,), F32, 4), 1, BF, qd.shape), dtype=F64)),
                    ("axis=0,tstride", dict(q=Q.QTensor(mk((64, 4), I8, 3).t(), mk((64,), F32, 4), 0, HF, qd.shape))),
                    ("axis=1,codes a slice", dict(q=Q.QTensor(mk((4, 256), I8, 3)[:, 64:128], mk((4,), F32, 4), 1, HF, qd.shape)))):
        add(f"dequantize/{tag}", "dequantize", kw)
    add("QTensor/fields", "QTensor", dict(int_data=qd, scale=mk((4,), F32, 4), axis=1, orig_dtype=BF, shape=qd.shape))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------------- the recorder
def _extent(t):
    return 0 if t.numel() == 0 else (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()


def _named(value, prefix):
    """(name, tensor) for every tensor in an argument or a result"""
    if isinstance(value, Q.QTensor):
        yield prefix + ".q", value.int_data
        yield prefix + ".s", value.scale
    elif isinstance(value, torch.Tensor):
        yield prefix, value
    elif isinstance(value, (tuple, list)):
        for i, v in enumerate(value):
            yield from _named(v, f"{prefix}{i}")


def _resolve(p, named):
    for n, t in named:
        if t.device.type == "cpu" and t.data_ptr() == p:
            return n
    for n, t in named:
        if t.device.type == "cpu" and t.data_ptr() < p < t.data_ptr() + _extent(t):
            return f"{n}+{p - t.data_ptr()}"
    return None


def _copy_of(p, named):
    """the input whose dense copy lies at p (read while the copy is alive: 8 bytes first, which every allocation has, the rest once they agree)"""
    for n, t in named:
        if t.device.type != "cpu" or t.is_contiguous() or t.numel() * t.element_size() < 8:
            continue
        want = bytes(t.contiguous().view(torch.uint8).reshape(-1).tolist()) if t.dim() else b""
        if ctypes.string_at(p, 8) == want[:8] and ctypes.string_at(p, len(want)) == want:
            return f"copy({n})"
    return None


class _Recorder:
    def __init__(self, real):
        self.real, self.log, self.inputs = real, [], []

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
                    rec.append(_resolve(a, self.inputs) or _copy_of(a, self.inputs) or a)
            self.log.append([sym, rec])
            return 0
        return call


def _describe(v):
    if isinstance(v, Q.QTensor):
        return {"QTensor": [_describe(v.int_data), _describe(v.scale), v.axis, str(v.orig_dtype)[6:], list(v.shape)]}
    if isinstance(v, torch.Tensor):
        d = [list(v.shape), str(v.dtype)[6:]] if v.is_contiguous() else [list(v.shape), list(v.stride()), str(v.dtype)[6:]]
        if v.dtype == F32 and v.device.type == "cpu" and 0 < v.numel() <= 8 and bool((v != 0).any()):
            d.append(v.tolist())          # written on the host (torch.empty gives zeros here)
        return d
    if isinstance(v, tuple):
        return {"tuple": [_describe(e) for e in v]}
    assert v is None or type(v) in (int, float, str), type(v)
    return v


def trace(fname, kw, mp):
    """one call of qtensor.<fname>(**kw) under the patches -> its JSON-able trace"""
    rec = _Recorder(_lib.lib())
    rec.inputs = [nt for n, v in kw.items() for nt in _named(v, n)]
    real_empty, real_check = torch.empty, _lib.check
    mp.setattr(_lib, "lib", lambda: rec)
    mp.setattr(_lib, "require_gpu", lambda t, name: rec.log.append((name[len(fname):] if name.startswith(fname + "(") else name)))
    mp.setattr(_lib, "check", lambda status, what: (rec.log.append("check" if what == fname else "check " + what), real_check(status, what))[1])
    mp.setattr(_lib, "stream_ptr", lambda t: 0)
    mp.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    mp.setattr(torch, "empty", lambda *a, **k: real_empty(*a, **k).zero_())
    mp.setattr(torch, "empty_strided", lambda *a, _real=torch.empty_strided, **k: _real(*a, **k).zero_())
    out = {}
    try:
        ret = getattr(Q, fname)(**kw)
    except Exception as e:          # noqa: BLE001  (whatever it raises is the behaviour recorded)
        ret = None
        out["raises"] = [type(e).__name__, str(e)[len(fname):] if str(e).startswith(fname + ":") else str(e)]
    finally:
        mp.undo()
    results = list(_named(ret, "r"))
    for entry in rec.log:
        if isinstance(entry, list):
            for i, a in enumerate(entry[1]):
                if type(a) is int and getattr(rec.real, entry[0]).argtypes[i] is ctypes.c_void_p:
                    entry[1][i] = _resolve(a, results)
                    assert entry[1][i] is not None, f"{fname}: argument {i} of {entry[0]} points into no named operand"
    out["log"] = rec.log if any(isinstance(e, list) for e in rec.log) else rec.log + ["no call"]
    if "raises" not in out:
        out["ret"] = _describe(ret)
        same = [f"{rn} is {n}" for rn, r in results for n, t in rec.inputs if r is t]
        if same:
            out["same"] = same
    return json.loads(json.dumps(out))


def record():
    with pytest.MonkeyPatch.context() as mp:
        return {cid: trace(fname, kw, mp) for cid, (fname, kw) in cases().items()}


CASES = cases()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return {f"{fn}/{tag}": t for fn, by_tag in json.load(f).items() for tag, t in by_tag.items()}


@pytest.mark.parametrize("cid", list(CASES))
def test_call_is_the_recorded_one(cid, golden, monkeypatch):
    fname, kw = CASES[cid]
    assert trace(fname, kw, monkeypatch) == golden[cid]


def test_golden_file_holds_these_cases_and_no_others(golden):
    assert sorted(golden) == sorted(CASES)


def test_every_public_callable_is_traced(golden):
    public = {n for n, v in vars(Q).items() if not n.startswith("_") and (inspect.isfunction(v) or inspect.isclass(v)) and v.__module__ == Q.__name__}
    assert public == {fname for fname, _ in CASES.values()} == set(CALLS) | set(NO_TENSOR)
    assert len(public) == 28          # 27 functions and QTensor
    called = {e[0] for t in golden.values() for e in t["log"] if isinstance(e, list)}
    assert called <= set(_lib.EXPORTS)
    for fname in CALLS:          # every shape of the list, and every function reaches the library on a plain input
        for layout in BASE:
            assert any(c.startswith(f"{fname}/{layout}") for c in CASES), (fname, layout)
        assert any(isinstance(e, list) for c, t in golden.items() if c.startswith(f"{fname}/2d") for e in t["log"]), fname


@pytest.mark.parametrize("fname", list(CALLS))
def test_no_cpu_path(fname):
    """with the real require_gpu the first operand on the CPU is refused, before anything else is looked at"""
    kw = _kwargs(fname, "2d")
    first = next(iter(kw))
    with pytest.raises(_lib.PQError) as e:
        getattr(Q, fname)(**kw)
    assert str(e.value).startswith(f"{fname}({first}) is on cpu")


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python -m tests.test_qtensor_calls_host --record"
    with open(GOLDEN, "w") as f:
        by_fn = {}
        for c, t in record().items():
            by_fn.setdefault(c.partition("/")[0], []).append(f" {json.dumps(c.partition('/')[2])}:{json.dumps(t, separators=(',', ':'))}")
        f.write("{\n" + ",\n".join(f"{json.dumps(fn)}:{{\n" + ",\n".join(lines) + "}" for fn, lines in by_fn.items()) + "\n}\n")
