"""The table of row forms: one `Form` per C-ABI row entry and form (K1 and its amax halves, K2, dequant, K1s, K1g, K1gg, K1u, K1n, K1a, K1l, K1al, K1pl / K1l2, K1ng,
K1ang, K1pang / K1pa, K1oq / K1oa / K1on, moe_combine), with the `calls` that drive the entry on a set of operands and the CPU specification `ref` of its outputs, and the small
helpers that go with it (seeded inputs, the bit-for-bit comparison with NaNs as a class).  Shared by tests/test_gpu_row_addressing.py (which also holds the test that fails
when an exported row entry has no row here), tests/test_gpu_amax_positions.py and tests/test_gpu_tail_slots.py."""
import contextlib
import zlib
from dataclasses import dataclass, field

import numpy as np

from oracle import c_oracle as C
from oracle import qspec_numpy as Q
from tests import act_spec as U
from tests import add2lnorm_spec as A2
from tests import addlnorm_spec as AL
from tests import addnorm_spec as A
from tests import gemma_postnorm_spec as GP
from tests import gemma_spec as GS
from tests import glu_spec as G
from tests import lnorm_spec as LS
from tests import olmo_spec as O
from tests.gpu_util import TD

EPS, EPS2, POST_EPS = 1e-5, 1e-6, 1e-6
LIMIT, ALPHA = 7.0, 1.702


@contextlib.contextmanager
def eps_values(eps, eps2, post_eps):
    """the three eps that every `calls` and `ref` of the table reads, changed for the calls inside the block (eps = 0 makes an all-zero row's rs Inf)"""
    global EPS, EPS2, POST_EPS
    saved = (EPS, EPS2, POST_EPS)
    EPS, EPS2, POST_EPS = eps, eps2, post_eps
    try:
        yield
    finally:
        EPS, EPS2, POST_EPS = saved


# ---------------------------------------------------------------------------------------------------------------- the table
class Ops(dict):
    """operand name -> a 2-D view (or a vector); a name that is absent reads as None (a null argument)"""
    __getattr__ = dict.get


def P(v):
    return None if v is None else v.data_ptr()


def D(v):
    return 0 if v is None else v.stride(0)


def T(b, code):
    return O.as_tensor(b, TD[code])


@dataclass
class Form:
    name: str
    calls: tuple                      # ((exported symbol, lambda L, o, code, rows, cols, st: status), ...)
    ref: object                       # lambda inputs (name -> storage bits), code: name -> expected output
    mats: tuple = ("x",)              # matrix inputs of the storage dtype
    vecs: tuple = ()                  # [cols] inputs of the storage dtype
    outs: tuple = ()                  # matrix outputs of the storage dtype
    nq: int = 1                       # code outputs q, q2 with their scales sc, sc2
    amax: bool = False                # a uint32 [rows] amax vector `am` between the two halves
    scale_len: str = "rows"
    wide: bool = False                # the op has kWideRows
    nan: bool = True                  # the specification defines a NaN row
    alias: tuple = ()                 # (output, input) that may be one operand
    extra_widths: tuple = ()
    many: int = 0                     # part 2: 1 = bf16, 2 = bf16 and f32 (once per kernel file)
    exact_sum: object = None          # part 2: lambda o: the torch expression of `s` on the GPU, where that is exact (the adds)
    custom: bool = False              # part 1 is a test of its own below (other operand kinds)
    smalls: tuple = ()                # CPU part: further small operands
    cnames: dict = field(default_factory=dict)
    clash: dict = field(default_factory=dict)      # CPU part: symbol -> (operand moved, operand it then overlaps by one element)


def _q1(t):
    return dict(q=t[0], sc=t[1])


def _qh(t):
    return dict(q=t[0], sc=t[1], h=t[2])


def _qsh(t):
    return dict(q=t[0], sc=t[1], s=t[2], h=t[3])


def _amax_ref(x, code):
    am = Q.row_amax_bits(x, code)
    q, sc = Q.quantize_rows_with_amax(x, code, am)
    return dict(am=am, q=q, sc=sc)


def _ln_groups(i, code, n):
    return [(T(i["w" + g], code), T(i["b" + g], code), eps) for g, eps in (("1", EPS), ("2", EPS2))[:n]]


def _pl_ref(i, code, n):
    s, gr = A2.add2_layernorm_quantize(T(i["a"], code), T(i["b"], code), T(i["c"], code), _ln_groups(i, code, n))
    out = dict(s=s, q=gr[0][0], sc=gr[0][1], h=gr[0][2])
    if n == 2:
        out.update(q2=gr[1][0], sc2=gr[1][1], h2=gr[1][2])
    return out


def _l2_ref(i, code):
    gr = A2.layernorm_quantize_groups(T(i["c"], code), _ln_groups(i, code, 2))
    return dict(q=gr[0][0], sc=gr[0][1], h=gr[0][2], q2=gr[1][0], sc2=gr[1][1], h2=gr[1][2])


def _pl_call(L, o, c, R, N, st):
    return L.pq_parallel_layernorm_quant_rowwise(P(o.a), D(o.a), P(o.b), D(o.b), P(o.c), D(o.c), P(o.s), D(o.s), P(o.w1), P(o.b1), EPS, P(o.w2), P(o.b2), EPS2, c, R, N,
                                                 P(o.q), D(o.q), P(o.sc), P(o.h), D(o.h), P(o.q2), D(o.q2), P(o.sc2), P(o.h2), D(o.h2), st)


def _pang_call(L, o, c, R, N, st):
    return L.pq_gemma_postnorm_add_rmsnorm_quant_rowwise(P(o.x), D(o.x), P(o.pw), POST_EPS, P(o.r), D(o.r), P(o.s), D(o.s), P(o.w), EPS, c, R, N, P(o.q), D(o.q), P(o.sc),
                                                         P(o.h), D(o.h), st)


def _olmo_call(L, o, c, R, N, st):
    return L.pq_olmo_postnorm_add_quant_rowwise(P(o.x), D(o.x), P(o.pw), POST_EPS, P(o.r), D(o.r), P(o.s), D(o.s), c, R, N, P(o.q), D(o.q), P(o.sc), st)


def _glu(kind):
    return Form(f"K1g_{G.KIND_NAMES[kind]}", mats=("g", "u"), outs=("h",), wide=True, many=2 if kind == 0 else 1,
                calls=(("pq_glu_quant_rowwise", lambda L, o, c, R, N, st: L.pq_glu_quant_rowwise(P(o.g), D(o.g), P(o.u), D(o.u), c, R, N, kind, LIMIT, ALPHA, P(o.q), D(o.q),
                                                                                                 P(o.sc), P(o.h), D(o.h), st)),),
                ref=lambda i, c: _qh(G.glu_quantize(i["g"], i["u"], c, kind, LIMIT, ALPHA)))


def _act(kind):
    return Form(f"K1u_{U.KIND_NAMES[kind]}", outs=("h",), wide=True, many=2 if kind == 1 else 1,
                calls=(("pq_act_quant_rowwise", lambda L, o, c, R, N, st: L.pq_act_quant_rowwise(P(o.x), D(o.x), c, R, N, kind, P(o.q), D(o.q), P(o.sc), P(o.h), D(o.h), st)),),
                ref=lambda i, c: _qh(U.act_quantize(i["x"], c, kind)))


def _ln(bias):
    return Form("K1l_bias" if bias else "K1l_nobias", vecs=("w1", "b1") if bias else ("w1",), outs=("h",), many=2 if bias else 1,
                calls=(("pq_layernorm_quant_rowwise", lambda L, o, c, R, N, st: L.pq_layernorm_quant_rowwise(P(o.x), D(o.x), P(o.w1), P(o.b1), EPS, c, R, N, P(o.q), D(o.q), P(o.sc),
                                                                                                             P(o.h), D(o.h), st)),),
                ref=lambda i, c: _qh(LS.layernorm_quantize(i["x"], i["w1"], i.get("b1"), EPS, c)))


def _dequant(axis):
    return Form(f"dequant_axis{axis}", custom=True, mats=(), outs=("out",), nq=0, smalls=("qin", "scv"), cnames=dict(out="out", qin="q"), ref=None,
                clash={"pq_dequant": ("out", "qin")},
                calls=(("pq_dequant", lambda L, o, c, R, N, st: L.pq_dequant(P(o.qin), D(o.qin), P(o.scv), axis, R, N, P(o.out), D(o.out), c, st)),))


FORMS = [
    Form("K1", extra_widths=(4104,),        # (K1 keeps one wave per row up to 512 vectors: 4104 16-bit columns are its first 256-thread width)
         calls=(("pq_quant_rowwise", lambda L, o, c, R, N, st: L.pq_quant_rowwise(P(o.x), c, R, N, D(o.x), P(o.q), D(o.q), P(o.sc), st)),),
         ref=lambda i, c: _q1(C.quant_rowwise(i["x"], c))),
    Form("K1_amax_halves", amax=True, many=2,
         calls=(("pq_quant_rowamax", lambda L, o, c, R, N, st: L.pq_quant_rowamax(P(o.x), c, R, N, D(o.x), P(o.am), st)),
                ("pq_quant_rowwise_amax", lambda L, o, c, R, N, st: L.pq_quant_rowwise_amax(P(o.x), c, R, N, D(o.x), P(o.am), P(o.q), D(o.q), P(o.sc), st))),
         clash={"pq_quant_rowamax": ("am", "x")}, cnames=dict(am="amax_bits"),
         ref=lambda i, c: _amax_ref(i["x"], c)),
    Form("K2", scale_len="cols", nan=False,
         calls=(("pq_quant_colwise", lambda L, o, c, R, N, st: L.pq_quant_colwise(P(o.x), c, R, N, D(o.x), P(o.q), D(o.q), P(o.sc), st)),),
         ref=lambda i, c: _q1(C.quant_colwise(i["x"], c))),
    _dequant(0), _dequant(1),
    Form("K1s", mats=("g", "u"), outs=("h",), wide=True, many=2,
         calls=(("pq_silu_mul_quant_rowwise", lambda L, o, c, R, N, st: L.pq_silu_mul_quant_rowwise(P(o.g), D(o.g), P(o.u), D(o.u), c, R, N, P(o.q), D(o.q), P(o.sc), P(o.h), D(o.h),
                                                                                                    st)),),
         ref=lambda i, c: _qh(C.silu_mul_quant_rowwise(i["g"], i["u"], c))),
    Form("K1s_amax_halves", mats=("g", "u"), amax=True, wide=True, many=1,
         calls=(("pq_silu_mul_rowamax", lambda L, o, c, R, N, st: L.pq_silu_mul_rowamax(P(o.g), D(o.g), P(o.u), D(o.u), c, R, N, P(o.am), st)),
                ("pq_silu_mul_quant_rowwise_amax", lambda L, o, c, R, N, st: L.pq_silu_mul_quant_rowwise_amax(P(o.g), D(o.g), P(o.u), D(o.u), c, R, N, P(o.am), P(o.q), D(o.q),
                                                                                                              P(o.sc), st))),
         clash={"pq_silu_mul_rowamax": ("am", "g")}, cnames=dict(am="amax_bits"),
         ref=lambda i, c: _amax_ref(C.silu_mul_quant_rowwise(i["g"], i["u"], c)[2], c)),
    _glu(0), _glu(1),
    Form("K1gg", mats=("g", "u"), outs=("h",), wide=True, many=2,
         calls=(("pq_gelu_mul_quant_rowwise", lambda L, o, c, R, N, st: L.pq_gelu_mul_quant_rowwise(P(o.g), D(o.g), P(o.u), D(o.u), c, R, N, 1, P(o.q), D(o.q), P(o.sc), P(o.h),
                                                                                                    D(o.h), st)),),
         ref=lambda i, c: _qh(GS.gelu_mul_quantize(i["g"], i["u"], c))),
    _act(0), _act(1), _act(2),
    Form("K1n", vecs=("w",), outs=("h",),
         calls=(("pq_rmsnorm_quant_rowwise", lambda L, o, c, R, N, st: L.pq_rmsnorm_quant_rowwise(P(o.x), D(o.x), P(o.w), EPS, c, R, N, P(o.q), D(o.q), P(o.sc), P(o.h), D(o.h), st)),),
         ref=lambda i, c: _qh(C.rmsnorm_quant_rowwise(i["x"], i["w"], EPS, c))),
    Form("K1a", mats=("x", "r"), vecs=("w",), outs=("s", "h"), alias=("s", "x"),
         calls=(("pq_add_rmsnorm_quant_rowwise", lambda L, o, c, R, N, st: L.pq_add_rmsnorm_quant_rowwise(P(o.x), D(o.x), P(o.r), D(o.r), P(o.s), D(o.s), P(o.w), EPS, c, R, N,
                                                                                                          P(o.q), D(o.q), P(o.sc), P(o.h), D(o.h), st)),),
         ref=lambda i, c: _qsh(A.add_rmsnorm_quantize(T(i["x"], c), T(i["r"], c), T(i["w"], c), EPS))),
    _ln(True), _ln(False),
    Form("K1al", mats=("x", "r"), vecs=("w1", "b1"), outs=("s", "h"), alias=("s", "x"),
         calls=(("pq_add_layernorm_quant_rowwise", lambda L, o, c, R, N, st: L.pq_add_layernorm_quant_rowwise(P(o.x), D(o.x), P(o.r), D(o.r), P(o.s), D(o.s), P(o.w1), P(o.b1), EPS,
                                                                                                              c, R, N, P(o.q), D(o.q), P(o.sc), P(o.h), D(o.h), st)),),
         ref=lambda i, c: _qsh(AL.add_layernorm_quantize(T(i["x"], c), T(i["r"], c), T(i["w1"], c), T(i["b1"], c), EPS))),
    Form("K1pl_one_group", mats=("a", "b", "c"), vecs=("w1", "b1"), outs=("s", "h"), alias=("s", "a"), cnames=dict(q="q1", h="h1", sc="scale1"),
         calls=(("pq_parallel_layernorm_quant_rowwise", _pl_call),), ref=lambda i, c: _pl_ref(i, c, 1)),
    Form("K1pl_two_groups", mats=("a", "b", "c"), vecs=("w1", "b1", "w2", "b2"), outs=("s", "h", "h2"), nq=2, alias=("s", "c"), cnames=dict(q="q1", h="h1", sc="scale1"),
         calls=(("pq_parallel_layernorm_quant_rowwise", _pl_call),), ref=lambda i, c: _pl_ref(i, c, 2), clash={"pq_parallel_layernorm_quant_rowwise": ("h2", "b")}),
    Form("K1l2", mats=("c",), vecs=("w1", "b1", "w2", "b2"), outs=("h", "h2"), nq=2, many=2, cnames=dict(q="q1", h="h1", sc="scale1"),
         calls=(("pq_parallel_layernorm_quant_rowwise", _pl_call),), ref=_l2_ref),
    Form("K1ng", vecs=("w",), outs=("h",), many=2,
         calls=(("pq_gemma_rmsnorm_quant_rowwise", lambda L, o, c, R, N, st: L.pq_gemma_rmsnorm_quant_rowwise(P(o.x), D(o.x), P(o.w), EPS, c, R, N, P(o.q), D(o.q), P(o.sc), P(o.h),
                                                                                                              D(o.h), st)),),
         ref=lambda i, c: _qh(GS.gemma_rmsnorm_quantize(i["x"], i["w"], EPS, c))),
    Form("K1ang", mats=("x", "r"), vecs=("w",), outs=("s", "h"), alias=("s", "x"), many=2, exact_sum=lambda o: o.r + o.x,
         calls=(("pq_add_gemma_rmsnorm_quant_rowwise", lambda L, o, c, R, N, st: L.pq_add_gemma_rmsnorm_quant_rowwise(P(o.x), D(o.x), P(o.r), D(o.r), P(o.s), D(o.s), P(o.w), EPS, c,
                                                                                                                      R, N, P(o.q), D(o.q), P(o.sc), P(o.h), D(o.h), st)),),
         ref=lambda i, c: _qsh(GS.add_gemma_rmsnorm_quantize(T(i["x"], c), T(i["r"], c), T(i["w"], c), EPS))),
    Form("K1pang", mats=("x", "r"), vecs=("pw", "w"), outs=("s", "h"), alias=("s", "x"), many=2, calls=(("pq_gemma_postnorm_add_rmsnorm_quant_rowwise", _pang_call),),
         ref=lambda i, c: _qsh(GP.postnorm_add_rmsnorm_quantize(T(i["x"], c), T(i["pw"], c), T(i["r"], c), T(i["w"], c), EPS, POST_EPS))),
    Form("K1pa", mats=("x", "r"), vecs=("pw",), outs=("s",), nq=0, alias=("s", "x"), many=1, calls=(("pq_gemma_postnorm_add_rmsnorm_quant_rowwise", _pang_call),),
         ref=lambda i, c: dict(s=A.to_bits(GP.postnorm_add(T(i["x"], c), T(i["pw"], c), T(i["r"], c), POST_EPS)))),
    Form("K1oq", mats=("x", "r"), vecs=("pw",), outs=("s",), alias=("s", "x"), many=2, calls=(("pq_olmo_postnorm_add_quant_rowwise", _olmo_call),),
         ref=lambda i, c: (lambda t: dict(q=t[0], sc=t[1], s=t[2]))(O.postnorm_add_quantize(T(i["x"], c), T(i["pw"], c), T(i["r"], c), POST_EPS))),
    Form("K1oa", mats=("x", "r"), vecs=("pw",), outs=("s",), nq=0, alias=("s", "x"), many=1, calls=(("pq_olmo_postnorm_add_quant_rowwise", _olmo_call),),
         ref=lambda i, c: dict(s=A.to_bits(O.postnorm_add(T(i["x"], c), T(i["pw"], c), T(i["r"], c), POST_EPS)))),
    Form("K1on", vecs=("pw",), outs=("s",), nq=0, alias=("s", "x"), many=1, calls=(("pq_olmo_postnorm_add_quant_rowwise", _olmo_call),),
         ref=lambda i, c: dict(s=A.to_bits(O.rmsnorm(T(i["x"], c), T(i["pw"], c), POST_EPS)))),
    Form("moe_combine", custom=True, mats=("y",), outs=("out",), nq=0, smalls=("ro", "so", "tw"), ref=None, cnames=dict(out="out", y="y"),
         calls=(("pq_moe_combine", lambda L, o, c, R, N, st: L.pq_moe_combine(P(o.y), D(o.y), c, R, P(o.ro), P(o.so), P(o.tw), 2, R, 2, N, P(o.out), D(o.out), st)),)),
]
BY_NAME = {f.name: f for f in FORMS}
GENERIC_FORMS = [f.name for f in FORMS if not f.custom]
CNAMES = dict(s="sum_out", h="h_out", sc="scale", r="residual", pw="post_weight", w="weight")


# ---------------------------------------------------------------------------------------------------------------- inputs and comparisons
def make_inputs(form, code, rows, cols, nan=None):
    """seeded inputs as storage bits: every matrix has an all-zero row (row 1); the first one a NaN in its last row where the specification defines that"""
    rng = np.random.default_rng(zlib.crc32(f"{form.name} {code} {cols}".encode()))
    i = {}
    for j, n in enumerate(form.mats):
        a = (rng.standard_normal((rows, cols)) * (2.0, 3.0, 0.5)[j % 3]).astype(np.float32)
        a[1] = 0.0
        if (form.nan if nan is None else nan) and j == 0:
            a[rows - 1, cols // 2] = np.nan
        i[n] = Q.from_f32(a, code)
    for n in form.vecs:
        i[n] = Q.from_f32((rng.standard_normal(cols) * 0.25 + (0.0 if n.startswith("b") else 1.0)).astype(np.float32), code)
    return i


def _u(a, code):
    """storage bits (or float32 values) as unsigned integers"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def compare(name, got, want, code, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, name, got.shape, want.shape)
    if name.startswith("q"):
        bad = got != want
    elif name.startswith("sc"):
        bad = _u(got, 2) != _u(want, 2)
    elif name == "am":
        nan = want > 0x7F800000
        assert np.array_equal(got > 0x7F800000, nan), f"{what}: {name}: NaN rows differ"
        bad = (got != want) & ~nan
    else:                                                     # a float output: NaNs as a class (gpu_util.same_f), everything else bit for bit
        g, w = _u(got, code), _u(want, code)
        gf = g.view(np.float32) if code == 2 else Q.to_f32(g, code)
        wf = w.view(np.float32) if code == 2 else Q.to_f32(w, code)
        assert np.array_equal(np.isnan(gf), np.isnan(wf)), f"{what}: {name}: NaN positions differ ({int(np.isnan(gf).sum())} vs {int(np.isnan(wf).sum())})"
        bad = (g != w) & ~np.isnan(wf)
    assert not bad.any(), f"{what}: {name}: {int(bad.sum())} of {bad.size} elements differ (first at {np.argwhere(bad)[:3].tolist()})"


def mismatch_rows(name, got, want, code):
    """the rows in which `compare` would find a difference (NaNs as a class where it does)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return list(range(max(len(got), len(want))))
    if name.startswith("q"):
        bad = got != want
    elif name.startswith("sc"):
        bad = _u(got, 2) != _u(want, 2)
    elif name == "am":
        nan = want > 0x7F800000
        bad = ((got > 0x7F800000) != nan) | ((got != want) & ~nan)
    else:
        g, w = _u(got, code), _u(want, code)
        gf = g.view(np.float32) if code == 2 else Q.to_f32(g, code)
        wf = w.view(np.float32) if code == 2 else Q.to_f32(w, code)
        bad = (np.isnan(gf) != np.isnan(wf)) | ((g != w) & ~np.isnan(wf))
    return np.flatnonzero(bad.reshape(len(bad), -1).any(axis=1)).tolist()


def launch(form, code, inp, pad=None):
    """drive the form's C-ABI entries on `inp` (storage bits) on the current device and return its outputs as `compare` takes them.  pad: [rows, k] storage bits that sit
    in the columns just behind every matrix input's row (the inputs are then column blocks of wider buffers)."""
    import torch

    from protoquant_amd import _lib
    from tests.gpu_util import bits, to_gpu
    L = _lib.lib()
    rows, cols = inp[form.mats[0]].shape
    o = Ops()
    for n in form.mats:
        if pad is None:
            o[n] = to_gpu(inp[n], code)
        else:
            o[n] = to_gpu(np.concatenate([inp[n], pad], axis=1), code)[:, :cols]
    for n in form.vecs:
        o[n] = to_gpu(inp[n], code)
    for n in form.outs:
        o[n] = torch.empty((rows, cols), dtype=TD[code], device="cuda")
    for k in range(form.nq):
        sfx = ("", "2")[k]
        o["q" + sfx] = torch.full((rows, cols), 0x5B, dtype=torch.int8, device="cuda")
        o["sc" + sfx] = torch.full((rows if form.scale_len == "rows" else cols,), -1.0, dtype=torch.float32, device="cuda")
    if form.amax:
        o["am"] = torch.zeros(rows, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for sym, fn in form.calls:
        _lib.check(fn(L, o, code, rows, cols, st), sym)
    torch.cuda.synchronize()
    got = {n: bits(o[n]) for n in form.outs}
    for k in range(form.nq):
        sfx = ("", "2")[k]
        got["q" + sfx], got["sc" + sfx] = o["q" + sfx].cpu().numpy(), bits(o["sc" + sfx])
    if form.amax:
        got["am"] = o["am"].cpu().numpy().view(np.uint32)
    return got
