"""The `base + row * ld` arithmetic of EVERY row kernel (K1 and its halves, K2, dequant, K1s, K1g, K1gg, K1u, K1n, K1a, K1l, K1al, K1pl / K1l2, K1ng, K1ang, K1pang / K1pa,
K1oq / K1oa / K1on, moe_combine) past 2^31 elements and byte 2^32, in every row layout (one wave per row, 256 / 512 threads per row, the generic kernel), for bf16, fp16 and
f32, through the C-ABI; the same kernels at more than 4 x 65 535 rows; and, on the CPU, the argument checks of the same entries on operands laid out the same way.

PART 1 (-m gpu).  Six rows (f32: four) with a leading dimension of LD = 2^30 + 64 elements: the offsets row * LD that a kernel forms lie on both sides of element 2^31 and of
element 2^32 of its operand (f32: of element 2^31 and of byte 2^32), at the cost of an allocation and no compute.  Every operand of the storage dtype is a column block of
ONE flat buffer with that one pitch (the use the fusions were built for: slices of wide fused outputs; the overlap checker's same-pitch rule admits it), the int8 codes live
in a second buffer with the same pitch in elements.  Outputs are compared bit for bit (NaNs as a class) with the CPU specification of each entry, never with another GPU call.

NO OUTCOME CAN LEAVE THE ALLOCATIONS.  Provoking a fault is not an option, so the buffers are built around what a wrong kernel could compute:
  - every operand base lies behind a FRONT margin: 2^31 elements in the int8 and the f32 buffer, 5 x 2^30 elements (5 x 2^31 bytes) in the 16-bit buffers;
  - every buffer extends more than 2^32 elements (f32: 2^32 bytes; its element offsets stay below 2^32) beyond its last operand base.
A truncation to 32 bits — signed or unsigned, of an element offset or of a byte offset, of the product row * ld or of the final sum — gives an offset in [-2^31, 2^32) of the
truncated unit, and base + that lies inside the buffer.  The larger front margin of the 16-bit buffers covers one case more: a leading dimension in BYTES (2^31 + 128) that is
itself truncated to a signed 32-bit value (-2^31 + 128) and then multiplied in 64 bits by up to row 5 (every other pitch here — LD in elements, 2^32 + 256 bytes for f32 —
keeps its value or becomes small and positive).
Detection: each buffer is filled with an integer sentinel once; a case writes its inputs into their windows, calls the entry, reads the output windows, writes the sentinel back
over every window and then checks that the WHOLE buffer is the sentinel again (min and max per 1 GiB chunk: no large temporary), so a wrapped store anywhere in the buffer is
seen; a wrapped load reads the sentinel and shows as a mismatch against the specification.

PART 2 (-m gpu).  262 149 rows (more than 4 x 65 535: rows ride on grid.x) by 64 columns and by 13 (generic), for the families that had no such test: sampled rows (the first,
the last, those around 262 140 and 262 144, and 4 096 random ones) against the specification, every other row pinned to them without a second kernel run (every scale > 0 and
a code of magnitude 127 in every row; the stored sums that are plain adds against the torch expression on the GPU for all rows).

PART 3 (CPU).  Every entry with never-dereferenced addresses laid out as in part 1 gets past its argument checks, and one element of overlap at that pitch is refused by name.
A table test fails when an exported row entry has no row in FORMS."""
import re

import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from oracle import qspec_numpy as Q
from tests import addnorm_spec as A
from tests.gpu_util import TD, bits, to_gpu
from tests.row_forms import BY_NAME, CNAMES, EPS, FORMS, GENERIC_FORMS, POST_EPS, Ops, T, compare, make_inputs

# ---------------------------------------------------------------------------------------------------------------- geometry of part 1
LD = (1 << 30) + 64                                  # elements, every matrix operand (a multiple of 16: the vector layouts stay reachable)
ROWS = {0: 6, 1: 6, 2: 4}
FRONT = {0: 5 << 30, 1: 5 << 30, 2: 1 << 31}         # elements in front of the first operand base
FRONT_Q = 1 << 31
BLK, NBLK, TAIL = 11264, 8, 1 << 16                  # column block per operand (>= the widest case + an odd offset, a multiple of 16), blocks, elements behind the last row
ESIZE = {0: 2, 1: 2, 2: 4}
SENT = {0: 0x5A5B, 1: 0x5A5B, 2: 0x5A5B5A5B}         # finite in every dtype: 1.5e16 as bf16 / f32, 203.4 as fp16
SENT_Q = 0x5B
WIDTHS = (512, 4096, 333)                            # one wave per row / 256 threads per row / ragged: generic (rowmap_kernels.h, rownorm_kernels.h)
WIDE = 11008                                         # bf16, kWideRows ops: 1376 vectors -> 512 threads x 3


def buf_elems(code, rows):
    return FRONT[code] + (rows - 1) * LD + NBLK * BLK + TAIL


def test_geometry_covers_the_boundaries_and_every_truncation():
    assert LD % 16 == 0 and LD < (1 << 31) and BLK % 16 == 0 and BLK > WIDE
    for code, rows in ROWS.items():
        offs = [r * LD for r in range(rows)]
        assert any(o < (1 << 31) for o in offs[1:]) and any(o > (1 << 31) for o in offs)                           # element 2^31 of the operand
        if code == 2:
            assert offs[1] * 4 > (1 << 32) and offs[0] * 4 < (1 << 32)                                               # byte 2^32
        else:
            assert any((1 << 31) < o < (1 << 32) for o in offs) and offs[-1] > (1 << 32)                            # element 2^32
        last_base = FRONT[code] + (NBLK - 1) * BLK + 1
        e = ESIZE[code]
        assert FRONT[code] >= (1 << 31)                                                                               # signed truncation of an element / a byte offset
        assert buf_elems(code, rows) >= last_base + min(1 << 32, offs[-1] + BLK) + BLK                              # unsigned truncation of an element offset
        assert buf_elems(code, rows) * e >= last_base * e + (1 << 32) + BLK * e                                     # ... of a byte offset
        ld_bytes_s32 = ((LD * e + (1 << 31)) % (1 << 32)) - (1 << 31)                                               # the pitch in bytes as a signed 32-bit value
        assert FRONT[code] * e + (rows - 1) * min(ld_bytes_s32, 0) >= 0 and last_base * e + (rows - 1) * max(ld_bytes_s32, 0) + BLK * e <= buf_elems(code, rows) * e
    assert buf_elems(0, 6) * 2 + (FRONT_Q + 5 * LD + NBLK * BLK + TAIL) < 34 * 10 ** 9 and buf_elems(2, 4) * 4 + (FRONT_Q + 3 * LD + NBLK * BLK + TAIL) < 34 * 10 ** 9


# ---------------------------------------------------------------------------------------------------------------- the table (tests/row_forms.py)
def test_every_exported_row_entry_has_a_row():
    from protoquant_amd import _lib
    pat = re.compile(r"pq_\w+_rowwise(_amax)?$|pq_\w+_rowamax$|pq_quant_\w+$|pq_dequant$|pq_moe_combine$")
    want = {s for s in _lib.EXPORTS if pat.match(s)}
    have = {sym for f in FORMS for sym, _ in f.calls}
    assert want and not (want - have), f"exported row entries without a row in FORMS: {sorted(want - have)}"
    assert not (have - set(_lib.EXPORTS)), sorted(have - set(_lib.EXPORTS))
    assert len(BY_NAME) == len(FORMS)


def _small(n, dtype=torch.float32):
    """a guarded vector output: 16 sentinel elements on either side of the n that the kernel writes"""
    t = torch.full((n + 32,), SENT[2], dtype=torch.int32, device="cuda")
    return t, t[16:16 + n].view(dtype)


def _small_clean(t, n):
    return bool((t[:16] == SENT[2]).all()) and bool((t[16 + n:] == SENT[2]).all())


# ---------------------------------------------------------------------------------------------------------------- part 1: the arena
def _need(nbytes):
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + (2 << 30):
        pytest.skip(f"needs {nbytes >> 20} MiB of free device memory, {free >> 20} MiB are free")


class Arena:
    """one flat buffer of the storage dtype and one of int8, filled with their sentinels; operands are column blocks of them with the pitch LD"""

    def __init__(self, code):
        self.code, self.rows = code, ROWS[code]
        ns, nq = buf_elems(code, self.rows), FRONT_Q + (self.rows - 1) * LD + NBLK * BLK + TAIL
        _need(ns * ESIZE[code] + nq)
        self.s = torch.empty(ns, dtype=TD[code], device="cuda")
        self.si = self.s.view(torch.int32 if code == 2 else torch.int16)
        self.q = torch.empty(nq, dtype=torch.int8, device="cuda")
        self.used = []
        self.refill()

    def refill(self):
        self.si.fill_(SENT[self.code])
        self.q.fill_(SENT_Q)

    def win(self, blk, cols, odd=0):
        assert 0 <= blk < NBLK and cols + odd <= BLK
        off = FRONT[self.code] + blk * BLK + odd
        self.used.append(self.si.as_strided((self.rows, cols), (LD, 1), off))
        return self.s.as_strided((self.rows, cols), (LD, 1), off)

    def qwin(self, blk, cols):
        assert 0 <= blk < NBLK and cols <= BLK
        v = self.q.as_strided((self.rows, cols), (LD, 1), FRONT_Q + blk * BLK)
        self.used.append(v)
        return v

    def restore_and_scan(self):
        """the sentinel back over every window handed out, then: is the WHOLE of both buffers the sentinel?  (min / max per 1 GiB chunk: no temporary of any size)"""
        for v in self.used:
            v.fill_(SENT_Q if v.dtype == torch.int8 else SENT[self.code])
        self.used = []
        parts = []
        for t, sent in ((self.si, SENT[self.code]), (self.q, SENT_Q)):
            step = (1 << 30) // t.element_size()
            for o in range(0, t.numel(), step):
                mn, mx = torch.aminmax(t[o:o + step])
                parts += [mn.to(torch.int64) - sent, mx.to(torch.int64) - sent]
        if bool((torch.stack(parts) == 0).all()):
            return ""
        where = []                                            # a stray store: say where (offsets relative to the first operand base), then repair the buffers for the next test
        for name, t, sent, front in (("storage", self.si, SENT[self.code], FRONT[self.code]), ("int8", self.q, SENT_Q, FRONT_Q)):
            step = (1 << 28)
            for o in range(0, t.numel(), step):
                idx = (t[o:o + step] != sent).nonzero()[:4, 0]
                where += [f"{name}[base{int(i) + o - front:+d}]" for i in idx.tolist()]
        self.refill()
        return "stores outside the output windows at " + ", ".join(where[:12])


@pytest.fixture(scope="module", params=[0, 1, 2], ids=["bf16", "fp16", "f32"])
def arena(request):
    from protoquant_amd import _lib
    _lib.lib()
    a = Arena(request.param)
    yield a
    a.s = a.si = a.q = None
    a.used = []
    del a
    torch.cuda.empty_cache()


def _status(st, sym):
    from protoquant_amd import _lib
    _lib.check(st, sym)


def run_case(arena, form, cols, odd=False, alias=False):
    """one call of `form` on column blocks of the arena: outputs against the specification, then the whole-buffer sentinel check"""
    from protoquant_amd import _lib
    L, code, rows = _lib.lib(), arena.code, arena.rows
    what = f"{form.name} {('bf16', 'fp16', 'f32')[code]} cols={cols}{' odd base' if odd else ''}{' sum_out is ' + form.alias[1] if alias else ''}"
    inp = make_inputs(form, code, rows, cols)
    o, blk = Ops(), 0
    for n in form.mats:
        o[n] = arena.win(blk, cols, odd=1 if odd and n == form.mats[0] else 0)
        o[n].copy_(to_gpu(inp[n], code))
        blk += 1
    for n in form.vecs:
        o[n] = to_gpu(inp[n], code)
    for n in form.outs:
        if alias and n == form.alias[0]:
            o[n] = o[form.alias[1]]
        else:
            o[n] = arena.win(blk, cols)
            blk += 1
    guards = []
    for k in range(form.nq):
        sfx = ("", "2")[k]
        o["q" + sfx] = arena.qwin(k, cols)
        n = rows if form.scale_len == "rows" else cols
        g, o["sc" + sfx] = _small(n)
        guards.append((g, n))
    if form.amax:
        g, o["am"] = _small(rows, torch.int32)
        guards.append((g, rows))
    st = torch.cuda.current_stream().cuda_stream
    for sym, fn in form.calls:
        _status(fn(L, o, code, rows, cols, st), sym)
    torch.cuda.synchronize()
    got = {n: bits(o[n]) for n in form.outs}
    for k in range(form.nq):
        sfx = ("", "2")[k]
        got["q" + sfx], got["sc" + sfx] = o["q" + sfx].contiguous().cpu().numpy(), bits(o["sc" + sfx])
    if form.amax:
        got["am"] = o["am"].cpu().numpy().view(np.uint32)
    stray = arena.restore_and_scan()
    want = form.ref(inp, code)
    assert set(want) >= set(got), (what, sorted(want), sorted(got))
    for n in sorted(got):
        compare(n, got[n], want[n], code, what)
    assert not stray, f"{what}: {stray}"
    assert all(_small_clean(g, n) for g, n in guards), f"{what}: a scale / amax vector was written outside its {rows} elements"


@pytest.mark.gpu
@pytest.mark.parametrize("name", GENERIC_FORMS)
def test_row_offsets_past_2g(arena, name):
    form = BY_NAME[name]
    widths = WIDTHS + form.extra_widths + ((WIDE,) if form.wide and arena.code == 0 else ())
    for cols in widths:
        run_case(arena, form, cols)
    run_case(arena, form, 512, odd=True)                      # the generic kernel by an odd element offset of the first operand's base


@pytest.mark.gpu
@pytest.mark.parametrize("name", [f.name for f in FORMS if f.alias])
def test_sum_out_is_its_input_past_2g(arena, name):
    """sum_out == x (K1pl: a resp. c): the same pointer and pitch, every layout"""
    form = BY_NAME[name]
    for cols in WIDTHS:
        run_case(arena, form, cols, alias=True)


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [0, 1])
def test_dequant_past_2g(arena, axis):
    from protoquant_amd import _lib
    L, code, rows = _lib.lib(), arena.code, arena.rows
    form = BY_NAME[f"dequant_axis{axis}"]
    st = torch.cuda.current_stream().cuda_stream
    for cols, odd in ((512, 0), (4096, 0), (333, 0), (512, 1)):
        what = f"{form.name} code {code} cols={cols} odd={odd}"
        rng = np.random.default_rng(cols * 7 + axis + code * 3 + odd)
        q = rng.integers(-128, 128, (rows, cols), dtype=np.int8)
        q[1] = 0
        sc = (rng.random(cols if axis == 0 else rows) * 0.05 + 1e-3).astype(np.float32)
        o = Ops(qin=arena.qwin(0, cols), out=arena.win(0, cols, odd=odd), scv=torch.from_numpy(sc).cuda())
        o.qin.copy_(torch.from_numpy(q).cuda())
        _status(form.calls[0][1](L, o, code, rows, cols, st), "pq_dequant")
        torch.cuda.synchronize()
        got = bits(o.out)
        stray = arena.restore_and_scan()
        compare("out", got, C.dequant(q, sc, axis, code), code, what)
        assert not stray, f"{what}: {stray}"


@pytest.mark.gpu
def test_moe_combine_past_2g(arena):
    """ldy and ld_out = LD; rows_of picks, for every token, one y row from either end: on both sides of every boundary"""
    from protoquant_amd import _lib, moe
    L, code, rows = _lib.lib(), arena.code, arena.rows
    form = BY_NAME["moe_combine"]
    st = torch.cuda.current_stream().cuda_stream
    for cols, odd in ((512, 0), (4096, 0), (333, 0), (512, 1)):      # one wave per token / 256 threads / ragged tail / element-wise
        what = f"moe_combine code {code} H={cols} odd={odd}"
        rng = np.random.default_rng(cols + code + odd)
        y = (rng.standard_normal((rows, cols)) * 2).astype(np.float32)
        y[1] = 0.0
        yb = Q.from_f32(y, code)
        tw = Q.from_f32(rng.random((rows, 2)).astype(np.float32), code)
        ro = np.array([[t, rows - 1 - t] for t in range(rows)], np.int32)
        so = np.array([[t & 1, 1 - (t & 1)] for t in range(rows)], np.int32)
        o = Ops(y=arena.win(0, cols, odd=odd), out=arena.win(1, cols), ro=torch.from_numpy(ro).cuda(), so=torch.from_numpy(so).cuda(), tw=to_gpu(tw, code))
        o.y.copy_(to_gpu(yb, code))
        _status(form.calls[0][1](L, o, code, rows, cols, st), "pq_moe_combine")
        torch.cuda.synchronize()
        got = bits(o.out)
        stray = arena.restore_and_scan()
        want = moe.combine(T(yb, code), torch.from_numpy(ro).long(), torch.from_numpy(so).long(), T(tw, code))
        compare("out", got, A.to_bits(want), code, what)
        assert not stray, f"{what}: {stray}"


# ---- the Python surface: a strided view is passed through, not copied
def _views(arena, cols, n):
    return [arena.win(b, cols) for b in range(n)]


@pytest.mark.gpu
def test_python_add_rmsnorm_quantize_takes_far_strided_views(arena):
    import protoquant_amd as pq
    from protoquant_amd import _lib
    code, rows, cols = arena.code, arena.rows, 512
    form = BY_NAME["K1a"]
    inp = make_inputs(form, code, rows, cols)
    xv, rv, sv = _views(arena, cols, 3)
    xv.copy_(to_gpu(inp["x"], code)); rv.copy_(to_gpu(inp["r"], code))
    assert xv.stride(0) == LD and _lib.row_major_2d(xv) is xv
    qt, summed = pq.add_rmsnorm_quantize(xv, rv, to_gpu(inp["w"], code), EPS, out=sv)
    torch.cuda.synchronize()
    assert summed.data_ptr() == sv.data_ptr() and summed.stride(0) == LD
    got = dict(q=qt.int_data.cpu().numpy(), sc=bits(qt.scale), s=bits(sv))
    stray = arena.restore_and_scan()
    want = form.ref(inp, code)
    for n in got:
        compare(n, got[n], want[n], code, "add_rmsnorm_quantize(x_view, r_view, w, out=s_view)")
    assert not stray, stray


@pytest.mark.gpu
def test_python_olmo_rmsnorm_takes_far_strided_views(arena):
    import protoquant_amd as pq
    code, rows, cols = arena.code, arena.rows, 512
    form = BY_NAME["K1on"]
    inp = make_inputs(form, code, rows, cols)
    xv, ov = _views(arena, cols, 2)
    xv.copy_(to_gpu(inp["x"], code))
    out = pq.olmo_rmsnorm(xv, to_gpu(inp["pw"], code), POST_EPS, out=ov)
    torch.cuda.synchronize()
    assert out.data_ptr() == ov.data_ptr() and out.stride(0) == LD
    got = bits(ov)
    stray = arena.restore_and_scan()
    compare("s", got, form.ref(inp, code)["s"], code, "olmo_rmsnorm(x_view, w, out=view)")
    assert not stray, stray


@pytest.mark.gpu
def test_python_silu_mul_quantize_takes_far_strided_views(arena):
    import protoquant_amd as pq
    from protoquant_amd import _lib
    code, rows, cols = arena.code, arena.rows, 512
    form = BY_NAME["K1s"]
    inp = make_inputs(form, code, rows, cols)
    gv, uv = _views(arena, cols, 2)
    gv.copy_(to_gpu(inp["g"], code)); uv.copy_(to_gpu(inp["u"], code))
    assert _lib.row_major_2d(gv) is gv and _lib.row_major_2d(uv) is uv and _lib.ld(uv) == LD
    qt = pq.silu_mul_quantize(gv, uv)
    torch.cuda.synchronize()
    got = dict(q=qt.int_data.cpu().numpy(), sc=bits(qt.scale))
    stray = arena.restore_and_scan()
    want = form.ref(inp, code)
    for n in got:
        compare(n, got[n], want[n], code, "silu_mul_quantize(g_view, u_view)")
    assert not stray, stray


# ---------------------------------------------------------------------------------------------------------------- part 2: more than 4 x 65 535 rows
MANY = 4 * 65535 + 9                                         # 262 149
EDGES = sorted({0, 1, 2, 65535, 65536, *range(262136, MANY)})
_BASE = {}


def _base(code, cols):
    """one seeded [MANY, cols] matrix per dtype and width, shared by every case (column 0 is positive, so that no row is all zero behind a relu)"""
    if (code, cols) not in _BASE:
        a = (np.random.default_rng(cols * 10 + code).standard_normal((MANY, cols)) * 2).astype(np.float32)
        a[:, 0] = np.abs(a[:, 0]) + 0.5
        _BASE[(code, cols)] = Q.from_f32(a, code)
    return _BASE[(code, cols)]


def _many_cases():
    return [(f.name, code, cols) for f in FORMS if f.many and not f.custom for code in ((0, 2) if f.many == 2 else (0,)) for cols in (64, 13)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,code,cols", _many_cases())
def test_more_than_4x65535_rows(name, code, cols):
    from protoquant_amd import _lib
    L, form, rows = _lib.lib(), BY_NAME[name], MANY
    what = f"{name} code {code} {rows} x {cols}"
    inp = {n: np.roll(_base(code, cols), 3 * j, axis=0) if j else _base(code, cols) for j, n in enumerate(form.mats)}
    inp.update({n: v for n, v in make_inputs(form, code, 2, cols, nan=False).items() if n in form.vecs})
    o = Ops({n: to_gpu(inp[n], code) for n in form.mats + form.vecs})
    for n in form.outs:
        o[n] = torch.empty((rows, cols), dtype=TD[code], device="cuda")
    for k in range(form.nq):
        o["q" + ("", "2")[k]] = torch.zeros((rows, cols), dtype=torch.int8, device="cuda")
        o["sc" + ("", "2")[k]] = torch.zeros(rows, dtype=torch.float32, device="cuda")
    if form.amax:
        o["am"] = torch.zeros(rows, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for sym, fn in form.calls:
        _status(fn(L, o, code, rows, cols, st), sym)
    torch.cuda.synchronize()
    # sampled rows against the specification (every op here is row by row)
    pick = np.array(sorted(set(EDGES) | set(np.random.default_rng(5).choice(rows, 4096, replace=False).tolist())))
    want = form.ref({n: (inp[n][pick] if n in form.mats else inp[n]) for n in inp}, code)
    idx = torch.from_numpy(pick).cuda()
    for n in sorted(want):
        g = o[n][idx]
        got = g.cpu().numpy().view(np.uint32) if n == "am" else (g.cpu().numpy() if n.startswith("q") else bits(g))
        compare(n, got, want[n], code, f"{what} (sampled rows)")
    # every other row is pinned to them without a second kernel run
    for k in range(form.nq):
        q, sc = o["q" + ("", "2")[k]], o["sc" + ("", "2")[k]]
        assert bool((sc > 0).all()), f"{what}: a scale is not > 0"
        assert bool((q.to(torch.int16).abs().amax(dim=1) == 127).all()), f"{what}: a row without a code of magnitude 127"
    if form.amax and name == "K1_amax_halves":                # the row amax of x itself is exact in torch
        assert torch.equal(o.am.view(torch.float32), o.x.float().abs().amax(dim=1)), f"{what}: amax"
    if form.exact_sum is not None:
        assert torch.equal(o.s.view(torch.uint8), form.exact_sum(o).view(torch.uint8)), f"{what}: sum_out against the torch add, all rows"


@pytest.mark.gpu
@pytest.mark.parametrize("code,H", [(0, 64), (0, 13), (2, 64)])
def test_moe_combine_more_than_4x65535_tokens(code, H):
    from protoquant_amd import _lib, moe
    L, T_, k = _lib.lib(), MANY, 2
    g = torch.Generator().manual_seed(H + code)
    y = (torch.randn(T_ * k, H, generator=g) * 2).to(TD[code])
    ro = torch.randperm(T_ * k, generator=g).reshape(T_, k).to(torch.int32)
    so = torch.stack([torch.arange(T_) & 1, 1 - (torch.arange(T_) & 1)], dim=1).to(torch.int32)
    tw = torch.rand(T_, k, generator=g).to(TD[code])
    yg, rg, sg, wg = y.cuda(), ro.cuda(), so.cuda(), tw.cuda()
    out = torch.empty((T_, H), dtype=TD[code], device="cuda")
    _status(L.pq_moe_combine(yg.data_ptr(), H, code, T_ * k, rg.data_ptr(), sg.data_ptr(), wg.data_ptr(), k, T_, k, H, out.data_ptr(), H,
                             torch.cuda.current_stream().cuda_stream), "pq_moe_combine")
    torch.cuda.synchronize()
    pick = torch.tensor(EDGES)
    want = moe.combine(y, ro[pick].long(), so[pick].long(), tw[pick])                          # on the CPU
    compare("out", bits(out[pick.cuda()]), A.to_bits(want), code, f"moe_combine {T_} tokens x {H}, code {code} (sampled tokens)")
    # all tokens: the eager expression whose bits the kernel promises (one rounded multiply and one rounded add per slot), on the GPU
    assert torch.equal(out.view(torch.uint8), moe.combine(yg, rg.long(), sg.long(), wg).view(torch.uint8))


# ---------------------------------------------------------------------------------------------------------------- part 3 (CPU): the argument checks at this layout
class Fake:
    """an operand that is an address and a pitch and is never dereferenced"""

    def __init__(self, ptr, ld=0):
        self.ptr, self.ld = ptr, ld

    def data_ptr(self):
        return self.ptr

    def stride(self, dim):
        return self.ld


S_BASE, Q_BASE, V_BASE = 0x7000_0000_0000, 0x7800_0000_0000, 0x7C00_0000_0000


def fake_operands(form, code, cols, alias=False):
    e = ESIZE[code]
    o, blk, small = Ops(), 0, 0
    for n in form.mats + form.outs:
        if alias and n == form.alias[0]:
            o[n] = o[form.alias[1]]
            continue
        o[n] = Fake(S_BASE + (FRONT[code] + blk * BLK) * e, LD)
        blk += 1
    for k in range(form.nq):
        o["q" + ("", "2")[k]] = Fake(Q_BASE + FRONT_Q + k * BLK, LD)
    names = form.vecs + tuple("sc" + ("", "2")[k] for k in range(form.nq)) + (("am",) if form.amax else ()) + form.smalls
    for n in names:
        o[n] = Fake(Q_BASE + FRONT_Q + NBLK * BLK, LD) if n == "qin" else Fake(V_BASE + small * (1 << 24))
        small += 1
    return o


def _elem(form, code, n):
    return 1 if n.startswith("q") else (4 if n.startswith("sc") or n == "am" else ESIZE[code])


ENTRY_CASES = [(f.name, sym) for f in FORMS for sym, _ in f.calls]


@pytest.mark.parametrize("code", [0, 2])
@pytest.mark.parametrize("name,sym", ENTRY_CASES)
def test_far_column_blocks_pass_the_checks_and_one_element_of_overlap_does_not(name, sym, code):
    """as tests/test_addnorm_host.py::test_allowed_aliases_and_column_blocks_pass_the_checks: status 3 (the launch fails) on a machine without a GPU, never 1; on one
    with a GPU these addresses must not be launched, so only the no-GPU case is exercised"""
    from protoquant_amd import _lib
    L = _lib.lib()
    if torch.cuda.is_available():
        pytest.skip("argument-check-only test: needs a machine without a GPU (the operands are not real memory)")
    form, rows, cols = BY_NAME[name], ROWS[code], 512
    fn = dict(form.calls)[sym]
    for alias in ((False, True) if form.alias else (False,)):
        st = fn(L, fake_operands(form, code, cols, alias), code, rows, cols, None)
        assert st == 3 and b"overlaps" not in L.pq_last_error(), (name, sym, alias, st, L.pq_last_error())
    # one element of overlap between two blocks at this pitch
    moved, onto = form.clash.get(sym) or ((form.outs[-1] if form.outs else "q"), form.mats[0])
    o = fake_operands(form, code, cols)
    o[moved] = Fake(o[onto].data_ptr() + cols * _elem(form, code, onto) - _elem(form, code, moved), o[moved].ld)
    st = fn(L, o, code, rows, cols, None)
    err = L.pq_last_error()
    cname = form.cnames.get(moved) or CNAMES.get(moved, moved)
    assert st == 1 and sym.encode() in err and b"overlaps" in err and re.search(rb"\b%s\b" % cname.encode(), err), (name, sym, moved, onto, st, err)
