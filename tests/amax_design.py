"""TEST INFRASTRUCTURE — designed operands for the one reduction of the library that does not react to most of its inputs: the row maximum of |h| that every quantising
row kernel computes.  A sum of squares changes when any element is dropped; an amax changes only when the dropped element IS the maximum.  So the operands built here put the
strict row maximum at one designed position per row, and the bookkeeping says which positions a layout has: (lane, slot, element of the 16-byte vector).  Nothing in this
module launches a kernel; tests/test_amax_design_host.py holds it to its claims on the CPU, tests/test_gpu_amax_positions.py and tests/test_gpu_tail_slots.py use it.

LAYOUT DECISIONS, restated as plain arithmetic (bookkeeping only, as tests/test_gemm_edges_host.py restates skinny_plan):
  k1_layout        quant_rowwise_dispatch (quant_kernels.hip): one wave per row x 1 / 2 / 4 / 8 vectors up to 512 vectors, 256 threads x 4 .. 32 up to 8192; the two-rows-per-
                   wave kernel (PQ_K1_RPW=2) and the 16-byte-store kernel (PQ_K1_ST16=1) are layouts of their own; everything else is the generic kernel
  rowmap_layout    rowmap_dispatch (rowmap_kernels.h): one wave x 1 / 2 / 4 up to 256 vectors, 512 threads x 3 for 1025 .. 1536 vectors of an op with kWideRows (unless
                   PQ_SILU_TPR=256), else 256 threads x 2 .. 16 up to 4096
  rownorm_layout   rownorm_dispatch (rownorm_kernels.h): one wave x 1 .. 8 up to PQ_RMS_WAVE_MAX vectors (default 256, at most 512), else 256 threads x 1 .. 16 up to 4096
In a row layout (TPR, VPT) vector v of the row sits on lane v mod TPR in slot v div TPR; a slot whose vector index is past the row's end is DEAD: it loads a clamped
duplicate of the last vector and must contribute nothing.

PLANTED MAXIMUM.  Every matrix row is the same background of magnitudes in [0.25, 1] (secondary operands a quarter of that); row i carries one planted value of magnitude
256 .. 480 at column p(i) of the operand that carries through to h (u for the gated ops, with g = 4 there; the residual for K1oq / K1pang; x otherwise).  Kinds: every planted position
(a column: lane, slot and element) is planted twice, with a finite value of each sign, and every planted vector (lane, slot) once more with NaN and once with +-Inf, in
elements that walk with the vector index (3 v + 1 and 5 v + 2 mod the vector length: never tied to the row index mod 4).  Conditions that are arithmetic and not choices:
  - an activation of one input (relu, gelu) sends a large negative x to zero, so K1u plants positive values only;
  - in a norm a NaN anywhere makes every h of the row NaN, so no position can be told from another: the norms take the Inf kind only (rs = 0, h = 0 everywhere else and
    NaN at p: p is still the strict maximum of the bit patterns); in a LayerNorm an Inf makes the mean Inf and every x - mean NaN as well, so K1l / K1al / K1pl / K1l2
    take the finite kinds only (tests/test_gpu_tail_slots.py has their NaN rows);
  - a LayerNorm of n columns cannot separate the maximum from the runner-up by more than n - 1: its narrowest design has 8 columns.
COVERAGE per layout.  Widths of at most 2048 elements: every column is planted (with both signs), at the smallest and at the largest width that reaches the layout.  Wider
layouts, at one width that leaves the last slot partly live ((VPT - 1) TPR + 101 vectors; 37 for one wave): every lane in its first and its last live slot, every slot at
the first and the last live lane of each wave, the last vector and its neighbour — each of these vectors in element 3 v + 1 mod the vector length with both signs, and
with NaN and Inf.  The generic kernels take 333 and 1003 columns with every column planted.

TAIL SLOTS.  tail_cases() puts +Inf, -Inf, NaN, +0, -0, the largest finite value and a subnormal — each in an element of its own — into the LAST 16-byte vector of one
[cols] parameter (and, as a control, into the first), at widths that leave part of a wave, whole waves and a whole slot index dead; tail_inputs() crosses them with six row
classes.

K2.  k2_plan() restates quant_colwise_dispatch's plan() for both passes, k2_position() the walk of col_amax (row block, loop iteration, unroll slot, wave, row group), and
k2_matrix() builds a matrix with a dominant diagonal: column c has its strict maximum at row c mod rows, and the column kinds alternate along the columns."""
import zlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from oracle import qspec_numpy as Q

EPV = {0: 8, 1: 8, 2: 4}
DT = ("bf16", "fp16", "f32")
ALL_COLUMNS_MAX = 2048                       # elements: up to here every column of a layout's smallest and largest width is planted
GENERIC_WIDTHS = (333, 1003)
PLANT_G = 4.0                                # the gate under a planted u: silu(4) = 3.93, gelu(4) = 4.0, inside every clamp


def pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


# ---------------------------------------------------------------------------------------------------------------- the restated dispatches
@dataclass(frozen=True)
class Layout:
    family: str                   # "k1" | "rowmap" | "rownorm"
    tpr: int                      # threads per row; 0: the generic kernel
    vpt: int = 0                  # 16-byte vectors per thread
    variant: str = ""             # k1: "rpw2", "st16"; rowmap: "tpr256" (PQ_SILU_TPR=256 where 512 x 3 would run)

    def __str__(self):
        return f"{self.family}:" + ("generic" if not self.tpr else f"{self.tpr}x{self.vpt}") + (f":{self.variant}" if self.variant else "")


def k1_layout(code, cols, rpw=0, st16=0):
    """quant_rowwise_dispatch + launch_rowwise_vec on a dense, aligned operand (ld = cols, 16-byte aligned bases)"""
    epv = EPV[code]
    if cols <= 0 or cols % epv or cols // epv > 256 * 32:
        return Layout("k1", 0)
    nvec = cols // epv
    if nvec <= 64 * 8:
        vpt = pow2((nvec + 63) // 64)
        if rpw == 2:
            return Layout("k1", 64, vpt, "rpw2")
        if st16 and epv == 8 and nvec % 2 == 0 and cols % 16 == 0 and 2 <= vpt <= 8:
            return Layout("k1", 64, vpt, "st16")
        return Layout("k1", 64, vpt)
    return Layout("k1", 256, pow2((nvec + 255) // 256))


def rowmap_layout(code, cols, wide, silu_tpr=0):
    epv = EPV[code]
    if cols <= 0 or cols % epv or cols // epv > 256 * 16:
        return Layout("rowmap", 0)
    nvec = cols // epv
    tpr = 64 if nvec <= 64 * 4 else 256
    vpt = 1
    while vpt * tpr < nvec:
        vpt <<= 1
    if tpr == 64:
        return Layout("rowmap", 64, min(vpt, 4))
    if wide and 1024 < nvec <= 1536:
        return Layout("rowmap", 512, 3) if silu_tpr != 256 else Layout("rowmap", 256, vpt, "tpr256")
    return Layout("rowmap", 256, min(vpt, 16))


def rownorm_layout(code, cols, wave_max=256):
    epv = EPV[code]
    if cols % epv or cols // epv > 256 * 16:
        return Layout("rownorm", 0)
    nvec = cols // epv
    wave = nvec <= min(max(wave_max, 0), 512)
    vpt = 1
    while vpt * (64 if wave else 256) < nvec:
        vpt <<= 1
    return Layout("rownorm", 64 if wave else 256, vpt)


def family(form):
    if form.name == "K1":
        return "k1"
    if form.name == "K2":
        return "k2"
    return "rownorm" if form.vecs else "rowmap"


# the switch settings under which each dispatch is walked (pq_set_option names -> values)
SWITCHES = {
    "k1": ({}, {"PQ_K1_RPW": 2}, {"PQ_K1_ST16": 1}),
    "rowmap": ({}, {"PQ_SILU_TPR": 256}),
    "rownorm": ({}, {"PQ_RMS_WAVE_MAX": 512}, {"PQ_RMS_WAVE_MAX": 0}),
}
MAX_NVEC = {"k1": 256 * 32, "rowmap": 256 * 16, "rownorm": 256 * 16}


def layout_of(form, code, cols, switches):
    fam = family(form)
    if fam == "k1":
        return k1_layout(code, cols, switches.get("PQ_K1_RPW", 0), switches.get("PQ_K1_ST16", 0))
    if fam == "rowmap":
        return rowmap_layout(code, cols, form.wide, switches.get("PQ_SILU_TPR", 0))
    return rownorm_layout(code, cols, switches.get("PQ_RMS_WAVE_MAX", 256))


@lru_cache(maxsize=None)
def _reach(fam, code, wide):
    """every layout of the family that SOME width reaches under SOME switch setting: layout -> (switches as a tuple, smallest nvec, largest nvec).  A layout that the
    default setting reaches is listed under the default; the vector layouts come from walking every legal vector count through the restated dispatch."""
    class F:                      # what layout_of reads of a form
        pass
    f = F()
    f.name, f.vecs, f.wide = {"k1": "K1", "rowmap": "", "rownorm": ""}[fam], (("w",) if fam == "rownorm" else ()), wide
    out = {}
    for sw in SWITCHES[fam]:
        for nvec in range(1, MAX_NVEC[fam] + 1):
            lay = layout_of(f, code, nvec * EPV[code], sw)
            assert lay.tpr, (fam, nvec)
            if lay in out and out[lay][0] != tuple(sorted(sw.items())):
                continue
            lo, hi = (out[lay][1], out[lay][2]) if lay in out else (nvec, nvec)
            out[lay] = (tuple(sorted(sw.items())), min(lo, nvec), max(hi, nvec))
    return out


def reachable(form, code):
    return _reach(family(form), code, bool(form.wide))


# ---------------------------------------------------------------------------------------------------------------- positions
def position(lay, code, col):
    """where column `col` of a row lives in the layout: the bookkeeping a failure message is made of"""
    epv = EPV[code]
    v, e = divmod(int(col), epv)
    if not lay.tpr:                               # the generic kernels: 256 threads; the norms walk by vector (vector v on thread v mod 256), the others element by element
        t = (v if lay.family == "rownorm" else int(col)) % 256
        return dict(col=int(col), vector=v, elem=e, lane=t % 64, wave=t // 64, slot=(v if lay.family == "rownorm" else int(col)) // 256)
    lane = v % lay.tpr
    return dict(col=int(col), vector=v, elem=e, lane=lane % 64, wave=lane // 64, slot=v // lay.tpr)


def describe(lay, code, col):
    p = position(lay, code, col)
    return f"column {p['col']} = vector {p['vector']} element {p['elem']}: wave {p['wave']} lane {p['lane']} slot {p['slot']} of {lay}"


def live_slots(lay, nvec, lane):
    """the slots of thread `lane` (0 .. TPR - 1) whose vector lies inside the row"""
    return [s for s in range(lay.vpt) if s * lay.tpr + lane < nvec]


def dead_slot_classes(lay, nvec):
    """which kinds of dead slots the width leaves: part of a wave, whole waves, a whole slot index"""
    out = set()
    for s in range(lay.vpt):
        live = [s * lay.tpr + t < nvec for t in range(lay.tpr)]
        if not any(live):
            out.add("slot")
            continue
        for w in range(lay.tpr // 64):
            n = sum(live[64 * w:64 * w + 64])
            if 0 < n < 64:
                out.add("part of a wave")
            elif n == 0:
                out.add("whole waves")
    return out


# ---------------------------------------------------------------------------------------------------------------- the cases of the planted maximum
@dataclass(frozen=True)
class Case:
    cols: int
    mode: str                     # "all": every column planted; "wide": the lanes, slot edges and last vectors of one layout
    layout: Layout
    switches: tuple               # ((name, value), ...)

    @property
    def id(self):
        sw = "-".join(f"{n}={v}" for n, v in self.switches)
        return f"{self.layout}-{self.cols}" + (f"-{sw}" if sw else "")


def is_layernorm(form):
    return form.name.startswith(("K1l", "K1al", "K1pl"))


def min_cols(form, code):
    return 8 if is_layernorm(form) else EPV[code]


def wide_nvec(lay, lo, hi):
    n = (lay.vpt - 1) * lay.tpr + (37 if lay.tpr == 64 else 101)
    if n > hi:                                                    # (PQ_SILU_TPR=256 at 1025 .. 1536 vectors: 256 x 8 with slot 4 partly live and three dead slot indices)
        n = lo + 100
    return n + 1 if lay.variant == "st16" else n                  # (the 16-byte-store kernel needs an even vector count)


def cases(form, code):
    """the designed widths of a form and dtype: every layout its dispatch can reach, and the generic kernel"""
    epv, out = EPV[code], []
    for lay, (sw, lo, hi) in sorted(reachable(form, code).items(), key=lambda kv: (kv[1][1], str(kv[0]))):
        lo = max(lo, -(-min_cols(form, code) // epv))
        if lay.variant == "st16":
            lo += lo % 2
        if hi * epv <= ALL_COLUMNS_MAX:
            out += [Case(n * epv, "all", lay, sw) for n in sorted({lo, hi})]
        else:
            n = wide_nvec(lay, lo, hi)
            assert lo <= n <= hi, (lay, lo, n, hi)
            out.append(Case(n * epv, "wide", lay, sw))
    out += [Case(c, "all", Layout(family(form), 0), ()) for c in GENERIC_WIDTHS]
    return out


def plant_operand(form):
    if "u" in form.mats:
        return "u"
    if "r" in form.mats and form.name in ("K1oq", "K1pang"):
        return "r"
    return form.mats[0]


def is_norm(form):
    return bool(form.vecs) and form.name != "K1oq"


def positive_only(form):
    return form.name.startswith("K1u")


def planted_rows(form, code, case):
    """[(column, kind)] — one row each; kind in '+', '-', 'nan', '+inf', '-inf'"""
    epv, cols, lay = EPV[code], case.cols, case.layout
    nvec = -(-cols // epv)
    width = lambda v: min(epv, cols - v * epv)                        # (a ragged last vector of the generic kernels)

    def specials(v):
        if is_layernorm(form):
            return []
        inf = [(v * epv + (5 * v + 2) % width(v), "+inf" if positive_only(form) or v % 2 == 0 else "-inf")]
        return inf if is_norm(form) else [(v * epv + (3 * v + 1) % width(v), "nan")] + inf

    finite = lambda c: [(c, "+")] if positive_only(form) else [(c, "+"), (c, "-")]
    rows = []
    if case.mode == "all":
        for c in range(cols):
            rows += finite(c)
        for v in range(nvec):
            rows += specials(v)
        return rows
    for v in wide_vectors(lay, nvec):
        rows += finite(v * epv + (3 * v + 1) % epv) + specials(v)
    return rows


def wide_vectors(lay, nvec):
    """the planted vectors of a wide layout: every lane's first and last live slot, every slot's first and last live lane of each wave, the last vector and its neighbour"""
    tpr, out = lay.tpr, {nvec - 1, nvec - 2}
    for t in range(tpr):
        ls = live_slots(lay, nvec, t)
        out |= {ls[0] * tpr + t, ls[-1] * tpr + t}
    for s in range(lay.vpt):
        for w in range(tpr // 64):
            lw = [t for t in range(64 * w, 64 * w + 64) if s * tpr + t < nvec]
            if lw:
                out |= {s * tpr + lw[0], s * tpr + lw[-1]}
    return sorted(out)


_KIND_VALUE = {"+": 1.0, "-": -1.0, "nan": np.nan, "+inf": np.inf, "-inf": -np.inf}


def _seed(*parts):
    return zlib.crc32(" ".join(map(str, parts)).encode())


def background(form, code, cols):
    """one row per matrix operand and the [cols] parameters, as float32: magnitudes in [0.25, 1] with a random sign (secondary matrices a quarter of that: sums stay of
    order 1), weights 1 +- 0.1 (the Gemma gains 1 + w then lie around 2), biases +- 0.05"""
    rng = np.random.default_rng(_seed("amax", form.name, code, cols))
    prim, out = plant_operand(form), {}
    for n in form.mats:
        a = (rng.uniform(0.25, 1.0, cols) * rng.choice((-1.0, 1.0), cols)).astype(np.float32)
        out[n] = a if n == prim or n == "g" else a * np.float32(0.25)
    for n in form.vecs:
        out[n] = (rng.uniform(-0.05, 0.05, cols) if n.startswith("b") else 1.0 + rng.uniform(-0.1, 0.1, cols)).astype(np.float32)
    return out


def planted_inputs(form, code, case):
    """(inputs as storage bits, [(column, kind)] per row)"""
    rows = planted_rows(form, code, case)
    bg, prim = background(form, code, case.cols), plant_operand(form)
    col = np.array([c for c, _ in rows])
    idx = np.arange(len(rows))
    inp = {}
    for n in form.mats:
        a = np.broadcast_to(bg[n], (len(rows), case.cols)).copy()
        if n == prim:
            mag = (256.0 + 32.0 * (idx % 8)).astype(np.float32)
            with np.errstate(invalid="ignore"):
                a[idx, col] = np.array([_KIND_VALUE[k] for _, k in rows], np.float32) * mag
        elif n == "g":
            a[idx, col] = PLANT_G
        inp[n] = Q.from_f32(a, code)
    for n in form.vecs:
        inp[n] = Q.from_f32(bg[n], code)
    return inp, rows


def h_of(form, inp, want, code):
    """the activation whose row maximum the form quantises, as float32"""
    if "h" in want:
        return Q.to_f32(want["h"], code)
    if form.name == "K1oq":
        return Q.to_f32(want["s"], code)
    if form.name == "K1s_amax_halves":
        from oracle import c_oracle as C
        return Q.to_f32(C.silu_mul_quant_rowwise(inp["g"], inp["u"], code)[2], code)
    return Q.to_f32(inp[form.mats[0]], code)


def elementwise_with_h(form):
    return family(form) == "rowmap" and "h" in form.outs


def reference(form, inp, rows, code):
    """the form's CPU specification on the planted operands.  An elementwise form with a stored h (K1s, K1g, K1gg, K1u: up to 1.8 us per element on the CPU) is evaluated
    where its rows differ — the shared background row once and the planted pairs as a one-column matrix, both through form.ref — and quantised with the oracle's Q1-Q6;
    tests/test_amax_design_host.py holds that to form.ref on the whole operands."""
    if not elementwise_with_h(form):
        return form.ref(inp, code)
    col = np.array([c for c, _ in rows])
    idx = np.arange(len(rows))
    bg = background(form, code, inp[form.mats[0]].shape[1])
    hb = form.ref({n: Q.from_f32(bg[n][None, :], code) for n in form.mats}, code)["h"]
    hp = form.ref({n: np.ascontiguousarray(inp[n][idx, col][:, None]) for n in form.mats}, code)["h"]
    h = np.broadcast_to(hb, inp[form.mats[0]].shape).copy()
    h[idx, col] = hp[:, 0]
    q, sc = Q.quantize(h, code, 1)
    return dict(q=q, sc=sc, h=h)


def check_planted(form, inp, rows, want, code, what=""):
    """the host condition that makes a GPU comparison mean "position p(i) was seen": per row the strict maximum of the |h| bit patterns is at p(i); a finite one exceeds the
    runner-up by a factor of 4 at least; the scale computed without that element differs from the row's.  A form with two groups (q2 / sc2 from h2) is held to it in both."""
    if "h2" in want:
        _check_planted_h(Q.to_f32(want["h2"], code), rows, what + " (second group)")
    return _check_planted_h(h_of(form, inp, want, code), rows, what)


def _check_planted_h(h, rows, what):
    b = np.abs(h).view(np.uint32) & np.uint32(0x7FFFFFFF)
    col = np.array([c for c, _ in rows])
    idx = np.arange(len(rows))
    top = b[idx, col].copy()
    assert np.array_equal(b.argmax(axis=1), col), f"{what}: the row maximum is not at the planted column in rows {np.flatnonzero(b.argmax(axis=1) != col)[:5].tolist()}"
    b[idx, col] = 0
    second = b.max(axis=1) if b.shape[1] > 1 else np.zeros(len(rows), np.uint32)
    assert (top > second).all(), f"{what}: the planted maximum is not strict in rows {np.flatnonzero(top <= second)[:5].tolist()}"
    finite = top < 0x7F800000
    ratio = top[finite].view(np.float32) / np.maximum(second[finite].view(np.float32), np.float32(1e-30))
    assert (ratio >= 4).all(), f"{what}: maximum / runner-up is {ratio.min()}"
    sc = lambda bits_: Q.quantize_rows_with_amax(np.zeros((len(rows), 1), np.float32), 2, bits_)[1].view(np.uint32)
    same = sc(top) == sc(second)
    assert not same.any(), f"{what}: the scale does not depend on the planted element in rows {np.flatnonzero(same)[:5].tolist()}"
    return top


def explain(form, code, case, rows, bad_rows):
    """the positions behind a set of mismatching rows"""
    return "; ".join(f"row {i} (planted {rows[i][1]}): {describe(case.layout, code, rows[i][0])}" for i in list(bad_rows)[:4])


# ---------------------------------------------------------------------------------------------------------------- tail slots
TAIL_NVEC = (67, 325, 600)                   # one wave x 2: part of a wave dead; 256 x 2: part of a wave and whole waves dead; 256 x 4: a whole slot index dead as well
TAIL_CLASSES = {67: {"part of a wave"}, 325: {"part of a wave", "whole waves"}, 600: {"part of a wave", "whole waves", "slot"}}
PAD = 64                                     # columns behind the row's end in the wider buffer that holds a matrix operand
ROW_CLASSES = ("ordinary", "zero under the special element", "all zero (eps = 0: rs = Inf)", "NaN row", "maximum in the last live vector", "last live vector all zero")
ROWS_PER_CLASS = 2


def special_values(code):
    """name -> float32 value: each goes into an element of its own"""
    big = {0: 3.3895314e38, 1: 65504.0, 2: 3.4028235e38}[code]
    sub = {0: 2.0 ** -130, 1: 2.0 ** -20, 2: 2.0 ** -140}[code]                    # subnormal in the storage dtype
    return (("+inf", np.inf), ("-inf", -np.inf), ("nan", np.nan), ("+0", 0.0), ("-0", -0.0), ("max", big), ("subnormal", sub))


def tail_cases(form, code):
    """(nvec, parameter name, 'last' | 'first', special name, element index)"""
    out = []
    for nvec in TAIL_NVEC:
        for pi, n in enumerate(form.vecs):
            for where in ("last", "first"):
                for k, (name, _) in enumerate(special_values(code)):
                    out.append((nvec, n, where, name, (k + pi) % EPV[code]))
    return out


def tail_inputs(form, code, nvec, pname, where, sname, elem):
    """inputs as storage bits for one tail case: ROWS_PER_CLASS rows of each class, the parameter `pname` with the special value in element `elem` of its last (first)
    vector.  Returns (inputs, the special's column, the class of each row)."""
    epv = EPV[code]
    cols = nvec * epv
    c_sp = (cols - epv if where == "last" else 0) + elem
    rng = np.random.default_rng(_seed("tail", form.name, code, nvec, pname, where, sname))
    cls = [c for c in range(len(ROW_CLASSES)) for _ in range(ROWS_PER_CLASS)]
    inp, prim = {}, plant_operand(form)
    for j, n in enumerate(form.mats):
        a = (rng.uniform(0.25, 1.0, (len(cls), cols)) * rng.choice((-1.0, 1.0), (len(cls), cols))).astype(np.float32)
        for i, c in enumerate(cls):
            if c == 1:
                a[i, c_sp] = 0.0
            elif c == 2:
                a[i] = 0.0
            elif c == 3 and j == 0:
                a[i, (7 * i + 3) % cols] = np.nan
            elif c == 4 and n == prim:
                a[i, cols - epv + (i % epv)] *= 64.0
            elif c == 5:
                a[i, cols - epv:] = 0.0
        inp[n] = Q.from_f32(a, code)
    val = dict(special_values(code))[sname]
    for n in form.vecs:
        v = (rng.uniform(-0.05, 0.05, cols) if n.startswith("b") else 1.0 + rng.uniform(-0.1, 0.1, cols)).astype(np.float32)
        if n == pname:
            v[c_sp] = val
        inp[n] = Q.from_f32(v, code)
    return inp, c_sp, cls


def pad_values(code, rows):
    """what the columns just behind a row's end hold: NaN and huge values, alternating"""
    big = {0: 3.0e38, 1: 60000.0, 2: 3.0e38}[code]
    a = np.empty((rows, PAD), np.float32)
    a[:, 0::2], a[:, 1::2] = np.nan, big
    a[:, 3::4] = -big
    return Q.from_f32(a, code)


# ---------------------------------------------------------------------------------------------------------------- K2: column maxima
K2_AMAX_WAVES, K2_AMAX_UNROLL, K2_COL_UNROLL = 16, 8, 8                  # kAmaxWaves, kAmaxUnroll, kColUnroll (quant_kernels.hip)
K2_KINDS = ("ordinary", "zero", "nan", "inf", "subnormal", "huge", "allones")
# The kinds alternate along the columns, so every 64-lane encode strip mixes columns that allow the division-free encode with columns that forbid it, and col_encode's
# wave-uniform choice therefore takes the true-division path in EVERY strip of these matrices (the division-free encode is held by the Gaussian K2 tests).  What forbids it:
# NaN / Inf; for bf16 / f32 a subnormal amax and the largest finite one (scales outside scale_fast_ok's 2^-60 .. 2^60; fp16 has no value whose scale leaves that range);
# "allones": an amax whose scale amax / 127 has an all-ones significand.  For f32 that is 0x437DFFFF (253.99998 -> scale 0x3FFFFFFF).  NO bf16 or fp16 value has such a
# scale (all 2^15 magnitudes of either format enumerated in tests/test_amax_design_host.py), so for the 16-bit types an "allones" column is one more ordinary column.
K2_ALLONES_F32 = 0x437DFFFF
# twice as many columns as rows (+ a ragged rest): every row holds the maximum of two columns whose kinds differ, so no row is left to the all-zero columns alone
K2_VEC = dict(rows=2 * 1024 + 8 * 16 + 5, cols=4368)                     # 546 16-bit / 1092 f32 vectors: no multiple of 8 or 64, so the clamped strips of both passes are live
K2_SCALAR = dict(rows=301, cols=603)
# (PQ_K2_BLOCKS_A, PQ_K2_BLOCKS_E): vector path — 1024-row amax blocks (three, the last one short) by default and at 100000; ONE block of three loop iterations at 30
K2_SWITCHES = {"vec": ((0, 0), (100000, 100000), (30, 7)), "scalar": ((0, 0), (100000, 100000), (3, 2), (40, 9))}


def k2_plan(code, rows, cols, blocks_a=0, blocks_e=0):
    """quant_colwise_dispatch's plan() for both passes on a dense, aligned operand: (vector path?, rows per block of the amax pass, of the encode pass)"""
    epv = EPV[code]
    vec = cols % epv == 0
    ncolv = cols // epv if vec else cols
    strips = -(-ncolv // 64)
    strips_a = -(-ncolv // 8) if vec else strips

    def plan(target, nstrips, batch):
        r = -(-rows * nstrips // target)
        r = -(-r // batch) * batch
        return min(max(r, batch), 1 << 20)
    return vec, plan(blocks_a or 256, strips_a, 8 * K2_AMAX_WAVES * K2_AMAX_UNROLL if vec else 4 * K2_COL_UNROLL), plan(blocks_e or 512, strips, 4 * K2_COL_UNROLL)


def k2_position(code, rows, cols, r, c, blocks_a=0, blocks_e=0):
    """where element (r, c) sits in col_amax's walk: row block, loop iteration, unroll slot, wave, row group; column strip and lane"""
    vec, rpb_a, _ = k2_plan(code, rows, cols, blocks_a, blocks_e)
    blk, rel = divmod(int(r), rpb_a)
    if vec:
        it, rel = divmod(rel, 8 * K2_AMAX_WAVES * K2_AMAX_UNROLL)
        u, rel = divmod(rel, 8 * K2_AMAX_WAVES)
        w, rsub = divmod(rel, 8)
        cv, e = divmod(int(c), EPV[code])
        return dict(block=blk, iteration=it, unroll=u, wave=w, row_group=rsub, strip=cv // 8, sub=cv % 8, elem=e, row=int(r), col=int(c))
    it, rel = divmod(rel, 4 * K2_COL_UNROLL)
    u, w = divmod(rel, 4)
    return dict(block=blk, iteration=it, unroll=u, wave=w, row_group=0, strip=int(c) // 64, sub=int(c) % 64, elem=0, row=int(r), col=int(c))


def k2_describe(code, rows, cols, r, c, blocks_a=0, blocks_e=0):
    p = k2_position(code, rows, cols, r, c, blocks_a, blocks_e)
    return (f"column {c} (maximum at row {r}): amax row block {p['block']} iteration {p['iteration']} unroll slot {p['unroll']} wave {p['wave']} row group {p['row_group']}, "
            f"column strip {p['strip']} lane / vector {p['sub']} element {p['elem']}")


def k2_kind(c):
    return K2_KINDS[(c + c // 64) % len(K2_KINDS)] if c % 11 != 3 else "ordinary"         # (the walk shifts by one per 64 columns; one column in eleven is ordinary whatever it says)


def k2_max_row(c, rows):
    return c % rows


def k2_matrix(code, rows, cols):
    """a dominant diagonal: column c has its strict maximum of |x| at row c mod rows; by rows the same matrix is a K1 case.  Storage bits."""
    rng = np.random.default_rng(_seed("k2", code, rows, cols))
    a = (rng.uniform(0.25, 1.0, (rows, cols)) * rng.choice((-1.0, 1.0), (rows, cols))).astype(np.float32)
    sub_small = {0: 2.0 ** -133, 1: 2.0 ** -24, 2: 2.0 ** -146}[code]
    sub_top = {0: 2.0 ** -128, 1: 2.0 ** -16, 2: 2.0 ** -130}[code]
    big = {0: 3.3895314e38, 1: 65504.0, 2: 3.4028235e38}[code]
    for c in range(cols):
        k, r = k2_kind(c), k2_max_row(c, rows)
        sgn = np.float32(-1.0 if (c + r) % 2 else 1.0)
        if k == "allones" and code == 2:
            a[r, c] = sgn * np.array([K2_ALLONES_F32], np.uint32).view(np.float32)[0]
        elif k in ("ordinary", "allones"):
            a[r, c] = sgn * np.float32(200.0 + 25.0 * (c % 9))
        elif k == "zero":
            a[:, c] = 0.0
        elif k == "nan":
            a[r, c] = np.nan
        elif k == "inf":
            a[r, c] = sgn * np.float32(np.inf)
        elif k == "subnormal":
            a[:, c] = np.where(rng.random(rows) < 0.5, np.float32(sub_small), np.float32(0.0)) * np.sign(a[:, c])
            a[r, c] = sgn * np.float32(sub_top)
        else:
            a[:, c] *= np.float32(big / 1024.0)
            a[r, c] = sgn * np.float32(big)
    return Q.from_f32(a, code)
