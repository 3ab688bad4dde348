"""-m gpu: ONE TABLE of dequant-epilogue implementations (QSPEC E1-E4), each run on the designed operands of tests/epilogue_domain.py — NaN, Inf, zero, subnormal, tiny,
huge and negative scales; accumulators that are ties of the 16-bit cast, fp16 fold hazards, 0 (the 0 * Inf case) and odd integers above 2^24; biases with +-0, +-Inf, NaN
and near-overflow values — for bf16, fp16 and f32 outputs, with and without bias.  Every result goes through tests.gpu_util.same_f against the numpy oracle (NaNs as a
class, every other element bit for bit, signs of zero included) and, where a switch is forced, through torch.equal on the bits against the default dispatch of the same
process.  tests/test_epilogue_domain_host.py (CPU) holds that the operands populate every class and that the two oracles agree on them.

Each row asserts, where the library can tell it, that its shape really takes the path it names (pq_gemm_variant_name, pq_qlinear_workspace_bytes, pq_kslabs_way_name,
pq_grouped_variant_name, pq_grouped_stream_plan_name).  Shapes and switch values are ones the older files already launch (test_gpu_parity.py, test_gpu_switch_paths.py,
test_gpu_grouped.py, test_gpu_grouped_stream.py); only the VALUES are new.

The second half drives the same domain end to end from activations: NaN, +-Inf, all-zero, subnormal and largest-finite tokens through qlinear / qlinear_dyn."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from oracle import qspec_numpy as Q
from tests import epilogue_domain as D
from tests.gpu_util import TD, same, same_f, to_gpu
from tests.test_gpu_grouped import TILES

pytestmark = pytest.mark.gpu

SEED, BIAS_SEED = 5, 7
N, K = 520, 1280                        # K = 2 * 5 * 128: two split-K slices of five K-tiles; all-127 rows against all-127 weights pass 2^24 from K = 1043 on
CASES = [(code, hb) for code in (0, 1, 2) for hb in (False, True)]
VARIANT_NAME = {"generic": b"generic64", "sp256_16": b"sp256_16x16x64", "sp128_16": b"sp128x256_16x16x64", "sp128x128": b"sp128x128_16x16x64",
                "ring128": b"ring128_16x16x64", "ring64x128": b"ring64x128_16x16x64", "ring64x64": b"ring64x64_16x16x64", "ring128x160": b"ring128x160_16x16x64",
                "auto": b"ring64x64_16x16x64"}           # (auto at 300 x 520: the mid-M planner's 64 x 64 ring tile on a 256-CU device)
TILE_VARIANTS = ["auto", "sp256_16", "sp128_16", "sp128x128", "ring128", "ring64x128", "ring64x64", "ring128x160"]


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    from protoquant_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return protoquant_amd


class Problem:
    """build(M, n, K) once: operands on both sides, the six references, and (lazily) the bits of the default dispatch"""

    def __init__(self, M, n=N):
        self.M, self.N, self.K = M, n, K
        self.a, self.b, self.acc, self.xs, self.ws = D.build(M, n, K, SEED)
        self.ag, self.bg, self.xg, self.wg = (torch.from_numpy(t).cuda() for t in (self.a, self.b, self.xs, self.ws))
        self.bias = {code: D.bias(n, code, BIAS_SEED) for code in (0, 1, 2)}
        self.bias_g = {code: to_gpu(self.bias[code], code) for code in (0, 1, 2)}
        self.want = {(code, hb): Q.epilogue(self.acc, self.xs, self.ws, self.bias[code] if hb else None, code) for code, hb in CASES}
        self._default = None

    def args(self, code, hb):
        return (self.ag, self.xg, self.bg, self.wg, self.bias_g[code] if hb else None, TD[code])

    def default(self, pq):
        """qlinear_s8 under no switch at all (call before forcing one)"""
        if self._default is None:
            self._default = {c: pq.qlinear_s8(*self.args(*c)) for c in CASES}
            for c in CASES:
                same_f(self._default[c], self.want[c], c[0], f"default dispatch {self.M}x{self.N}x{self.K} {c}")
        return self._default


_PROBLEMS = {}


def problem(M, n=N):
    if (M, n) not in _PROBLEMS:
        _PROBLEMS[(M, n)] = Problem(M, n)
    return _PROBLEMS[(M, n)]


def _ibits(t):
    """the bit patterns, with every NaN replaced by one pattern.  QSPEC v2 leaves open the payload and sign of a NaN that arithmetic produces, and on an MI355X the paths do
    differ there: with a literal comparison every forced path differed from the default dispatch at bf16 with bias, on NaN elements only (same_f had pinned all others
    and the NaN positions).  The shipped ISA adds the bias with either operand first (v_add_f32 bias, t in the direct epilogues), and an add of two NaNs keeps one
    operand's sign; which elements differ, and why fp16 and f32 do not show it, has not been traced further.  Which of NaN or Inf, and the sign of a zero, stay bits."""
    t = t.contiguous()
    i = t.view(torch.int32 if t.element_size() == 4 else torch.int16)
    return torch.where(torch.isnan(t), torch.full_like(i, 0x7FC0 << (16 if t.element_size() == 4 else 0)), i)


def _both(y, p, c, default, what):
    """against the oracle (same_f), then against the default dispatch with NaNs as a class.  same_f has already pinned the NaN positions and every other bit of BOTH sides
    to the oracle, so the second comparison can only restate that: it is kept as a cross-check of the harness (a stale reference, a wrong case key), not as a second proof"""
    same_f(y, p.want[c], c[0], what)
    if default is not None:
        assert torch.equal(_ibits(y), _ibits(default[c])), f"{what}: bits differ from the default dispatch"


def _lib():
    from protoquant_amd import _lib as m
    return m.lib()


# ---------------------------------------------------------------- the table: one runner per kind of path
def run_variant(pq, pq_opt, variant, extra=()):
    """a tile kernel's staged epilogue (interior tiles of 300 x 520) and the direct one next to it (the ragged tiles), y and — the SWAP / BIAS == 2 specialisations — y^T"""
    p = problem(300)
    d = p.default(pq)
    pq_opt("PQ_FORCE_VARIANT", "" if variant == "auto" else variant)
    for name, value in extra:
        pq_opt(name, value)
    assert _lib().pq_gemm_variant_name(p.M, p.N, p.K, p.K, p.K) == VARIANT_NAME[variant]
    assert _lib().pq_qlinear_workspace_bytes(p.M, p.N, p.K) == 0, "single pass"
    same(pq.int_mm(p.ag, p.bg), p.acc, f"{variant} acc")
    for c in CASES:
        _both(pq.qlinear_s8(*p.args(*c)), p, c, d, f"{variant} {extra} {c}")
        _both(pq.qlinear_s8_t(*p.args(*c)).t().contiguous(), p, c, d, f"{variant} {extra} y^T {c}")


def run_unaligned(pq, pq_opt, variant):
    """outputs the staged 16-byte stores refuse (a view at an odd element offset of a wider buffer), scale vectors 4 bytes off a 16-byte line: the direct epilogue of every
    tile; and N = 521 contiguous, whose odd leading dimension takes the staged epilogue's element-aligned stores (y_any_align) or, with PQ_EPI_ANY_ALIGN=0, the direct one"""
    p = problem(300)
    d = p.default(pq)
    p1 = problem(300, 521)
    d1 = p1.default(pq)
    pq_opt("PQ_FORCE_VARIANT", "" if variant == "auto" else variant)
    assert _lib().pq_gemm_variant_name(p.M, p.N, p.K, p.K, p.K) == VARIANT_NAME[variant]
    xs_off = torch.from_numpy(np.concatenate([[7.0], p.xs]).astype(np.float32)).cuda()[1:]
    ws_off = torch.from_numpy(np.concatenate([[7.0], p.ws]).astype(np.float32)).cuda()[1:]
    assert xs_off.data_ptr() % 16 == 4 and ws_off.data_ptr() % 16 == 4
    for c in CASES:
        code, hb = c
        bias = p.bias_g[code] if hb else None
        _both(pq.qlinear_s8(p.ag, xs_off, p.bg, ws_off, bias, TD[code]), p, c, d, f"{variant} scales + 4 bytes {c}")
        big = torch.full((p.M, p.N + 8), 7.0, dtype=TD[code], device="cuda")
        pq.qlinear_s8(p.ag, p.xg, p.bg, p.wg, bias, TD[code], out=big[:, 1:p.N + 1])
        _both(big[:, 1:p.N + 1].contiguous(), p, c, d, f"{variant} out at an odd element offset {c}")
        assert bool((big[:, 0] == 7.0).all()) and bool((big[:, p.N + 1:] == 7.0).all()), "wrote outside its view"
    for setting in ("", "0"):
        pq_opt("PQ_EPI_ANY_ALIGN", setting)
        for c in CASES:
            _both(pq.qlinear_s8(*p1.args(*c)), p1, c, d1, f"{variant} N = 521, PQ_EPI_ANY_ALIGN={setting!r} {c}")


def run_splitk(pq, pq_opt):
    """the two-pass split-K: int32 slabs, then the reduction pass's own epilogue"""
    p = problem(300)
    d = p.default(pq)
    pq_opt("PQ_FORCE_SPLITK", "2")
    assert _lib().pq_qlinear_workspace_bytes(p.M, p.N, p.K) == 2 * p.M * p.N * 4
    for c in CASES:
        _both(pq.qlinear_s8(*p.args(*c)), p, c, d, f"PQ_FORCE_SPLITK=2 {c}")


def run_fsk(pq, pq_opt, symmetric):
    """the fused split-K hand-over forms: the ticket form, and the symmetric exchange"""
    p = problem(300)
    d = p.default(pq)
    pq_opt("PQ_FSK", "2")
    pq_opt("PQ_FSK_SYMMETRIC", "1" if symmetric else "")
    tiles = ((p.M + 255) // 256) * ((p.N + 255) // 256)
    assert _lib().pq_qlinear_workspace_bytes(p.M, p.N, p.K) == ((tiles * 4 * 2 + 255) // 256) * 256 + tiles * 256 * 256 * 4
    for c in CASES:
        for rep in range(2):            # (the launcher re-zeroes the hand-over flags: a second call on the same workspace)
            _both(pq.qlinear_s8(*p.args(*c)), p, c, d, f"PQ_FSK=2 symmetric={symmetric} {c} rep {rep}")


def run_skinny(pq, pq_opt, M, stage):
    """the weight-streaming kernel, staged and (PQ_SKINNY_STAGE=0) unstaged; with EPI_STORE_T through qlinear_s8_t"""
    p = problem(M)
    d = p.default(pq)
    assert _lib().pq_gemm_variant_name(p.M, p.N, p.K, p.K, p.K) == b"skinny_16x16x64"
    if not stage:
        assert M > 1, "const bool stage = opt().skinny_stage && M > 1"
        pq_opt("PQ_SKINNY_STAGE", "0")
    for c in CASES:
        _both(pq.qlinear_s8(*p.args(*c)), p, c, d, f"skinny M={M} stage={stage} {c}")
        _both(pq.qlinear_s8_t(*p.args(*c)).t().contiguous(), p, c, d, f"skinny M={M} stage={stage} EPI_STORE_T {c}")


def run_kslabs(pq, pq_opt, G):
    """stacked K-slabs walked in place by the planner's ring tile"""
    p = problem(300)
    d = p.default(pq)
    kps = p.K // G
    stacked = torch.from_numpy(np.ascontiguousarray(p.a.reshape(p.M, G, kps).transpose(1, 0, 2))).cuda()
    L = _lib()
    need = L.pq_qlinear_kslabs_workspace_bytes_for(stacked.data_ptr(), kps, p.M * kps, kps, p.bg.data_ptr(), p.K, p.M, p.N, p.K)
    way = L.pq_kslabs_way_name(stacked.data_ptr(), kps, p.M * kps, kps, p.bg.data_ptr(), p.K, p.M, p.N, p.K, need)
    assert way == b"in place: ring64x64" and need == 0, (way, need)
    for c in CASES:
        code, hb = c
        _both(pq.qlinear_s8_kslabs(stacked, p.xg, p.bg, p.wg, p.bias_g[code] if hb else None, TD[code]), p, c, d, f"kslabs G={G} {c}")


class Grouped:
    """the rows of build(M, ...) dealt to E = 3 experts (the middle one empty); expert e's weight rows, scales and bias are those of the dense problem rotated by 5 e
    (bias: 7 e) columns, so every designed (v_n, ws) pair stays together and meets another bias; the reference is the per-expert oracle of tests/test_gpu_grouped.py"""

    def __init__(self, M, counts):
        from tests.test_gpu_grouped import _oracle
        self.d = problem(M)
        d = self.d
        assert sum(counts) == M
        self.p = {}
        self.want = {}
        for code, hb in CASES:
            p = dict(xq=d.a, idx=None, xs=d.xs, wq=np.stack([np.roll(d.b, 5 * e, axis=0) for e in range(3)]), ws=np.stack([np.roll(d.ws, 5 * e) for e in range(3)]),
                     bias=np.stack([np.roll(d.bias[code], 7 * e) for e in range(3)]) if hb else None,
                     off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), E=3, M=M, N=d.N, K=d.K, code=code)
            self.p[(code, hb)] = p
            self.want[(code, hb)] = _oracle(p)


_GROUPED = {}


def grouped(M, counts):
    key = (M, tuple(counts))
    if key not in _GROUPED:
        _GROUPED[key] = Grouped(M, counts)
    return _GROUPED[key]


def run_grouped(pq, pq_opt, tile):
    """the grouped GEMM's staged and direct epilogues, both tiles and the planner's own choice"""
    from tests.test_gpu_grouped import _launch
    g = grouped(300, [170, 0, 130])
    outs = {}
    for setting in dict.fromkeys(("", tile)):
        pq_opt("PQ_GROUPED_TILE", setting)
        name = _lib().pq_grouped_variant_name(3, 300, N, K)
        assert name == {"": b"grouped64x64_16x16x64", "64x128": b"grouped64x128_16x16x64", "64x64": b"grouped64x64_16x16x64"}[setting], name
        for c in CASES:
            y = _launch(pq, g.p[c])
            same_f(y, g.want[c], c[0], f"grouped tile {setting!r} {c}")
            outs[(setting, c)] = y
    for c in CASES:
        assert torch.equal(_ibits(outs[(tile, c)]), _ibits(outs[("", c)])), f"grouped tile {tile!r} {c}: bits differ from the default tile"


def run_grouped_stream(pq, pq_opt, forced):
    """the grouped weight-streaming kernel: the planner's plan, and a forced (K-slices, rows-per-block) pair"""
    from tests.test_gpu_grouped_stream import PLAN
    g = grouped(48, [20, 0, 28])
    L = _lib()
    outs = []
    for plan in [None] + ([forced] if forced else []):
        if plan is not None:
            pq_opt("PQ_GROUPED_STREAM_KS", plan[0]); pq_opt("PQ_GROUPED_STREAM_RB", plan[1])
        m = PLAN.match(L.pq_grouped_stream_plan_name(3, 48, N, K))
        assert m and int(m.group(1)) == 4, "48 rows: four token tiles"
        if plan is not None:
            assert int(m.group(3)) == plan[0] and int(m.group(2)) == 1, m.groups()           # (rb is 1 above 32 rows, as test_forced_plans_give_the_same_bits holds)
        got = {}
        for c in CASES:
            p = g.p[c]
            code = p["code"]
            y = pq.qlinear_s8_grouped_stream(torch.from_numpy(p["xq"]).cuda(), torch.from_numpy(p["xs"]).cuda(), torch.from_numpy(p["wq"]).cuda(), torch.from_numpy(p["ws"]).cuda(),
                                             to_gpu(p["bias"], code) if p["bias"] is not None else None, torch.from_numpy(p["off"]).cuda(), TD[code])
            same_f(y, g.want[c], code, f"grouped stream plan {m.group(0)} {c}")
            got[c] = y
        outs.append(got)
    for c in CASES:
        assert torch.equal(_ibits(outs[-1][c]), _ibits(outs[0][c])), f"forced plan {forced} {c}: bits differ from the planner's"


TABLE = (
    # the staged + direct edge epilogue of each tile kernel (gemm_s8_fast.hip's three call sites, gemm_s8_ring.hip), interior and ragged tiles of 300 x 520
    [(f"variant-{v}", run_variant, (v,)) for v in TILE_VARIANTS]
    + [("sp256_16-2deep-ring", run_variant, ("sp256_16", (("PQ_SP256_P3", "0"),))),
       ("generic", run_variant, ("generic",))]
    + [(f"unaligned-{v}", run_unaligned, (v,)) for v in TILE_VARIANTS + ["generic"]]
    + [("splitk-2-reduce", run_splitk, ()),
       ("fsk-2-ticket", run_fsk, (False,)),
       ("fsk-2-symmetric", run_fsk, (True,))]
    + [(f"skinny-M{M}", run_skinny, (M, True)) for M in (48, 17, 1)]
    + [(f"skinny-unstaged-M{M}", run_skinny, (M, False)) for M in (48, 17)]
    + [(f"kslabs-G{G}", run_kslabs, (G,)) for G in (2, 5)]
    + [(f"grouped-{t or 'planned'}", run_grouped, (t,)) for t in ("",) + tuple(TILES)]
    # (a forced RB is inert above 32 rows — the plan keeps rb = 1 at 48 — so the forced pair (4, 2) of test_forced_plans_give_the_same_bits moves the K-slices only)
    + [("grouped-stream-planned", run_grouped_stream, (None,)), ("grouped-stream-ks4", run_grouped_stream, ((4, 2),))]
)


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_epilogue_path(pq, pq_opt, row):
    _, runner, args = row
    runner(pq, pq_opt, *args)


def test_transposed_product_at_300_rows_runs_the_swapped_tile_form(pq):
    """qlinear_s8_t at M = 300 is the 520 x 300 problem with EPI_COL_FIRST (and EPI_BIAS_ROWS): the planner's tile for THAT orientation; at M = 17 the weight-streaming
    kernel stores transposed (EPI_STORE_T).  The token scale must still be applied first: with xs = 2.3e36 against ws = 2^-100 the other order is a number instead of Inf."""
    p = problem(300)
    assert _lib().pq_gemm_variant_name(p.N, p.M, p.K, p.K, p.K) == b"ring64x64_16x16x64"
    assert _lib().pq_gemm_variant_name(17, p.N, p.K, p.K, p.K) == b"skinny_16x16x64"
    for q in (p, problem(17)):
        for c in CASES:
            yt = pq.qlinear_s8_t(*q.args(*c))
            assert yt.shape == (q.N, q.M)
            same_f(yt.t().contiguous(), q.want[c], c[0], f"y^T M={q.M} {c}")


# ---------------------------------------------------------------- end to end from activations
E2E_K, E2E_N = 640, 520
KINDS = ("nan", "+inf", "-inf and nan", "zero", "subnormal", "largest")
TINY = {0: 2.0 ** -133, 1: 2.0 ** -24, 2: 1e-40}               # bf16's and fp16's smallest subnormal; an f32 subnormal
HUGE = {0: 3.3895313892515355e38, 1: 65504.0, 2: 3.4028234663852886e38}


def _plant(xf, row, kind, code):
    cols = xf.shape[1]
    if kind == "nan":
        xf[row, cols // 3] = np.nan
    elif kind == "+inf":
        xf[row, 5] = np.inf
    elif kind == "-inf and nan":
        xf[row, 1] = -np.inf
        xf[row, cols - 1] = np.nan
    elif kind == "zero":
        xf[row] = 0
    elif kind == "subnormal":
        xf[row] = 0
        xf[row, ::3] = TINY[code]
        xf[row, 1::7] = -TINY[code]
    elif kind == "largest":
        xf[row, 7] = HUGE[code]
        xf[row, 8] = -HUGE[code]


def _special_rows(M):
    if M == 300:
        return {3: "nan", 70: "+inf", 130: "-inf and nan", 200: "zero", 257: "subnormal", 299: "largest"}      # in different 64-row tiles, first and last tile included
    if M == 24:
        return {1: "nan", 5: "+inf", 9: "-inf and nan", 13: "zero", 17: "subnormal", 23: "largest"}
    raise AssertionError(M)


@pytest.fixture(scope="module")
def model(pq):
    """the weights of the three Linear layers (one per dtype) and their oracle codes"""
    out = {}
    for code in (0, 1, 2):
        rng = np.random.default_rng(40 + code)
        w = Q.from_f32((rng.standard_normal((E2E_N, E2E_K)) * 0.05).astype(np.float32), code)
        b = Q.from_f32(rng.standard_normal(E2E_N).astype(np.float32), code)
        lin = torch.nn.Linear(E2E_K, E2E_N, bias=True, device="cuda", dtype=TD[code])
        with torch.no_grad():
            lin.weight.copy_(to_gpu(w, code)); lin.bias.copy_(to_gpu(b, code))
        m = pq.qlinear.from_linear(lin)
        wq, ws = C.quant_rowwise(w, code)
        same(m.wq, wq, "weight codes"); same(m.ws, ws, "weight scales")
        out[code] = (m, wq, ws, b)
    return out


def _e2e(pq, model, code, x, x_plain, special, what):
    m, wq, ws, b = model[code]
    xq, xs = C.quant_rowwise(x, code)
    want = C.qlinear_s8(xq, xs, wq, ws, b, code)
    wf = Q.to_f32(want, code)
    # QSPEC: a NaN token has the scale 0x7FC00000 and codes 0; an Inf token the scale Inf and — x / Inf = 0, Inf / Inf = NaN -> 0 — codes 0 as well: acc = 0, 0 * Inf = NaN
    nan_rows = sorted(r for r, k in special.items() if k in ("nan", "+inf", "-inf and nan"))
    assert np.flatnonzero(np.isnan(wf).all(axis=1)).tolist() == nan_rows and not np.isnan(np.delete(wf, nan_rows, axis=0)).any(), "the reference itself"
    xg, xpg = to_gpu(x, code), to_gpu(x_plain, code)
    ordinary = torch.tensor([r for r in range(x.shape[0]) if r not in special], dtype=torch.long, device="cuda")
    for name, f in (("module", lambda t: m(t)), ("qlinear_dyn", lambda t: pq.qlinear_dyn(t, m.wq, m.ws, m.bias))):
        y = f(xg)
        same_f(y, want, code, f"{what} {name}")
        got_nan = torch.isnan(y.float()).all(dim=1).cpu().numpy()
        assert np.flatnonzero(got_nan).tolist() == nan_rows, f"{what} {name}: all-NaN rows {np.flatnonzero(got_nan).tolist()}, QSPEC says {nan_rows}"
        if len(ordinary):
            y_plain = f(xpg)
            assert not bool(torch.isnan(y_plain.float()).any())
            assert torch.equal(_ibits(y[ordinary]), _ibits(y_plain[ordinary])), f"{what} {name}: a special token changed an ordinary row"


@pytest.mark.parametrize("M", (300, 24))
@pytest.mark.parametrize("code", (0, 1, 2), ids=("bf16", "fp16", "f32"))
def test_special_tokens_end_to_end(pq, model, code, M):
    rng = np.random.default_rng(M + code)
    xf = (rng.standard_normal((M, E2E_K)) * 1.5).astype(np.float32)
    plain = Q.from_f32(xf, code)
    special = _special_rows(M)
    for row, kind in special.items():
        _plant(xf, row, kind, code)
    _e2e(pq, model, code, Q.from_f32(xf, code), plain, special, f"M={M} code={code}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("code", (0, 1, 2), ids=("bf16", "fp16", "f32"))
def test_one_special_token_alone(pq, model, code, kind):
    """M = 1: the decode step whose only token is the special one"""
    rng = np.random.default_rng(len(kind) + code)
    xf = (rng.standard_normal((1, E2E_K)) * 1.5).astype(np.float32)
    plain = Q.from_f32(xf, code)
    _plant(xf, 0, kind, code)
    _e2e(pq, model, code, Q.from_f32(xf, code), plain, {0: kind}, f"M=1 {kind} code={code}")
