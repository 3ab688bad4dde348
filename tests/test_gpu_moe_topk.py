"""GPU: pq_moe_topk / pq.moe_topk (kernel K-rt) bit for bit against QSPEC RT (tests/router_spec.py) — every layout of the kernel (E = 1 .. 1024), k from 1 to
min(E, 64), both kinds, both renormalisation values, logits and weights in bf16 / fp16 / f32 independently, int32 and int64 ids, T = 1 .. 320 rows, logits read through
a view with ld = E + 3 and both outputs written as column blocks of wider buffers whose sentinels are compared as a whole; rows: random ones, the designed rows of
router_spec (tie groups across the k boundary, the all-equal row, the maximum at every edge of the layout, NaN, +-Inf, +-0, subnormals, the largest finite value, a
spread above 30).  A graph captured once follows the contents of the logits.

Eager-close: the kernel against the eager chain it replaces, on rows whose f32 probabilities are pairwise distinct (asserted on eager's output alone; no row is left
out) and whose values differ from row to row (every row draws its own E distinct logits).  Measured on an MI355X, 2 x 10^5 rows per kind and 16-bit dtype over (E, k) =
(8, 2), (64, 8), (128, 8), (32, 4), 1 100 000 stored weights each: ids equal everywhere;
  softmax_topk: bf16 weights 10 differ from eager's (9.09e-06), fp16 weights 77 (7.00e-05), none by more than 1 ulp;
  topk_softmax: bf16 weights  9 differ (8.18e-06),              fp16 weights 80 (7.27e-05), none by more than 1 ulp
(two binary32 results about 3e-7 apart, rounded to 8 or 11 significant bits: EAGER_SHARE / EAGER_ULP below; the test holds max(4 x share, 1e-5) and 1 ulp);
f32 weights, largest relative error against binary64: softmax_topk kernel 5.39e-07 / eager 5.39e-07, topk_softmax kernel 5.44e-07 / eager 5.83e-07 (held: kernel <= 4 x
eager; both printed)."""
import numpy as np
import pytest
import torch

from oracle.qspec_numpy import from_f32
from tests import router_spec as RS
from tests.gpu_util import TD, bits, to_gpu

pytestmark = pytest.mark.gpu

DT = ("bf16", "fp16", "f32")
CODE = {"bf16": 0, "fp16": 1, "f32": 2}
NP_W = {"bf16": np.uint16, "fp16": np.uint16, "f32": np.uint32}
ES = (1, 2, 3, 8, 31, 32, 33, 60, 64, 65, 128, 160, 384, 1000, 1024)
TS = (1, 2, 3, 5, 63, 64, 65, 257)
ROWS = 320          # the whole matrix is one call; the windows take the lengths of TS
W_SENTINEL = {"bf16": 0x4D4D, "fp16": 0x4D4D, "f32": 0x4D4D4D4D}
ID_SENTINEL = -7

# measured (see the module docstring): the share of stored 16-bit weights that differ from eager's, and the largest distance in units of the last place
EAGER_SHARE = {("softmax_topk", "bf16"): 9.091e-06, ("softmax_topk", "fp16"): 7.000e-05, ("topk_softmax", "bf16"): 8.182e-06, ("topk_softmax", "fp16"): 7.273e-05}
EAGER_ULP = {"bf16": 1, "fp16": 1}


def ks_of(E):
    return sorted({k for k in (1, 2, 4, 8, min(E, 64)) if k <= min(E, 64)} | ({E} if E <= 64 else set()))


def rows_of(E, dtype):
    """ROWS rows stored in `dtype`: the designed rows for every k of ks_of(E) (they differ in their tie groups), then random rows of three scales"""
    parts, seen = [], set()
    for k in ks_of(E):
        names, m = RS.designed_matrix(E, k, dtype)
        for n, r in zip(names, m):
            key = (n, r.tobytes())
            if key not in seen:
                seen.add(key)
                parts.append(r)
    assert len(parts) <= ROWS - 40, f"E={E}: {len(parts)} designed rows do not leave 40 random ones in {ROWS}"          # (no designed row is dropped)
    rng = np.random.default_rng(E)
    n = ROWS - len(parts)
    rnd = rng.standard_normal((n, E)).astype(np.float32) * np.repeat(np.array([0.05, 2.0, 12.0], np.float32), (n + 2) // 3)[:n, None]
    return np.concatenate([np.stack(parts), from_f32(rnd, dtype)], axis=0)


def call(L, logits, k, kind, renorm, wbuf, wcol, ibuf, icol, T0, T):
    """pq_moe_topk on rows T0 .. T0 + T - 1 of the logits view, into the column blocks [wcol, wcol + k) of wbuf and [icol, icol + k) of ibuf, rows 1 .. T"""
    from protoquant_amd import _lib
    lv, wv, iv = logits[T0:T0 + T], wbuf[1:1 + T, wcol:wcol + k], ibuf[1:1 + T, icol:icol + k]
    st = L.pq_moe_topk(lv.data_ptr(), _lib.dtype_code(lv.dtype), logits.stride(0), T, lv.shape[1], k, _lib.ROUTER_KINDS[kind], int(renorm), wv.data_ptr(),
                       _lib.dtype_code(wbuf.dtype), wbuf.stride(0), iv.data_ptr(), int(ibuf.dtype == torch.int64), ibuf.stride(0), torch.cuda.current_stream().cuda_stream)
    assert st == 0, L.pq_last_error()


@pytest.mark.parametrize("E", ES)
def test_bits_against_the_specification(E):
    from protoquant_amd import _lib
    L = _lib.lib()
    combo = 0
    for ldt in DT:
        stored = rows_of(E, ldt)
        wide = torch.full((ROWS, E + 3), 7.0, dtype=TD[CODE[ldt]], device="cuda")
        wide[:, 1:E + 1] = to_gpu(stored, CODE[ldt])
        logits = wide[:, 1:E + 1]                                  # ld = E + 3, the base one element into the buffer
        sums = RS.row_sums(stored, ldt)
        for k in ks_of(E):
            for kind in RS.KINDS:
                for renorm in (False, True):
                    _, want_ids, want_f = RS.moe_topk(stored, ldt, k, kind, renorm, "f32", sums=sums)
                    for wdt in DT:
                        want_w = from_f32(want_f, wdt)
                        for idt in (torch.int32, torch.int64):
                            # the whole matrix, and a window of another length T that moves through the rows from combination to combination
                            T = TS[combo % len(TS)]
                            T0 = (combo * 37) % (ROWS - T + 1)
                            combo += 1
                            for (a, n) in ((0, ROWS), (T0, T)):
                                wbuf = torch.from_numpy(np.full((n + 2, k + 5), W_SENTINEL[wdt], NP_W[wdt]).view(np.int16 if wdt != "f32" else np.int32)).cuda().view(TD[CODE[wdt]])
                                ibuf = torch.full((n + 2, k + 4), ID_SENTINEL, dtype=idt, device="cuda")
                                call(L, logits, k, kind, renorm, wbuf, 3, ibuf, 1, a, n)
                                exp_w = np.full((n + 2, k + 5), W_SENTINEL[wdt], NP_W[wdt])
                                exp_w[1:1 + n, 3:3 + k] = want_w[a:a + n].view(NP_W[wdt])
                                exp_i = np.full((n + 2, k + 4), ID_SENTINEL, np.int64)
                                exp_i[1:1 + n, 1:1 + k] = want_ids[a:a + n]
                                what = f"E={E} k={k} {kind} renorm={renorm} logits={ldt} weights={wdt} ids={idt} rows {a}..{a + n - 1}"
                                got_i = ibuf.cpu().numpy().astype(np.int64)
                                bad = np.argwhere(got_i != exp_i)
                                assert bad.size == 0, f"{what}: ids (or their guard) differ, first at {bad[:3].tolist()}: got {got_i[tuple(bad[0])]}, want {exp_i[tuple(bad[0])]}"
                                got_w = bits(wbuf)
                                bad = np.argwhere(got_w != exp_w)
                                assert bad.size == 0, f"{what}: weights (or their guard) differ, first at {bad[:3].tolist()}: got {got_w[tuple(bad[0])]:#x}, want {exp_w[tuple(bad[0])]:#x}"
        assert torch.equal(wide[:, 0], torch.full_like(wide[:, 0], 7.0)) and torch.equal(wide[:, E + 1:], torch.full_like(wide[:, E + 1:], 7.0)), "the logits were written"
        assert np.array_equal(bits(logits), stored.view(NP_W[ldt])), "the logits were written"


def test_python_entry_shapes_views_and_dtypes():
    import protoquant_amd as pq
    E, k = 60, 4
    stored = rows_of(E, "bf16")[:240]
    x = to_gpu(stored, 0)
    want_w, want_ids, _ = RS.moe_topk(stored, "bf16", k, "softmax_topk", True)
    w, ids = pq.moe_topk(x.reshape(4, 60, E), k, renormalise=True)
    assert w.shape == (4, 60, k) and ids.shape == (4, 60, k) and w.dtype == torch.bfloat16 and ids.dtype == torch.int64
    assert np.array_equal(bits(w).reshape(-1, k), want_w) and np.array_equal(ids.cpu().numpy().reshape(-1, k), want_ids)
    w, ids = pq.moe_topk(x.t().contiguous().t(), k, renormalise=True, out_dtype=torch.float32, ids_dtype=torch.int32)      # a column-major view: copied once
    assert w.dtype == torch.float32 and ids.dtype == torch.int32
    assert np.array_equal(bits(w), RS.moe_topk(stored, "bf16", k, "softmax_topk", True, "f32")[0].view(np.uint32)) and np.array_equal(ids.cpu().numpy(), want_ids)
    w, ids = pq.moe_topk(x[:0], k)
    assert w.shape == (0, k) and ids.shape == (0, k)
    w, ids = pq.moe_topk(x[3], k, "topk_softmax")                                                                         # one row without a leading axis
    assert w.shape == (k,) and np.array_equal(bits(w)[None], RS.moe_topk(stored[3:4], "bf16", k, "topk_softmax")[0])
    from protoquant_amd import _lib
    for bad_k in (0, E + 1):
        with pytest.raises(_lib.PQError, match="k ="):
            pq.moe_topk(x, bad_k)


def test_graph_captured_once_follows_the_logits():
    import protoquant_amd as pq
    E, k, T = 128, 8, 32
    stored = rows_of(E, "bf16")
    x = to_gpu(stored[:T], 0).clone()
    pq.moe_topk(x, k, renormalise=True, ids_dtype=torch.int32)          # warm-up outside capture
    torch.cuda.synchronize()
    s, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            w, ids = pq.moe_topk(x, k, renormalise=True, ids_dtype=torch.int32)
    for start in (40, 100, 225):
        new = stored[start:start + T]
        x.copy_(to_gpu(new, 0))
        w.fill_(-1.0); ids.fill_(-7)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want_w, want_ids, _ = RS.moe_topk(new, "bf16", k, "softmax_topk", True)
        assert np.array_equal(bits(w), want_w) and np.array_equal(ids.cpu().numpy(), want_ids), f"replay on rows {start}.."


# ---------------------------------------------------------------------------------------------------- eager-close
def eager_chain(l, k, kind, out_dtype, dt=torch.float32):
    """the routers' recipes after their F.linear: Qwen3-MoE's with norm_topk_prob (softmax in f32, top-k, renormalise, cast) and GPT-OSS's (top-k, softmax, cast)"""
    if kind == "softmax_topk":
        p = torch.softmax(l, dim=-1, dtype=dt)
        w, ids = torch.topk(p, k, dim=-1)
        w = w / w.sum(dim=-1, keepdim=True)
        return w.to(out_dtype), ids, p
    v, ids = torch.topk(l, k, dim=-1)
    return torch.softmax(v.to(dt), dim=-1).to(out_dtype), ids, torch.softmax(l, dim=-1, dtype=dt)


def distinct_rows(T, E, dtype, seed):
    """[T, E] on the GPU, every row E DISTINCT values of its own, other values in every row: E of the 2049 multiples of 1/128 in [-8, 8] (each exact in bf16 and in fp16:
    at most 11 bits below 8 would not be in bf16 — so bf16 rows take E of the 513 multiples of 1/32, whose numerators fit its 8 bits, moved by a row offset that is a
    multiple of 1/32 too), drawn per row without replacement.  f32 rows are such rows moved element by element by less than a quarter step.  Logits at least a step apart
    have pairwise distinct f32 probabilities (a ratio of at least e^(1/128)); the test asserts that on eager's output."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    step, n = (1.0 / 32, 513) if dtype == torch.bfloat16 else (1.0 / 128, 2049)
    grid = (torch.arange(n, dtype=torch.float32, device="cuda") - n // 2) * step
    rows = grid[torch.rand(T, n, generator=g, device="cuda").argsort(dim=1)[:, :E]]
    if dtype == torch.float32:
        return rows + (torch.rand(T, E, generator=g, device="cuda") - 0.5) * (step / 2)
    out = rows.to(dtype)
    assert torch.equal(out.float(), rows), "the grid is exact in the storage dtype"
    return out


@pytest.mark.parametrize("kind", RS.KINDS)
def test_eager_close(kind):
    import protoquant_amd as pq
    T = 50000
    n = {d: 0 for d in EAGER_ULP}
    differ = {d: 0 for d in EAGER_ULP}
    ulp = {d: 0 for d in EAGER_ULP}
    err_k = err_e = 0.0
    for i, (E, k) in enumerate(((8, 2), (64, 8), (128, 8), (32, 4))):
        for wname, wdt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
            l = distinct_rows(T, E, torch.bfloat16, 10 * i + len(wname))
            w_e, ids_e, p = eager_chain(l, k, kind, wdt)
            srt = torch.sort(p, dim=1).values
            assert bool((srt[:, 1:] != srt[:, :-1]).all()), "the rows were meant to have pairwise distinct f32 probabilities"
            w_k, ids_k = pq.moe_topk(l, k, kind, renormalise=True, out_dtype=wdt)
            assert torch.equal(ids_k, ids_e), f"E={E} k={k} {kind}: ids differ from eager's in {int((ids_k != ids_e).any(dim=1).sum())} rows"
            d = (w_k.view(torch.int16).int() - w_e.view(torch.int16).int()).abs()
            n[wname] += d.numel(); differ[wname] += int((d != 0).sum()); ulp[wname] = max(ulp[wname], int(d.max()))
        l = distinct_rows(T, E, torch.float32, 100 + i)
        w_e, ids_e, p = eager_chain(l, k, kind, torch.float32)
        srt = torch.sort(p, dim=1).values
        assert bool((srt[:, 1:] != srt[:, :-1]).all())
        w_k, ids_k = pq.moe_topk(l, k, kind, renormalise=True)
        assert torch.equal(ids_k, ids_e)
        w64 = eager_chain(l.double(), k, kind, torch.float64, torch.float64)[0]
        err_k = max(err_k, float(((w_k.double() - w64).abs() / w64).max()))
        err_e = max(err_e, float(((w_e.double() - w64).abs() / w64).max()))
    for d in EAGER_ULP:
        print(f"{kind}: {d} weights: {differ[d]} of {n[d]} differ from eager's ({differ[d] / n[d]:.3e}), at most {ulp[d]} ulp")
    print(f"{kind}: f32 weights: largest relative error against binary64: kernel {err_k:.3e}, eager {err_e:.3e}")
    for d in EAGER_ULP:
        assert ulp[d] <= EAGER_ULP[d], (d, ulp[d])
        assert differ[d] / n[d] <= max(4 * EAGER_SHARE[(kind, d)], 1e-5), (d, differ[d] / n[d])
    assert err_k <= 4 * err_e, (err_k, err_e)
