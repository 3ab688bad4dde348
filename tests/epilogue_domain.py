"""TEST INFRASTRUCTURE — operands that drive the dequant epilogue (QSPEC E1-E4: cast_rne(((f32(acc) * xs[m]) * ws[n]) + f32(bias[n]))) over its whole value domain.
numpy only: importable without a GPU and without protoquant_amd.

build(M, N, K, seed) DESIGNS its accumulators, it does not sample them:

  b[n, 0] = q_n, b[n, 1] = r_n with v_n = 127 q_n + r_n; v_n cycles through TARGETS (0, +-1, 9-bit / 12-bit integers that are bf16 / fp16 ties — 4095 * 16 and 8190 * 8 are 65520, the tie below fp16's Inf — and +-16191) over the
  first three quarters of the columns; behind them it is a fold hazard of the column's scale (fold_hazards) where there is one, else a seeded integer in +-16192.  The other columns of b are seeded full-range codes (-128 included); every 7th row
  of b is 127 from k = 2 on.

  rows of a, by m % 4:   0  [127, 1, 0, ...]     acc[m, n] = v_n exactly
                         1  seeded full-range codes
                         2  all 127               against the "every 7th" rows of b: |acc| = 127 (q_n + r_n + 127 (K - 2)) > 2^24 once K >= 1043, odd where q_n + r_n + K is
                         3  all zero              acc = 0: the 0 * Inf case

  xs[m] = XS[(m // 4) % 16], ws[n] = WS[n % 17]: a row class holds one row of each kind, and with 16 row classes against 17 column classes (coprime, and 47 targets
  coprime with both) the pairs drift across any tile grid: every (row class, column class, row kind) triple occurs in interior tiles and in ragged edge tiles of a few
  hundred rows and columns.  XS[0] = 1, so a one-row problem still computes numbers.

bias(N, code, seed): seeded normal values with +0, -0, +-Inf, NaN and a value near the dtype's largest finite number planted by n % 12.

classes(want, code, t, acc) counts what a reference output holds of each class the epilogue must get right."""
import numpy as np

from oracle import qspec_numpy as Q


def _f(u):
    return np.array([u], np.uint32).view(np.float32)[0]


_TIES = (257, 259, 261, 383, 509, 511, 514, 1025, 1027, 1030, 2049, 2051, 2053, 4095, 4097, 4098, 4099, 8190, 8193, 8195, 8196)
TARGETS = (0, 1, -1) + tuple(s * v for v in _TIES for s in (1, -1)) + (16191, -16191)          # 47 values: coprime with 17, 12 and 7

NAN = _f(0x7FC00000)            # what Q3 makes of a NaN token
# the first classes are the ones a short problem still meets: M = 1 sees XS[0] only, M = 17 five of them, M = 48 twelve
XS = np.array([1.0, NAN, np.inf, 0.0, 1e-40, 2.0 ** -126, 2.0 ** -24, 2.3e36, 2.0 ** -14, 2.0 ** -133, 4.0, 3.1e-5, 16.0, 1e-3, 0.0123, 7.7], np.float32)
WS = np.array([1.0, 2.0 ** -100, 0.0171, 2.0 ** 100, -0.5, 1e-38, 0.004, NAN, 2.0 ** -10, np.inf, 1.9e-3, 0.0, 0.25, 2.0, 1e-4, 2.0 ** -24, 0.37], np.float32)
assert len(TARGETS) == 47 and len(XS) == 16 and len(WS) == 17

BIG = {0: 3.3e38, 1: 60000.0, 2: 3.3e38}         # near the largest finite value of bf16 / fp16 / f32


_HAZARDS = {}


def fold_hazards(w):
    """The integers v in +-16192 for which v * w, rounded to f32 and THEN to fp16 (QSPEC), is not v * w rounded to fp16 ONCE: the f32 rounding lands on an fp16 tie the
    exact product misses.  A multiply folded into the fp16 convert (v_fma_mixlo_f16) stores another value exactly there.  Empty for powers of two and non-finite scales."""
    key = float(w)
    if key not in _HAZARDS:
        v = np.arange(-16192, 16193, dtype=np.int64)
        with np.errstate(all="ignore"):
            exact = v.astype(np.float64) * np.float64(w)                  # 15 x 24 bits: exact in binary64
            twice = exact.astype(np.float32).astype(np.float16)
            once = exact.astype(np.float16)
        ok = np.isfinite(exact) & (np.abs(exact) >= 2.0 ** -14) & (once.view(np.uint16) != twice.view(np.uint16))
        _HAZARDS[key] = v[ok]
    return _HAZARDS[key]


def fp16_fold_hazards(acc, xs, ws):
    """how many elements of an fp16 output (no bias) a multiply-convert fold of E3 into the cast would change"""
    with np.errstate(all="ignore"):
        t2 = (acc.astype(np.float32) * xs.astype(np.float32)[:, None]).astype(np.float32)
        exact = t2.astype(np.float64) * ws.astype(np.float64)[None, :]
        once, twice = exact.astype(np.float16), exact.astype(np.float32).astype(np.float16)
    return int((np.isfinite(exact) & (once.view(np.uint16) != twice.view(np.uint16))).sum())


def build(M, N, K, seed):
    """a[M, K], b[N, K] int8, acc[M, N] exact int32, xs[M], ws[N] f32"""
    assert K >= 2
    rng = np.random.default_rng(seed)
    n = np.arange(N)
    v = np.where(n < (3 * N) // 4, np.array(TARGETS, np.int64)[n % len(TARGETS)], rng.integers(-16192, 16193, N))
    for j in range((3 * N) // 4, N):                    # behind the targets: a fold hazard of the column's scale where it has one, else the seeded integer
        hz = fold_hazards(WS[j % len(WS)])
        if len(hz):
            v[j] = hz[(j // len(WS)) % len(hz)]
    q = np.rint(v / 127.0).astype(np.int64)
    r = v - 127 * q
    assert np.abs(q).max(initial=0) <= 127 and np.abs(r).max(initial=0) <= 63
    b = rng.integers(-128, 128, (N, K), dtype=np.int8)
    b[::7, 2:] = 127
    b[:, 0], b[:, 1] = q, r
    a = rng.integers(-128, 128, (M, K), dtype=np.int8)
    a[0::4] = 0
    a[0::4, 0], a[0::4, 1] = 127, 1
    a[2::4] = 127
    a[3::4] = 0
    acc = (a.astype(np.int64) @ b.astype(np.int64).T)
    assert np.abs(acc).max(initial=0) < 2 ** 31
    assert np.array_equal(acc[0::4], np.broadcast_to(v, acc[0::4].shape))
    xs = XS[(np.arange(M) // 4) % len(XS)].copy()
    ws = WS[n % len(WS)].copy()
    return a, b, acc.astype(np.int32), xs, ws


def bias(N, code, seed):
    """[N] in the storage of output dtype `code` (uint16 bit patterns for the half types)"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal(N).astype(np.float32)
    n = np.arange(N)
    for k, val in ((0, 0.0), (1, -0.0), (3, np.inf), (5, -0.0), (6, np.nan), (8, 0.0), (9, -np.inf), (10, BIG[code])):
        f[n % 12 == k] = val
    f[(n % 24) == 10] *= -1
    return Q.from_f32(f, code)


def pre_cast(acc, xs, ws, bias_v, code):
    """E1-E3 (+ E4's add): the f32 value the output cast sees"""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        t = acc.astype(np.float32)
        t = (t * xs.astype(np.float32)[:, None]).astype(np.float32)
        t = (t * ws.astype(np.float32)[None, :]).astype(np.float32)
        if bias_v is not None:
            t = (t + Q.to_f32(bias_v, code)[None, :]).astype(np.float32)
    return t


MANT = {0: 8, 1: 11, 2: 24}             # significand bits
EMIN = {0: -126, 1: -14, 2: -126}       # exponent of the smallest normal


def classes(want, code, t, acc=None):
    """{class: count} of a reference output `want` (storage of dtype `code`) whose cast saw the f32 values `t`"""
    w = Q.to_f32(want, code).astype(np.float64)
    sign = np.signbit(w)
    c = {"nan": int(np.isnan(w).sum()), "+inf": int((w == np.inf).sum()), "-inf": int((w == -np.inf).sum()),
         "+0": int(((w == 0) & ~sign).sum()), "-0": int(((w == 0) & sign).sum()),
         "subnormal": int(((w != 0) & (np.abs(w) < 2.0 ** EMIN[code])).sum())}
    if code != 2:
        # a tie of the cast: |t| / ulp has the fraction one half, ulp being the spacing of the output type at |t| (its subnormal spacing below the smallest normal);
        # for fp16 this includes 65520, halfway between 65504 and the 65536 that rounds to Inf
        tt = np.abs(t.astype(np.float64))
        fin = np.isfinite(tt) & (tt > 0) & ((tt < 65536.0) if code == 1 else True)
        e = np.frexp(np.where(fin, tt, 1.0))[1] - 1                      # |t| = 1.f x 2^e
        u = np.where(fin, tt, 0.0) / np.exp2(np.maximum(e, EMIN[code]) - (MANT[code] - 1.0))
        c["tie"] = int((fin & (u - np.floor(u) == 0.5)).sum())
    if acc is not None:
        a64 = acc.astype(np.int64)
        c["odd acc > 2^24"] = int(((np.abs(a64) > 2 ** 24) & (a64 % 2 != 0)).sum())
    return c
