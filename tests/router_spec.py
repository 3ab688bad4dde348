"""TEST INFRASTRUCTURE — numpy restatement of QSPEC RT1-RT5: the expert selection of a mixture-of-experts router behind its GEMM, as pq_moe_topk
computes it.  Torch-free; half types are uint16 bit patterns with a dtype tag, as in oracle.qspec_numpy.  Also the DESIGNED rows the host and GPU tests share."""
import numpy as np

from oracle.qspec_numpy import exp_spec, from_f32, to_f32

KINDS = ("softmax_topk", "topk_softmax")
_CANON_NAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def layout(E: int):
    """(G, S): the lanes a row is dealt to — the power of two >= E, at least 4, at most 64 — and the slots per lane, ceil(E / G).  Expert e: lane e mod G, slot e // G."""
    G = 4
    while G < E and G < 64:
        G *= 2
    return G, (E + G - 1) // G


def order_keys(l: np.ndarray) -> np.ndarray:
    """RT1 as unsigned integers: larger key = earlier in the selection.  Every NaN the largest key, -0 the key of +0."""
    u = np.ascontiguousarray(l, np.float32).view(np.uint32)
    u = np.where(u == np.uint32(0x80000000), np.uint32(0), u)
    key = np.where(u & np.uint32(0x80000000) != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(l), np.uint32(0xFFFFFFFF), key).astype(np.uint32)


def select(l: np.ndarray, k: int) -> np.ndarray:
    """RT2: ids[T, k] int64 — value descending, equal values to the lower expert id."""
    T, E = l.shape
    ident = (np.uint64(0xFFFFFFFF) - np.arange(E, dtype=np.uint64))[None, :]
    combined = (order_keys(l).astype(np.uint64) << np.uint64(32)) | ident          # unique per row
    return np.argsort(combined, axis=1)[:, ::-1][:, :k].astype(np.int64)


def pinned_sum(x: np.ndarray) -> np.ndarray:
    """RT3's sum of x[T, E] (float32): per lane the slots in order from +0, then the xor butterfly G/2 .. 1; absent lanes and slots add +0."""
    T, E = x.shape
    G, S = layout(E)
    pad = np.zeros((T, S * G), np.float32)
    pad[:, :E] = x
    v = pad.reshape(T, S, G)
    acc = np.zeros((T, G), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(S):
            acc = (acc + v[:, i, :]).astype(np.float32)
        lanes, off = np.arange(G), G // 2
        while off >= 1:
            acc = (acc + acc[:, lanes ^ off]).astype(np.float32)
            off //= 2
    return acc[:, 0]


def _seq_sum(p: np.ndarray) -> np.ndarray:
    s = p[:, 0].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(1, p.shape[1]):
            s = (s + p[:, j]).astype(np.float32)
    return s


def row_sums(logits: np.ndarray, dtype) -> np.ndarray:
    """RT3's S of every row: it depends on the row alone (not on k), so a test that walks many k computes it once and hands it to moe_topk"""
    l = to_f32(logits, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        m = l[np.arange(l.shape[0])[:, None], select(l, 1)]
        return pinned_sum(exp_spec((l - m).astype(np.float32)))


def moe_topk(logits: np.ndarray, dtype, k: int, kind: str = "softmax_topk", renormalise: bool = False, w_dtype=None, sums=None):
    """logits[T, E] stored in `dtype` -> (weights[T, k] stored in w_dtype (default: dtype), ids[T, k] int64, weights before the storage rounding as float32).
    sums: row_sums(logits, dtype), if the caller has them."""
    assert kind in KINDS
    l = to_f32(logits, dtype)
    T, E = l.shape
    assert 1 <= k <= min(E, 64) and E <= 1024
    ids = select(l, k)
    rows = np.arange(T)[:, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = l[rows, ids[:, :1]]                                                      # [T, 1]
        xsel = exp_spec((l[rows, ids] - m).astype(np.float32))                       # x[ids[j]]: the same function of the same inputs as x[e] at e = ids[j]
        if kind == "softmax_topk":
            S = pinned_sum(exp_spec((l - m).astype(np.float32))) if sums is None else sums
            w = (xsel / S[:, None]).astype(np.float32)
            if renormalise:
                w = (w / _seq_sum(w)[:, None]).astype(np.float32)
        else:
            w = (xsel / _seq_sum(xsel)[:, None]).astype(np.float32)
    w = np.where(np.isnan(w), _CANON_NAN, w).astype(np.float32)
    return from_f32(w, dtype if w_dtype is None else w_dtype), ids, w


# ---------------------------------------------------------------------------------------------------- designed rows
_MAXF = {"bf16": float(np.array([0x7F7F0000], np.uint32).view(np.float32)[0]), "fp16": 65504.0, "f32": float(np.finfo(np.float32).max)}
_SUBN = {"bf16": float(np.array([0x00010000], np.uint32).view(np.float32)[0]), "fp16": 2.0 ** -24, "f32": float(np.array([1], np.uint32).view(np.float32)[0])}


def edge_positions(E: int):
    """the first and last expert, and the first and last lane and slot of the layout of E"""
    G, S = layout(E)
    pos = {0, E - 1, min(G - 1, E - 1), (S - 1) * G, max((S - 1) * G - 1, 0), min((S - 1) * G + G - 1, E - 1)}
    if S > 1:
        pos |= {G, 2 * G - 1}
    return sorted(p for p in pos if 0 <= p < E)


def designed_rows(E: int, k: int, dtype: str):
    """[(name, row float32 [E])]: every value is exactly representable in `dtype`.  Conditions the host test holds the reference to are in the names' prefixes:
    "ties:n:j" — j experts above a group of n equal values with j < k < j + n (the group straddles the k boundary); "equal" — one value everywhere; "max@p" — the
    maximum planted at expert p."""
    rng = np.random.default_rng(1000 * E + k)
    base = (rng.permutation(E).astype(np.float32) - np.float32(E // 2)) / np.float32(4)        # pairwise distinct quarters, |v| <= 256
    rows = [("equal", np.full(E, 1.5, np.float32)), ("zeros", np.where(np.arange(E) % 2 == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32))]
    for p in edge_positions(E):
        r = base.copy()
        r[p] = np.float32(300.0)
        rows.append((f"max@{p}", r))
        r = np.full(E, -2.0, np.float32)                     # everything else equal: the rest of the selection is the lowest ids
        r[p] = np.float32(1.0)
        rows.append((f"max@{p}:flat", r))
    for n in sorted({2, 3, 4, 5, 8, E}):                     # a tie group of every multiplicity that fits, straddling the k boundary
        for j in sorted({0, k - 1, max(k - n + 1, 0)}):
            if n > E or j >= k or j + n <= k or j + n > E:
                continue
            r = np.full(E, -8.0, np.float32) - np.arange(E, dtype=np.float32) / np.float32(4)
            where = rng.permutation(E)
            r[where[:j]] = np.float32(20.0) + np.arange(j, dtype=np.float32)
            r[where[j:j + n]] = np.float32(3.25)
            rows.append((f"ties:{n}:{j}", r))
    special = base.copy()
    vals = [np.nan, np.inf, -np.inf, 0.0, -0.0, _SUBN[dtype], -_SUBN[dtype], _MAXF[dtype], -_MAXF[dtype]]
    for name, planted in (("nan", [np.nan]), ("nan2", [np.nan, -np.nan]), ("+inf", [np.inf]), ("-inf", [-np.inf]), ("allinf", None), ("maxfinite", [_MAXF[dtype], -_MAXF[dtype]]),
                          ("subnormal", [_SUBN[dtype], -_SUBN[dtype], 0.0, -0.0]), ("mixed", vals)):
        if planted is None:
            rows.append((name, np.full(E, -np.inf, np.float32)))
            continue
        if name == "-inf" and E == 1:
            continue                                         # (a lone -Inf is the "allinf" row)
        r = special.copy() if name != "subnormal" else np.full(E, -1.0, np.float32) - np.arange(E, dtype=np.float32)
        where = rng.permutation(E)[:len(planted)]
        r[where] = np.asarray(planted[:len(where)], np.float32)
        rows.append((name, r))
    spread = np.full(E, -40.0, np.float32) - (np.arange(E, dtype=np.float32) % 7)                # more than 30 below the maximum: exp_spec's clamp
    spread[rng.integers(E)] = np.float32(2.0)
    rows.append(("spread", spread))
    return rows


def designed_matrix(E: int, k: int, dtype: str):
    rows = designed_rows(E, k, dtype)
    return [n for n, _ in rows], from_f32(np.stack([r for _, r in rows]), dtype)
