"""CPU: the operands of tests/epilogue_domain.py do what they claim before any kernel sees them — the two independent restatements of QSPEC E1-E4 (oracle/qspec_numpy.py,
oracle/qspec_oracle.c) agree on them, the designed accumulators are the exact products, and every class of value the epilogue must get right (NaN, +-Inf, +-0, subnormal
outputs, exact ties of the 16-bit cast, odd accumulators above 2^24) is POPULATED in the reference.  The floors are conditions on the inputs: if one is missed, the
construction is what changes.

The reference's class counts at K = 1280 are RECORDED below and asserted, so the record cannot drift from the builder (`pytest -s` prints them for every case)."""
import numpy as np
import pytest

from oracle import c_oracle as C
from oracle import qspec_numpy as Q
from tests import epilogue_domain as D

SEED, BIAS_SEED = 5, 7
SHAPES = [(300, 520, 1280), (48, 520, 1280), (1, 520, 1280)]
NAMES = {0: "bf16", 1: "fp16", 2: "f32"}
FLOOR = {300: 64, 48: 16, 1: 1}
# M = 1 is one row of kind 0 (acc = v_n) with xs = 1: it cannot give an odd accumulator above 2^24, and a subnormal only where v_n = +-1 meets the subnormal column scale
ONE_ROW = ("nan", "+inf", "-inf", "+0", "-0", "tie")
# (M, dtype, bias) -> counts of D.classes() on the reference, seed 5 / bias seed 7; f32 has no cast, so no ties
RECORDED = {
    (300, "bf16", False): {"nan": 25000, "+inf": 9243, "-inf": 9448, "+0": 36483, "-0": 10039, "subnormal": 3131, "tie": 1886, "odd acc > 2^24": 3825},
    (300, "bf16", True): {"nan": 37590, "+inf": 16966, "-inf": 17331, "+0": 13561, "-0": 1699, "subnormal": 1090, "tie": 634, "odd acc > 2^24": 3825},
    (300, "fp16", False): {"nan": 25000, "+inf": 13730, "-inf": 14150, "+0": 47312, "-0": 20818, "subnormal": 4534, "tie": 1562, "odd acc > 2^24": 3825},
    (300, "fp16", True): {"nan": 37590, "+inf": 20204, "-inf": 20968, "+0": 16973, "-0": 5471, "subnormal": 1511, "tie": 546, "odd acc > 2^24": 3825},
    (300, "f32", False): {"nan": 25000, "+inf": 9243, "-inf": 9448, "+0": 35664, "-0": 9207, "subnormal": 4782, "odd acc > 2^24": 3825},
    (300, "f32", True): {"nan": 37590, "+inf": 16966, "-inf": 17331, "+0": 13319, "-0": 1426, "subnormal": 1605, "odd acc > 2^24": 3825},
    (48, "bf16", False): {"nan": 4532, "+inf": 1732, "-inf": 1727, "+0": 5819, "-0": 1821, "subnormal": 627, "tie": 329, "odd acc > 2^24": 612},
    (48, "bf16", True): {"nan": 6534, "+inf": 2852, "-inf": 2865, "+0": 2185, "-0": 322, "subnormal": 215, "tie": 110, "odd acc > 2^24": 612},
    (48, "fp16", False): {"nan": 4532, "+inf": 2200, "-inf": 2252, "+0": 7649, "-0": 3757, "subnormal": 822, "tie": 267, "odd acc > 2^24": 612},
    (48, "fp16", True): {"nan": 6534, "+inf": 3180, "-inf": 3274, "+0": 2767, "-0": 997, "subnormal": 277, "tie": 93, "odd acc > 2^24": 612},
    (48, "f32", False): {"nan": 4532, "+inf": 1732, "-inf": 1727, "+0": 5661, "-0": 1646, "subnormal": 960, "odd acc > 2^24": 612},
    (48, "f32", True): {"nan": 6534, "+inf": 2852, "-inf": 2865, "+0": 2143, "-0": 260, "subnormal": 319, "odd acc > 2^24": 612},
}


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def problem(request):
    M, N, K = request.param
    return (M, N, K) + D.build(M, N, K, SEED)


def test_acc_is_the_exact_product(problem):
    M, N, K, a, b, acc, xs, ws = problem
    want = a.astype(np.int64) @ b.astype(np.int64).T
    assert acc.dtype == np.int32 and np.array_equal(acc.astype(np.int64), want)
    assert np.array_equal(acc, C.gemm_s8s8s32(a, b)) and np.array_equal(acc, Q.gemm_s8s8s32(a, b))
    assert a.min() == -128 or M == 1
    assert b.min() == -128 and b.max() == 127
    assert np.array_equal(acc[0::4], np.broadcast_to(acc[0], acc[0::4].shape)), "rows of kind 0 give v_n"
    assert set(D.TARGETS) <= set(acc[0].tolist())
    assert not acc[3::4].any()


def test_builder_is_deterministic():
    one, two = D.build(48, 130, 256, 3), D.build(48, 130, 256, 3)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(one, two))
    for code in (0, 1, 2):
        assert np.array_equal(D.bias(130, code, 4), D.bias(130, code, 4), equal_nan=True)


def test_scale_classes_are_what_quantize_produces(problem):
    M, N, K, a, b, acc, xs, ws = problem
    assert xs.dtype == np.float32 and ws.dtype == np.float32
    assert np.array_equal(xs.view(np.uint32), D.XS.view(np.uint32)[(np.arange(M) // 4) % 16])
    assert np.array_equal(ws.view(np.uint32), D.WS.view(np.uint32)[np.arange(N) % 17])
    x = D.XS.view(np.uint32)
    assert 0x7FC00000 in x and 0x7F800000 in x and 0 in x                                  # Q3's NaN scale, an Inf scale, zero
    assert ((x & 0x7F800000) == 0).sum() >= 3 and (D.XS == np.float32(2.0 ** -126)).any()     # zero and two subnormals; the smallest normal
    assert (D.WS < 0).sum() == 1 and np.isnan(D.WS).sum() == 1 and np.isinf(D.WS).sum() == 1 and (D.WS == 0).sum() == 1
    # the scale order is visible: (acc * xs) * ws and (acc * ws) * xs differ as Inf differs from a number
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        v = np.float32(16191)
        assert np.isinf((v * np.float32(2.3e36)) * np.float32(2.0 ** -100)) and np.isfinite((v * np.float32(2.0 ** -100)) * np.float32(2.3e36))
    if M > 1:       # ... in the problem itself: the column scale first, or the two scales multiplied together first, gives other bits in many places (f32 output, NaNs as a class)
        want = Q.epilogue(acc, xs, ws, None, 2)
        nan = np.isnan(want)
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            col_first = ((acc.astype(np.float32) * ws[None, :]).astype(np.float32) * xs[:, None]).astype(np.float32)
            premul = (acc.astype(np.float32) * (xs[:, None] * ws[None, :]).astype(np.float32)).astype(np.float32)
        for name, other in (("column scale first", col_first), ("scales multiplied first", premul)):
            n_diff = int((np.isnan(other) != nan).sum() + ((other.view(np.uint32) != want.view(np.uint32)) & ~nan & ~np.isnan(other)).sum())
            print(f"\n{M}x{N}x{K}: '{name}' would differ from E2-E3 on {n_diff} elements")
            assert n_diff >= FLOOR[M] * 4, (name, n_diff)


@pytest.mark.parametrize("has_bias", (False, True), ids=("nobias", "bias"))
@pytest.mark.parametrize("code", (0, 1, 2), ids=("bf16", "fp16", "f32"))
def test_two_oracles_agree_and_every_class_is_populated(problem, code, has_bias):
    M, N, K, a, b, acc, xs, ws = problem
    bv = D.bias(N, code, BIAS_SEED) if has_bias else None
    want = Q.epilogue(acc, xs, ws, bv, code)
    other = C.qlinear_s8(a, xs, b, ws, bv, code)
    nan = np.isnan(Q.to_f32(want, code))
    assert np.array_equal(nan, np.isnan(Q.to_f32(other, code))), "the two oracles disagree on where the NaNs are"
    wb, ob = (want.view(np.uint32), other.view(np.uint32)) if code == 2 else (want, other)
    assert int(((wb != ob) & ~nan).sum()) == 0, "the two oracles disagree on bits (signs of zero included)"
    t = D.pre_cast(acc, xs, ws, bv, code)
    tb = Q.from_f32(t, code)
    assert np.array_equal((tb.view(np.uint32) if code == 2 else tb)[~nan], wb[~nan]), "pre_cast() is not the value the reference casts"
    got = D.classes(want, code, t, acc)
    print(f"\n{M}x{N}x{K} {NAMES[code]} bias={has_bias}: {got}")
    need = set(got) if M > 1 else set(ONE_ROW) & set(got)
    thin = {k: n for k, n in got.items() if k in need and n < FLOOR[M]}
    assert not thin, f"classes below the floor of {FLOOR[M]}: {thin}"
    if M > 1:
        assert got == RECORDED[(M, NAMES[code], has_bias)], "the builder changed: update RECORDED (and check the floors still hold by construction)"
    if has_bias:
        f = Q.to_f32(bv, code)
        assert np.isnan(f).any() and (f == np.inf).any() and (f == -np.inf).any() and ((f == 0) & np.signbit(f)).any() and ((f == 0) & ~np.signbit(f)).any()
        assert (np.abs(f[np.isfinite(f)]) >= D.BIG[code] * 0.99).any()


def test_fp16_meets_the_overflow_tie_and_the_single_rounding_hazard():
    """65520 = 4095 * 16 is halfway between 65504 and the 65536 that rounds to Inf; and products whose EXACT value is not an fp16 tie but whose f32 rounding is (or the
    reverse) exist in the reference: a multiply fused into the fp16 cast (one rounding instead of two) would store another value there"""
    M, N, K = 300, 520, 1280
    a, b, acc, xs, ws = D.build(M, N, K, SEED)
    t = D.pre_cast(acc, xs, ws, None, 1)
    assert (np.abs(t) == np.float32(65520.0)).sum() >= 4
    for M_, floor in ((300, 64), (48, 16), (1, 16)):
        a, b, acc, xs, ws = D.build(M_, N, K, SEED)
        n_h = D.fp16_fold_hazards(acc, xs, ws)
        print(f"\n{M_}x{N}x{K}: a multiply folded into the fp16 convert would change {n_h} elements")
        assert n_h >= floor, (M_, n_h)
