"""-m gpu: the ROTATED K WALK of the loader / consumer tiles ("K ROTATION in chunks", gemm_s8_ring.hip), asked for by name and at ragged shapes.

The workgroups that stream one weight panel walk each chunk of `ct` K-tiles from different starting points and wrap inside the chunk.  A wrong START is invisible (an
integer sum has no order); a K-tile visited twice, skipped or taken from past K is not — so the cases aim at the chunk bookkeeping: K-tile counts that leave a SHORT LAST
CHUNK under the chunk length in force (the branch `clen = NT - cbase < ct ? NT - cbase : ct`), forced chunk lengths from 3 K-tiles to more than K holds, ragged M and N,
every output kind.  Every comparison is bit for bit against the oracle (exact integer sums + the QSPEC epilogue) and, where a switch is set, against the bits of the
default setting in the same process.

Which switch reaches which tile (read from the launchers):
  * ring128 (launch_gemm_ring128) and sp128_16, the 128 x 256 tile (launch_gemm_fast): PQ_RING_ROT — "" = the rule's chunk, 0 = no rotation, n > 1 = n K-tiles per chunk.
    Both rotate only when `N * K >= (6 << 20)`; the rotation offset is (m-tile index in its band) * chunk / sharers, zero for a single m-tile.
  * ring128x160, ring64x128, ring64x64 (launch_gemm_ringt, rot_plan): PQ_MIDM_CT — "" = the rule's chunk, 1 = no rotation, n > 1 = n K-tiles per chunk.  The 128 x 160
    tile has the 6-MiB rule too; the 64-row tiles rotate at any size.
The split-K forms (two-pass and fused) run the 256 x 256 tile without a loader / consumer split: they never rotate.  What can be held is that a forced chunk length
leaves them alone and that they agree with the rotated single pass (test_split_k_forms_agree_with_the_rotated_single_pass)."""
import functools

import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from oracle import qspec_numpy as Q
from tests.gpu_util import TD, same, to_gpu

pytestmark = pytest.mark.gpu

# Shapes (M, N, K).  For the 128-row tiles a case is VACUOUS unless N * K >= 6 MiB (below it the launchers switch the rotation off) and M > 128 (one m-tile rotates
# by zero): every shape here has both, asserted in _walk().  Ragged in M and in N; K-tile counts (K / 128): 65 (odd), 64, 25 (odd), 101 (prime), 9 — under the rule's
# chunk (8 .. 16 K-tiles for these grids) all but the second leave a short last chunk on the 128 x 128 tile; the second does under every forced length but 16.
SHAPES = [(300, 1000, 8320), (700, 777, 8192), (257, 2100, 3200), (1100, 520, 12928), (130, 6200, 1152)]
KINDS = (0, 1, 2, None)                      # bf16, fp16, f32, the int32 twin
NAMES = {"ring128": b"ring128_16x16x64", "sp128_16": b"sp128x256_16x16x64", "ring128x160": b"ring128x160_16x16x64", "ring64x128": b"ring64x128_16x16x64",
         "ring64x64": b"ring64x64_16x16x64"}


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    from protoquant_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return protoquant_amd


class Problem:
    def __init__(self, M, N, K, pattern):
        rng = np.random.default_rng(M * 1000003 + N * 1009 + K)
        if pattern == "full":                # the whole int8 range, -128 included
            self.a = rng.integers(-128, 128, (M, K), dtype=np.int8)
            self.b = rng.integers(-128, 128, (N, K), dtype=np.int8)
        else:                                # "ktile": activation codes that GROW with the K-tile index against positive weights — replacing K-tile t by K-tile t'
            k = np.arange(K)                 # moves every sum of the row by (t' - t) x (a positive number): one revisit cannot cancel against anything
            self.a = ((k // 128) % 120 + 1 + (np.arange(M) % 7)[:, None]).astype(np.int8)
            self.b = (1 + (np.arange(N)[:, None] + k) % 5).astype(np.int8)
        self.acc = Q.gemm_s8s8s32(self.a, self.b)            # exact (f64 BLAS on integers below 2^53)
        self.xs = (rng.random(M, dtype=np.float32) * 0.1 + 1e-3).astype(np.float32)
        self.ws = (rng.random(N, dtype=np.float32) * 0.01 + 1e-4).astype(np.float32)
        self.bias = {c: Q.from_f32(rng.standard_normal(N).astype(np.float32), c) for c in (0, 1, 2)}
        self.a_g, self.b_g = torch.from_numpy(self.a).cuda(), torch.from_numpy(self.b).cuda()
        self.xs_g, self.ws_g = torch.from_numpy(self.xs).cuda(), torch.from_numpy(self.ws).cuda()
        self.bias_g = {c: to_gpu(self.bias[c], c) for c in (0, 1, 2)}
        self._want = {}

    def want(self, kind, bias):
        key = (kind, bias)
        if key not in self._want:
            self._want[key] = self.acc if kind is None else Q.epilogue(self.acc, self.xs, self.ws, self.bias[kind] if bias else None, kind)
        return self._want[key]

    def run(self, pq, kind, bias):
        if kind is None:
            return pq.int_mm(self.a_g, self.b_g)
        return pq.qlinear_s8(self.a_g, self.xs_g, self.b_g, self.ws_g, self.bias_g[kind] if bias else None, TD[kind])


@functools.lru_cache(maxsize=4)
def problem(M, N, K, pattern="full"):
    return Problem(M, N, K, pattern)


FORMS = [(kind, bias) for kind in KINDS for bias in ((False, True) if kind is not None else (False,))]      # the seven forms of one problem


def _rule_chunk(sharers, tn):
    """rot_chunk_ktiles (gemm_tile_common.h)"""
    panels = (32 + sharers - 1) // sharers
    return min(16, max(4, (2 << 20) // (panels * tn * 128)))


def _walk(variant, M, N, K, ring_rot="", midm_ct=""):
    """(chunk length, sharers) the launcher hands the kernel for this case — and the proof that the case is not vacuous: the rotation is ON (or switched off on purpose)."""
    nt = K // 128
    if variant in ("ring128", "sp128_16", "ring128x160"):
        assert N * K >= (6 << 20) and M > 128, "a 128-row tile rotates only from 6 MiB of weights on and with at least two m-tiles"
    tiles_m = -(-M // (64 if variant.startswith("ring64") else 128))
    if variant == "ring128":                 # gmx = min(tiles_m, 8); ct = ring_rot > 1 ? ring_rot : rot_chunk_ktiles(gmx, 128)
        sh = min(tiles_m, 8)
        ct = int(ring_rot) if ring_rot not in ("", "0") and int(ring_rot) > 1 else _rule_chunk(sh, 128)
    elif variant == "sp128_16":              # ct = ring_rot > 1 ? ring_rot : rot_chunk_ktiles(min(tiles_m, 4), 256)
        sh = min(tiles_m, 4)
        ct = int(ring_rot) if ring_rot not in ("", "0") and int(ring_rot) > 1 else _rule_chunk(sh, 256)
    else:                                    # rot_plan: ct = force > 1 ? force : rot_chunk_ktiles(min(tiles_m, 8), TN)
        sh = min(tiles_m, 8)
        tn = {"ring128x160": 160, "ring64x128": 128, "ring64x64": 64}[variant]
        ct = int(midm_ct) if midm_ct not in ("", "1") else _rule_chunk(sh, tn)
    assert sh >= 2
    return ct, nt


def _check_all_forms(pq, p, what, ref=None):
    """every output kind, with and without bias: == the oracle; returns the outputs (the `ref` of a later call: == those bits too)"""
    outs = {}
    for kind, bias in FORMS:
        got = p.run(pq, kind, bias)
        same(got, p.want(kind, bias), f"{what} kind={kind} bias={bias}")
        if ref is not None:
            assert torch.equal(got.view(torch.uint8), ref[(kind, bias)].view(torch.uint8)), f"{what} kind={kind} bias={bias}: differs from the default setting's bits"
        outs[(kind, bias)] = got
    return outs


def _force(pq_opt, variant, M, N, K):
    from protoquant_amd import _lib
    pq_opt("PQ_FORCE_VARIANT", variant)
    assert _lib.lib().pq_gemm_variant_name(M, N, K, K, K) == NAMES[variant]


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("variant", ["ring128", "sp128_16"])
def test_ring_rot_chunk_lengths(pq, pq_opt, variant, M, N, K):
    """PQ_RING_ROT on the 128 x 128 ring tile and the 128 x 256 tile: the rule's chunk, no rotation, chunks of 3, 5 and 16 K-tiles, and 200 (longer than any K here: one
    chunk that is all of K, rotated as a whole).  Seven forms each, against the oracle and the default's bits."""
    _force(pq_opt, variant, M, N, K)
    p = problem(M, N, K)
    ref = None
    short = []
    for rot in ("", "0", "3", "5", "16", "200"):
        pq_opt("PQ_RING_ROT", rot)
        ct, nt = _walk(variant, M, N, K, ring_rot=rot)
        if rot != "0" and nt % ct != 0 and ct < nt:
            short.append(rot)
        outs = _check_all_forms(pq, p, f"{variant} {M}x{N}x{K} PQ_RING_ROT={rot!r} (chunks of {ct}, {nt} K-tiles)", ref)
        ref = ref or outs
    assert len(short) >= 2, "the short last chunk must run under at least two chunk lengths"


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("variant", ["ring128x160", "ring64x128", "ring64x64"])
def test_midm_ct_chunk_lengths(pq, pq_opt, variant, M, N, K):
    """PQ_MIDM_CT on the tiles of gemm_s8_ringt (two K-tiles per ring slot on the 64-row tiles, so an odd chunk also splits a slot): the rule's chunk, no rotation,
    chunks of 3, 7 and 64 K-tiles."""
    _force(pq_opt, variant, M, N, K)
    p = problem(M, N, K)
    ref = None
    short = []
    for ctv in ("", "1", "3", "7", "64"):
        pq_opt("PQ_MIDM_CT", ctv)
        ct, nt = _walk(variant, M, N, K, midm_ct=ctv)
        if ctv != "1" and nt % ct != 0 and ct < nt:
            short.append(ctv)
        outs = _check_all_forms(pq, p, f"{variant} {M}x{N}x{K} PQ_MIDM_CT={ctv!r} (chunks of {ct}, {nt} K-tiles)", ref)
        ref = ref or outs
    assert len(short) >= 1, "the short last chunk must run under at least one chunk length"


def test_rule_chunk_leaves_a_short_last_chunk_on_every_tile():
    """the shape list does what its comment says: under the RULE's chunk (no switch) every kernel meets at least one K-tile count that is not a multiple of it"""
    for variant in NAMES:
        hits = [(M, N, K) for (M, N, K) in SHAPES if (lambda ct, nt: ct < nt and nt % ct != 0)(*_walk(variant, M, N, K))]
        assert len(hits) >= 2, (variant, hits)


@pytest.mark.parametrize("variant,rot,ctv", [("ring128", "", ""), ("ring128", "5", ""), ("sp128_16", "", ""), ("sp128_16", "3", ""), ("ring128x160", "", ""), ("ring128x160", "", "7"),
                                             ("ring64x128", "", "3"), ("ring64x64", "", "")])
@pytest.mark.parametrize("M,N,K", [(300, 1000, 8320), (1100, 520, 12928)])
def test_a_revisited_k_tile_cannot_cancel(pq, pq_opt, variant, rot, ctv, M, N, K):
    """Activation codes that grow with the K-tile index against positive weights: a walk that takes one K-tile twice and leaves another out moves every sum."""
    _force(pq_opt, variant, M, N, K)
    pq_opt("PQ_RING_ROT", rot)
    pq_opt("PQ_MIDM_CT", ctv)
    _walk(variant, M, N, K, ring_rot=rot, midm_ct=ctv)
    p = problem(M, N, K, "ktile")
    _check_all_forms(pq, p, f"{variant} {M}x{N}x{K} K-tile pattern rot={rot!r} ct={ctv!r}")
    # the C oracle's own integer loop on a few rows, the first and last of every m-tile edge among them (the f64 BLAS route above shares nothing with it)
    rows = sorted({0, 1, 63, 64, 127, 128, M - 2, M - 1})
    assert np.array_equal(p.acc[rows], C.gemm_s8s8s32(p.a[rows], p.b))


@pytest.mark.parametrize("M,N,K", [(2100, 1000, 6528), (2100, 1000, 6656)])
def test_split_k_forms_agree_with_the_rotated_single_pass(pq, pq_opt, M, N, K):
    """The planner's own choice for these shapes is the 128 x 128 ring tile in one pass, rotated (6.5 MiB of weights, 17 m-tiles), here in chunks of 5 K-tiles: 51 and 52
    K-tiles both leave a short last chunk.  PQ_FORCE_SPLITK=3 takes the two-pass split-K only where the slices are whole (`K % (128 * force_splitk) == 0`, splitk_plan:
    51 K-tiles yes, 52 no — the single pass runs again); PQ_FSK=3 deals 52 K-tiles 18 / 17 / 17 in the ticket form.  None of the split-K kernels rotates: the forced chunk
    length must leave them alone.  All of them: the bits of the single pass and of the oracle."""
    from protoquant_amd import _lib
    L = _lib.lib()
    nt = K // 128
    p = problem(M, N, K)
    pq_opt("PQ_RING_ROT", "5")
    pq_opt("PQ_NO_SPLITK", "1")
    assert L.pq_gemm_variant_name(M, N, K, K, K) == NAMES["ring128"] and L.pq_qlinear_workspace_bytes(M, N, K) == 0
    _walk("ring128", M, N, K, ring_rot="5")
    assert nt % 5 != 0
    single = {f: p.run(pq, *f) for f in FORMS if f[0] is not None}
    for f, y in single.items():
        same(y, p.want(*f), f"single pass, chunks of 5 {f}")
    pq_opt("PQ_NO_SPLITK", "")
    pq_opt("PQ_FORCE_SPLITK", "3")
    if nt % 3 == 0:
        assert L.pq_qlinear_workspace_bytes(M, N, K) == 3 * M * N * 4, "three whole slices: the two-pass split-K"
    else:
        assert L.pq_qlinear_workspace_bytes(M, N, K) != 3 * M * N * 4, "slices that are not whole K-tiles are refused"
    for f, y in single.items():
        assert torch.equal(p.run(pq, *f).view(torch.uint8), y.view(torch.uint8)), f"PQ_FORCE_SPLITK=3 {f}"
    pq_opt("PQ_FORCE_SPLITK", "")
    pq_opt("PQ_FSK", "3")
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    assert L.pq_qlinear_workspace_bytes(M, N, K) == ((tiles * 4 * 2 + 255) // 256) * 256 + tiles * 2 * 256 * 256 * 4, "three slices handed over inside the kernel"
    for rep in range(2):
        for f, y in single.items():
            assert torch.equal(p.run(pq, *f).view(torch.uint8), y.view(torch.uint8)), f"PQ_FSK=3 {f} (rep {rep})"


@pytest.mark.parametrize("rot", ["", "5", "0"])
def test_stacked_activation_operand_with_rotation(pq, pq_opt, rot):
    """pq_qlinear_s8_kslabs: three K-slabs of 17 K-tiles walked in place by the rotated 128 x 128 ring tile — the chunk walk composed with the slab arithmetic (K-tile kt
    lives in slab kt / 17), chunks of 16 (the rule) and of 5: neither divides a slab, so chunks straddle slab boundaries."""
    from protoquant_amd import _lib
    from tests.test_gpu_int8_exchange import _way
    M, N, K, G = 2100, 1000, 6528, 3
    kps = K // G
    p = problem(M, N, K)
    pq_opt("PQ_RING_ROT", rot)
    _walk("ring128", M, N, K, ring_rot=rot)
    stacked = p.a_g.reshape(M, G, kps).permute(1, 0, 2).contiguous()
    name, need = _way(_lib.lib(), stacked, p.b_g, M, N, K, kps)
    assert name == "in place: ring128" and need == 0, (name, need)
    for kind, bias in FORMS:
        if kind is None:
            continue
        b = p.bias_g[kind] if bias else None
        got = pq.qlinear_s8_kslabs(stacked, p.xs_g, p.b_g, p.ws_g, b, TD[kind])
        same(got, p.want(kind, bias), f"stacked operand, PQ_RING_ROT={rot!r} kind={kind} bias={bias}")
        assert torch.equal(got.view(torch.uint8), p.run(pq, kind, bias).view(torch.uint8))
