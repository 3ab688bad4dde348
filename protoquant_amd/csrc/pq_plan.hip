// pq_plan.hip — the planners behind the C-ABI of libpq_hip.so (pq_plan.h): which variant, split and tile a shape gets, and the names the query entry points report.
// Nothing here launches; each threshold carries the measurement it came from.
#include <atomic>
#include <climits>
#include <cstdio>
#include <cstring>

#include "pq_launch.h"
#include "pq_plan.h"

namespace pq {

// a GEMM variant: its value, its PQ_FORCE_VARIANT string and the name pq_gemm_variant_name reports
namespace {
const struct { Variant v; const char* option; const char* display; } kVariants[] = {
    {V_GENERIC, "generic", "generic64"},           {V_SP256_16, "sp256_16", "sp256_16x16x64"},          {V_SP128_16, "sp128_16", "sp128x256_16x16x64"},
    {V_SP128X128, "sp128x128", "sp128x128_16x16x64"}, {V_RING128, "ring128", "ring128_16x16x64"},        {V_SKINNY, "skinny", "skinny_16x16x64"},
    {V_RING64X128, "ring64x128", "ring64x128_16x16x64"}, {V_RING64X64, "ring64x64", "ring64x64_16x16x64"}, {V_RING128X160, "ring128x160", "ring128x160_16x16x64"}};

// one attribute of the current device (hipDeviceGetAttribute, cached per device ordinal); `dflt` when it cannot be read or lies outside 1 .. max
template <hipDeviceAttribute_t ATTR>
int device_attr(int dflt, int max) {
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return dflt; }
    int n = cache[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, ATTR, dev) != hipSuccess || n <= 0 || n > max) { (void)hipGetLastError(); n = dflt; }
        cache[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}
}  // namespace

Variant parse_variant(const char* e) {
    if (e && *e)
        for (const auto& r : kVariants)
            if (!strcmp(e, r.option)) return r.v;
    return V_AUTO;
}
Variant forced_variant() { return static_cast<Variant>(opt().variant); }

// CUs of the current device (hipDeviceGetAttribute, cached per device ordinal; a CU-masked or partitioned device reports fewer); PQ_FAKE_CUS overrides
int device_cus() { return opt().fake_cus > 0 ? opt().fake_cus : device_attr<hipDeviceAttributeMultiprocessorCount>(256, INT_MAX); }
// XCDs (L2 domains) of the current device for the tile remaps (hipDeviceAttributeNumberOfXccs, cached; a partitioned device reports fewer); with PQ_FAKE_CUS: one per 32 CUs
int device_xcds() {
    if (opt().fake_cus > 0) return opt().fake_cus >= 32 ? opt().fake_cus / 32 : 1;
    return device_attr<hipDeviceAttributeNumberOfXccs>(8, 64);
}

Variant pick_variant(const int8_t* a, int64_t lda, const int8_t* b, int64_t ldb, int64_t M, int64_t N, int64_t K) {
    const bool ok = pq::gemm_fast_eligible(a, lda, b, ldb, M, N, K);
    const Variant f = forced_variant();
    if (f == V_GENERIC || !ok) return V_GENERIC;
    if (f == V_SKINNY) return M <= 64 ? V_SKINNY : V_RING128;      // the skinny kernel holds at most 4 token tiles
    if (f != V_AUTO) return f;
    // decode-like: stream the weights straight into MFMA fragments (HBM-bound).  One 16-token tile: always (4096x4096 6 us vs 18 us tiled); two token tiles while the tiled
    // grid cannot fill the chip (N <= 8192); three and four token tiles (33 .. 64 tokens) only against narrow matrices (N <= 4096: one round of 16-row blocks; a 5120-wide matrix is a round and a quarter — 64 x 5120 x 11008 43.7 us streaming, 30.7 on 64 x 64 ring tiles) — beyond, the
    // 64-row ring tiles of round 4 have enough tiles and win (HBM-fed: 64 x 6144 x 4096 17.9 -> 13.2 us, 64 x 28672 x 4096 46.7 -> 31.6; but 64 x 4096 x 4096 10.4 against
    // 12.7 and 64 x 4096 x 14336 26.3 against 36.3 stay here: profiles/r04_midm_decode.txt).  PQ_NO_MIDM=1: the round-3 split (<= 64 tokens, N <= 8192).
    // (round 4 audit, tools/dispatch_audit.py --small, two boxes: 17 .. 24 tokens against the widest matrices with K <= 4096 stay with the streaming kernel — 17 x 28672 x 4096
    // 32.2 us against 34.8 for the 64 x 128 ring tile)
    // ... and 9 .. 16 tokens against wide matrices with a LONG K (K >= 8192, N >= 14336: Llama-70B's gate / up at batch 16) go to the ring tiles: 16 x 28672 x 8192 55.5 - 57 us
    // against 59.7 streaming, 16 x 14336 x 8192 28.4 against 30.0 (8 tokens: the streaming kernel still wins at N = 28672, 49 against 55)
    const bool long_k_ring = !opt().no_midm && M > 8 && M <= 16 && N >= 14336 && K >= 8192;
    if ((M <= 16 && !long_k_ring) || (M <= 32 && N <= 8192) || (M <= 64 && N < (opt().no_midm ? 8193 : 4097)) || (!opt().no_midm && M <= 24 && N >= 16384 && K <= 4096)) return V_SKINNY;
    if (M * N < 128 * 128) return V_GENERIC;   // a 256^2 tile would be mostly padding
    // 256x256 tiles unless they fill well under one round of the 256 CUs: then 128(m) x 256(n) tiles double the
    // blocks at ~3/4 of the per-CU rate (ingest-bound) — worth it when they keep everything in one round.
    const int64_t t256 = ((M + 255) / 256) * ((N + 255) / 256), t128 = ((M + 127) / 128) * ((N + 255) / 256);
    const int64_t t128sq = ((M + 127) / 128) * ((N + 127) / 128);
    const int64_t cus = device_cus();          // one workgroup of these tiles per CU: every "fills the chip" threshold below is a share of the CUs THIS device reports (round 5; 256 on a whole MI355X)
    // even 128-row tiles fill at most half the chip: 128 x 128 tiles from a 4-deep DMA ring (gemm_s8_ring128; latency-bound
    // on operand ingest, ~2/3 of the 128 x 256 tile's rate per CU, but twice the blocks and no slab traffic).  Measured:
    // k/v 4096x1024x4096 31 -> 24 us, 70B q/o shard 47 (split-K) -> 40 us, 70B down shard 124 (split-K) -> 119 us.
    if (t128 <= cus / 2 && t128sq > t128) {
        // 64 < M <= 512 (gemm_s8_ring.hip): when the 128 x 128 ring tiles fill well under the chip, SMALLER tiles on every CU — the regime is bound by the L2 -> CU path
        // (profiles/r04_ablate_ring.txt), and a K split over workgroups costs more hand-over than it saves on launches this short (measured: profiles/r04_midm_fsk.txt).  Rounds of the 256 CUs x the measured time of one tile relative to the 128 x 128 ring tile (K = 4096: 14.0 / 13.4 / 9.2 us; profiles/r04_midm.txt);
        // PQ_NO_MIDM=1 restores the round-3 dispatch.
        if (!opt().no_midm && opt().force_splitk <= 1 && opt().fsk <= 1) {      // (a forced slice count — experiments, tests — means the split-K forms)
            auto rounds = [cus](int64_t tiles) { return (double)((tiles + cus - 1) / cus); };
            const double c128 = rounds(t128sq) * 1.00, c64x128 = rounds(((M + 63) / 64) * ((N + 127) / 128)) * 0.95, c64x64 = rounds(((M + 63) / 64) * ((N + 63) / 64)) * 0.66;
            if (c64x64 < c128 && c64x64 <= c64x128) return V_RING64X64;
            if (c64x128 < c128) return V_RING64X128;
        }
        return V_RING128;
    }
    if (t256 <= cus * 5 / 8 && t128 > t256 && t128 <= cus) {
        // round 6: where the 128 x 256 tiles fill at most two thirds of the chip but 128 x 160 tiles make (almost) exactly one round of it — the Llama-3-70B fused-qkv shard
        // 4096 x 1280: 160 against 256 workgroups — the 128 x 160 ring tile (gemm_s8_ringt<128, 160>).  Measured over that class, weights from HBM, two boxes
        // (profiles/r06_dispatch_audit_tile160.txt, r06_ab_tile160.txt): 8 - 14 % ahead on 11 of 12 shapes with K >= 4096 (4096 x 1280 x 4096: +-3 %); everywhere outside the
        // class it loses 8 - 90 %.  PQ_NO_RING160=1 restores the round-5 choice.
        const int64_t t160 = ((M + 127) / 128) * ((N + 159) / 160);
        if (!opt().no_ring160 && opt().force_splitk <= 1 && opt().fsk <= 1 &&      // (a forced slice count — experiments, tests — means the split-K forms, as for the mid-M tiles)
            K >= 4096 && t160 <= cus && t160 * 10 >= cus * 9 && t128 * 3 <= cus * 2) return V_RING128X160;
        return V_SP128_16;
    }
    return V_SP256_16;
}

// Tail split: a grid of T > 256 tiles runs ceil(T/256) rounds of one 256x256 tile per CU, and the last round is as long as
// the others however few tiles it holds.  When that round is poorly filled, the trailing tile columns (or rows) go to a
// second launch of 128(m) x 256(n) tiles instead — twice the blocks, each ~0.65 of a full tile's time (measured) — so
// e.g. 344 tiles cost 1 + 0.65 rounds instead of 2.  Both launches are plain sub-problems (pointer offsets), results are
// unchanged bit for bit.  Returns the split axis (0 none, 1 along N, 2 along M) and the extent of the leading part.
constexpr double kHalfTileCost = 0.58, kSecondLaunchCost = 0.06;   // (round 2: the loader/consumer form of the 128-row tile: 29 vs 51 us per tile at K = 4096)

int tail_split_plan(int64_t M, int64_t N, int64_t* lead) {
    if (opt().no_tailsplit) return 0;
    const int64_t tm = (M + 255) / 256, tn = (N + 255) / 256, tiles = tm * tn, cus = device_cus();
    if (tiles <= cus) return 0;
    auto rounds = [cus](int64_t blocks) { return (double)((blocks + cus - 1) / cus); };
    double best = rounds(tiles) - 0.12;   // a split must save at least ~1/8 of a round to be worth a second launch
    int axis = 0;
    const int64_t hm = (M + 127) / 128;
    for (int64_t c = 1; c < tn; ++c) {    // trailing c tile columns, all rows, as 128-row tiles
        if (hm * c > 2 * cus) break;
        const double cost = rounds(tm * (tn - c)) + rounds(hm * c) * kHalfTileCost + kSecondLaunchCost;
        if (cost < best) { best = cost; axis = 1; *lead = (tn - c) * 256; }
    }
    for (int64_t r = 1; r < tm; ++r) {    // trailing r tile rows, all columns
        const int64_t tail_h = (M - (tm - r) * 256 + 127) / 128;
        if (tail_h * tn > 2 * cus) break;
        const double cost = rounds((tm - r) * tn) + rounds(tail_h * tn) * kHalfTileCost + kSecondLaunchCost;
        if (cost < best) { best = cost; axis = 2; *lead = (tm - r) * 256; }
    }
    return axis;
}

// split-K plan: how many K-slices (1 = none) and which tile height.  Only when the tile grid fills at most half of the
// 256 CUs even with 128-row tiles, K is long enough to amortise the extra pass, and the slices stay multiples of 128.
int splitk_plan(int64_t M, int64_t N, int64_t K, int* tm_out) {
    if (opt().no_splitk) return 1;
    if (opt().force_splitk > 1 && M > 64 && K % (128 * opt().force_splitk) == 0) { *tm_out = 256; return opt().force_splitk; }   // (experiments)
    if (M <= 64 || N < 1 || K < 2048) return 1;    // (M <= 64: the skinny kernel splits K inside the workgroup)
    const int64_t t256 = ((M + 255) / 256) * ((N + 255) / 256), t128 = ((M + 127) / 128) * ((N + 255) / 256);
    // (round 3 split the quarter-filled 256 x 256 grid with a very long K — the Llama-70B `down` shard, 4096 x 1024 x 28672 — four ways here, 99 us against 128 for the
    // ring tile fed from HBM; since round 4 the ring tile's loaders rotate their K walk and it runs 102 us from HBM in ONE launch without a workspace: profiles/r04_rotation.txt)
    const int64_t cus = device_cus();
    const int tm = (t256 <= cus * 5 / 8 && t128 > t256 && t128 <= cus) ? 128 : 256;
    const int64_t tiles = tm == 128 ? t128 : t256;
    if (tiles > cus / 2) return 1;
    // the slab reduction costs ~15 us, and the single-pass alternative for these grids is the 128 x 128 ring tile: split-K
    // only pays when the grid fills at most a quarter of the chip and K is long (measured: 4096x512x8192 32 vs 35 us,
    // 1024x1024x8192 25 vs 34 us; at half-filled grids the ring tile wins at every K)
    if (tiles > cus / 4 || K < 8192) return 1;
    int s = (tiles <= cus / 8 && K >= 12288) ? 8 : 4;       // (128 x 4096 x 14336: 40 us with 4 slices, 28 us with 8)
    while (s > 1 && (K % (128 * s) != 0 || K / s < 1024)) s >>= 1;
    *tm_out = tm;
    return s;
}

// fused split-K (gemm_s8_sp256<..., FSK>: the partial sums of a tile's K-slices are handed over inside the GEMM kernel).  Planned for the half-filled 256 x 256
// grid with a long K (cfg-3 `down`, 2048 x 4096 x 11008): two workgroups per tile, TICKET hand-over (placement-independent: pq_hip.h).  Measured, weights from HBM — what a
// layer inside a model sees (profiles/r04_ab_fsk_forms.txt, r04_rotation.txt): 78.3 us against 86.0 for the 128 x 256 tile (79.2 with its rotated K walk); the symmetric
// exchange of round 3, 76.8, is opt-in (PQ_FSK_SYMMETRIC=1).  PQ_FSK=0 turns the plan off, PQ_FSK=S (experiments) forces S slices wherever the shape admits them.
int fsk_plan(int64_t M, int64_t N, int64_t K) {
    const int f = opt().fsk;
    if (f == 0 || opt().no_splitk || opt().force_splitk > 1 || M <= 64 || f > 8) return 0;
    // (experiments: any grid in the ticket form, which never waits for a workgroup that is not running; the symmetric forms only when every workgroup is resident)
    // (the ticket form deals the K-tiles unevenly where they do not divide — round 6; the symmetric forms keep equal slices)
    if (f > 1) return (K % 128 == 0 && (K / 128) / f >= 5 && (!opt().fsk_symmetric || (K % (128 * f) == 0 && f * (((M + 255) / 256) * ((N + 255) / 256)) <= device_cus()))) ? f : 0;
    const int64_t t256 = ((M + 255) / 256) * ((N + 255) / 256);
    // residency guard: the slices of a tile hand over inside the kernel, one workgroup per CU (160 KiB of LDS): plan it only when the whole grid fits the CUs
    // this device reports (a CU-masked or partitioned device reports fewer) — otherwise the two-pass split-K or the single-pass tile runs
    const int cus = device_cus();
    if (t256 > cus / 4 && t256 <= cus / 2 && K >= 10240 && K % 256 == 0) return 2;          // (2 * t256 <= cus: the whole grid resident)
    // the quarter-filled grid with a very long K — the Llama-70B `down` shard, 4096 x 1024 x 28672 — in four slices (4 * t256 <= cus).  Round 3 ran it with the symmetric
    // exchange (91 us), round 4 dropped the plan when the symmetric form became opt-in (ticket 104 us against 102 for the rotated 128 x 128 ring tile in one pass).
    // Round 5, three runs on two boxes, weights from HBM (profiles/r05_ab_down_shard_forms.txt): ticket 99.1 - 99.5 us, ring tile 106.0 - 114.6, symmetric 93.4 — the
    // placement-independent ticket form is 6 - 13 % ahead, so it is planned again (with the caller's workspace; without one the ring tile runs).  Smaller grids
    // (2048 x 1024 x 28672: 85 us either way) stay with the ring tiles.
    // (the K threshold from tools/dispatch_audit.py on the round-5 build, profiles/r05_dispatch_audit_longk.txt: at K = 16384 the four slices LOSE 10 - 15 % to the ring
    // tile on every such grid — 4096 x 1024 x 16384 68.8 against 62.8 us — at K = 28672 they win 2 - 6 %)
    if (t256 > cus / 8 && t256 <= cus / 4 && K >= 24576 && K % 512 == 0) return 4;
    return 0;
}

// ---- qlinear on STACKED activation codes (what an all-gather of the ranks' int8 column blocks leaves: [G][M][K / G])
// the stacked operand can be walked in place by the loaders of the ring tiles (gemm_s8_ring128, gemm_s8_ringt: KSlabs) when one of them is what the planner picks for the
// shape and runs it single-pass; returns that variant, or V_GENERIC for "take the layout pass"
Variant kslabs_in_place(const int8_t* a, int64_t lda, int64_t slab_stride, int64_t kps, const int8_t* b, int64_t ldb, int64_t M, int64_t N, int64_t K) {
    if (opt().no_kslabs || forced_variant() != V_AUTO || kps % 128 != 0 || K / 128 >= 65536 || (slab_stride & 15) != 0) return V_GENERIC;
    // (eligibility of the fast path is decided on the slab's own leading dimension and base; K itself is the whole K)
    const Variant v = pick_variant(a, lda, b, ldb, M, N, K);
    return (v == V_RING128 || v == V_RING64X128 || v == V_RING64X64 || v == V_RING128X160) ? v : V_GENERIC;
}
// ... and (round 6) by the TICKET form of the fused split-K of the 256 x 256 tile, where that is what the planner runs on the row-major operand (the Llama-70B `down` shard,
// 4096 x 1024 x 28672: four slices over eight slabs, 99 us against 106 - 115 for the ring tile: profiles/r05_ab_down_shard_forms.txt): each slice's K range covers whole
// slabs (or sits inside one) and the asm K-loop's activation cursor jumps at the slab boundaries (gemm_s8_sp256<..., KSL>).  Returns the slice count, 0 = not this way.
int kslabs_fsk_in_place(const int8_t* a, int64_t lda, int64_t slab_stride, int64_t kps, const int8_t* b, int64_t ldb, int64_t M, int64_t N, int64_t K) {
    if (opt().no_kslabs || forced_variant() != V_AUTO || (slab_stride & 15) != 0 || slab_stride >= ((int64_t)1 << 40)) return 0;
    const Variant v = pick_variant(a, lda, b, ldb, M, N, K);
    if (!(v == V_SP256_16 || v == V_SP128_16 || v == V_RING128)) return 0;        // (qlinear_core's `tiled`)
    const int f = fsk_plan(M, N, K);
    return (f > 1 && pq::fsk_kslabs_ok(K, kps, f)) ? f : 0;
}

// ---- grouped GEMM over the experts of a mixture-of-experts layer (gemm_s8_grouped.hip)
// tile of the grouped launch: 0 = 64(m) x 128(n), 1 = 64 x 64.  The host knows only the upper bound of the m-tiles, ceil(M_total / 64) + E.  pick_variant's rule for these
// two tiles — rounds of the device's CUs x (0.95, 0.66), the measured time of one tile — reduces to: 64 x 64 exactly while its grid still fits ONE round of the CUs
// ((2 r - 1) x 0.66 < r x 0.95 only for r = 1).  Those constants were measured on plain M x N grids on one fleet; for grouped grids, where up to E of the counted tiles
// do not exist, the rule is unmeasured.
int grouped_plan(int32_t E, int64_t M_total, int64_t N) {
    if (opt().grouped_tile > 0) return opt().grouped_tile - 1;
    const int64_t mt = (M_total + 63) / 64 + E;
    return mt * ((N + 63) / 64) <= device_cus() ? 1 : 0;
}

// ---- the names the query entry points report
const char* gemm_variant_name(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb) {
    // alignment of the pointers is unknown here: assume 16-byte aligned bases
    const Variant v = pick_variant(reinterpret_cast<const int8_t*>(16), lda, reinterpret_cast<const int8_t*>(16), ldb, M, N, K);
    if (v == V_SP256_16) {
        int64_t lead = 0;
        const int axis = forced_variant() == V_AUTO ? tail_split_plan(M, N, &lead) : 0;
        return axis == 1 ? "sp256_16x16x64 + sp128 tail (N)" : axis == 2 ? "sp256_16x16x64 + sp128 tail (M)" : "sp256_16x16x64";
    }
    for (const auto& r : kVariants)
        if (r.v == v) return r.display;
    return "generic64";
}

// which of the three ways (pq_hip.h) a pq_qlinear_s8_kslabs call with these operands and a workspace of `workspace_bytes` takes (dispatch audits, tests)
const char* kslabs_way_name(const int8_t* a, int64_t lda, int64_t slab_stride, int64_t k_per_slab, const int8_t* b, int64_t ldb, int64_t M, int64_t N, int64_t K,
                            size_t workspace_bytes) {
    if (M <= 0 || N <= 0 || K <= 0 || k_per_slab <= 0 || K % k_per_slab != 0) return "invalid";
    if (K == k_per_slab) return "one slab: pq_qlinear_s8";
    if (const int f = kslabs_fsk_in_place(a, lda, slab_stride, k_per_slab, b, ldb, M, N, K); f > 1 && workspace_bytes >= fsk_workspace_bytes(M, N, f))
        return f == 2 ? "in place: fused split-K x2" : f == 4 ? "in place: fused split-K x4" : f == 8 ? "in place: fused split-K x8" : "in place: fused split-K";
    static const struct Names {      // "in place: " + the variant's option string, built once
        char s[sizeof kVariants / sizeof kVariants[0]][32];
        Names() { for (size_t i = 0; i < sizeof s / sizeof s[0]; ++i) snprintf(s[i], sizeof s[i], "in place: %s", kVariants[i].option); }
    } names;
    const Variant v = kslabs_in_place(a, lda, slab_stride, k_per_slab, b, ldb, M, N, K);      // (a ring tile, or V_GENERIC)
    for (size_t i = 0; v != V_GENERIC && i < sizeof names.s / sizeof names.s[0]; ++i)
        if (kVariants[i].v == v) return names.s[i];
    return "layout pass";
}

const char* grouped_variant_name(int32_t E, int64_t M_total, int64_t N) { return grouped_plan(E, M_total, N) == 0 ? "grouped64x128_16x16x64" : "grouped64x64_16x16x64"; }

}  // namespace pq
