// moe_topk_kernels.hip — K-rt: the expert selection of a mixture-of-experts router after its GEMM — top-k, softmax, renormalisation — in one launch (QSPEC RT1-RT5,
// DESIGN.md §2).
//   logits[T, E] (bf16 / fp16 / f32, leading dimension ld) -> weights[T, k] (bf16 / fp16 / f32, chosen by the caller) and ids[T, k] (int32 / int64), slot 0 the largest
// A row of E <= 1024 logits lives in the registers of G lanes: G = the power of two >= E, at least 4 and at most 64; expert e on lane e mod G, slot e / G (so a slot is
// one coalesced run of the row), NS = the power of two >= ceil(E / G) slots per lane, every index into the per-lane arrays a compile-time constant.  64 / G tokens share
// a wave (K1hn's packing), four waves a block, no barrier, no LDS, no atomics, no workspace.  Nothing depends on T or on which tokens share a wave: a group of G lanes
// sees its own token only (xor offsets below G stay inside the group).
// Selection (RT1-RT2): k rounds of a group-wide arg-max on a 64-bit key — the order-preserving bits of the value (every NaN the largest key, -0 the key of +0), then the
// complemented expert id — so ONE unsigned max is "value descending, id ascending".  The winner's slot gets the key 0, which no value has (-Inf is 0x007FFFFF), and
// lane j of the group keeps round j's winner: it owns output slot j (k <= E <= G while G < 64, k <= 64 = G beyond).
// Weights (RT3 / RT4): lane j decodes its logit and the row maximum from their keys (exact but for the sign of a zero and the payload of a NaN, neither of which the
// result shows: exp_spec(+-0) = 1 and a NaN weight is stored as the canonical NaN) and evaluates exp_spec(l - m) itself.  softmax_topk sums exp_spec over the whole row
// in the pinned order — per lane the slots in order from +0, then the xor butterfly G/2 .. 1 — absent lanes and slots adding +0 (the terms are positive: a + 0 = a).
// The sums over the k selected are sequential in slot order, one lane broadcast per term.  Divisions are IEEE `/`.
// Aliasing: the outputs overlap neither each other nor the logits (pq_api.hip refuses it).
#include "producer_device.h"
#include "pq_launch.h"

namespace pq {

// RT1: the order of the selection on unsigned integers.  NaN (either sign) above +Inf, -0 == +0, and 0 left free for "absent or already taken"
__device__ __forceinline__ uint32_t topk_order_key(float f) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the value a key stands for: +0 for either zero, the canonical NaN for every NaN
__device__ __forceinline__ float topk_key_value(uint32_t key) {
    if (key == 0xFFFFFFFFu) return __builtin_bit_cast(float, 0x7FC00000u);
    return __builtin_bit_cast(float, (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// exp_spec (QSPEC S1-S4) of N values, two per instruction; a NaN argument is put back (exp_spec_stage's clamp makes it finite)
template <int N>
__device__ __forceinline__ void topk_exp(const float (&a)[N], float (&out)[N]) {
    constexpr int NP = N == 1 ? 1 : N / 2;
    v2f av[NP], ov[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) av[p] = N == 1 ? v2f{a[0], a[0]} : v2f{a[2 * p], a[2 * p + (N == 1 ? 0 : 1)]};
    exp_spec_stage<NP, true>(av, ov);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float e = (i & 1) ? ov[i / 2].y : ov[i / 2].x;
        out[i] = a[i] != a[i] ? a[i] : e;
    }
}

template <int DT, int G, int NS>
__global__ __launch_bounds__(256) void moe_topk_kernel(const void* __restrict__ logits, int64_t ld_logits, int64_t T, int E, int k, int kind, int renormalise,
                                                       void* __restrict__ weights, int w_dtype, int64_t ld_w, void* __restrict__ ids, int ids_are_int64, int64_t ld_ids) {
    static_assert(G >= 4 && G <= 64 && (G & (G - 1)) == 0, "G lanes per token: a power of two, 4 .. 64");
    static_assert(NS == 1 || (G == 64 && NS <= 16 && (NS & (NS - 1)) == 0), "more than one slot per lane only on a whole wave");
    using S = typename Elem<DT>::store_t;
    constexpr int TPW = 64 / G;                                // tokens per wave
    const int lane = threadIdx.x & 63, t = lane & (G - 1);
    int64_t tok = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * TPW + lane / G;
    const bool active = tok < T;                               // a group past the last token walks a duplicate of the last token and stores nothing
    tok = active ? tok : T - 1;
    const S* row = reinterpret_cast<const S*>(logits) + tok * ld_logits;
    float l[NS];
    uint32_t key[NS];                                          // 0: no expert here (past E) or already selected
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int e = i * G + t;
        l[i] = Elem<DT>::to_f32(row[e < E ? e : 0]);
        key[i] = e < E ? topk_order_key(l[i]) : 0u;
    }
    uint32_t my_key = 0u, my_id = 0u, max_key = 0u;
    for (int j = 0; j < k; ++j) {                              // RT2: round j finds ids[j]
        uint32_t hi = 0u, id = 0u;
#pragma unroll
        for (int i = 0; i < NS; ++i) {                         // this lane's best: a later slot is a higher id, so only a larger value replaces
            if (key[i] > hi) {
                hi = key[i];
                id = (uint32_t)(i * G + t);
            }
        }
        uint32_t lo = hi ? ~id : 0u;
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) {
            const uint32_t ohi = (uint32_t)__shfl_xor((int)hi, off, 64), olo = (uint32_t)__shfl_xor((int)lo, off, 64);
            const bool take = ohi > hi || (ohi == hi && olo > lo);
            hi = take ? ohi : hi;
            lo = take ? olo : lo;
        }
        const uint32_t win = ~lo;
        if (j == 0) max_key = hi;
        if (t == j) {
            my_key = hi;
            my_id = win;
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) key[i] = (uint32_t)(i * G + t) == win ? 0u : key[i];
    }
    const float m = topk_key_value(max_key);
    float total = 1.0f;
    if (kind == PQ_ROUTER_SOFTMAX_TOPK) {                      // RT3: the sum over the whole row in the pinned order
        float a[NS], x[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) a[i] = l[i] - m;
        topk_exp<NS>(a, x);
        float acc = 0.0f;
#pragma unroll
        for (int i = 0; i < NS; ++i) acc = acc + (i * G + t < E ? x[i] : 0.0f);
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
        total = acc;
    }
    const float mine[1] = {topk_key_value(my_key) - m};
    float xe[1];
    topk_exp<1>(mine, xe);
    float w = xe[0];
    if (kind == PQ_ROUTER_SOFTMAX_TOPK) w = w / total;
    if (kind == PQ_ROUTER_TOPK_SOFTMAX || renormalise) {       // the sum over the k selected, sequential in slot order (lanes past k hold values nobody reads)
        const int base = lane - t;
        float s = __shfl(w, base, 64);
        for (int j = 1; j < k; ++j) s = s + __shfl(w, base + j, 64);
        w = w / s;
    }
    if (w != w) w = __builtin_bit_cast(float, 0x7FC00000u);
    if (!active || t >= k) return;
    const int64_t wo = tok * ld_w + t, io = tok * ld_ids + t;
    if (w_dtype == PQ_BF16) reinterpret_cast<uint16_t*>(weights)[wo] = Elem<PQ_BF16>::from_f32(w);
    else if (w_dtype == PQ_FP16) reinterpret_cast<uint16_t*>(weights)[wo] = Elem<PQ_FP16>::from_f32(w);
    else reinterpret_cast<float*>(weights)[wo] = w;
    if (ids_are_int64) reinterpret_cast<int64_t*>(ids)[io] = (int64_t)my_id;
    else reinterpret_cast<int32_t*>(ids)[io] = (int32_t)my_id;
}

template <int DT>
void moe_topk_dispatch(const void* logits, int64_t ld_logits, int64_t T, int E, int k, int kind, int renormalise, void* weights, int w_dtype, int64_t ld_w, void* ids,
                       bool ids_are_int64, int64_t ld_ids, hipStream_t st) {
    int g_lanes = 4;
    while (g_lanes < E && g_lanes < 64) g_lanes <<= 1;
    int slots = 1;
    while (slots * 64 < E) slots <<= 1;
    const auto go = [&](auto gl, auto ns) {
        constexpr int G = decltype(gl)::value, NS = decltype(ns)::value;
        constexpr int64_t TPB = 4 * (64 / G);                  // tokens per block
        const dim3 grid((unsigned)((T + TPB - 1) / TPB));
        moe_topk_kernel<DT, G, NS><<<grid, dim3(256), 0, st>>>(logits, ld_logits, T, E, k, kind, renormalise, weights, w_dtype, ld_w, ids, ids_are_int64 ? 1 : 0, ld_ids);
    };
    using std::integral_constant;
    const integral_constant<int, 1> one;
    const integral_constant<int, 64> wave;
    if (g_lanes == 4) go(integral_constant<int, 4>{}, one);
    else if (g_lanes == 8) go(integral_constant<int, 8>{}, one);
    else if (g_lanes == 16) go(integral_constant<int, 16>{}, one);
    else if (g_lanes == 32) go(integral_constant<int, 32>{}, one);
    else if (slots == 1) go(wave, one);
    else if (slots == 2) go(wave, integral_constant<int, 2>{});
    else if (slots == 4) go(wave, integral_constant<int, 4>{});
    else if (slots == 8) go(wave, integral_constant<int, 8>{});
    else go(wave, integral_constant<int, 16>{});
}

template decltype(moe_topk_dispatch<PQ_BF16>) moe_topk_dispatch<PQ_BF16>;
template decltype(moe_topk_dispatch<PQ_FP16>) moe_topk_dispatch<PQ_FP16>;
template decltype(moe_topk_dispatch<PQ_F32>) moe_topk_dispatch<PQ_F32>;

}  // namespace pq
