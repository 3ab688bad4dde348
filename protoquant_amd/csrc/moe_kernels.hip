// moe_kernels.hip — the plumbing of a mixture-of-experts layer between the library's GEMM launches (kernels R and C):
//   R  moe_route    topk_ids[T, k] -> offsets[E + 1], row_index[T k], rows_of[T, k], slot_of[T, k] (+ the row scales in grouped order): a STABLE counting sort of the flat
//                   (token, slot) pairs by expert — the result of protoquant_amd.moe.route_plan, element for element
//   C  moe_combine  out[t] = sum_s y[rows_of[t, s]] * w[t, slot_of[t, s]], every product and every partial sum rounded to y's dtype — the bits of moe.combine
// Nothing here waits on another workgroup, takes a ticket or lets the arrival order of an atomic decide a result: the only atomics are LDS counts (sums have no order) and
// one LDS add per (wave, expert, 64-pair step) issued by ONE lane, whose order is the wave's own program order.
#include "pq_common.h"
#include "pq_launch.h"

namespace pq {

// ---------------------------------------------------------------------------------------------------------------------------------------------------- kernel R
constexpr int kRouteThreads = 512, kRouteWaves = kRouteThreads / kWave;
constexpr int kRouteMaxE = 1024;
constexpr int64_t kRouteSingleMax = 4096;       // pairs one workgroup sorts alone, in ONE launch (every decode step)
constexpr int64_t kRouteBlockPairs = 2048;      // pairs per workgroup of the three-launch form ...
constexpr int kRouteMaxBlocks = 256;            // ... until there are this many workgroups; then the blocks grow

struct RouteGeom { int nblk; int64_t ppb; };
static RouteGeom route_geom(int64_t npairs) {
    if (npairs <= kRouteSingleMax) return {1, npairs};
    int64_t ppb = (npairs + kRouteMaxBlocks - 1) / kRouteMaxBlocks;
    ppb = ppb < kRouteBlockPairs ? kRouteBlockPairs : (ppb + kRouteThreads - 1) / kRouteThreads * kRouteThreads;
    return {(int)((npairs + ppb - 1) / ppb), ppb};
}
// workspace of the three-launch form: int32 [nblk][E] (counts of pass 1, turned by pass 2 into each block's exclusive prefix over the blocks before it) + [E] totals.
// Sized from an upper bound of nblk that is monotone in the pair count (nblk itself is not, where the blocks start to grow).
size_t moe_route_workspace_bytes(int64_t npairs, int E) {
    if (npairs <= kRouteSingleMax) return 0;
    int64_t nb = (npairs + kRouteBlockPairs - 1) / kRouteBlockPairs;
    if (nb > kRouteMaxBlocks) nb = kRouteMaxBlocks;
    return ((size_t)(nb + 1) * (size_t)E * sizeof(int32_t) + 255) & ~(size_t)255;
}

// an id as the sort sees it: CLAMPED into [0, E) on its full width (an int64 id is never truncated first)
template <bool I64>
__device__ __forceinline__ int route_id(const void* __restrict__ ids, int64_t ld_ids, int64_t t, int j, int E) {
    if constexpr (I64) {
        const int64_t v = reinterpret_cast<const int64_t*>(ids)[t * ld_ids + j];
        return (int)(v < 0 ? 0 : (v > E - 1 ? E - 1 : v));
    } else {
        const int32_t v = reinterpret_cast<const int32_t*>(ids)[t * ld_ids + j];
        return v < 0 ? 0 : (v > E - 1 ? E - 1 : v);
    }
}
__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int t = __shfl_up(v, off, kWave);
        if (lane >= off) v += t;
    }
    return v;
}

// pass 1 of the three-launch form: counts[block][e] = pairs of expert e among the block's pairs.  Every word of the row is written: the workspace needs no initialisation.
template <bool I64>
__global__ __launch_bounds__(kRouteThreads) void moe_route_count(const void* __restrict__ ids, int64_t ld_ids, int64_t npairs, int k, int E, int64_t ppb,
                                                                 int32_t* __restrict__ counts) {
    __shared__ int32_t cnt[kRouteMaxE];
    for (int e = threadIdx.x; e < E; e += kRouteThreads) cnt[e] = 0;
    __syncthreads();
    const int64_t p0 = (int64_t)blockIdx.x * ppb, p1 = p0 + ppb < npairs ? p0 + ppb : npairs;
    for (int64_t p = p0 + threadIdx.x; p < p1; p += kRouteThreads) {
        const int64_t t = (uint32_t)p / (uint32_t)k;      // (T k < 2^31: a 32-bit division)
        atomicAdd(&cnt[route_id<I64>(ids, ld_ids, t, (int)(p - t * k), E)], 1);      // a count: the order of the adds does not matter
    }
    __syncthreads();
    for (int e = threadIdx.x; e < E; e += kRouteThreads) counts[(int64_t)blockIdx.x * E + e] = cnt[e];
}

// pass 2: one wave per expert walks the blocks in order: counts[b][e] <- sum of counts[b'][e], b' < b; the expert's total goes behind the table
__global__ __launch_bounds__(256) void moe_route_scan(int32_t* __restrict__ counts, int nblk, int E) {
    const int lane = threadIdx.x & 63, e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E) return;
    int run = 0;
    for (int b0 = 0; b0 < nblk; b0 += kWave) {
        const int b = b0 + lane;
        const int v = b < nblk ? counts[(int64_t)b * E + e] : 0;
        const int incl = wave_inclusive_scan(v, lane);
        if (b < nblk) counts[(int64_t)b * E + e] = run + incl - v;
        run += __shfl(incl, kWave - 1, kWave);
    }
    if (lane == 0) counts[(int64_t)nblk * E + e] = run;
}

// pass 3, and with SINGLE the whole routing in one workgroup.  The block's pairs are cut into one contiguous segment per wave.  (1) every wave counts its segment into its own
// LDS row; (2) the totals per expert (SINGLE: summed here; else pass 2's) are scanned into offsets; (3) hist[w][e] becomes the grouped row of the FIRST pair of expert e in
// wave w's segment: offsets[e] + the pairs of e in earlier blocks + in earlier waves of this block; (4) every wave walks its segment 64 pairs at a time, in order: the lanes
// that hold the same expert find each other with one ballot per id bit, a pair's row is the running counter + the number of such lanes below it, and the lowest of them
// advances the counter — flat-pair order, whatever the waves' timing.  A pair then ranks itself among the k pairs of its token (by expert id, ties by slot) for rows_of / slot_of.
template <bool I64, bool SINGLE>
__global__ __launch_bounds__(kRouteThreads) void moe_route_rank(const void* __restrict__ ids, int64_t ld_ids, int64_t npairs, int k, int E, int nbits, int64_t ppb,
                                                                const int32_t* __restrict__ prefix, int nblk, int32_t* __restrict__ offsets,
                                                                int32_t* __restrict__ row_index, int32_t* __restrict__ rows_of, int32_t* __restrict__ slot_of,
                                                                const float* __restrict__ xs, float* __restrict__ xs_sorted) {
    __shared__ int32_t hist[kRouteWaves * kRouteMaxE];
    __shared__ int32_t offs[kRouteMaxE + 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t p0 = (int64_t)blockIdx.x * ppb, p1 = p0 + ppb < npairs ? p0 + ppb : npairs;
    const int64_t seg = ((p1 - p0 + kRouteWaves - 1) / kRouteWaves + kWave - 1) / kWave * kWave;
    const int64_t s0 = p0 + w * seg < p1 ? p0 + w * seg : p1, s1 = s0 + seg < p1 ? s0 + seg : p1;
    int32_t* const mine = hist + w * E;

    for (int i = tid; i < kRouteWaves * E; i += kRouteThreads) hist[i] = 0;
    __syncthreads();
    for (int64_t p = s0 + lane; p < s1; p += kWave) {
        const int64_t t = (uint32_t)p / (uint32_t)k;
        atomicAdd(&mine[route_id<I64>(ids, ld_ids, t, (int)(p - t * k), E)], 1);
    }
    __syncthreads();
    for (int e = tid; e < E; e += kRouteThreads) {
        int tot = 0;
        if constexpr (SINGLE) {
#pragma unroll
            for (int v = 0; v < kRouteWaves; ++v) tot += hist[v * E + e];
        } else {
            tot = prefix[(int64_t)nblk * E + e];
        }
        offs[e + 1] = tot;
    }
    if (tid == 0) offs[0] = 0;
    __syncthreads();
    if (w == 0) {
        int run = 0;
        for (int c = 0; c < E; c += kWave) {
            const int e = c + lane;
            const int incl = wave_inclusive_scan(e < E ? offs[e + 1] : 0, lane);
            if (e < E) offs[e + 1] = run + incl;
            run += __shfl(incl, kWave - 1, kWave);
        }
    }
    __syncthreads();
    if (blockIdx.x == 0)
        for (int e = tid; e <= E; e += kRouteThreads) offsets[e] = offs[e];
    for (int e = tid; e < E; e += kRouteThreads) {
        int run = offs[e];
        if constexpr (!SINGLE) run += prefix[(int64_t)blockIdx.x * E + e];
#pragma unroll
        for (int v = 0; v < kRouteWaves; ++v) {
            const int c = hist[v * E + e];
            hist[v * E + e] = run;
            run += c;
        }
    }
    __syncthreads();

    const int64_t last = npairs - 1;
    for (int64_t base = s0; base < s1; base += kWave) {
        const int64_t p = base + lane;
        const bool valid = p < s1;
        const int64_t t = valid ? (uint32_t)p / (uint32_t)k : 0;
        const int j = valid ? (int)(p - t * k) : 0;
        const int id = valid ? route_id<I64>(ids, ld_ids, t, j, E) : 0;
        unsigned long long same = __ballot(valid);
        for (int b = 0; b < nbits; ++b) {
            const bool bit = (id >> b) & 1;
            const unsigned long long m = __ballot(valid && bit);
            same &= bit ? m : ~m;
        }
        const int leader = valid ? __ffsll((long long)same) - 1 : lane;      // (a valid lane is in its own set: same != 0)
        int first = 0;
        if (valid && lane == leader) first = atomicAdd(&mine[id], __popcll(same));      // one lane per expert and step, steps in the wave's program order
        first = __shfl(first, leader, kWave);
        if (valid) {
            int64_t r = (int64_t)first + __popcll(same & ((1ull << lane) - 1ull));
            r = r < 0 ? 0 : (r > last ? last : r);      // (in range by construction; holds even if the ids are overwritten while the call runs)
            row_index[r] = (int32_t)t;
            if (xs_sorted) xs_sorted[r] = xs[t];
            int s = 0;
            for (int jj = 0; jj < k; ++jj) {
                const int other = route_id<I64>(ids, ld_ids, t, jj, E);
                s += (other < id || (other == id && jj < j)) ? 1 : 0;
            }
            rows_of[t * k + s] = (int32_t)r;
            slot_of[t * k + s] = j;
        }
    }
}

void launch_moe_route(const void* ids, bool ids_are_int64, int64_t ld_ids, int64_t T, int k, int E, int32_t* offsets, int32_t* row_index, int32_t* rows_of,
                      int32_t* slot_of, const float* xs, float* xs_sorted, void* workspace, hipStream_t st) {
    const int64_t npairs = T * k;
    const RouteGeom g = route_geom(npairs);
    int nbits = 0;
    while ((1 << nbits) < E) ++nbits;
    const dim3 block(kRouteThreads);
    if (g.nblk == 1) {
        if (ids_are_int64) moe_route_rank<true, true><<<dim3(1), block, 0, st>>>(ids, ld_ids, npairs, k, E, nbits, npairs, nullptr, 1, offsets, row_index, rows_of, slot_of, xs, xs_sorted);
        else moe_route_rank<false, true><<<dim3(1), block, 0, st>>>(ids, ld_ids, npairs, k, E, nbits, npairs, nullptr, 1, offsets, row_index, rows_of, slot_of, xs, xs_sorted);
        return;
    }
    int32_t* counts = static_cast<int32_t*>(workspace);
    const dim3 grid(g.nblk);
    if (ids_are_int64) moe_route_count<true><<<grid, block, 0, st>>>(ids, ld_ids, npairs, k, E, g.ppb, counts);
    else moe_route_count<false><<<grid, block, 0, st>>>(ids, ld_ids, npairs, k, E, g.ppb, counts);
    moe_route_scan<<<dim3((E + 3) / 4), dim3(256), 0, st>>>(counts, g.nblk, E);
    if (ids_are_int64) moe_route_rank<true, false><<<grid, block, 0, st>>>(ids, ld_ids, npairs, k, E, nbits, g.ppb, counts, g.nblk, offsets, row_index, rows_of, slot_of, xs, xs_sorted);
    else moe_route_rank<false, false><<<grid, block, 0, st>>>(ids, ld_ids, npairs, k, E, nbits, g.ppb, counts, g.nblk, offsets, row_index, rows_of, slot_of, xs, xs_sorted);
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------- kernel C
// One token per TPR threads (a wave for short rows, the workgroup otherwise); a thread owns 16 bytes of the row at a time (VEC) or one element, holds their accumulators
// in registers and streams the token's k source rows once: up to 8 row loads in flight per thread, then the k roundings in order.  Rows and weights of a token are
// wave-uniform: scalar loads.  acc starts at +0 and every step is  p = rne(f32(y) * f32(w)); acc = rne(f32(acc) + f32(p))  — one binary32 operation, then the rounding to
// the element type (Elem<DT>::from_f32 pins the binary32 value for fp16, so no mixed-precision instruction folds the two roundings).
template <int DT> __device__ __forceinline__ float round_to(float f) { return Elem<DT>::to_f32(Elem<DT>::from_f32(f)); }
template <int N> struct CombineAcc { float v[N]; };

template <int DT, bool VEC> struct CombineItem {
    using S = typename Elem<DT>::store_t;
    static constexpr int kElems = VEC ? 16 / Elem<DT>::kBytes : 1;
    static constexpr int kWords = VEC ? 4 : 1;
    uint32_t w[kWords];
    __device__ __forceinline__ void load(const uint8_t* p) {
        if constexpr (VEC) { const v4u v = *reinterpret_cast<const v4u*>(p); w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3]; }
        else if constexpr (DT == PQ_F32) w[0] = *reinterpret_cast<const uint32_t*>(p);
        else w[0] = *reinterpret_cast<const uint16_t*>(p);
    }
    __device__ __forceinline__ float elem(int e) const {
        if constexpr (DT == PQ_F32) return __builtin_bit_cast(float, w[e]);
        else return Elem<DT>::to_f32((uint16_t)(w[e >> 1] >> (16 * (e & 1))));
    }
    __device__ static __forceinline__ void store(uint8_t* p, const float* acc) {
        if constexpr (DT == PQ_F32) {
            if constexpr (VEC) *reinterpret_cast<v4f*>(p) = v4f{acc[0], acc[1], acc[2], acc[3]};
            else *reinterpret_cast<float*>(p) = acc[0];
        } else if constexpr (VEC) {
            v4u v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = (uint32_t)Elem<DT>::from_f32(acc[2 * i]) | ((uint32_t)Elem<DT>::from_f32(acc[2 * i + 1]) << 16);
            *reinterpret_cast<v4u*>(p) = v;
        } else {
            *reinterpret_cast<uint16_t*>(p) = Elem<DT>::from_f32(acc[0]);
        }
    }
};

template <int DT, bool VEC, int U, int NE>
__device__ __forceinline__ void combine_step(CombineAcc<NE>& acc, const uint8_t* __restrict__ ycol, int64_t ldy_bytes, int64_t m_last,
                                             const int32_t* __restrict__ rows, const int32_t* __restrict__ slots, const typename Elem<DT>::store_t* __restrict__ wrow, int k) {
    CombineItem<DT, VEC> it[U];
    float wf[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        int64_t r = rows[u];
        r = r < 0 ? 0 : (r > m_last ? m_last : r);                 // device data: clamped into [0, M_total)
        it[u].load(ycol + r * ldy_bytes);
        int sl = slots[u];
        sl = sl < 0 ? 0 : (sl > k - 1 ? k - 1 : sl);
        wf[u] = Elem<DT>::to_f32(wrow[sl]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const float p = round_to<DT>(it[u].elem(e) * wf[u]);
            acc.v[e] = round_to<DT>(acc.v[e] + p);
        }
}

template <int DT, bool VEC>
__device__ __forceinline__ void combine_item(const uint8_t* __restrict__ ycol, int64_t ldy_bytes, int64_t m_last, const int32_t* __restrict__ rows,
                                             const int32_t* __restrict__ slots, const typename Elem<DT>::store_t* __restrict__ wrow, int k, uint8_t* __restrict__ dst) {
    CombineAcc<CombineItem<DT, VEC>::kElems> acc;
#pragma unroll
    for (int e = 0; e < CombineItem<DT, VEC>::kElems; ++e) acc.v[e] = 0.0f;
    int s = 0;
    for (; s + 8 <= k; s += 8) combine_step<DT, VEC, 8>(acc, ycol, ldy_bytes, m_last, rows + s, slots + s, wrow, k);
    if (k - s >= 4) { combine_step<DT, VEC, 4>(acc, ycol, ldy_bytes, m_last, rows + s, slots + s, wrow, k); s += 4; }
    if (k - s >= 2) { combine_step<DT, VEC, 2>(acc, ycol, ldy_bytes, m_last, rows + s, slots + s, wrow, k); s += 2; }
    if (k - s >= 1) combine_step<DT, VEC, 1>(acc, ycol, ldy_bytes, m_last, rows + s, slots + s, wrow, k);
    CombineItem<DT, VEC>::store(dst, acc.v);
}

template <int DT, int TPR, bool VEC>
__global__ __launch_bounds__(256) void moe_combine_kernel(const uint8_t* __restrict__ y, int64_t ldy_bytes, int64_t M_total, const int32_t* __restrict__ rows_of,
                                                          const int32_t* __restrict__ slot_of, const void* __restrict__ wts, int64_t ld_w, int64_t T, int k, int64_t H,
                                                          uint8_t* __restrict__ out, int64_t ldo_bytes) {
    using S = typename Elem<DT>::store_t;
    constexpr int EPV = 16 / Elem<DT>::kBytes, RPB = 256 / TPR;
    const int lt = threadIdx.x % TPR;
    // (wave-uniform by construction — TPR is a multiple of the wave — and said so to the compiler: rows, slots and weights then come through scalar loads)
    const int64_t t = (int64_t)blockIdx.x * RPB + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / TPR));
    if (t >= T) return;
    const int32_t* rows = rows_of + t * k;
    const int32_t* slots = slot_of + t * k;
    const S* wrow = reinterpret_cast<const S*>(wts) + t * ld_w;
    uint8_t* orow = out + t * ldo_bytes;
    const int64_t m_last = M_total - 1;
    int64_t done = 0;                                              // elements served by the 16-byte path
    if constexpr (VEC) {
        const int64_t nvec = H / EPV;
        for (int64_t v = lt; v < nvec; v += TPR) combine_item<DT, true>(y + v * 16, ldy_bytes, m_last, rows, slots, wrow, k, orow + v * 16);
        done = nvec * EPV;
    }
    for (int64_t c = done + lt; c < H; c += TPR)
        combine_item<DT, false>(y + c * Elem<DT>::kBytes, ldy_bytes, m_last, rows, slots, wrow, k, orow + c * Elem<DT>::kBytes);
}

template <int DT>
void moe_combine_dispatch(const void* y, int64_t ldy, int64_t M_total, const int32_t* rows_of, const int32_t* slot_of, const void* w, int64_t ld_w, int64_t T, int k, int64_t H,
                          void* out, int64_t ld_out, hipStream_t st) {
    constexpr int B = Elem<DT>::kBytes, EPV = 16 / B;
    const uint8_t* yb = static_cast<const uint8_t*>(y);
    uint8_t* ob = static_cast<uint8_t*>(out);
    const bool vec = H >= EPV && ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(out) | (uintptr_t)(ldy * B) | (uintptr_t)(ld_out * B)) & 15) == 0;
    const bool wave = (vec ? (H + EPV - 1) / EPV : H) <= 2 * kWave;          // a row of at most two items per lane: one wave per token, four tokens per workgroup
    const dim3 grid((unsigned)(wave ? (T + 3) / 4 : T)), block(256);
#define PQ_COMBINE(TPR, VEC) moe_combine_kernel<DT, TPR, VEC><<<grid, block, 0, st>>>(yb, ldy * B, M_total, rows_of, slot_of, w, ld_w, T, k, H, ob, ld_out * B)
    if (vec) { if (wave) PQ_COMBINE(64, true); else PQ_COMBINE(256, true); }
    else { if (wave) PQ_COMBINE(64, false); else PQ_COMBINE(256, false); }
#undef PQ_COMBINE
}
template void moe_combine_dispatch<PQ_BF16>(const void*, int64_t, int64_t, const int32_t*, const int32_t*, const void*, int64_t, int64_t, int, int64_t, void*, int64_t, hipStream_t);
template void moe_combine_dispatch<PQ_FP16>(const void*, int64_t, int64_t, const int32_t*, const int32_t*, const void*, int64_t, int64_t, int, int64_t, void*, int64_t, hipStream_t);
template void moe_combine_dispatch<PQ_F32>(const void*, int64_t, int64_t, const int32_t*, const int32_t*, const void*, int64_t, int64_t, int, int64_t, void*, int64_t, hipStream_t);

}  // namespace pq
