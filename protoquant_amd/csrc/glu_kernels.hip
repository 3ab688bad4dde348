// glu_kernels.hip — K1 fused into the CLAMPED gates of a gated expert MLP (QSPEC G1-G6):
//   kind 0, CLAMPED_SILU   (DeepSeek-V4):  h = silu(min(g, L)) * clamp(u, -L, +L)
//   kind 1, ALPHA_SIGMOID  (GPT-OSS):      h = (clamp(u, -L, +L) + 1) * gc * sigmoid(alpha * gc),  gc = min(g, L)
//   -> per-token int8 codes + row scales (the `down` input of the experts), without the 16-bit activation ever going to HBM.
// The kernels and the layout decision are the activation family's (rowmap_kernels.h), the exponential and the quotient producer_device.h's; this file holds the
// op's arithmetic, its trait, the self-test kernel, the host helpers and the instantiations, in an object file of its own.
// Algorithmic traffic: read 2 x elem bytes, write 1 B/elem + 4 B/row (+ elem bytes when h is also requested).
#include <cmath>
#include <cstring>

#include "rowmap_kernels.h"
#include "pq_launch.h"

namespace pq {

enum { GLU_CLAMPED_SILU = PQ_GLU_CLAMPED_SILU, GLU_ALPHA_SIGMOID = PQ_GLU_ALPHA_SIGMOID };

template <int DT> __device__ __forceinline__ v2f store_round(v2f x) {          // "cast" of the specification: a round trip through the storage dtype
    if constexpr (DT == PQ_F32) return x;
    else return Pair<DT>::unpack(Pair<DT>::pack(x));
}

// G1-G5 on NP pairs at once, stage by stage as silu_mul_stage.  Returns the products BEFORE their storage rounding.  Notes on the forms used:
//  - G1 is two v_med3_f32 (min(g, L) = med3(g, -Inf, L)), which turn a NaN into a finite value; the NaN the specification propagates is put back at the end
//    by ONE select per element on "g unordered u" (v_cmp_u_f32 is true when either is a NaN).  -0 passes a med3 unchanged.
//  - CLAMPED_SILU is silu_mul_stage on (gc, uc): gc is a value of the storage dtype, so every short-cut that stage takes for 16-bit rows was admitted for it
//    already (all patterns of the fast-division domain, pq_selftest_silu_short).
//  - ALPHA_SIGMOID keeps the specified polynomial exponential for every dtype.  FASTDIV: the IEEE quotient 1 / d as the arithmetic core of the hardware's own
//    correctly rounded sequence (rcp, one Newton step, the quotient and two residual corrections) without the operand scaling, which is only needed when an
//    intermediate can overflow or lose bits to underflow.  For |a| <= 86 none can: d lies in [1, 2^125), 1 / d in (2^-125, 1], the residuals 1 - d q are exact.
//    A zero needs no exception here (d = 2, every step exact; the sign of a -0 gate comes from gc in gc * s).  Waves holding an |a| that may exceed 86, an Inf or
//    a NaN take the `/` path (GluOp::fast_ok, decided once per wave on the raw bits of g).  pq_selftest_glu_short runs every 16-bit pattern through both.
template <int DT, int KIND, bool FASTDIV, int NP>
__device__ __forceinline__ void glu_stage(const v2f (&g)[NP], const v2f (&u)[NP], float L, float alpha, v2f (&h)[NP]) {
    v2f gc[NP], uc[NP];
    const float ninf = -__builtin_inff();
#pragma unroll
    for (int k = 0; k < NP; ++k) gc[k] = v2f{__builtin_amdgcn_fmed3f(g[k].x, ninf, L), __builtin_amdgcn_fmed3f(g[k].y, ninf, L)};
#pragma unroll
    for (int k = 0; k < NP; ++k) uc[k] = v2f{__builtin_amdgcn_fmed3f(u[k].x, -L, L), __builtin_amdgcn_fmed3f(u[k].y, -L, L)};
    if constexpr (KIND == GLU_CLAMPED_SILU) {
        silu_mul_stage<DT, FASTDIV, NP, FASTDIV && DT != PQ_F32>(gc, uc, h);
    } else {
        v2f a[NP], na[NP], d[NP], s[NP], glu[NP], v[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) a[k] = store_round<DT>(gc[k] * splat(alpha));                                      // G2
        // G3: 1 + exp_spec(-a) (the clamp is a med3 again: a NaN a is a NaN gc, put back below)
#pragma unroll
        for (int k = 0; k < NP; ++k) na[k] = v2f{-a[k].x, -a[k].y};
        exp_spec_stage<NP, true, true>(na, d);
        if constexpr (FASTDIV) {
            v2f one[NP];
#pragma unroll
            for (int k = 0; k < NP; ++k) one[k] = splat(1.0f);
            fast_div_stage<NP>(one, d, s);
        } else {
#pragma unroll
            for (int k = 0; k < NP; ++k) s[k] = v2f{1.0f / d[k].x, 1.0f / d[k].y};
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) s[k] = store_round<DT>(s[k]);                                                       // G3
#pragma unroll
        for (int k = 0; k < NP; ++k) glu[k] = store_round<DT>(gc[k] * s[k]);                                             // G4
#pragma unroll
        for (int k = 0; k < NP; ++k) v[k] = store_round<DT>(uc[k] + splat(1.0f));
#pragma unroll
        for (int k = 0; k < NP; ++k) h[k] = glu[k] * v[k];                                                               // G5 (rounded by the caller)
    }
    const float qnan = __builtin_bit_cast(float, 0x7FC00000u);
#pragma unroll
    for (int k = 0; k < NP; ++k) h[k] = v2f{__builtin_isunordered(g[k].x, u[k].x) ? qnan : h[k].x, __builtin_isunordered(g[k].y, u[k].y) ? qnan : h[k].y};
}
// The fast-division test on the min / max of the |g| bit patterns of a wave (vec_absminmax_bits).  |gc| <= |g| (the clamp only lowers a positive gate), so a
// bound on |g| bounds what the division sees.  CLAMPED_SILU: silu_fast_div_ok as it is (0 < |g| <= 86).  ALPHA_SIGMOID: |g| <= gmax, the largest storage value
// with gmax |alpha| <= 86 and gmax <= 86 (computed on the host, rounded DOWN: 86 is a value of every storage dtype and rounding is monotone, so |a| <= 86).
template <int KIND>
struct GluOp {
    static constexpr int kInputs = 2;
    static constexpr bool kFastSplit = true, kWideRows = true, kSplitModes = false;
    struct Params { float L, alpha; uint32_t gmax_bits; };
    template <int DT> __device__ static __forceinline__ bool fast_ok(uint32_t mn, uint32_t mx, const Params& p) {
        if constexpr (KIND == GLU_CLAMPED_SILU) return silu_fast_div_ok<DT>(mn, mx);
        else return mx <= p.gmax_bits;
    }
    template <int DT, bool FASTDIV> __device__ static __forceinline__ v4u vec(const v4u& gv, const v4u& uv, const Params& p) {
        return map_vec<DT>(gv, uv, [&](const auto& g, const auto& u, auto& h) { glu_stage<DT, KIND, FASTDIV, DT == PQ_F32 ? 2 : 4>(g, u, p.L, p.alpha, h); });
    }
    template <int DT> __device__ static __forceinline__ float spec(float g, float u, const Params& p) {
        return map_one(g, u, [&](const auto& ga, const auto& ua, auto& h) { glu_stage<DT, KIND, false, 1>(ga, ua, p.L, p.alpha, h); });
    }
};

// dev/test kernel: every 16-bit pattern g that fast_ok admits through the shipped sequence (FASTDIV) and the specified one (`/`), against u = 1 and u = -1/2.
// out[0] += patterns admitted, out[1] += patterns whose stored h differs in either.
template <int DT, int KIND>
__global__ __launch_bounds__(256) void glu_short_check(float L, float alpha, uint32_t gmax_bits, unsigned long long* __restrict__ out) {
    const uint32_t pat = blockIdx.x * 256u + threadIdx.x;            // 256 blocks x 256 threads = all 65 536 patterns
    const uint32_t mag = pat & 0x7FFFu;
    const typename GluOp<KIND>::Params p{L, alpha, gmax_bits};
    if (!GluOp<KIND>::template fast_ok<DT>(mag, mag, p)) return;
    const uint32_t one = DT == PQ_BF16 ? 0x3F80u : 0x3C00u, mhalf = DT == PQ_BF16 ? 0xBF00u : 0xB800u;
    const uint32_t gw = pat | (pat << 16), uw = one | (mhalf << 16);
    const v4u gv = v4u{gw, gw, gw, gw}, uv = v4u{uw, uw, uw, uw};
    const v4u a = GluOp<KIND>::template vec<DT, true>(gv, uv, p), b = GluOp<KIND>::template vec<DT, false>(gv, uv, p);
    atomicAdd(&out[0], 1ull);
    if (a[0] != b[0]) atomicAdd(&out[1], 1ull);
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
// limit in the storage dtype (round to nearest even: what torch's clamp does with a Python scalar on a 16-bit tensor); finite, positive input
float glu_limit_in_dtype(int dtype, float limit) {
    if (dtype == PQ_FP16) return (float)(_Float16)limit;
    if (dtype == PQ_BF16) {
        uint32_t b;
        memcpy(&b, &limit, 4);
        b = (b + 0x7FFFu + ((b >> 16) & 1u)) & 0xFFFF0000u;
        memcpy(&limit, &b, 4);
    }
    return limit;
}
// the bit pattern (in vec_absminmax_bits' domain) of the largest storage value gmax with gmax <= 86 and gmax |alpha| <= 86, rounded down
static uint32_t glu_gmax_bits(int dtype, float alpha) {
    float b = 86.0f;
    const float aa = std::fabs(alpha);
    if (aa > 1.0f) {
        b = 86.0f / aa;
        while (b * aa > 86.0f) b = std::nextafterf(b, 0.0f);          // (the f32 product the kernel forms, monotone in b)
    }
    uint32_t bits;
    memcpy(&bits, &b, 4);
    if (dtype == PQ_F32) return bits;
    if (dtype == PQ_BF16) return bits >> 16;                             // truncation rounds a positive value down
    _Float16 hf = (_Float16)b;
    uint16_t hb;
    memcpy(&hb, &hf, 2);
    if ((float)hf > b) hb -= 1;                                          // one pattern down (b >= 2^-14: no wrap)
    return hb;
}

void launch_glu_short_check(int dtype, int kind, float limit, float alpha, unsigned long long* out, hipStream_t st) {
    const float L = glu_limit_in_dtype(dtype, limit);
    const uint32_t gb = glu_gmax_bits(dtype, alpha);
    const dim3 grid(256), block(256);
    if (dtype == PQ_BF16) {
        if (kind == GLU_CLAMPED_SILU) glu_short_check<PQ_BF16, GLU_CLAMPED_SILU><<<grid, block, 0, st>>>(L, alpha, gb, out);
        else glu_short_check<PQ_BF16, GLU_ALPHA_SIGMOID><<<grid, block, 0, st>>>(L, alpha, gb, out);
    } else {
        if (kind == GLU_CLAMPED_SILU) glu_short_check<PQ_FP16, GLU_CLAMPED_SILU><<<grid, block, 0, st>>>(L, alpha, gb, out);
        else glu_short_check<PQ_FP16, GLU_ALPHA_SIGMOID><<<grid, block, 0, st>>>(L, alpha, gb, out);
    }
}

template <int DT>
void glu_quant_dispatch(int kind, const void* g, int64_t ldg, const void* u, int64_t ldu, int64_t rows, int64_t cols, float limit, float alpha, int8_t* q,
                        int64_t ldq, float* scale, void* h_out, int64_t ldh, hipStream_t st) {
    const float L = glu_limit_in_dtype(DT, limit);
    const uint32_t gb = glu_gmax_bits(DT, alpha);
    if (kind == GLU_CLAMPED_SILU) rowmap_dispatch<GluOp<GLU_CLAMPED_SILU>, DT>(g, ldg, u, ldu, rows, cols, {L, alpha, gb}, q, ldq, scale, h_out, ldh, nullptr, st);
    else rowmap_dispatch<GluOp<GLU_ALPHA_SIGMOID>, DT>(g, ldg, u, ldu, rows, cols, {L, alpha, gb}, q, ldq, scale, h_out, ldh, nullptr, st);
}

template void glu_quant_dispatch<PQ_BF16>(int, const void*, int64_t, const void*, int64_t, int64_t, int64_t, float, float, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void glu_quant_dispatch<PQ_FP16>(int, const void*, int64_t, const void*, int64_t, int64_t, int64_t, float, float, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void glu_quant_dispatch<PQ_F32>(int, const void*, int64_t, const void*, int64_t, int64_t, int64_t, float, float, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);

}  // namespace pq
