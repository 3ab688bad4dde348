// geglu_kernels.hip — K1gg: the tanh-GELU gate of a gated MLP fused into the per-token int8 quantisation (QSPEC GG1-GG3, then Q1-Q6):
//   a = cast(gelu_tanh(g))   (QSPEC U2, stored)      h = cast(a * u)      ->  per-token int8 codes + row scales
// the `down` input of a Gemma, Gemma-2 or Gemma-3 MLP (down(act_fn(gate(x)) * up(x)), act_fn = gelu_pytorch_tanh), without the 16-bit intermediate ever going
// to HBM.  Algorithmic traffic: K1s's — read 2 x elem bytes, write 1 B/elem + 4 B/row (5 B/elem for 16-bit rows against 13 for torch's gelu, mul and K1).
// The kernels and the layout decision are the activation family's (rowmap_kernels.h); the exponential and the quotient are producer_device.h's, the ones K1u's
// GELU (act_kernels.hip) is built from, and tests/test_gpu_geglu.py holds the two gates together on every 16-bit pattern — as rows of 512 sorted by magnitude, where
// whole waves take the division-free quotient on all of its domain, and as wide rows and through the generic kernel, which divide.  This file holds the op's
// arithmetic, its trait and the instantiations, in an object file of its own.
#include "rowmap_kernels.h"
#include "pq_launch.h"

namespace pq {

// GG1-GG2 on NP pairs at once, stage by stage as silu_mul_stage.  Returns the products BEFORE their storage rounding.
//  - U2: gelu_tanh(g) = g / (1 + exp_spec(-a)), a = g * fma(g * g, K1, K0).
//  - FASTDIV (decided once per wave on the raw bits of g, GegluOp::fast_ok — K1u's test): 0 < |g| <= 9.5 keeps a >= -76.4, so d lies in [1, 2^111) and the IEEE
//    quotient is the arithmetic core of the hardware's own correctly rounded sequence (rcp, one Newton step, the quotient and two residual corrections) without
//    the operand scaling: no intermediate can overflow or lose bits to underflow, the residuals g - d q are exact.  Other waves (a zero, whose sign the residual
//    steps would lose, a large |g|, Inf, NaN) take `/`; -Inf gives -0 (the limit), chosen on that path only.  A NaN g gives NaN through the quotient.
//  - GG1's storage rounding comes BEFORE the product, as the eager chain stores act_fn(gate) before it multiplies.
template <int DT, bool FASTDIV, int NP>
__device__ __forceinline__ void geglu_stage(const v2f (&g)[NP], const v2f (&u)[NP], v2f (&h)[NP]) {
    v2f s[NP], w[NP], a[NP], ex[NP], d[NP], ge[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) s[k] = g[k] * g[k];
#pragma unroll
    for (int k = 0; k < NP; ++k) w[k] = pk_fma(s[k], splat(fbits(0x3D922279u)), splat(fbits(0x3FCC422Au)));
#pragma unroll
    for (int k = 0; k < NP; ++k) a[k] = -(g[k] * w[k]);
    exp_spec_stage<NP, true>(a, ex);
#pragma unroll
    for (int k = 0; k < NP; ++k) d[k] = splat(1.0f) + ex[k];
    if constexpr (FASTDIV) {
        fast_div_stage<NP>(g, d, ge);
    } else {
        const float ninf = -__builtin_inff();
#pragma unroll
        for (int k = 0; k < NP; ++k) ge[k] = v2f{g[k].x == ninf ? -0.0f : g[k].x / d[k].x, g[k].y == ninf ? -0.0f : g[k].y / d[k].y};
    }
    if constexpr (DT != PQ_F32) {
#pragma unroll
        for (int k = 0; k < NP; ++k) ge[k] = Pair<DT>::unpack(Pair<DT>::pack(ge[k]));          // GG1
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) h[k] = ge[k] * u[k];                                           // GG2 (rounded by the caller)
}
// the fast-division test on the min / max of the |g| bit patterns of a wave (vec_absminmax_bits): no zero, |g| <= 9.5 — K1u's test
struct GegluOp {
    static constexpr int kInputs = 2;
    static constexpr bool kFastSplit = true, kWideRows = true, kSplitModes = false;
    struct Params {};
    template <int DT> __device__ static __forceinline__ bool fast_ok(uint32_t mn, uint32_t mx, Params) {
        constexpr uint32_t k9_5 = DT == PQ_F32 ? 0x41180000u : (DT == PQ_BF16 ? 0x4118u : 0x48C0u);
        return mn != 0u && mx <= k9_5;
    }
    template <int DT, bool FASTDIV> __device__ static __forceinline__ v4u vec(const v4u& gv, const v4u& uv, Params) {
        return map_vec<DT>(gv, uv, [](const auto& g, const auto& u, auto& h) { geglu_stage<DT, FASTDIV, DT == PQ_F32 ? 2 : 4>(g, u, h); });
    }
    template <int DT> __device__ static __forceinline__ float spec(float g, float u, Params) {
        return map_one(g, u, [](const auto& ga, const auto& ua, auto& h) { geglu_stage<DT, false, 1>(ga, ua, h); });
    }
};

template <int DT>
void gelu_mul_quant_dispatch(const void* g, int64_t ldg, const void* u, int64_t ldu, int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale, void* h_out,
                             int64_t ldh, hipStream_t st) {
    rowmap_dispatch<GegluOp, DT>(g, ldg, u, ldu, rows, cols, {}, q, ldq, scale, h_out, ldh, nullptr, st);
}

template void gelu_mul_quant_dispatch<PQ_BF16>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void gelu_mul_quant_dispatch<PQ_FP16>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void gelu_mul_quant_dispatch<PQ_F32>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);

}  // namespace pq
