// act_kernels.hip — K1u: a unary activation fused into the per-token int8 quantisation (QSPEC U1-U4, then Q1-Q6):
//   kind 0, RELU        h = x < 0 ? +0 : x
//   kind 1, GELU_TANH   h = x / (1 + exp(-a)),  a = x (K0 + K1 x^2) = 2 sqrt(2/pi) (x + 0.044715 x^3)       (gelu_new, gelu_pytorch_tanh)
//   kind 2, GELU_ERF    h = x Phi(x),  Phi(x) = 0.5 erfc(-x / sqrt 2)                                          (F.gelu's default)
//   -> per-token int8 codes + row scales (the input of the second projection of a plain two-linear MLP: GPT-2's c_proj, StarCoder2's, GPT-NeoX's
//   dense_4h_to_h), without the 16-bit activation ever going to HBM.  Algorithmic traffic: read elem bytes, write 1 B/elem + 4 B/row (3 B/elem for 16-bit rows
//   against 7 for torch's activation followed by K1).
// The kernels and the layout decision are the activation family's (rowmap_kernels.h) with one input instead of two, the exponential and the quotient
// producer_device.h's; this file holds the op's arithmetic, its trait and the instantiations, in an object file of its own.
#include "rowmap_kernels.h"
#include "pq_launch.h"

namespace pq {

enum { ACT_RELU = PQ_ACT_RELU, ACT_GELU_TANH = PQ_ACT_GELU_TANH, ACT_GELU_ERF = PQ_ACT_GELU_ERF };

// U1-U3 on NP pairs at once, stage by stage as silu_mul_stage.  Returns h BEFORE its storage rounding.
//  - RELU: one compare and select per element (a NaN and -0 fail the compare and pass).
//  - GELU_TANH is silu's division with another argument.  FASTDIV (decided once per wave on the raw bits of x, ActOp::fast_ok): 0 < |x| <= 9.5 keeps a >= -76.4, so
//    d = 1 + exp(-a) lies in [1, 2^111) and the quotient is fast_div_stage's; other waves (a zero, a large |x|, Inf, NaN) take `/`.  -Inf gives -0 (the limit; x / d
//    would be -Inf / Inf), chosen on the `/` path only — the fast path never sees an Inf.
//  - GELU_ERF has one path: |x| is clamped to 12 FIRST (a v_med3_f32: a NaN comes out finite and returns through x * Phi), so every intermediate is in the range
//    the fast quotient and the unclamped exponential need: v = (t - 4) / (t + 4) with t + 4 in [4, 16]; exp(-t^2 / 2) as the fourth power of
//    exp_spec(-t^2 / 8) (argument >= -18: exp_spec clamps at -30); for f32 rows the rounding error of t * t is carried to first order (an fma recovers it exactly;
//    it is zero for a t of a 16-bit type — at most 11 significant bits — and those rows skip the two operations).
template <int DT, int KIND, bool FASTDIV, int NP>
__device__ __forceinline__ void act_stage(const v2f (&x)[NP], v2f (&h)[NP]) {
    if constexpr (KIND == ACT_RELU) {
#pragma unroll
        for (int k = 0; k < NP; ++k) h[k] = v2f{x[k].x < 0.0f ? 0.0f : x[k].x, x[k].y < 0.0f ? 0.0f : x[k].y};
    } else if constexpr (KIND == ACT_GELU_TANH) {
        v2f s[NP], w[NP], a[NP], ex[NP], d[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) s[k] = x[k] * x[k];
#pragma unroll
        for (int k = 0; k < NP; ++k) w[k] = pk_fma(s[k], splat(fbits(0x3D922279u)), splat(fbits(0x3FCC422Au)));
#pragma unroll
        for (int k = 0; k < NP; ++k) a[k] = -(x[k] * w[k]);
        exp_spec_stage<NP, true>(a, ex);
#pragma unroll
        for (int k = 0; k < NP; ++k) d[k] = splat(1.0f) + ex[k];
        if constexpr (FASTDIV) {
            fast_div_stage<NP>(x, d, h);
        } else {
            const float ninf = -__builtin_inff();
#pragma unroll
            for (int k = 0; k < NP; ++k) h[k] = v2f{x[k].x == ninf ? -0.0f : x[k].x / d[k].x, x[k].y == ninf ? -0.0f : x[k].y / d[k].y};
        }
    } else {
        v2f t[NP], g[NP], d[NP], v[NP], p[NP], s[NP], a[NP], ex[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) t[k] = v2f{__builtin_amdgcn_fmed3f(__builtin_fabsf(x[k].x), 0.0f, 12.0f), __builtin_amdgcn_fmed3f(__builtin_fabsf(x[k].y), 0.0f, 12.0f)};
#pragma unroll
        for (int k = 0; k < NP; ++k) g[k] = t[k] - splat(4.0f);
#pragma unroll
        for (int k = 0; k < NP; ++k) d[k] = t[k] + splat(4.0f);
        fast_div_stage<NP>(g, d, v);
        constexpr uint32_t kQ[11] = {0x3DC15A5Eu, 0xBE2E7CBEu, 0x3DFEBA8Bu, 0xBD92DB41u, 0x3CFCD8BAu, 0xBC0B29CDu, 0x3A046D68u, 0x3A29677Du, 0xB93891BBu, 0xB866CA2Du, 0x370ACBB8u};
#pragma unroll
        for (int k = 0; k < NP; ++k) p[k] = splat(fbits(kQ[10]));
#pragma unroll
        for (int c = 9; c >= 0; --c) {
#pragma unroll
            for (int k = 0; k < NP; ++k) p[k] = pk_fma(p[k], v[k], splat(fbits(kQ[c])));
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) s[k] = t[k] * t[k];
#pragma unroll
        for (int k = 0; k < NP; ++k) a[k] = s[k] * splat(-0.125f);
        exp_spec_stage<NP, false>(a, ex);
#pragma unroll
        for (int k = 0; k < NP; ++k) ex[k] = ex[k] * ex[k];
#pragma unroll
        for (int k = 0; k < NP; ++k) ex[k] = ex[k] * ex[k];
        if constexpr (DT == PQ_F32) {
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const v2f e = pk_fma(t[k], t[k], -s[k]);
                ex[k] = pk_fma(ex[k], e * splat(-0.5f), ex[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const v2f pn = ex[k] * p[k];
            const v2f pp = splat(1.0f) - pn;
            const v2f phi = v2f{x[k].x < 0.0f ? pn.x : pp.x, x[k].y < 0.0f ? pn.y : pp.y};
            const v2f hh = x[k] * phi;
            h[k] = v2f{x[k].x < -12.0f ? -0.0f : hh.x, x[k].y < -12.0f ? -0.0f : hh.y};
        }
    }
}
// One input: u is never read.  Only GELU_TANH has a division that some waves may skip (its test on the min / max of the |x| bit patterns of a wave,
// vec_absminmax_bits: no zero, |x| <= 9.5); RELU and GELU_ERF have one form.
template <int KIND>
struct ActOp {
    static constexpr int kInputs = 1;
    static constexpr bool kFastSplit = KIND == ACT_GELU_TANH, kWideRows = true, kSplitModes = false;
    struct Params {};
    template <int DT> __device__ static __forceinline__ bool fast_ok(uint32_t mn, uint32_t mx, Params) {
        constexpr uint32_t k9_5 = DT == PQ_F32 ? 0x41180000u : (DT == PQ_BF16 ? 0x4118u : 0x48C0u);
        return mn != 0u && mx <= k9_5;
    }
    template <int DT, bool FASTDIV> __device__ static __forceinline__ v4u vec(const v4u& xv, const v4u&, Params) {
        return map_vec<DT>(xv, xv, [](const auto& x, const auto&, auto& h) { act_stage<DT, KIND, FASTDIV, DT == PQ_F32 ? 2 : 4>(x, h); });
    }
    template <int DT> __device__ static __forceinline__ float spec(float x, float, Params) {
        return map_one(x, x, [](const auto& xa, const auto&, auto& h) { act_stage<DT, KIND, false, 1>(xa, h); });
    }
};

template <int DT>
void act_quant_dispatch(int kind, const void* x, int64_t ldx, int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale, void* h_out, int64_t ldh,
                        hipStream_t st) {
    switch (kind) {
        case ACT_RELU: rowmap_dispatch<ActOp<ACT_RELU>, DT>(x, ldx, nullptr, 0, rows, cols, {}, q, ldq, scale, h_out, ldh, nullptr, st); break;
        case ACT_GELU_TANH: rowmap_dispatch<ActOp<ACT_GELU_TANH>, DT>(x, ldx, nullptr, 0, rows, cols, {}, q, ldq, scale, h_out, ldh, nullptr, st); break;
        default: rowmap_dispatch<ActOp<ACT_GELU_ERF>, DT>(x, ldx, nullptr, 0, rows, cols, {}, q, ldq, scale, h_out, ldh, nullptr, st); break;
    }
}

template void act_quant_dispatch<PQ_BF16>(int, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void act_quant_dispatch<PQ_FP16>(int, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void act_quant_dispatch<PQ_F32>(int, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);

}  // namespace pq
