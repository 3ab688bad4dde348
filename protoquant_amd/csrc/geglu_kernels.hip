// geglu_kernels.hip — K1gg: the tanh-GELU gate of a gated MLP fused into the per-token int8 quantisation (QSPEC GG1-GG3, then Q1-Q6):
//   a = cast(gelu_tanh(g))   (QSPEC U2, stored)      h = cast(a * u)      ->  per-token int8 codes + row scales
// the `down` input of a Gemma, Gemma-2 or Gemma-3 MLP (down(act_fn(gate(x)) * up(x)), act_fn = gelu_pytorch_tanh), without the 16-bit intermediate ever going
// to HBM.  Algorithmic traffic: K1s's — read 2 x elem bytes, write 1 B/elem + 4 B/row (5 B/elem for 16-bit rows against 13 for torch's gelu, mul and K1).
// The skeleton is silu_mul_quant_vec's (producer_kernels.hip): TPR threads own a row, every 16-byte load is issued before the first use, the row of h lives in
// registers between the amax reduction and the encode; g and u have leading dimensions of their own (the column halves of one fused gate+up output qualify).
// The U2 sequence is RESTATED here from act_kernels.hip (exp_spec, the fast quotient, the -Inf rule), operation for operation: act_kernels.o keeps its source,
// its kernel list and its register allocation, and tests/test_gpu_geglu.py holds the two statements together on every 16-bit pattern — as rows of 512 sorted by
// magnitude, where whole waves take the division-free quotient on all of its domain, and as wide rows and through the generic kernel, which divide.  The other device helpers
// are CALLED from producer_device.h; the kernels here are templates of their own in an object file of their own.
#include "producer_device.h"
#include "pq_launch.h"

namespace pq {

__device__ __forceinline__ float gg_fbits(uint32_t u) { return __builtin_bit_cast(float, u); }

// QSPEC S1-S4 on NP pairs: exp_spec(a) = p * 2^n (Cody-Waite + degree-7 Horner with fma); ldexp(p, n) equals the specification's two exact power-of-two
// multiplications for every n in [-43, 144] (producer_device.h)
template <int NP>
__device__ __forceinline__ void gg_exp_spec_stage(const v2f (&a)[NP], v2f (&out)[NP]) {
    v2f tc[NP], n[NP], r[NP], p[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) tc[k] = v2f{__builtin_amdgcn_fmed3f(a[k].x, -30.0f, 100.0f), __builtin_amdgcn_fmed3f(a[k].y, -30.0f, 100.0f)};
#pragma unroll
    for (int k = 0; k < NP; ++k) n[k] = tc[k] * splat(gg_fbits(0x3FB8AA3Bu));
#pragma unroll
    for (int k = 0; k < NP; ++k) n[k] = v2f{__builtin_rintf(n[k].x), __builtin_rintf(n[k].y)};
#pragma unroll
    for (int k = 0; k < NP; ++k) r[k] = pk_fma(n[k], splat(-gg_fbits(0x3F317200u)), tc[k]);
#pragma unroll
    for (int k = 0; k < NP; ++k) r[k] = pk_fma(n[k], splat(-gg_fbits(0x35BFBE8Eu)), r[k]);
#pragma unroll
    for (int k = 0; k < NP; ++k) p[k] = pk_fma(splat(gg_fbits(0x39500D01u)), r[k], splat(gg_fbits(0x3AB60B61u)));
    constexpr uint32_t kC[6] = {0x3C088889u, 0x3D2AAAABu, 0x3E2AAAABu, 0x3F000000u, 0x3F800000u, 0x3F800000u};
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int k = 0; k < NP; ++k) p[k] = pk_fma(p[k], r[k], splat(gg_fbits(kC[c])));
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) out[k] = v2f{__builtin_ldexpf(p[k].x, (int)n[k].x), __builtin_ldexpf(p[k].y, (int)n[k].y)};
}

// GG1-GG2 on NP pairs at once, stage by stage as silu_mul_stage.  Returns the products BEFORE their storage rounding.
//  - U2: gelu_tanh(g) = g / (1 + exp_spec(-a)), a = g * fma(g * g, K1, K0).
//  - FASTDIV (decided once per wave on the raw bits of g, geglu_fast_ok — K1u's test): 0 < |g| <= 9.5 keeps a >= -76.4, so d lies in [1, 2^111) and the IEEE
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
    for (int k = 0; k < NP; ++k) w[k] = pk_fma(s[k], splat(gg_fbits(0x3D922279u)), splat(gg_fbits(0x3FCC422Au)));
#pragma unroll
    for (int k = 0; k < NP; ++k) a[k] = -(g[k] * w[k]);
    gg_exp_spec_stage<NP>(a, ex);
#pragma unroll
    for (int k = 0; k < NP; ++k) d[k] = splat(1.0f) + ex[k];
    if constexpr (FASTDIV) {
        v2f y0[NP], y[NP], q[NP], e[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) y0[k] = v2f{__builtin_amdgcn_rcpf(d[k].x), __builtin_amdgcn_rcpf(d[k].y)};
#pragma unroll
        for (int k = 0; k < NP; ++k) e[k] = pk_fma(-d[k], y0[k], splat(1.0f));
#pragma unroll
        for (int k = 0; k < NP; ++k) y[k] = pk_fma(e[k], y0[k], y0[k]);
#pragma unroll
        for (int k = 0; k < NP; ++k) q[k] = g[k] * y[k];
#pragma unroll
        for (int k = 0; k < NP; ++k) e[k] = pk_fma(-d[k], q[k], g[k]);
#pragma unroll
        for (int k = 0; k < NP; ++k) q[k] = pk_fma(e[k], y[k], q[k]);
#pragma unroll
        for (int k = 0; k < NP; ++k) e[k] = pk_fma(-d[k], q[k], g[k]);
#pragma unroll
        for (int k = 0; k < NP; ++k) ge[k] = pk_fma(e[k], y[k], q[k]);
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
template <int DT>
__device__ __forceinline__ float geglu_spec(float g, float u) {
    const v2f ga[1] = {v2f{g, g}}, ua[1] = {v2f{u, u}};
    v2f h[1];
    geglu_stage<DT, false, 1>(ga, ua, h);
    return h[0].x;
}

// the fast-division test on the min / max of the |g| bit patterns of a wave (vec_absminmax_bits): no zero, |g| <= 9.5
template <int DT> __device__ __forceinline__ bool geglu_fast_ok(uint32_t mn, uint32_t mx) {
    constexpr uint32_t k9_5 = DT == PQ_F32 ? 0x41180000u : (DT == PQ_BF16 ? 0x4118u : 0x48C0u);
    return mn != 0u && mx <= k9_5;
}

// one 16-byte vector of g and of u -> one 16-byte vector of h in the storage dtype
template <int DT, bool FASTDIV>
__device__ __forceinline__ v4u geglu_vec(const v4u& gv, const v4u& uv) {
    constexpr int NP = DT == PQ_F32 ? 2 : 4;
    v2f g[NP], u[NP], h[NP];
    v4u out;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        if constexpr (DT == PQ_F32) {
            const uint32_t g0 = gv[2 * j], g1 = gv[2 * j + 1], u0 = uv[2 * j], u1 = uv[2 * j + 1];   // copies first (hipcc quirk, as silu_mul_vec)
            g[j] = v2f{__builtin_bit_cast(float, g0), __builtin_bit_cast(float, g1)};
            u[j] = v2f{__builtin_bit_cast(float, u0), __builtin_bit_cast(float, u1)};
        } else {
            const uint32_t gw = gv[j], uw = uv[j];
            g[j] = Pair<DT>::unpack(gw);
            u[j] = Pair<DT>::unpack(uw);
        }
    }
    geglu_stage<DT, FASTDIV, NP>(g, u, h);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        if constexpr (DT == PQ_F32) {
            const float hx = h[j].x, hy = h[j].y;
            out[2 * j] = __builtin_bit_cast(uint32_t, hx);
            out[2 * j + 1] = __builtin_bit_cast(uint32_t, hy);
        } else {
            out[j] = Pair<DT>::pack(h[j]);
        }
    }
    return out;
}

template <int DT, int VPT, int TPR, bool WRITE_H>
__global__ __launch_bounds__(TPR > 256 ? TPR : 256) void gelu_mul_quant_vec(const uint8_t* __restrict__ g, int64_t ldg_bytes, const uint8_t* __restrict__ u,
                                                                            int64_t ldu_bytes, int64_t rows, int nvec, int8_t* __restrict__ q, int64_t ldq,
                                                                            float* __restrict__ scale, uint8_t* __restrict__ h_out, int64_t ldh_bytes) {
    constexpr int BS = TPR > 256 ? TPR : 256;
    constexpr int RPB = BS / TPR;
    const int t = threadIdx.x % TPR;
    int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / TPR;
    const bool active = row < rows;
    row = active ? row : rows - 1;
    const uint8_t* gr = g + row * ldg_bytes;
    const uint8_t* ur = u + row * ldu_bytes;

    // every load is issued before the first use (clamped addresses: the slots past the row's end are zeroed below)
    v4u gv[VPT], uv[VPT];
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int idx = i * TPR + t;
        const int64_t off = (int64_t)(idx < nvec ? idx : nvec - 1) * 16;
        gv[i] = *reinterpret_cast<const v4u*>(gr + off);
        uv[i] = *reinterpret_cast<const v4u*>(ur + off);
    }
    v4u hv[VPT];
    uint32_t ab = 0;
    uint32_t gmn = 0xFFFFFFFFu, gmx = 0u;
#pragma unroll
    for (int i = 0; i < VPT; ++i) vec_absminmax_bits<DT>(gv[i], gmn, gmx);
    const bool fast_div = __builtin_amdgcn_ballot_w64(!geglu_fast_ok<DT>(gmn, gmx)) == 0ull;   // wave-uniform
    auto produce = [&](auto fast) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int idx = i * TPR + t;
            // slots past the row's end (whole waves of them when the width is not VPT * TPR vectors) skip the arithmetic
            hv[i] = idx < nvec ? geglu_vec<DT, decltype(fast)::value>(gv[i], uv[i]) : v4u{0u, 0u, 0u, 0u};
            ab = vec_amax_bits<DT>(hv[i], ab);
            if constexpr (WRITE_H) {
                if (active && idx < nvec) store_wt_b128(h_out + row * ldh_bytes + (int64_t)idx * 16, hv[i]);
            }
        }
    };
    if (fast_div) produce(std::true_type{});
    else produce(std::false_type{});
    reduce_and_encode<DT, VPT, TPR>(hv, ab, t, nvec, active, row, q, ldq, scale);
}

// generic path: any cols / leading dimensions / alignment.  One block per row; h is recomputed in the second pass (the specified sequence, with `/`).
template <int DT>
__global__ __launch_bounds__(256) void gelu_mul_quant_generic(const void* __restrict__ g, int64_t ldg, const void* __restrict__ u, int64_t ldu, int64_t cols,
                                                              int8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale, void* __restrict__ h_out,
                                                              int64_t ldh) {
    using S = typename Elem<DT>::store_t;
    const int64_t row = blockIdx.x;
    const S* gr = reinterpret_cast<const S*>(g) + row * ldg;
    const S* ur = reinterpret_cast<const S*>(u) + row * ldu;
    auto h_at = [&](int64_t c) -> S { return Elem<DT>::from_f32(geglu_spec<DT>(Elem<DT>::to_f32(gr[c]), Elem<DT>::to_f32(ur[c]))); };
    float amax = 0.0f;
    for (int64_t c = threadIdx.x; c < cols; c += 256) {
        const S h = h_at(c);
        if (h_out) reinterpret_cast<S*>(h_out)[row * ldh + c] = h;
        amax = amax_step(amax, Elem<DT>::to_f32(h));
    }
    amax = wave_max(amax);
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = amax;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) amax = amax_merge(amax, part[w]);
    const float s = scale_of(amax);
    if (threadIdx.x == 0) scale[row] = s;
    int8_t* qr = q + row * ldq;
    for (int64_t c = threadIdx.x; c < cols; c += 256) qr[c] = (int8_t)code_of(Elem<DT>::to_f32(h_at(c)), s);
}

template <int DT, int TPR, bool WRITE_H>
static void launch_gelu_mul_vec(int vpt, const uint8_t* g, int64_t ldg_b, const uint8_t* u, int64_t ldu_b, int64_t rows, int nvec, int8_t* q, int64_t ldq,
                                float* scale, uint8_t* h, int64_t ldh_b, hipStream_t st) {
    constexpr int BS = TPR > 256 ? TPR : 256, RPB = BS / TPR;
    const dim3 grid((unsigned)((rows + RPB - 1) / RPB)), block(BS);
#define PQ_GEGLU_LAUNCH(V) gelu_mul_quant_vec<DT, V, TPR, WRITE_H><<<grid, block, 0, st>>>(g, ldg_b, u, ldu_b, rows, nvec, q, ldq, scale, h, ldh_b)
    switch (vpt) {
        case 1:
            if constexpr (TPR != 512) PQ_GEGLU_LAUNCH(1);
            break;
        case 2:
            if constexpr (TPR != 512) PQ_GEGLU_LAUNCH(2);
            break;
        case 3:
            if constexpr (TPR == 512) PQ_GEGLU_LAUNCH(3);
            break;
        case 4:
            if constexpr (TPR != 512) PQ_GEGLU_LAUNCH(4);
            break;
        case 8:
            if constexpr (TPR == 256) PQ_GEGLU_LAUNCH(8);
            break;
        default:
            if constexpr (TPR == 256) PQ_GEGLU_LAUNCH(16);
            break;
    }
#undef PQ_GEGLU_LAUNCH
}

// Row layouts as silu_mul_quant_dispatch: one wave per row up to 256 vectors (1, 2, 4 per lane), 512 threads x 3 vectors for rows of 1025 .. 1536 vectors
// (pq_set_option("PQ_SILU_TPR", "256") turns that one off, as for K1s), else 256 threads x 1 .. 16 vectors; anything else — ragged width, unaligned pointer or
// leading dimension, more than 4096 vectors — is generic.  Time only, never bits.
template <int DT>
void gelu_mul_quant_dispatch(const void* g, int64_t ldg, const void* u, int64_t ldu, int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale, void* h_out,
                             int64_t ldh, hipStream_t st) {
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    const bool vec_ok = cols > 0 && (cols % EPV == 0) && (ldg % EPV == 0) && (ldu % EPV == 0) && aligned_to(g, 16) && aligned_to(u, 16) && (ldq % EPV == 0) &&
                        aligned_to(q, EPV) && cols / EPV <= 256 * 16 && (!h_out || ((ldh % EPV == 0) && aligned_to(h_out, 16)));
    if (!vec_ok) {
        gelu_mul_quant_generic<DT><<<dim3((unsigned)rows), dim3(256), 0, st>>>(g, ldg, u, ldu, cols, q, ldq, scale, h_out, ldh);
        return;
    }
    const int nvec = (int)(cols / EPV);
    auto pow2 = [](int v) { int p = 1; while (p < v) p <<= 1; return p; };
    const uint8_t* gb = reinterpret_cast<const uint8_t*>(g);
    const uint8_t* ub = reinterpret_cast<const uint8_t*>(u);
    uint8_t* hb = reinterpret_cast<uint8_t*>(h_out);
    const int64_t kb = Elem<DT>::kBytes;
#define PQ_GEGLU_ROWS(TPR, VPT)                                                                                                      \
    do {                                                                                                                             \
        if (h_out) launch_gelu_mul_vec<DT, TPR, true>(VPT, gb, ldg * kb, ub, ldu * kb, rows, nvec, q, ldq, scale, hb, ldh * kb, st);  \
        else launch_gelu_mul_vec<DT, TPR, false>(VPT, gb, ldg * kb, ub, ldu * kb, rows, nvec, q, ldq, scale, hb, 0, st);              \
    } while (0)
    if (nvec <= 64 * 4) PQ_GEGLU_ROWS(64, pow2((nvec + 63) / 64));
    else if (nvec > 1024 && nvec <= 1536 && opt().silu_tpr != 256) PQ_GEGLU_ROWS(512, 3);
    else PQ_GEGLU_ROWS(256, pow2((nvec + 255) / 256));
#undef PQ_GEGLU_ROWS
}

template void gelu_mul_quant_dispatch<PQ_BF16>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void gelu_mul_quant_dispatch<PQ_FP16>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void gelu_mul_quant_dispatch<PQ_F32>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);

}  // namespace pq
