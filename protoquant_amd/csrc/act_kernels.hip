// act_kernels.hip — K1u: a unary activation fused into the per-token int8 quantisation (QSPEC U1-U4, then Q1-Q6):
//   kind 0, RELU        h = x < 0 ? +0 : x
//   kind 1, GELU_TANH   h = x / (1 + exp(-a)),  a = x (K0 + K1 x^2) = 2 sqrt(2/pi) (x + 0.044715 x^3)       (gelu_new, gelu_pytorch_tanh)
//   kind 2, GELU_ERF    h = x Phi(x),  Phi(x) = 0.5 erfc(-x / sqrt 2)                                          (F.gelu's default)
//   -> per-token int8 codes + row scales (the input of the second projection of a plain two-linear MLP: GPT-2's c_proj, StarCoder2's, GPT-NeoX's
//   dense_4h_to_h), without the 16-bit activation ever going to HBM.  Algorithmic traffic: read elem bytes, write 1 B/elem + 4 B/row (3 B/elem for 16-bit rows
//   against 7 for torch's activation followed by K1).
// The skeleton is silu_mul_quant_vec's (producer_kernels.hip) with one input instead of two: TPR threads own a row, every 16-byte load is issued before the first
// use, the row of h lives in registers between the amax reduction and the encode.  The device helpers are CALLED from producer_device.h; the kernels here are
// templates of their own in an object file of their own.
#include "producer_device.h"
#include "pq_launch.h"

namespace pq {

enum { ACT_RELU = PQ_ACT_RELU, ACT_GELU_TANH = PQ_ACT_GELU_TANH, ACT_GELU_ERF = PQ_ACT_GELU_ERF };

__device__ __forceinline__ float fbits(uint32_t u) { return __builtin_bit_cast(float, u); }

// QSPEC S1-S4 on NP pairs: exp_spec(a) = p * 2^n.  CLAMP = false when the caller guarantees -30 <= a <= 100 (the clamp is then the identity).
template <int NP, bool CLAMP>
__device__ __forceinline__ void exp_spec_stage(const v2f (&a)[NP], v2f (&out)[NP]) {
    v2f tc[NP], n[NP], r[NP], p[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        if constexpr (CLAMP) tc[k] = v2f{__builtin_amdgcn_fmed3f(a[k].x, -30.0f, 100.0f), __builtin_amdgcn_fmed3f(a[k].y, -30.0f, 100.0f)};
        else tc[k] = a[k];
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) n[k] = tc[k] * splat(fbits(0x3FB8AA3Bu));
#pragma unroll
    for (int k = 0; k < NP; ++k) n[k] = v2f{__builtin_rintf(n[k].x), __builtin_rintf(n[k].y)};
#pragma unroll
    for (int k = 0; k < NP; ++k) r[k] = pk_fma(n[k], splat(-fbits(0x3F317200u)), tc[k]);
#pragma unroll
    for (int k = 0; k < NP; ++k) r[k] = pk_fma(n[k], splat(-fbits(0x35BFBE8Eu)), r[k]);
#pragma unroll
    for (int k = 0; k < NP; ++k) p[k] = pk_fma(splat(fbits(0x39500D01u)), r[k], splat(fbits(0x3AB60B61u)));
    constexpr uint32_t kC[6] = {0x3C088889u, 0x3D2AAAABu, 0x3E2AAAABu, 0x3F000000u, 0x3F800000u, 0x3F800000u};
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int k = 0; k < NP; ++k) p[k] = pk_fma(p[k], r[k], splat(fbits(kC[c])));
    }
    // ldexp(p, n) equals the specification's two exact power-of-two multiplications for every n in [-43, 144] (producer_device.h)
#pragma unroll
    for (int k = 0; k < NP; ++k) out[k] = v2f{__builtin_ldexpf(p[k].x, (int)n[k].x), __builtin_ldexpf(p[k].y, (int)n[k].y)};
}

// The IEEE quotient g / d as the arithmetic core of the hardware's own correctly rounded sequence (rcp, one Newton step, the quotient and two residual
// corrections) without the operand scaling: exact for 0 <= |g| <= 86 and d in [1, 2^125) (producer_device.h, silu_mul_stage).  A zero g loses its sign in the
// residual steps: callers that care keep zeros out (GELU_TANH) or need +0 from +0 (GELU_ERF, where g = t - 4 is never -0).
template <int NP>
__device__ __forceinline__ void fast_div_stage(const v2f (&g)[NP], const v2f (&d)[NP], v2f (&out)[NP]) {
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
    for (int k = 0; k < NP; ++k) out[k] = pk_fma(e[k], y[k], q[k]);
}

// U1-U3 on NP pairs at once, stage by stage as silu_mul_stage.  Returns h BEFORE its storage rounding.
//  - RELU: one compare and select per element (a NaN and -0 fail the compare and pass).
//  - GELU_TANH is silu's division with another argument.  FASTDIV (decided once per wave on the raw bits of x, act_fast_ok): 0 < |x| <= 9.5 keeps a >= -76.4, so
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
template <int DT, int KIND>
__device__ __forceinline__ float act_spec(float x) {
    const v2f xa[1] = {v2f{x, x}};
    v2f h[1];
    act_stage<DT, KIND, false, 1>(xa, h);
    return h[0].x;
}

// the fast-division test of GELU_TANH on the min / max of the |x| bit patterns of a wave (vec_absminmax_bits): no zero, |x| <= 9.5
template <int DT> __device__ __forceinline__ bool act_fast_ok(uint32_t mn, uint32_t mx) {
    constexpr uint32_t k9_5 = DT == PQ_F32 ? 0x41180000u : (DT == PQ_BF16 ? 0x4118u : 0x48C0u);
    return mn != 0u && mx <= k9_5;
}

// one 16-byte vector of x -> one 16-byte vector of h in the storage dtype
template <int DT, int KIND, bool FASTDIV>
__device__ __forceinline__ v4u act_vec(const v4u& xv) {
    constexpr int NP = DT == PQ_F32 ? 2 : 4;
    v2f x[NP], h[NP];
    v4u out;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        if constexpr (DT == PQ_F32) {
            const uint32_t x0 = xv[2 * j], x1 = xv[2 * j + 1];   // copies first (hipcc quirk, as silu_mul_vec)
            x[j] = v2f{__builtin_bit_cast(float, x0), __builtin_bit_cast(float, x1)};
        } else {
            const uint32_t xw = xv[j];
            x[j] = Pair<DT>::unpack(xw);
        }
    }
    act_stage<DT, KIND, FASTDIV, NP>(x, h);
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

template <int DT, int KIND, int VPT, int TPR, bool WRITE_H>
__global__ __launch_bounds__(TPR > 256 ? TPR : 256) void act_quant_vec(const uint8_t* __restrict__ x, int64_t ldx_bytes, int64_t rows, int nvec,
                                                                       int8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale,
                                                                       uint8_t* __restrict__ h_out, int64_t ldh_bytes) {
    constexpr int BS = TPR > 256 ? TPR : 256;
    constexpr int RPB = BS / TPR;
    const int t = threadIdx.x % TPR;
    int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / TPR;
    const bool active = row < rows;
    row = active ? row : rows - 1;
    const uint8_t* xr = x + row * ldx_bytes;

    // every load is issued before the first use (clamped addresses: the slots past the row's end are zeroed below)
    v4u xv[VPT];
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int idx = i * TPR + t;
        xv[i] = *reinterpret_cast<const v4u*>(xr + (int64_t)(idx < nvec ? idx : nvec - 1) * 16);
    }
    v4u hv[VPT];
    uint32_t ab = 0;
    bool fast_div = false;
    if constexpr (KIND == ACT_GELU_TANH) {
        uint32_t mn = 0xFFFFFFFFu, mx = 0u;
#pragma unroll
        for (int i = 0; i < VPT; ++i) vec_absminmax_bits<DT>(xv[i], mn, mx);
        fast_div = __builtin_amdgcn_ballot_w64(!act_fast_ok<DT>(mn, mx)) == 0ull;   // wave-uniform
    }
    auto produce = [&](auto fast) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int idx = i * TPR + t;
            // slots past the row's end (whole waves of them when the width is not VPT * TPR vectors) skip the arithmetic
            hv[i] = idx < nvec ? act_vec<DT, KIND, decltype(fast)::value>(xv[i]) : v4u{0u, 0u, 0u, 0u};
            ab = vec_amax_bits<DT>(hv[i], ab);
            if constexpr (WRITE_H) {
                if (active && idx < nvec) store_wt_b128(h_out + row * ldh_bytes + (int64_t)idx * 16, hv[i]);
            }
        }
    };
    if constexpr (KIND == ACT_GELU_TANH) {
        if (fast_div) produce(std::true_type{});
        else produce(std::false_type{});
    } else {
        produce(std::false_type{});
    }
    reduce_and_encode<DT, VPT, TPR>(hv, ab, t, nvec, active, row, q, ldq, scale);
}

// generic path: any cols / leading dimensions / alignment.  One block per row; h is recomputed in the second pass (the specified sequence, with `/`).
template <int DT, int KIND>
__global__ __launch_bounds__(256) void act_quant_generic(const void* __restrict__ x, int64_t ldx, int64_t cols, int8_t* __restrict__ q, int64_t ldq,
                                                         float* __restrict__ scale, void* __restrict__ h_out, int64_t ldh) {
    using S = typename Elem<DT>::store_t;
    const int64_t row = blockIdx.x;
    const S* xr = reinterpret_cast<const S*>(x) + row * ldx;
    auto h_at = [&](int64_t c) -> S { return Elem<DT>::from_f32(act_spec<DT, KIND>(Elem<DT>::to_f32(xr[c]))); };
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

template <int DT, int KIND, int TPR, bool WRITE_H>
static void launch_act_vec(int vpt, const uint8_t* x, int64_t ldx_b, int64_t rows, int nvec, int8_t* q, int64_t ldq, float* scale, uint8_t* h, int64_t ldh_b,
                           hipStream_t st) {
    constexpr int BS = TPR > 256 ? TPR : 256, RPB = BS / TPR;
    const dim3 grid((unsigned)((rows + RPB - 1) / RPB)), block(BS);
    switch (vpt) {
        case 1:
            if constexpr (TPR != 512) act_quant_vec<DT, KIND, 1, TPR, WRITE_H><<<grid, block, 0, st>>>(x, ldx_b, rows, nvec, q, ldq, scale, h, ldh_b);
            break;
        case 2:
            if constexpr (TPR != 512) act_quant_vec<DT, KIND, 2, TPR, WRITE_H><<<grid, block, 0, st>>>(x, ldx_b, rows, nvec, q, ldq, scale, h, ldh_b);
            break;
        case 3:
            if constexpr (TPR == 512) act_quant_vec<DT, KIND, 3, TPR, WRITE_H><<<grid, block, 0, st>>>(x, ldx_b, rows, nvec, q, ldq, scale, h, ldh_b);
            break;
        case 4:
            if constexpr (TPR != 512) act_quant_vec<DT, KIND, 4, TPR, WRITE_H><<<grid, block, 0, st>>>(x, ldx_b, rows, nvec, q, ldq, scale, h, ldh_b);
            break;
        case 8:
            if constexpr (TPR == 256) act_quant_vec<DT, KIND, 8, TPR, WRITE_H><<<grid, block, 0, st>>>(x, ldx_b, rows, nvec, q, ldq, scale, h, ldh_b);
            break;
        default:
            if constexpr (TPR == 256) act_quant_vec<DT, KIND, 16, TPR, WRITE_H><<<grid, block, 0, st>>>(x, ldx_b, rows, nvec, q, ldq, scale, h, ldh_b);
            break;
    }
}

// Row layouts as silu_mul_quant_dispatch: one wave per row up to 256 vectors (1, 2, 4 per lane), 512 threads x 3 vectors for rows of 1025 .. 1536 vectors
// (pq_set_option("PQ_SILU_TPR", "256") turns that one off, as for K1s), else 256 threads x 1 .. 16 vectors; anything else is generic.  Time only, never bits.
template <int DT, int KIND>
static void act_quant_dispatch_kind(const void* x, int64_t ldx, int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale, void* h_out, int64_t ldh,
                                    hipStream_t st) {
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    const bool vec_ok = cols > 0 && (cols % EPV == 0) && (ldx % EPV == 0) && aligned_to(x, 16) && (ldq % EPV == 0) && aligned_to(q, EPV) &&
                        cols / EPV <= 256 * 16 && (!h_out || ((ldh % EPV == 0) && aligned_to(h_out, 16)));
    if (!vec_ok) {
        act_quant_generic<DT, KIND><<<dim3((unsigned)rows), dim3(256), 0, st>>>(x, ldx, cols, q, ldq, scale, h_out, ldh);
        return;
    }
    const int nvec = (int)(cols / EPV);
    auto pow2 = [](int v) { int p = 1; while (p < v) p <<= 1; return p; };
    const uint8_t* xb = reinterpret_cast<const uint8_t*>(x);
    uint8_t* hb = reinterpret_cast<uint8_t*>(h_out);
    const int64_t kb = Elem<DT>::kBytes;
    if (nvec <= 64 * 4) {
        const int vpt = pow2((nvec + 63) / 64);
        if (h_out) launch_act_vec<DT, KIND, 64, true>(vpt, xb, ldx * kb, rows, nvec, q, ldq, scale, hb, ldh * kb, st);
        else launch_act_vec<DT, KIND, 64, false>(vpt, xb, ldx * kb, rows, nvec, q, ldq, scale, hb, 0, st);
    } else if (nvec > 1024 && nvec <= 1536 && opt().silu_tpr != 256) {
        if (h_out) launch_act_vec<DT, KIND, 512, true>(3, xb, ldx * kb, rows, nvec, q, ldq, scale, hb, ldh * kb, st);
        else launch_act_vec<DT, KIND, 512, false>(3, xb, ldx * kb, rows, nvec, q, ldq, scale, hb, 0, st);
    } else {
        const int vpt = pow2((nvec + 255) / 256);
        if (h_out) launch_act_vec<DT, KIND, 256, true>(vpt, xb, ldx * kb, rows, nvec, q, ldq, scale, hb, ldh * kb, st);
        else launch_act_vec<DT, KIND, 256, false>(vpt, xb, ldx * kb, rows, nvec, q, ldq, scale, hb, 0, st);
    }
}

template <int DT>
void act_quant_dispatch(int kind, const void* x, int64_t ldx, int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale, void* h_out, int64_t ldh,
                        hipStream_t st) {
    switch (kind) {
        case ACT_RELU: act_quant_dispatch_kind<DT, ACT_RELU>(x, ldx, rows, cols, q, ldq, scale, h_out, ldh, st); break;
        case ACT_GELU_TANH: act_quant_dispatch_kind<DT, ACT_GELU_TANH>(x, ldx, rows, cols, q, ldq, scale, h_out, ldh, st); break;
        default: act_quant_dispatch_kind<DT, ACT_GELU_ERF>(x, ldx, rows, cols, q, ldq, scale, h_out, ldh, st); break;
    }
}

template void act_quant_dispatch<PQ_BF16>(int, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void act_quant_dispatch<PQ_FP16>(int, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void act_quant_dispatch<PQ_F32>(int, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);

}  // namespace pq
