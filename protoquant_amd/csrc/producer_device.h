// producer_device.h — the device helpers shared by the producer-fused quantisation kernels (rowmap_kernels.h: K1s, K1g, K1gg, K1u; rownorm_kernels.h: the norm
// family): two-elements-per-instruction arithmetic, the arithmetic stages every activation is built from (the specified exponential, the division-free quotient,
// the unpack / stage / pack wrapper, each stated ONCE), the QSPEC S1-S5 stage, and the second half of K1 (row amax + exact encode) on a row of h held in registers.
// Every function is __forceinline__: a translation unit that includes this header instantiates its own kernels only.
#pragma once
#include <type_traits>

#include "quant_device.h"

namespace pq {

typedef float v2f __attribute__((ext_vector_type(2)));

// Two elements at a time: gfx950 issues v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 at the rate of their scalar forms,
// and one v_cvt_pk_bf16_f32 rounds both.  This kernel is VALU-bound before it is HBM-bound (about 50 scalar VALU ops
// per element against 5 bytes), so the pairing is what moves it.
__device__ __forceinline__ v2f splat(float v) { return v2f{v, v}; }
__device__ __forceinline__ v2f pk_fma(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }

template <int DT> struct Pair;            // one 32-bit word of storage <-> two floats
template <> struct Pair<PQ_BF16> {
    typedef __bf16 st2 __attribute__((ext_vector_type(2)));
    __device__ static __forceinline__ v2f unpack(uint32_t w) { return v2f{__builtin_bit_cast(float, w << 16), __builtin_bit_cast(float, w & 0xFFFF0000u)}; }
    __device__ static __forceinline__ uint32_t pack(v2f f) { return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, st2)); }
};
template <> struct Pair<PQ_FP16> {
    typedef _Float16 st2 __attribute__((ext_vector_type(2)));
    __device__ static __forceinline__ v2f unpack(uint32_t w) { return __builtin_convertvector(__builtin_bit_cast(st2, w), v2f); }
    __device__ static __forceinline__ uint32_t pack(v2f f) {
        asm volatile("" : "+v"(f));     // a materialised f32 pair: no v_fma_mixlo_f16 folding (see Elem<PQ_FP16>::from_f32)
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, st2));
    }
};

__device__ __forceinline__ float fbits(uint32_t u) { return __builtin_bit_cast(float, u); }

// QSPEC S1-S4 on NP pairs: exp_spec(a) = p * 2^n (Cody-Waite + degree-7 Horner with fma), stage by stage (see silu_mul_stage).  The clamp is v_med3_f32 (a NaN comes
// out finite: every caller puts the NaN back or divides a NaN by the result); CLAMP = false when the caller guarantees -30 <= a <= 100 (the clamp is then the
// identity).  ldexp(p, n) equals the specification's two exact power-of-two multiplications for every n in [-43, 144].  PLUS1: out = 1 + exp_spec(a), the add
// in the statement of the ldexp (where K1s and K1g had it: a loop of its own after this one gives them another schedule).
template <int NP, bool CLAMP, bool PLUS1 = false>
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
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        if constexpr (PLUS1) out[k] = splat(1.0f) + v2f{__builtin_ldexpf(p[k].x, (int)n[k].x), __builtin_ldexpf(p[k].y, (int)n[k].y)};
        else out[k] = v2f{__builtin_ldexpf(p[k].x, (int)n[k].x), __builtin_ldexpf(p[k].y, (int)n[k].y)};
    }
}

// The IEEE quotient g / d without v_div_scale / v_div_fmas / v_div_fixup: the arithmetic core of the hardware's own correctly rounded sequence (rcp, one Newton
// step, the quotient and two residual corrections) without the operand scaling.  Exact for 0 <= |g| <= 86 and d in [1, 2^125) (see silu_mul_stage).  A zero g loses
// its sign in the residual steps: callers that care keep zeros out or need +0 from +0.  K1g's 1 / d hands it an array of ones (the product 1 * y folds to y).
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

// one 16-byte vector of g and of u -> NP pairs of floats each -> stage(g, u, h) -> one 16-byte vector of h rounded to the storage dtype
template <int DT, class Stage>
__device__ __forceinline__ v4u map_vec(const v4u& gv, const v4u& uv, Stage&& stage) {
    constexpr int NP = DT == PQ_F32 ? 2 : 4;
    v2f g[NP], u[NP], h[NP];
    v4u out;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        if constexpr (DT == PQ_F32) {
            const uint32_t g0 = gv[2 * j], g1 = gv[2 * j + 1], u0 = uv[2 * j], u1 = uv[2 * j + 1];   // copies first (hipcc quirk)
            g[j] = v2f{__builtin_bit_cast(float, g0), __builtin_bit_cast(float, g1)};
            u[j] = v2f{__builtin_bit_cast(float, u0), __builtin_bit_cast(float, u1)};
        } else {
            const uint32_t gw = gv[j], uw = uv[j];
            g[j] = Pair<DT>::unpack(gw);
            u[j] = Pair<DT>::unpack(uw);
        }
    }
    stage(g, u, h);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        if constexpr (DT == PQ_F32) {
            const float hx = h[j].x, hy = h[j].y;   // copies first: bit_cast of a vector-element lvalue reads element 0
            out[2 * j] = __builtin_bit_cast(uint32_t, hx);
            out[2 * j + 1] = __builtin_bit_cast(uint32_t, hy);
        } else {
            out[j] = Pair<DT>::pack(h[j]);
        }
    }
    return out;
}

// QSPEC S1-S5 on NP pairs at once, written stage by stage so that NP independent instructions follow each other: one
// wave's dependent v_pk_fma chain leaves the VALU idle most of the time (measured: 2x off the issue rate), NP chains do
// not.  Notes on the forms used:
//  - the clamp is v_med3_f32 (a NaN comes out finite): the only consumer divides g by 1 + exp(-g), so a NaN g still
//    yields NaN, exactly as the specification's pass-through does;
//  - ldexp(p, n) equals the specification's two exact power-of-two multiplications for every n in [-43, 144];
//  - FASTDIV: the IEEE quotient g / d without v_div_scale / v_div_fmas / v_div_fixup, which serialise on VCC and run at
//    ~6 results/clk/CU against ~100 for an fma (tools/ubench/valu_rate).  It is the arithmetic core of the hardware's own
//    correctly rounded sequence — rcp, one Newton step, the quotient and two residual corrections — without the operand
//    scaling, which is only needed when an intermediate can overflow or lose bits to underflow.  For 0 < |g| <= 86 none
//    can: d lies in [1, 2^125), the residuals g - d*q are exact (for |g| < 2^-25, d is exactly 2 and every step is an exact
//    scaling).  Waves holding a zero (whose sign the residual steps would lose), |g| > 86, Inf or NaN take the `/` path
//    (silu_fast_div_ok, decided once per wave).
// Returns the products BEFORE their storage rounding.
//  - SHORT (16-bit storage only): silu(g) is rounded to the storage format before the product, and g itself is a 16-bit value, so
//    the stored silu(g) is a function of 65 536 inputs.  On ALL of the fast-division domain ONE residual correction on the raw rcp
//    (q = g*y0; e = fma(-d, q, g); q = fma(e, y0, q)) rounds to the same stored value as the correctly rounded quotient — enumerated on
//    the GPU (pq_selftest_silu_short, tests/test_gpu_parity.py::test_silu_short_division_whole_domain); the Newton step and the second
//    correction (4 of ~40 VALU results per element) are dropped for bf16 / fp16 rows.
template <int DT, bool FASTDIV, int NP, bool SHORT = false>
__device__ __forceinline__ void silu_mul_stage(const v2f (&g)[NP], const v2f (&u)[NP], v2f (&h)[NP]) {
    v2f d[NP], sg[NP];
    if constexpr (FASTDIV && SHORT && DT == PQ_BF16) {
        // bf16 rows on the fast-division domain: 1 + exp(-g) from the hardware's exp2 (v_exp_f32, ~1 ulp).  The STORED silu(g) is a function of
        // the 16-bit g alone, and on every one of the 34 136 patterns of the domain this sequence stores the value the specified polynomial
        // exponential + correctly rounded quotient store (tools/ubench/silu_variants enumerates the candidates; pq_selftest_silu_short
        // re-checks the shipped one on the GPU it runs on).  Fourteen VALU results per element fewer.  (fp16 keeps the polynomial: with its
        // 11-bit significand two patterns differ.)
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const v2f a = g[k] * splat(-fbits(0x3FB8AA3Bu));          // -g * log2(e)
            d[k] = splat(1.0f) + v2f{__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y)};
        }
    } else {
        v2f a[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) a[k] = v2f{-g[k].x, -g[k].y};
        exp_spec_stage<NP, true, true>(a, d);
    }
    if constexpr (FASTDIV && SHORT) {
        v2f y0[NP], q[NP], e[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) y0[k] = v2f{__builtin_amdgcn_rcpf(d[k].x), __builtin_amdgcn_rcpf(d[k].y)};
#pragma unroll
        for (int k = 0; k < NP; ++k) q[k] = g[k] * y0[k];
#pragma unroll
        for (int k = 0; k < NP; ++k) e[k] = pk_fma(-d[k], q[k], g[k]);
#pragma unroll
        for (int k = 0; k < NP; ++k) sg[k] = pk_fma(e[k], y0[k], q[k]);
    } else if constexpr (FASTDIV) {
        fast_div_stage<NP>(g, d, sg);
    } else {
#pragma unroll
        for (int k = 0; k < NP; ++k) sg[k] = v2f{g[k].x / d[k].x, g[k].y / d[k].y};
    }
    if constexpr (DT != PQ_F32) {
#pragma unroll
        for (int k = 0; k < NP; ++k) sg[k] = Pair<DT>::unpack(Pair<DT>::pack(sg[k]));
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) h[k] = sg[k] * u[k];
}
// one element through a stage (the specified sequence of the generic kernels): the first lane of one pair
template <class Stage>
__device__ __forceinline__ float map_one(float g, float u, Stage&& stage) {
    const v2f ga[1] = {v2f{g, g}}, ua[1] = {v2f{u, u}};
    v2f h[1];
    stage(ga, ua, h);
    return h[0].x;
}

// min / max of |g| over one 16-byte vector, on raw bit patterns (the same ordering trick as vec_amax_bits)
template <int DT>
__device__ __forceinline__ void vec_absminmax_bits(const v4u& v, uint32_t& mn, uint32_t& mx) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (DT == PQ_F32) {
            const uint32_t a = v[i] & 0x7FFFFFFFu;
            mn = a < mn ? a : mn;
            mx = a > mx ? a : mx;
        } else {
            const uint32_t a = v[i] & 0x7FFF7FFFu, lo = a & 0xFFFFu, hi = a >> 16;
            mn = min(mn, min(lo, hi));
            mx = max(mx, max(lo, hi));
        }
    }
}
template <int DT> __device__ __forceinline__ bool silu_fast_div_ok(uint32_t mn, uint32_t mx) {
    constexpr uint32_t k86 = DT == PQ_F32 ? 0x42AC0000u : (DT == PQ_BF16 ? 0x42ACu : 0x5560u);   // 86.0
    return mn != 0u && mx <= k86;
}

// one 16-byte vector of g and of u -> one 16-byte vector of h in the storage dtype
template <int DT, bool FASTDIV, bool SHORT = (DT != PQ_F32)>
__device__ __forceinline__ v4u silu_mul_vec(const v4u& gv, const v4u& uv) {
    return map_vec<DT>(gv, uv, [](const auto& g, const auto& u, auto& h) { silu_mul_stage<DT, FASTDIV, DT == PQ_F32 ? 2 : 4, SHORT && DT != PQ_F32>(g, u, h); });
}

// division-free exact encode (quant_device.h) of one 16-byte vector of h, two elements per instruction
template <int DT>
__device__ __forceinline__ void fast_encode_vec(const v4u& hv, float s, float r, uint32_t (&pk)[(16 / Elem<DT>::kBytes) / 4]) {
    const v2f vs = splat(s), vr = splat(r);
    uint32_t mb[16 / Elem<DT>::kBytes];
#pragma unroll
    for (int j = 0; j < (16 / Elem<DT>::kBytes) / 2; ++j) {
        v2f x;
        if constexpr (DT == PQ_F32) {
            const uint32_t a = hv[2 * j], b = hv[2 * j + 1];
            x = v2f{__builtin_bit_cast(float, a), __builtin_bit_cast(float, b)};
        } else {
            const uint32_t w = hv[j];
            x = Pair<DT>::unpack(w);
        }
        v2f q = x * vr;
        v2f e = pk_fma(-q, vs, x);
        q = pk_fma(e, vr, q);
        if constexpr (kQuotientSteps<DT> == 2) {          // 16-bit h: one step is exact for the code (quant_device.h)
            e = pk_fma(-q, vs, x);
            q = pk_fma(e, vr, q);
        }
        const v2f m = q + splat(kMagic);
        const float mx = m.x, my = m.y;       // copies first (same hipcc quirk)
        mb[2 * j] = __builtin_bit_cast(uint32_t, mx);
        mb[2 * j + 1] = __builtin_bit_cast(uint32_t, my);
    }
#pragma unroll
    for (int k = 0; k < (16 / Elem<DT>::kBytes) / 4; ++k)
        pk[k] = __builtin_amdgcn_perm(mb[4 * k + 1], mb[4 * k], 0x0c0c0400u) | __builtin_amdgcn_perm(mb[4 * k + 3], mb[4 * k + 2], 0x04000c0cu);
}

// The second half of K1, shared by the producer-fused kernels, in two steps: the row amax of the h vectors held in registers (bit-pattern
// max: a NaN propagates into the scale) as an f32 bit pattern, then scale + the division-free exact encode (or the true-division
// path for NaN/Inf data and extreme scales) for a GIVEN row amax.  TPR threads own the row; t = thread's index in the row.
// The split is what the column-sharded gated MLP needs (pq_silu_mul_rowamax / pq_silu_mul_quant_rowwise_amax): a rank holds only I/G of a
// token's intermediate channels, the row amax is an exact max over the ranks (an integer max of these bit patterns), and the encode
// then runs locally against the GLOBAL amax — the codes are the unsharded kernel's, bit for bit.
template <int DT, int TPR>
__device__ __forceinline__ uint32_t row_amax_f32_bits(uint32_t ab) {           // `ab` arrives as vec_amax_bits' accumulator
    ab = wave_max_u32(amax_acc_finish<DT>(ab));
    constexpr int NW = (TPR > 256 ? TPR : 256) / kWave;      // waves of the block (a row group wider than a wave is the whole block)
    __shared__ uint32_t part[NW];
    if constexpr (TPR > kWave) {
        if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = ab;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NW; ++w) ab = part[w] > ab ? part[w] : ab;
    }
    // widened to the f32 pattern of the same value: non-negative floats (and NaNs, which sort above +Inf) order as unsigned integers in every format
    return __builtin_bit_cast(uint32_t, amax_bits_to_f32<DT>(ab)) & 0x7FFFFFFFu;
}
template <int DT, int VPT, int TPR>
__device__ __forceinline__ void encode_with_amax(const v4u (&hv)[VPT], uint32_t amax_f32_bits, int t, int nvec, bool active, int64_t row,
                                                 int8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale) {
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    const bool has_nan = amax_f32_bits > 0x7F800000u;        // QSPEC v2: a NaN propagates (scale = canonical NaN, codes 0 by the true-division path)
    const float s = scale_of(__builtin_bit_cast(float, amax_f32_bits));
    if (!active) return;
    if (t == 0) scale[row] = s;
    int8_t* qr = q + row * ldq;
    auto store_vec = [&](int idx, const uint32_t (&pk)[EPV / 4]) {          // write-through (pq_common.h)
        if constexpr (EPV == 8) store_wt_b64(qr + (int64_t)idx * 8, v2u{pk[0], pk[1]});
        else store_wt_b32(qr + (int64_t)idx * 4, pk[0]);
    };
    if (!has_nan && scale_fast_ok(s)) {
        const float r = 1.0f / s;
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int idx = i * TPR + t;
            uint32_t pk[EPV / 4];
            fast_encode_vec<DT>(hv[i], s, r, pk);
            if (idx < nvec) store_vec(idx, pk);
        }
    } else {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int idx = i * TPR + t;
            float f[EPV];
            Unpack<DT, EPV>::run(hv[i], f);
            uint32_t pk[EPV / 4];
#pragma unroll
            for (int k = 0; k < EPV / 4; ++k)
                pk[k] = pack4(code_of(f[4 * k], s), code_of(f[4 * k + 1], s), code_of(f[4 * k + 2], s), code_of(f[4 * k + 3], s));
            if (idx < nvec) store_vec(idx, pk);
        }
    }
}
template <int DT, int VPT, int TPR>
__device__ __forceinline__ void reduce_and_encode(const v4u (&hv)[VPT], uint32_t ab, int t, int nvec, bool active, int64_t row,
                                                  int8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale) {
    encode_with_amax<DT, VPT, TPR>(hv, row_amax_f32_bits<DT, TPR>(ab), t, nvec, active, row, q, ldq, scale);
}

// ------------------------------------------------------------------------------------------------
// QSPEC N1-N5 for the norm family (rownorm_kernels.h): ONE copy of the pinned summation order.  The reduction order N1-N3 is the 256-thread layout: vector v on
// lane v mod 256, xor butterfly per 64 lanes, the four wave sums left to right.
// The butterfly on N independent sums at once, step by step: every lane ends with the sums over its wave.
template <int N>
__device__ __forceinline__ void wave_sums(float (&acc)[N]) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int gi = 0; gi < N; ++gi) acc[gi] = acc[gi] + __shfl_xor(acc[gi], off, 64);
    }
}
// one block per row: this lane's sum -> the row's.  The wave sums meet in ONE array per kernel: a barrier goes between two calls.
__device__ __forceinline__ float rms_block_sum(float acc) {
    float a[1] = {acc};
    wave_sums(a);
    __shared__ float wsum[4];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = a[0];
    __syncthreads();
    return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}
// the row's sum in either layout of rownorm_kernels.h.  One wave per row: the wave holds all four 64-lane groups of the specification, one accumulator each.
template <int TPR>
__device__ __forceinline__ float row_sum(float (&acc)[TPR == 64 ? 4 : 1]) {
    if constexpr (TPR == 64) {
        wave_sums(acc);
        return ((acc[0] + acc[1]) + acc[2]) + acc[3];
    } else {
        return rms_block_sum(acc[0]);
    }
}
__device__ __forceinline__ float rms_rs(float ss, int cols, float eps) {
    const float var = ss / (float)cols;
    return 1.0f / __builtin_sqrtf(var + eps);
}
template <int DT>
__device__ __forceinline__ float rms_h(float x, float w, float rs) {
    const float xn = Elem<DT>::to_f32(Elem<DT>::from_f32(x * rs));
    return w * xn;       // the caller rounds to the storage dtype
}

// one 16-byte vector of x and of the weight -> one 16-byte vector of h (QSPEC N5), two elements per instruction
template <int DT>
__device__ __forceinline__ v4u rms_h_vec(const v4u& xv, const v4u& wv, float rs) {
    v4u out;
    if constexpr (DT == PQ_F32) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t xb = xv[j], wb = wv[j];      // copies first (hipcc quirk with vector-element lvalues)
            out[j] = __builtin_bit_cast(uint32_t, rms_h<DT>(__builtin_bit_cast(float, xb), __builtin_bit_cast(float, wb), rs));
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t xw = xv[j], ww = wv[j];
            const v2f xn = Pair<DT>::unpack(Pair<DT>::pack(Pair<DT>::unpack(xw) * splat(rs)));
            out[j] = Pair<DT>::pack(Pair<DT>::unpack(ww) * xn);
        }
    }
    return out;
}

}  // namespace pq
