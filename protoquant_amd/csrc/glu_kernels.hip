// glu_kernels.hip — K1 fused into the CLAMPED gates of a gated expert MLP (QSPEC G1-G6):
//   kind 0, CLAMPED_SILU   (DeepSeek-V4):  h = silu(min(g, L)) * clamp(u, -L, +L)
//   kind 1, ALPHA_SIGMOID  (GPT-OSS):      h = (clamp(u, -L, +L) + 1) * gc * sigmoid(alpha * gc),  gc = min(g, L)
//   -> per-token int8 codes + row scales (the `down` input of the experts), without the 16-bit activation ever going to HBM.
// The skeleton is silu_mul_quant_vec's (producer_kernels.hip): TPR threads own a row, every 16-byte load is issued before the first use, the row of h lives in
// registers between the amax reduction and the encode.  The device helpers are CALLED from producer_device.h; the kernels here are templates of their own in an
// object file of their own, so the register allocation of K1s / K1n does not depend on this file.
// Algorithmic traffic: read 2 x elem bytes, write 1 B/elem + 4 B/row (+ elem bytes when h is also requested).
#include <cmath>
#include <cstring>

#include "producer_device.h"
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
//    a NaN take the `/` path (glu_fast_ok, decided once per wave on the raw bits of g).  pq_selftest_glu_short runs every 16-bit pattern through both.
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
        v2f a[NP], tc[NP], n[NP], r[NP], p[NP], d[NP], s[NP], glu[NP], v[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) a[k] = store_round<DT>(gc[k] * splat(alpha));                                      // G2
        // G3: 1 + exp_spec(-a), QSPEC S1-S4 as in silu_mul_stage (the clamp is a med3 again: a NaN a is a NaN gc, put back below)
#pragma unroll
        for (int k = 0; k < NP; ++k) tc[k] = v2f{__builtin_amdgcn_fmed3f(-a[k].x, -30.0f, 100.0f), __builtin_amdgcn_fmed3f(-a[k].y, -30.0f, 100.0f)};
#pragma unroll
        for (int k = 0; k < NP; ++k) n[k] = tc[k] * splat(__builtin_bit_cast(float, 0x3FB8AA3Bu));
#pragma unroll
        for (int k = 0; k < NP; ++k) n[k] = v2f{__builtin_rintf(n[k].x), __builtin_rintf(n[k].y)};
#pragma unroll
        for (int k = 0; k < NP; ++k) r[k] = pk_fma(n[k], splat(-__builtin_bit_cast(float, 0x3F317200u)), tc[k]);
#pragma unroll
        for (int k = 0; k < NP; ++k) r[k] = pk_fma(n[k], splat(-__builtin_bit_cast(float, 0x35BFBE8Eu)), r[k]);
#pragma unroll
        for (int k = 0; k < NP; ++k) p[k] = pk_fma(splat(__builtin_bit_cast(float, 0x39500D01u)), r[k], splat(__builtin_bit_cast(float, 0x3AB60B61u)));
        constexpr uint32_t kC[6] = {0x3C088889u, 0x3D2AAAABu, 0x3E2AAAABu, 0x3F000000u, 0x3F800000u, 0x3F800000u};
#pragma unroll
        for (int c = 0; c < 6; ++c) {
#pragma unroll
            for (int k = 0; k < NP; ++k) p[k] = pk_fma(p[k], r[k], splat(__builtin_bit_cast(float, kC[c])));
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) d[k] = splat(1.0f) + v2f{__builtin_ldexpf(p[k].x, (int)n[k].x), __builtin_ldexpf(p[k].y, (int)n[k].y)};
        if constexpr (FASTDIV) {
            v2f y0[NP], y[NP], q[NP], e[NP];
#pragma unroll
            for (int k = 0; k < NP; ++k) y0[k] = v2f{__builtin_amdgcn_rcpf(d[k].x), __builtin_amdgcn_rcpf(d[k].y)};
#pragma unroll
            for (int k = 0; k < NP; ++k) e[k] = pk_fma(-d[k], y0[k], splat(1.0f));
#pragma unroll
            for (int k = 0; k < NP; ++k) y[k] = pk_fma(e[k], y0[k], y0[k]);
#pragma unroll
            for (int k = 0; k < NP; ++k) e[k] = pk_fma(-d[k], y[k], splat(1.0f));          // (the quotient 1 * y is y)
#pragma unroll
            for (int k = 0; k < NP; ++k) q[k] = pk_fma(e[k], y[k], y[k]);
#pragma unroll
            for (int k = 0; k < NP; ++k) e[k] = pk_fma(-d[k], q[k], splat(1.0f));
#pragma unroll
            for (int k = 0; k < NP; ++k) s[k] = pk_fma(e[k], y[k], q[k]);
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
template <int DT, int KIND>
__device__ __forceinline__ float glu_spec(float g, float u, float L, float alpha) {
    const v2f ga[1] = {v2f{g, g}}, ua[1] = {v2f{u, u}};
    v2f h[1];
    glu_stage<DT, KIND, false, 1>(ga, ua, L, alpha, h);
    return h[0].x;
}

// The fast-division test on the min / max of the |g| bit patterns of a wave (vec_absminmax_bits).  |gc| <= |g| (the clamp only lowers a positive gate), so a
// bound on |g| bounds what the division sees.  CLAMPED_SILU: silu_fast_div_ok as it is (0 < |g| <= 86).  ALPHA_SIGMOID: |g| <= gmax, the largest storage value
// with gmax |alpha| <= 86 and gmax <= 86 (computed on the host, rounded DOWN: 86 is a value of every storage dtype and rounding is monotone, so |a| <= 86).
template <int DT, int KIND> __device__ __forceinline__ bool glu_fast_ok(uint32_t mn, uint32_t mx, uint32_t gmax_bits) {
    if constexpr (KIND == GLU_CLAMPED_SILU) return silu_fast_div_ok<DT>(mn, mx);
    else return mx <= gmax_bits;
}

// one 16-byte vector of g and of u -> one 16-byte vector of h in the storage dtype
template <int DT, int KIND, bool FASTDIV>
__device__ __forceinline__ v4u glu_vec(const v4u& gv, const v4u& uv, float L, float alpha) {
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
    glu_stage<DT, KIND, FASTDIV, NP>(g, u, L, alpha, h);
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
__global__ __launch_bounds__(TPR > 256 ? TPR : 256) void glu_quant_vec(const uint8_t* __restrict__ g, int64_t ldg_bytes, const uint8_t* __restrict__ u,
                                                                       int64_t ldu_bytes, int64_t rows, int nvec, float L, float alpha, uint32_t gmax_bits,
                                                                       int8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale,
                                                                       uint8_t* __restrict__ h_out, int64_t ldh_bytes) {
    constexpr int BS = TPR > 256 ? TPR : 256;
    constexpr int RPB = BS / TPR;
    const int t = threadIdx.x % TPR;
    int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / TPR;
    const bool active = row < rows;
    row = active ? row : rows - 1;
    const uint8_t* gr = g + row * ldg_bytes;
    const uint8_t* ur = u + row * ldu_bytes;

    // every load is issued before the first use (clamped addresses: a duplicate of the tail vector changes no max)
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
    const bool fast_div = __builtin_amdgcn_ballot_w64(!glu_fast_ok<DT, KIND>(gmn, gmx, gmax_bits)) == 0ull;   // wave-uniform
    auto produce = [&](auto fast) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int idx = i * TPR + t;
            // slots past the row's end (whole waves of them when the width is not VPT * TPR vectors) skip the arithmetic
            hv[i] = idx < nvec ? glu_vec<DT, KIND, decltype(fast)::value>(gv[i], uv[i], L, alpha) : v4u{0u, 0u, 0u, 0u};
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
template <int DT, int KIND>
__global__ __launch_bounds__(256) void glu_quant_generic(const void* __restrict__ g, int64_t ldg, const void* __restrict__ u, int64_t ldu, int64_t cols,
                                                         float L, float alpha, int8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale,
                                                         void* __restrict__ h_out, int64_t ldh) {
    using S = typename Elem<DT>::store_t;
    const int64_t row = blockIdx.x;
    const S* gr = reinterpret_cast<const S*>(g) + row * ldg;
    const S* ur = reinterpret_cast<const S*>(u) + row * ldu;
    auto h_at = [&](int64_t c) -> S { return Elem<DT>::from_f32(glu_spec<DT, KIND>(Elem<DT>::to_f32(gr[c]), Elem<DT>::to_f32(ur[c]), L, alpha)); };
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

// dev/test kernel: every 16-bit pattern g that glu_fast_ok admits through the shipped sequence (FASTDIV) and the specified one (`/`), against u = 1 and u = -1/2.
// out[0] += patterns admitted, out[1] += patterns whose stored h differs in either.
template <int DT, int KIND>
__global__ __launch_bounds__(256) void glu_short_check(float L, float alpha, uint32_t gmax_bits, unsigned long long* __restrict__ out) {
    const uint32_t pat = blockIdx.x * 256u + threadIdx.x;            // 256 blocks x 256 threads = all 65 536 patterns
    const uint32_t mag = pat & 0x7FFFu;
    if (!glu_fast_ok<DT, KIND>(mag, mag, gmax_bits)) return;
    const uint32_t one = DT == PQ_BF16 ? 0x3F80u : 0x3C00u, mhalf = DT == PQ_BF16 ? 0xBF00u : 0xB800u;
    const uint32_t gw = pat | (pat << 16), uw = one | (mhalf << 16);
    const v4u gv = v4u{gw, gw, gw, gw}, uv = v4u{uw, uw, uw, uw};
    const v4u a = glu_vec<DT, KIND, true>(gv, uv, L, alpha), b = glu_vec<DT, KIND, false>(gv, uv, L, alpha);
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

template <int DT, int KIND, int TPR, bool WRITE_H>
static void launch_glu_vec(int vpt, const uint8_t* g, int64_t ldg_b, const uint8_t* u, int64_t ldu_b, int64_t rows, int nvec, float L, float alpha, uint32_t gb,
                           int8_t* q, int64_t ldq, float* scale, uint8_t* h, int64_t ldh_b, hipStream_t st) {
    constexpr int BS = TPR > 256 ? TPR : 256, RPB = BS / TPR;
    const dim3 grid((unsigned)((rows + RPB - 1) / RPB)), block(BS);
#define PQ_GLU_LAUNCH(V) glu_quant_vec<DT, KIND, V, TPR, WRITE_H><<<grid, block, 0, st>>>(g, ldg_b, u, ldu_b, rows, nvec, L, alpha, gb, q, ldq, scale, h, ldh_b)
    switch (vpt) {
        case 1:
            if constexpr (TPR != 512) PQ_GLU_LAUNCH(1);
            break;
        case 2:
            if constexpr (TPR != 512) PQ_GLU_LAUNCH(2);
            break;
        case 3:
            if constexpr (TPR == 512) PQ_GLU_LAUNCH(3);
            break;
        case 4:
            if constexpr (TPR != 512) PQ_GLU_LAUNCH(4);
            break;
        case 8:
            if constexpr (TPR == 256) PQ_GLU_LAUNCH(8);
            break;
        default:
            if constexpr (TPR == 256) PQ_GLU_LAUNCH(16);
            break;
    }
#undef PQ_GLU_LAUNCH
}

// Row layouts as silu_mul_quant_dispatch: one wave per row up to 256 vectors (4096 16-bit elements), 512 threads x 3 vectors for 1025 .. 1536 vectors, else 256
// threads x 1 .. 16 vectors (up to 4096 vectors = 65 536 16-bit elements); anything else — ragged width, unaligned pointer or leading dimension — is generic.
template <int DT, int KIND>
static void glu_quant_dispatch_kind(const void* g, int64_t ldg, const void* u, int64_t ldu, int64_t rows, int64_t cols, float L, float alpha, uint32_t gb,
                                    int8_t* q, int64_t ldq, float* scale, void* h_out, int64_t ldh, hipStream_t st) {
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    const bool vec_ok = (cols % EPV == 0) && (ldg % EPV == 0) && (ldu % EPV == 0) && aligned_to(g, 16) && aligned_to(u, 16) && (ldq % EPV == 0) &&
                        aligned_to(q, EPV) && cols / EPV <= 256 * 16 && (!h_out || ((ldh % EPV == 0) && aligned_to(h_out, 16)));
    if (!vec_ok) {
        glu_quant_generic<DT, KIND><<<dim3((unsigned)rows), dim3(256), 0, st>>>(g, ldg, u, ldu, cols, L, alpha, q, ldq, scale, h_out, ldh);
        return;
    }
    const int nvec = (int)(cols / EPV);
    auto pow2 = [](int v) { int p = 1; while (p < v) p <<= 1; return p; };
    const uint8_t* gb8 = reinterpret_cast<const uint8_t*>(g);
    const uint8_t* ub8 = reinterpret_cast<const uint8_t*>(u);
    uint8_t* hb = reinterpret_cast<uint8_t*>(h_out);
    const int64_t kb = Elem<DT>::kBytes;
#define PQ_GLU_ROWS(TPR, VPT)                                                                                                                          \
    do {                                                                                                                                               \
        if (h_out) launch_glu_vec<DT, KIND, TPR, true>(VPT, gb8, ldg * kb, ub8, ldu * kb, rows, nvec, L, alpha, gb, q, ldq, scale, hb, ldh * kb, st);   \
        else launch_glu_vec<DT, KIND, TPR, false>(VPT, gb8, ldg * kb, ub8, ldu * kb, rows, nvec, L, alpha, gb, q, ldq, scale, hb, 0, st);               \
    } while (0)
    if (nvec <= 64 * 4) PQ_GLU_ROWS(64, pow2((nvec + 63) / 64));
    else if (nvec > 1024 && nvec <= 1536) PQ_GLU_ROWS(512, 3);
    else PQ_GLU_ROWS(256, pow2((nvec + 255) / 256));
#undef PQ_GLU_ROWS
}

template <int DT>
void glu_quant_dispatch(int kind, const void* g, int64_t ldg, const void* u, int64_t ldu, int64_t rows, int64_t cols, float limit, float alpha, int8_t* q,
                        int64_t ldq, float* scale, void* h_out, int64_t ldh, hipStream_t st) {
    const float L = glu_limit_in_dtype(DT, limit);
    const uint32_t gb = glu_gmax_bits(DT, alpha);
    if (kind == GLU_CLAMPED_SILU) glu_quant_dispatch_kind<DT, GLU_CLAMPED_SILU>(g, ldg, u, ldu, rows, cols, L, alpha, gb, q, ldq, scale, h_out, ldh, st);
    else glu_quant_dispatch_kind<DT, GLU_ALPHA_SIGMOID>(g, ldg, u, ldu, rows, cols, L, alpha, gb, q, ldq, scale, h_out, ldh, st);
}

template void glu_quant_dispatch<PQ_BF16>(int, const void*, int64_t, const void*, int64_t, int64_t, int64_t, float, float, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void glu_quant_dispatch<PQ_FP16>(int, const void*, int64_t, const void*, int64_t, int64_t, int64_t, float, float, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void glu_quant_dispatch<PQ_F32>(int, const void*, int64_t, const void*, int64_t, int64_t, int64_t, float, float, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);

}  // namespace pq
