// producer_kernels.hip — K1 fused into the op that produces the activation:
//   silu(g) * u           ->  per-token int8 codes + row scales   (K1s: the `down` input of a gated MLP)
//   RMSNorm(x; weight)    ->  per-token int8 codes + row scales   (K1n: the q/k/v and gate/up input of a decoder layer; kernels in rownorm_kernels.h)
// without the bf16 activation ever going to HBM.
// Same skeleton as K1 (quant_kernels.hip): TPR threads own a row, the row of h lives in registers between the amax
// reduction and the encode; here it is COMPUTED from one 16-byte vector of g and one of u per slot instead of loaded.
// Arithmetic follows QSPEC S1-S6: a specified exponential (Cody-Waite + degree-7 Horner with fma),
// IEEE division, storage-dtype rounding after silu and after the product — bit-identical to oracle/qspec_oracle.c.
// Algorithmic traffic: read 2 x elem bytes, write 1 B/elem + 4 B/row (+ elem bytes when h is also requested).
#include "rownorm_kernels.h"
#include "pq_launch.h"

namespace pq {

// TPR = 512 (a 512-thread block per row, wide rows): round 1 held such rows with 256 threads x 8 vectors of g and of u —
// 143 VGPRs, 3 waves per SIMD in a kernel that is VALU-bound before it is HBM-bound; 512 threads x 3-4 vectors need < 100.
// MODE 0: K1s (amax + encode).  MODE 1: the row amax only (amax_io[row] = f32 bit pattern of max |h| over these columns; nothing else is written).
// MODE 2: encode against the row amax GIVEN in amax_io (the max over every rank's columns): no reduction; writes codes and the scale.
// IDENT (MODE 1 / 2 only): h = g itself — the same two halves for a PLAIN column-sharded activation (a rank's heads of the attention output feeding a
// column-sharded `o` projection: pq_quant_rowamax / pq_quant_rowwise_amax); u is not read.
template <int DT, int VPT, int TPR, bool WRITE_H, int MODE = 0, bool IDENT = false>
__global__ __launch_bounds__(TPR > 256 ? TPR : 256) void silu_mul_quant_vec(const uint8_t* __restrict__ g, int64_t ldg_bytes,
                                                          const uint8_t* __restrict__ u, int64_t ldu_bytes, int64_t rows,
                                                          int nvec, int8_t* __restrict__ q, int64_t ldq,
                                                          float* __restrict__ scale, uint8_t* __restrict__ h_out,
                                                          int64_t ldh_bytes, uint32_t* __restrict__ amax_io = nullptr) {
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
        if constexpr (!IDENT) uv[i] = *reinterpret_cast<const v4u*>(ur + off);
    }
    v4u hv[VPT];
    uint32_t ab = 0;
    uint32_t gmn = 0xFFFFFFFFu, gmx = 0u;
    if constexpr (!IDENT) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) vec_absminmax_bits<DT>(gv[i], gmn, gmx);
    }
    const bool fast_div = IDENT || __builtin_amdgcn_ballot_w64(!silu_fast_div_ok<DT>(gmn, gmx)) == 0ull;   // wave-uniform
    auto produce = [&](auto fast) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int idx = i * TPR + t;
            // slots past the row's end (whole waves of them when the width is not VPT * TPR vectors) skip the arithmetic
            if constexpr (IDENT) hv[i] = idx < nvec ? gv[i] : v4u{0u, 0u, 0u, 0u};
            else hv[i] = idx < nvec ? silu_mul_vec<DT, decltype(fast)::value>(gv[i], uv[i]) : v4u{0u, 0u, 0u, 0u};
            if constexpr (MODE != 2) ab = vec_amax_bits<DT>(hv[i], ab);
            if constexpr (WRITE_H) {
                if (active && idx < nvec) store_wt_b128(h_out + row * ldh_bytes + (int64_t)idx * 16, hv[i]);
            }
        }
    };
    if (fast_div) produce(std::true_type{});
    else produce(std::false_type{});
    if constexpr (MODE == 1) {
        const uint32_t fb = row_amax_f32_bits<DT, TPR>(ab);
        if (active && t == 0) amax_io[row] = fb;
    } else if constexpr (MODE == 2) {
        encode_with_amax<DT, VPT, TPR>(hv, amax_io[row], t, nvec, active, row, q, ldq, scale);
    } else {
        reduce_and_encode<DT, VPT, TPR>(hv, ab, t, nvec, active, row, q, ldq, scale);
    }
}

// generic path: any cols / leading dimensions / alignment.  One block per row; h is recomputed in the second pass.
template <int DT, int MODE = 0, bool IDENT = false>
__global__ __launch_bounds__(256) void silu_mul_quant_generic(const void* __restrict__ g, int64_t ldg, const void* __restrict__ u,
                                                              int64_t ldu, int64_t cols, int8_t* __restrict__ q, int64_t ldq,
                                                              float* __restrict__ scale, void* __restrict__ h_out, int64_t ldh,
                                                              uint32_t* __restrict__ amax_io = nullptr) {
    using S = typename Elem<DT>::store_t;
    const int64_t row = blockIdx.x;
    const S* gr = reinterpret_cast<const S*>(g) + row * ldg;
    const S* ur = reinterpret_cast<const S*>(u) + row * ldu;
    auto h_at = [&](int64_t c) -> S {
        if constexpr (IDENT) return gr[c];
        else return Elem<DT>::from_f32(silu_mul_spec<DT>(Elem<DT>::to_f32(gr[c]), Elem<DT>::to_f32(ur[c])));
    };
    float amax = 0.0f;
    if constexpr (MODE == 2) {
        amax = __builtin_bit_cast(float, amax_io[row]);
    } else {
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
    }
    if constexpr (MODE == 1) {
        if (threadIdx.x == 0) amax_io[row] = __builtin_bit_cast(uint32_t, amax);
        return;
    }
    const float s = scale_of(amax);
    if (threadIdx.x == 0) scale[row] = s;
    int8_t* qr = q + row * ldq;
    for (int64_t c = threadIdx.x; c < cols; c += 256) qr[c] = (int8_t)code_of(Elem<DT>::to_f32(h_at(c)), s);
}

// dev/test kernel: every 16-bit pattern g of the fast-division domain (0 < |g| <= 86) through the three division forms, u = 1 (so h is the
// stored silu(g)).  out[0] += patterns in the domain, out[1] += patterns whose SHORT result differs from the two-correction form,
// out[2] += patterns whose two-correction form differs from true division.
template <int DT>
__global__ __launch_bounds__(256) void silu_short_check(unsigned long long* __restrict__ out) {
    const uint32_t pat = blockIdx.x * 256u + threadIdx.x;            // 256 blocks x 256 threads = all 65 536 patterns
    const uint32_t mag = pat & 0x7FFFu;
    if (!silu_fast_div_ok<DT>(mag, mag)) return;
    const uint32_t one = DT == PQ_BF16 ? 0x3F80u : 0x3C00u;
    const v4u gv = v4u{pat | (pat << 16), pat | (pat << 16), pat | (pat << 16), pat | (pat << 16)};
    const v4u uv = v4u{one | (one << 16), one | (one << 16), one | (one << 16), one | (one << 16)};
    const v4u a = silu_mul_vec<DT, true, true>(gv, uv), b = silu_mul_vec<DT, true, false>(gv, uv), c = silu_mul_vec<DT, false, false>(gv, uv);
    atomicAdd(&out[0], 1ull);
    if (a[0] != b[0]) atomicAdd(&out[1], 1ull);
    if (b[0] != c[0]) atomicAdd(&out[2], 1ull);
}
void launch_silu_short_check(int dtype, unsigned long long* out, hipStream_t st) {
    if (dtype == PQ_BF16) silu_short_check<PQ_BF16><<<dim3(256), dim3(256), 0, st>>>(out);
    else silu_short_check<PQ_FP16><<<dim3(256), dim3(256), 0, st>>>(out);
}

template <int DT, int TPR, bool WRITE_H, int MODE = 0, bool IDENT = false>
static void launch_silu_mul_vec(int vpt, const uint8_t* g, int64_t ldg_b, const uint8_t* u, int64_t ldu_b, int64_t rows, int nvec,
                                int8_t* q, int64_t ldq, float* scale, uint8_t* h, int64_t ldh_b, hipStream_t st, uint32_t* amax_io = nullptr) {
    constexpr int BS = TPR > 256 ? TPR : 256, RPB = BS / TPR;
    const dim3 grid((unsigned)((rows + RPB - 1) / RPB)), block(BS);
    switch (vpt) {
        case 1: silu_mul_quant_vec<DT, 1, TPR, WRITE_H, MODE, IDENT><<<grid, block, 0, st>>>(g, ldg_b, u, ldu_b, rows, nvec, q, ldq, scale, h, ldh_b, amax_io); break;
        case 2: silu_mul_quant_vec<DT, 2, TPR, WRITE_H, MODE, IDENT><<<grid, block, 0, st>>>(g, ldg_b, u, ldu_b, rows, nvec, q, ldq, scale, h, ldh_b, amax_io); break;
        case 3:
            if constexpr (TPR == 512) silu_mul_quant_vec<DT, 3, TPR, WRITE_H, MODE, IDENT><<<grid, block, 0, st>>>(g, ldg_b, u, ldu_b, rows, nvec, q, ldq, scale, h, ldh_b, amax_io);
            break;
        case 4: silu_mul_quant_vec<DT, 4, TPR, WRITE_H, MODE, IDENT><<<grid, block, 0, st>>>(g, ldg_b, u, ldu_b, rows, nvec, q, ldq, scale, h, ldh_b, amax_io); break;
        case 8:
            if constexpr (TPR != 512) silu_mul_quant_vec<DT, 8, TPR, WRITE_H, MODE, IDENT><<<grid, block, 0, st>>>(g, ldg_b, u, ldu_b, rows, nvec, q, ldq, scale, h, ldh_b, amax_io);
            break;
        default:
            if constexpr (TPR == 256) silu_mul_quant_vec<DT, 16, TPR, WRITE_H, MODE, IDENT><<<grid, block, 0, st>>>(g, ldg_b, u, ldu_b, rows, nvec, q, ldq, scale, h, ldh_b, amax_io);
            break;
    }
}

// the two halves of K1s for a column-sharded intermediate (MODE 1: row amax of these columns -> amax_io; MODE 2: encode against the amax in amax_io).
// Same layouts as the fused kernel (the h vectors are recomputed in MODE 2 — g and u are read twice, from the Infinity Cache the second time — instead of
// parking a 16-bit h in HBM between the two passes: the same 9 bytes per element either way, and no extra buffer).
template <int DT, int MODE, bool IDENT>
void silu_mul_split_dispatch(const void* g, int64_t ldg, const void* u, int64_t ldu, int64_t rows, int64_t cols, uint32_t* amax_io, int8_t* q,
                             int64_t ldq, float* scale, hipStream_t st) {
    static_assert(MODE == 1 || MODE == 2, "split modes");
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    if constexpr (IDENT) { u = g; ldu = ldg; }          // (never read)
    const bool vec_ok = cols > 0 && (cols % EPV == 0) && (ldg % EPV == 0) && (ldu % EPV == 0) && aligned_to(g, 16) && aligned_to(u, 16) &&
                        cols / EPV <= 256 * 16 && (MODE == 1 || ((ldq % EPV == 0) && aligned_to(q, EPV)));
    if (!vec_ok) {
        silu_mul_quant_generic<DT, MODE, IDENT><<<dim3((unsigned)rows), dim3(256), 0, st>>>(g, ldg, u, ldu, cols, q, ldq, scale, nullptr, 0, amax_io);
        return;
    }
    const int nvec = (int)(cols / EPV);
    auto pow2 = [](int v) { int p = 1; while (p < v) p <<= 1; return p; };
    const uint8_t* gb = reinterpret_cast<const uint8_t*>(g);
    const uint8_t* ub = reinterpret_cast<const uint8_t*>(u);
    const int64_t kb = Elem<DT>::kBytes;
    if (nvec <= 64 * 4) launch_silu_mul_vec<DT, 64, false, MODE, IDENT>(pow2((nvec + 63) / 64), gb, ldg * kb, ub, ldu * kb, rows, nvec, q, ldq, scale, nullptr, 0, st, amax_io);
    else if (!IDENT && nvec > 1024 && nvec <= 1536 && opt().silu_tpr != 256) launch_silu_mul_vec<DT, 512, false, MODE, IDENT>((nvec + 511) / 512, gb, ldg * kb, ub, ldu * kb, rows, nvec, q, ldq, scale, nullptr, 0, st, amax_io);
    else launch_silu_mul_vec<DT, 256, false, MODE, IDENT>(pow2((nvec + 255) / 256), gb, ldg * kb, ub, ldu * kb, rows, nvec, q, ldq, scale, nullptr, 0, st, amax_io);
}

template <int DT>
void silu_mul_quant_dispatch(const void* g, int64_t ldg, const void* u, int64_t ldu, int64_t rows, int64_t cols, int8_t* q,
                             int64_t ldq, float* scale, void* h_out, int64_t ldh, hipStream_t st) {
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    const bool vec_ok = cols > 0 && (cols % EPV == 0) && (ldg % EPV == 0) && (ldu % EPV == 0) && aligned_to(g, 16) && aligned_to(u, 16) &&
                        (ldq % EPV == 0) && aligned_to(q, EPV) && cols / EPV <= 256 * 16 &&
                        (!h_out || ((ldh % EPV == 0) && aligned_to(h_out, 16)));
    if (!vec_ok) {
        silu_mul_quant_generic<DT><<<dim3((unsigned)rows), dim3(256), 0, st>>>(g, ldg, u, ldu, cols, q, ldq, scale, h_out, ldh);
        return;
    }
    const int nvec = (int)(cols / EPV);
    auto pow2 = [](int v) { int p = 1; while (p < v) p <<= 1; return p; };
    const uint8_t* gb = reinterpret_cast<const uint8_t*>(g);
    const uint8_t* ub = reinterpret_cast<const uint8_t*>(u);
    uint8_t* hb = reinterpret_cast<uint8_t*>(h_out);
    const int64_t kb = Elem<DT>::kBytes;
    if (nvec <= 64 * 4) {
        const int vpt = pow2((nvec + 63) / 64);
        if (h_out) launch_silu_mul_vec<DT, 64, true>(vpt, gb, ldg * kb, ub, ldu * kb, rows, nvec, q, ldq, scale, hb, ldh * kb, st);
        else launch_silu_mul_vec<DT, 64, false>(vpt, gb, ldg * kb, ub, ldu * kb, rows, nvec, q, ldq, scale, hb, 0, st);
    } else if (nvec > 1024 && nvec <= 1536 && opt().silu_tpr != 256) {
        // rows of 1025..1536 vectors (e.g. 11008 columns): 512 threads x 3 vectors fill 90 % of their slots where 256 threads x 8
        // fill 67 % (the kernel is VALU-bound, idle slots are idle lanes): 2048 x 11008 30.4 -> 28.1 us.  At 1537..2048 vectors
        // (14336, 16384 columns) both layouts have the same slots and measured the same (profiles/r02_k1s_threads_per_row.txt).
        const int vpt = (nvec + 511) / 512;        // 3
        if (h_out) launch_silu_mul_vec<DT, 512, true>(vpt, gb, ldg * kb, ub, ldu * kb, rows, nvec, q, ldq, scale, hb, ldh * kb, st);
        else launch_silu_mul_vec<DT, 512, false>(vpt, gb, ldg * kb, ub, ldu * kb, rows, nvec, q, ldq, scale, hb, 0, st);
    } else {
        const int vpt = pow2((nvec + 255) / 256);
        if (h_out) launch_silu_mul_vec<DT, 256, true>(vpt, gb, ldg * kb, ub, ldu * kb, rows, nvec, q, ldq, scale, hb, ldh * kb, st);
        else launch_silu_mul_vec<DT, 256, false>(vpt, gb, ldg * kb, ub, ldu * kb, rows, nvec, q, ldq, scale, hb, 0, st);
    }
}

// K1n: the kernels and the layout decision are the norm family's (rownorm_kernels.h), ADD = false
template <int DT>
void rmsnorm_quant_dispatch(const void* x, int64_t ldx, const void* wgt, float eps, int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale,
                            void* h_out, int64_t ldh, hipStream_t st) {
    const int64_t kb = Elem<DT>::kBytes;
    rownorm_dispatch<DT>(
        {{x, ldx}, {wgt, 0}}, rows, cols, q, ldq, h_out, ldh,
        [&](auto vpt, auto tpr, auto write_h, dim3 grid, int nvec) {
            rmsnorm_quant_rows<DT, decltype(vpt)::value, decltype(tpr)::value, decltype(write_h)::value, false><<<grid, dim3(256), 0, st>>>(
                reinterpret_cast<const uint8_t*>(x), ldx * kb, nullptr, 0, nullptr, 0, reinterpret_cast<const uint8_t*>(wgt), eps, (int)cols, nvec, rows, q, ldq,
                scale, reinterpret_cast<uint8_t*>(h_out), ldh * kb);
        },
        [&](dim3 grid) { rmsnorm_quant_generic<DT, false><<<grid, dim3(256), 0, st>>>(x, ldx, nullptr, 0, nullptr, 0, wgt, eps, cols, q, ldq, scale, h_out, ldh); });
}

template void rmsnorm_quant_dispatch<PQ_BF16>(const void*, int64_t, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void rmsnorm_quant_dispatch<PQ_FP16>(const void*, int64_t, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void rmsnorm_quant_dispatch<PQ_F32>(const void*, int64_t, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);

#define PQ_SPLIT_INST(DT) \
    template void silu_mul_split_dispatch<DT, 1, false>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, uint32_t*, int8_t*, int64_t, float*, hipStream_t); \
    template void silu_mul_split_dispatch<DT, 2, false>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, uint32_t*, int8_t*, int64_t, float*, hipStream_t); \
    template void silu_mul_split_dispatch<DT, 1, true>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, uint32_t*, int8_t*, int64_t, float*, hipStream_t); \
    template void silu_mul_split_dispatch<DT, 2, true>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, uint32_t*, int8_t*, int64_t, float*, hipStream_t);
PQ_SPLIT_INST(PQ_BF16) PQ_SPLIT_INST(PQ_FP16) PQ_SPLIT_INST(PQ_F32)
#undef PQ_SPLIT_INST
template void silu_mul_quant_dispatch<PQ_BF16>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void silu_mul_quant_dispatch<PQ_FP16>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void silu_mul_quant_dispatch<PQ_F32>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);

}  // namespace pq
