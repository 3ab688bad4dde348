// rowmap_kernels.h — the kernels and the dispatch of the activation-into-quantisation family: an elementwise producer h = op(g, u) fused into the per-token int8
// quantisation, without the 16-bit activation ever going to HBM.
//   rowmap_quant_rows<SiluMulOp, ..>            K1s   silu(g) * u                              (instantiated in producer_kernels.hip)
//   rowmap_quant_rows<SiluMulOp | IdentOp, .., MODE 1 | 2>   the two halves of K1s / of K1 for a column-sharded activation (producer_kernels.hip)
//   rowmap_quant_rows<GluOp<KIND>, ..>          K1g   the clamped gates of GPT-OSS and DeepSeek-V4     (glu_kernels.hip)
//   rowmap_quant_rows<GegluOp, ..>              K1gg  gelu_tanh(g) * u                         (geglu_kernels.hip)
//   rowmap_quant_rows<ActOp<KIND>, ..>          K1u   relu / gelu_tanh / gelu_erf of one input (act_kernels.hip)
// and one generic kernel for ragged widths and unaligned operands.  The kernels are templates: a translation unit instantiates those that its *_quant_dispatch
// launches and no others, so each member of the family keeps an object file, and a register allocation, of its own.
// The skeleton is K1's (quant_kernels.hip): TPR threads own a row, every 16-byte load is issued before the first use, and the row of h lives in registers between
// the amax reduction and the encode; here it is COMPUTED from one vector of g (and one of u) per slot instead of loaded.
// An op is a struct of statics:
//   kInputs               1 (g alone; u is never read) or 2
//   kFastSplit            whether the op has a division-free form that only some waves may take; without it vec<.., false> is the op's one form
//   kWideRows             whether rows of 1025 .. 1536 vectors take 512 threads x 3 vectors
//   Params                passed by value to the kernel (empty, or the GLU's L / alpha / gmax_bits)
//   fast_ok<DT>(mn, mx, p)            the wave's test on the min / max of the |g| bit patterns (vec_absminmax_bits)
//   vec<DT, FASTDIV>(gv, uv, p)       one 16-byte vector of g and of u -> one of h in the storage dtype
//   spec<DT>(g, u, p)                 the specified sequence on one element, before the storage rounding (the generic kernel)
// MODE 0: amax + encode.  MODE 1: the row amax only (amax_io[row] = f32 bit pattern of max |h| over these columns; nothing else is written).  MODE 2: encode against
// the row amax GIVEN in amax_io (the max over every rank's columns): no reduction; writes codes and the scale.  Ops with kSplitModes only (silu * u and the identity).
// Register allocation: as in rownorm_kernels.h the body is the __global__ template itself and the row's arrays are declared in the order g, u, h
// (profiles/r21_rowmap_kernels.txt compares every kernel with its predecessor).
#pragma once
#include "producer_device.h"

namespace pq {

template <class OP, int DT, int VPT, int TPR, bool WRITE_H, int MODE = 0>
__global__ __launch_bounds__(TPR > 256 ? TPR : 256) void rowmap_quant_rows(const uint8_t* __restrict__ g, int64_t ldg_bytes, const uint8_t* __restrict__ u,
                                                                           int64_t ldu_bytes, int64_t rows, int nvec, typename OP::Params p,
                                                                           int8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale,
                                                                           uint8_t* __restrict__ h_out, int64_t ldh_bytes, uint32_t* __restrict__ amax_io) {
    static_assert(MODE == 0 || OP::kSplitModes, "the split halves exist for silu * u and the identity only");
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
        if constexpr (OP::kInputs == 2) uv[i] = *reinterpret_cast<const v4u*>(ur + off);
    }
    v4u hv[VPT];
    uint32_t ab = 0;
    bool fast_div = false;
    if constexpr (OP::kFastSplit) {
        uint32_t gmn = 0xFFFFFFFFu, gmx = 0u;
#pragma unroll
        for (int i = 0; i < VPT; ++i) vec_absminmax_bits<DT>(gv[i], gmn, gmx);
        fast_div = __builtin_amdgcn_ballot_w64(!OP::template fast_ok<DT>(gmn, gmx, p)) == 0ull;   // wave-uniform
    }
    auto produce = [&](auto fast) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int idx = i * TPR + t;
            // slots past the row's end (whole waves of them when the width is not VPT * TPR vectors) skip the arithmetic
            hv[i] = idx < nvec ? OP::template vec<DT, decltype(fast)::value>(gv[i], uv[i], p) : v4u{0u, 0u, 0u, 0u};
            if constexpr (MODE != 2) ab = vec_amax_bits<DT>(hv[i], ab);
            if constexpr (WRITE_H) {
                if (active && idx < nvec) store_wt_b128(h_out + row * ldh_bytes + (int64_t)idx * 16, hv[i]);
            }
        }
    };
    if constexpr (OP::kFastSplit) {
        if (fast_div) produce(std::true_type{});
        else produce(std::false_type{});
    } else {
        produce(std::false_type{});
    }
    if constexpr (MODE == 1) {
        const uint32_t fb = row_amax_f32_bits<DT, TPR>(ab);
        if (active && t == 0) amax_io[row] = fb;
    } else if constexpr (MODE == 2) {
        encode_with_amax<DT, VPT, TPR>(hv, amax_io[row], t, nvec, active, row, q, ldq, scale);
    } else {
        reduce_and_encode<DT, VPT, TPR>(hv, ab, t, nvec, active, row, q, ldq, scale);
    }
}

// generic path: any cols / leading dimensions / alignment.  One block per row; h is recomputed in the second pass (the specified sequence, with `/`).
template <class OP, int DT, int MODE = 0>
__global__ __launch_bounds__(256) void rowmap_quant_generic(const void* __restrict__ g, int64_t ldg, const void* __restrict__ u, int64_t ldu, int64_t cols,
                                                            typename OP::Params p, int8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale,
                                                            void* __restrict__ h_out, int64_t ldh, uint32_t* __restrict__ amax_io) {
    static_assert(MODE == 0 || OP::kSplitModes, "the split halves exist for silu * u and the identity only");
    using S = typename Elem<DT>::store_t;
    const int64_t row = blockIdx.x;
    const S* gr = reinterpret_cast<const S*>(g) + row * ldg;
    const S* ur = reinterpret_cast<const S*>(u) + row * ldu;
    auto h_at = [&](int64_t c) -> S {
        const float uf = OP::kInputs == 2 ? Elem<DT>::to_f32(ur[c]) : 0.0f;
        return Elem<DT>::from_f32(OP::template spec<DT>(Elem<DT>::to_f32(gr[c]), uf, p));
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

// The layout decision of the family, made once.  Rows of whole 16-byte vectors behind aligned pointers and leading dimensions, at most 4096 vectors:
//   up to 256 vectors          one wave per row (four rows per block), 1 / 2 / 4 vectors per lane
//   1025 .. 1536 vectors       512 threads x 3 vectors (e.g. 11008 columns: 90 % of the slots filled where 256 threads x 8 fill 67 %; the kernels are VALU-bound, idle
//                              slots are idle lanes: K1s 2048 x 11008 30.4 -> 28.1 us, profiles/r02_k1s_threads_per_row.txt) unless pq_set_option("PQ_SILU_TPR", "256")
//   otherwise                  256 threads x 1 .. 16 vectors
// anything else — ragged width, unaligned pointer or leading dimension, more than 4096 vectors — is generic.  The layout changes time only, never bits.
// u / ldu are ignored by a one-input op; h_out is nullable (always null in the split modes); amax_io is read or written in the split modes only.
template <class OP, int DT, int MODE = 0>
static void rowmap_dispatch(const void* g, int64_t ldg, const void* u, int64_t ldu, int64_t rows, int64_t cols, typename OP::Params p, int8_t* q, int64_t ldq,
                            float* scale, void* h_out, int64_t ldh, uint32_t* amax_io, hipStream_t st) {
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    const bool vec_ok = cols > 0 && (cols % EPV == 0) && (ldg % EPV == 0) && aligned_to(g, 16) && (OP::kInputs == 1 || ((ldu % EPV == 0) && aligned_to(u, 16))) &&
                        cols / EPV <= 256 * 16 && (MODE == 1 || ((ldq % EPV == 0) && aligned_to(q, EPV))) && (!h_out || ((ldh % EPV == 0) && aligned_to(h_out, 16)));
    if (!vec_ok) {
        rowmap_quant_generic<OP, DT, MODE><<<dim3((unsigned)rows), dim3(256), 0, st>>>(g, ldg, u, ldu, cols, p, q, ldq, scale, h_out, ldh, amax_io);
        return;
    }
    const int nvec = (int)(cols / EPV);
    const int64_t kb = Elem<DT>::kBytes;
    auto go = [&](auto tpr, auto vpt) {
        constexpr int TPR = decltype(tpr)::value, VPT = decltype(vpt)::value, BS = TPR > 256 ? TPR : 256, RPB = BS / TPR;
        const dim3 grid((unsigned)((rows + RPB - 1) / RPB)), block(BS);
        const uint8_t* gb = reinterpret_cast<const uint8_t*>(g);
        const uint8_t* ub = reinterpret_cast<const uint8_t*>(u);
        uint8_t* hb = reinterpret_cast<uint8_t*>(h_out);
        if constexpr (MODE == 0) {
            if (h_out) {
                rowmap_quant_rows<OP, DT, VPT, TPR, true, MODE><<<grid, block, 0, st>>>(gb, ldg * kb, ub, ldu * kb, rows, nvec, p, q, ldq, scale, hb, ldh * kb, amax_io);
                return;
            }
        }
        rowmap_quant_rows<OP, DT, VPT, TPR, false, MODE><<<grid, block, 0, st>>>(gb, ldg * kb, ub, ldu * kb, rows, nvec, p, q, ldq, scale, hb, 0, amax_io);
    };
    using std::integral_constant;
    int vpt = 1;
    const int tpr = nvec <= 64 * 4 ? 64 : 256;
    while (vpt * tpr < nvec) vpt <<= 1;
    if (tpr == 64) {
        switch (vpt) {
            case 1: go(integral_constant<int, 64>{}, integral_constant<int, 1>{}); break;
            case 2: go(integral_constant<int, 64>{}, integral_constant<int, 2>{}); break;
            default: go(integral_constant<int, 64>{}, integral_constant<int, 4>{}); break;
        }
    } else if (OP::kWideRows && nvec > 1024 && nvec <= 1536 && opt().silu_tpr != 256) {
        if constexpr (OP::kWideRows) go(integral_constant<int, 512>{}, integral_constant<int, 3>{});
    } else {
        switch (vpt) {
            case 1: go(integral_constant<int, 256>{}, integral_constant<int, 1>{}); break;   // (no width reaches it while rows of up to 256 vectors take a wave)
            case 2: go(integral_constant<int, 256>{}, integral_constant<int, 2>{}); break;
            case 4: go(integral_constant<int, 256>{}, integral_constant<int, 4>{}); break;
            case 8: go(integral_constant<int, 256>{}, integral_constant<int, 8>{}); break;
            default: go(integral_constant<int, 256>{}, integral_constant<int, 16>{}); break;
        }
    }
}

}  // namespace pq
