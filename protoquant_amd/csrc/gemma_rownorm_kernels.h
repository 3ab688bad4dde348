// gemma_rownorm_kernels.h — the Gemma members of the norm-into-quantisation family (QSPEC NG1-NG6):
//   gemma_rmsnorm_quant_rows<.., ADD = false>   K1ng   GemmaRMSNorm(x; weight)  -> codes + row scales            (instantiated in gemma_norm_kernels.hip)
//   gemma_rmsnorm_quant_rows<.., ADD = true>    K1ang  s = x + residual (stored), then K1ng on s                 (add_gemma_norm_kernels.hip)
// and one generic kernel for ragged widths and unaligned operands.  GemmaRMSNorm is ((x.float() * rs) * (1 + w.float())).type_as(x): the gain is 1 + w, every
// operation is a binary32 one and there is ONE storage rounding (NG5), where the Llama form (N5) rounds x * rs to the storage dtype before the gain.  Everything
// else — the pinned order of the sum of squares, rs, the row layouts, the aliasing rules, the order of the loads and of the stores of the sum, Q1-Q6 — is
// rownorm_kernels.h's, whose helpers are called from here.  The row kernel is a template of its own and not a parameter of rmsnorm_quant_rows: a changed template
// changes the register allocation of the kernels that exist (rownorm_kernels.h, "Register allocation"), and this one is instantiated in its own two object files.
#pragma once
#include "rownorm_kernels.h"

namespace pq {

// NG5 for one element: g = 1 + w, h = (x * rs) * g, every operation rounded in binary32 (the build has no contraction); the caller rounds to the storage dtype
__device__ __forceinline__ float gemma_h(float x, float w, float rs) {
    const float g = 1.0f + w;
    return (x * rs) * g;
}

// one 16-byte vector of x and of the weight -> one 16-byte vector of h (NG5), two elements per instruction
template <int DT>
__device__ __forceinline__ v4u gemma_h_vec(const v4u& xv, const v4u& wv, float rs) {
    v4u out;
    if constexpr (DT == PQ_F32) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t xb = xv[j], wb = wv[j];      // copies first (hipcc quirk with vector-element lvalues)
            out[j] = __builtin_bit_cast(uint32_t, gemma_h(__builtin_bit_cast(float, xb), __builtin_bit_cast(float, wb), rs));
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t xw = xv[j], ww = wv[j];
            const v2f g = splat(1.0f) + Pair<DT>::unpack(ww);
            out[j] = Pair<DT>::pack((Pair<DT>::unpack(xw) * splat(rs)) * g);
        }
    }
    return out;
}

// K1ng / K1ang (QSPEC A1, NG1-NG6, Q1-Q6): rmsnorm_quant_rows with NG5 in place of N5.  Same traffic, same register budget.
template <int DT, int VPT, int TPR, bool WRITE_H, bool ADD>
__global__ __launch_bounds__(256) void gemma_rmsnorm_quant_rows(row_in_bytes<ADD> x, int64_t ldx_bytes, const uint8_t* res, int64_t ldr_bytes, uint8_t* sum_out,
                                                                int64_t lds_bytes, const uint8_t* __restrict__ wgt, float eps, int cols, int nvec, int64_t rows,
                                                                int8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale, uint8_t* __restrict__ h_out,
                                                                int64_t ldh_bytes) {
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    constexpr int NACC = TPR == 64 ? 4 : 1;
    const int t = TPR == 256 ? threadIdx.x : threadIdx.x & 63;
    int64_t row = TPR == 256 ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool active = TPR == 256 || row < rows;          // TPR == 64: a wave past the last row walks a duplicate of the last row and stores nothing
    if constexpr (TPR == 64) row = active ? row : rows - 1;
    const uint8_t* xr = x + row * ldx_bytes;
    [[maybe_unused]] const uint8_t* rr = ADD ? res + row * ldr_bytes : nullptr;
    v4u sv[VPT];
    if constexpr (ADD) {
        // every load of x and of the residual is issued before the first use
        v4u rv[VPT];
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int64_t off = clamped_vec_off(i * TPR + t, nvec);
            sv[i] = *reinterpret_cast<const v4u*>(xr + off);
            rv[i] = *reinterpret_cast<const v4u*>(rr + off);
        }
#pragma unroll
        for (int i = 0; i < VPT; ++i) sv[i] = add_vec<DT>(sv[i], rv[i]);          // A1: the sum takes the place of x
        pin_before_loads(sv);
    }
    // the weight row (cache-resident).  Plain: with x, every load before the first use.  ADD: asked for once the residual's registers are free, and BEFORE the
    // stores of the sum, so that waiting for it does not wait for them
    v4u wv[VPT];
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int64_t off = clamped_vec_off(i * TPR + t, nvec);
        if constexpr (!ADD) sv[i] = *reinterpret_cast<const v4u*>(xr + off);
        wv[i] = *reinterpret_cast<const v4u*>(wgt + off);
    }
    if constexpr (ADD) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int idx = i * TPR + t;
            if (active && idx < nvec) store_wt_b128(sum_out + row * lds_bytes + (int64_t)idx * 16, sv[i]);
        }
    }
    float acc[NACC] = {};                   // NG2 (on s AS STORED): this lane's vectors in increasing v, elements in order
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        if (i * TPR + t >= nvec) sv[i] = v4u{0u, 0u, 0u, 0u};      // past the row: fma(0, 0, acc) = acc
        float f[EPV];
        Unpack<DT, EPV>::run(sv[i], f);
#pragma unroll
        for (int j = 0; j < EPV; ++j) acc[i & (NACC - 1)] = __builtin_fmaf(f[j], f[j], acc[i & (NACC - 1)]);
    }
    float ss;                               // NG3
    if constexpr (TPR == 64) {
        // row_sum<64>'s butterfly, written out as rmsnorm_quant_rows has it (through the helper hipcc orders the 4- and 8-vector kernels differently)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
            for (int gi = 0; gi < 4; ++gi) acc[gi] = acc[gi] + __shfl_xor(acc[gi], off, 64);
        }
        ss = ((acc[0] + acc[1]) + acc[2]) + acc[3];
    } else {
        ss = rms_block_sum(acc[0]);
    }
    const float rs = rms_rs(ss, cols, eps);                        // NG4
    v4u hv[VPT];
    uint32_t ab = 0;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int idx = i * TPR + t;
        // a slot past the row holds a duplicate of the weight's last vector and rs may be Inf or NaN: its h is zero, not their product.  Zeroed AFTER the arithmetic:
        // selecting before it costs the 4-vector wave layout four VGPRs (68, seven waves per SIMD, where K1n has 64 and eight: 8 % at 4096 x 2048)
        hv[i] = gemma_h_vec<DT>(sv[i], wv[i], rs);
        if (idx >= nvec) hv[i] = v4u{0u, 0u, 0u, 0u};
        ab = vec_amax_bits<DT>(hv[i], ab);
        if constexpr (WRITE_H) {
            if (active && idx < nvec) store_wt_b128(h_out + row * ldh_bytes + (int64_t)idx * 16, hv[i]);
        }
    }
    reduce_and_encode<DT, VPT, TPR>(hv, ab, t, nvec, active, row, q, ldq, scale);
}

// generic path (rmsnorm_quant_generic with NG5).  ADD: every pass walks the elements in the SAME thread order, so a thread only ever reads back the sums it stored.
template <int DT, bool ADD>
__global__ __launch_bounds__(256) void gemma_rmsnorm_quant_generic(row_in_void<ADD> x, int64_t ldx, const void* res, int64_t ldr, void* sum_out, int64_t lds,
                                                                   const void* __restrict__ wgt, float eps, int64_t cols, int8_t* __restrict__ q, int64_t ldq,
                                                                   float* __restrict__ scale, void* __restrict__ h_out, int64_t ldh) {
    using S = typename Elem<DT>::store_t;
    const int64_t row = blockIdx.x;
    const S* xr = reinterpret_cast<const S*>(x) + row * ldx;
    const S* rr = reinterpret_cast<const S*>(res) + row * ldr;
    S* sr = reinterpret_cast<S*>(sum_out) + row * lds;
    const S* wr = reinterpret_cast<const S*>(wgt);
    const S* in = ADD ? sr : xr;            // what is normalised
    float acc = 0.0f;
    walk_row<DT, true>(cols, [&](int64_t c) {
        const S s = ADD ? add_elem<DT>(rr[c], xr[c]) : xr[c];
        if constexpr (ADD) sr[c] = s;
        const float f = Elem<DT>::to_f32(s);
        acc = __builtin_fmaf(f, f, acc);
    });
    const float rs = rms_rs(rms_block_sum(acc), (int)cols, eps);
    generic_amax_and_encode<DT, ADD>(
        row, cols, [&](int64_t c) -> S { return Elem<DT>::from_f32(gemma_h(Elem<DT>::to_f32(in[c]), Elem<DT>::to_f32(wr[c]), rs)); }, q, ldq, scale, h_out, ldh);
}

}  // namespace pq
