// scaled_addnorm_kernels.hip — K1ma and its add-only form K1mo: the SCALED residual add of the Granite decoders fused into RMSNorm + per-token int8 quantisation
// (QSPEC S1, A1, then N1-N6 and Q1-Q6).  These decoders compute r1 = x + attn(norm(x)) * m and out = r1 + mlp(norm(r1)) * m with one scalar m per model:
//   p = cast_rne(f32(x) * m)          S1: one binary32 product, one storage rounding (f32 rows: the binary32 product itself); NEVER stored, never fused into the add
//   K1ma:  s = cast_rne(f32(residual) + f32(p))  STORED (A1: the new residual stream)  ->  RMSNorm(s; weight)  ->  int8 codes + row scales   (+ h when asked for)
//   K1mo:  s STORED, nothing else (weight == q == scale == nullptr: the end of a chain)
// which is what `residual + x * m` computes in eager torch — two roundings, where fma(x, m, residual) would round once (and differs in about 15 % of random elements).
// Algorithmic traffic for 16-bit rows: K1ma 7 B/elem (K1a's), K1mo 6; against 13 for the eager multiply, the eager add and K1n.
// The row template is this file's own (rownorm_kernels.h: a parameter added to a shipped template changes the register allocation of the shipped kernels); A1 (add_vec),
// the pinned order of the sum of squares, rs (rms_rs), h (rms_h_vec), the row layouts (rownorm_dispatch), the clamped loads and the dead-slot rule, the order of the weight
// loads (pin_before_loads) and the second half of K1 (reduce_and_encode) are the family's.
// Aliasing: sum_out may be exactly x or exactly residual.  A row belongs to one wave or workgroup and a thread reads every element of x and of the residual before it
// writes that element of the sum; the generic kernel's later passes start from the stored sum and never touch x or the residual again.
// Registers: K1a's — the product takes the place of x before the add, so nothing more is live at the peak (x + residual, then sum + weight, then sum + weight + h).
#include "rownorm_kernels.h"
#include "pq_launch.h"

namespace pq {

// S1 for one binary32 value: the product rounded on its own.  The empty statement makes it a materialised register, so no contraction mode can fold it into the add
// that follows (the build has -ffp-contract=off; the kernel does not depend on it)
__device__ __forceinline__ float scaled_f32(float x, float m) {
    float p = x * m;
    asm("" : "+v"(p));          // (not volatile: the scheduler may still move the products among each other)
    return p;
}

// S1 for one element of the storage dtype
template <int DT>
__device__ __forceinline__ typename Elem<DT>::store_t scale_elem(typename Elem<DT>::store_t x, float m) {
    return Elem<DT>::from_f32(scaled_f32(Elem<DT>::to_f32(x), m));
}

// S1 on one 16-byte vector, two elements per instruction for the 16-bit types (Pair<PQ_FP16>::pack materialises the f32 pair: no single-rounding convert)
template <int DT>
__device__ __forceinline__ v4u scale_vec(const v4u& xv, float m) {
    v4u out;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t xw = xv[j];      // a copy first (hipcc quirk with vector-element lvalues)
        if constexpr (DT == PQ_F32) out[j] = __builtin_bit_cast(uint32_t, scaled_f32(__builtin_bit_cast(float, xw), m));
        else out[j] = Pair<DT>::pack(Pair<DT>::unpack(xw) * splat(m));
    }
    return out;
}

// K1ma (QUANT) / K1mo (!QUANT: wgt, q, scale and h_out are null and never touched)
template <int DT, int VPT, int TPR, bool WRITE_H, bool QUANT>
__global__ __launch_bounds__(256) void scaled_add_rmsnorm_quant_rows(const uint8_t* x, int64_t ldx_bytes, const uint8_t* res, int64_t ldr_bytes, float mult,
                                                                     uint8_t* sum_out, int64_t lds_bytes, const uint8_t* __restrict__ wgt, float eps, int cols, int nvec,
                                                                     int64_t rows, int8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale,
                                                                     uint8_t* __restrict__ h_out, int64_t ldh_bytes) {
    static_assert(QUANT || !WRITE_H, "h is the normalised sum: the add-only form has none");
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    constexpr int NACC = TPR == 64 ? 4 : 1;
    const int t = TPR == 256 ? threadIdx.x : threadIdx.x & 63;
    int64_t row = TPR == 256 ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool active = TPR == 256 || row < rows;          // TPR == 64: a wave past the last row walks a duplicate of the last row and stores nothing
    if constexpr (TPR == 64) row = active ? row : rows - 1;
    const uint8_t* xr = x + row * ldx_bytes;
    const uint8_t* rr = res + row * ldr_bytes;
    v4u sv[VPT];
    {
        // every load of x and of the residual is issued before the first use
        v4u rv[VPT];
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int64_t off = clamped_vec_off(i * TPR + t, nvec);
            sv[i] = *reinterpret_cast<const v4u*>(xr + off);
            rv[i] = *reinterpret_cast<const v4u*>(rr + off);
        }
#pragma unroll
        for (int i = 0; i < VPT; ++i) sv[i] = add_vec<DT>(scale_vec<DT>(sv[i], mult), rv[i]);          // S1, then A1: the sum takes the place of x
        if constexpr (QUANT) pin_before_loads(sv);
    }
    if constexpr (!QUANT) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int idx = i * TPR + t;
            if (active && idx < nvec) store_wt_b128(sum_out + row * lds_bytes + (int64_t)idx * 16, sv[i]);
        }
    } else {
        // the weight row (shared by every workgroup: cache-resident): asked for once the residual's registers are free, and BEFORE the stores of the sum, so that
        // waiting for it does not wait for them
        v4u wv[VPT];
#pragma unroll
        for (int i = 0; i < VPT; ++i) wv[i] = *reinterpret_cast<const v4u*>(wgt + clamped_vec_off(i * TPR + t, nvec));
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int idx = i * TPR + t;
            if (active && idx < nvec) store_wt_b128(sum_out + row * lds_bytes + (int64_t)idx * 16, sv[i]);
        }
        float acc[NACC] = {};                   // N2 (on s AS STORED): this lane's vectors in increasing v, elements in order
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            if (i * TPR + t >= nvec) sv[i] = v4u{0u, 0u, 0u, 0u};      // past the row: fma(0, 0, acc) = acc
            float f[EPV];
            Unpack<DT, EPV>::run(sv[i], f);
#pragma unroll
            for (int j = 0; j < EPV; ++j) acc[i & (NACC - 1)] = __builtin_fmaf(f[j], f[j], acc[i & (NACC - 1)]);
        }
        float ss;                               // N3
        if constexpr (TPR == 64) {
            // row_sum<64>'s butterfly, written out, as K1a has it (through the helper hipcc orders and allocates the 4- and 8-vector kernels differently)
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
                for (int gi = 0; gi < 4; ++gi) acc[gi] = acc[gi] + __shfl_xor(acc[gi], off, 64);
            }
            ss = ((acc[0] + acc[1]) + acc[2]) + acc[3];
        } else {
            ss = rms_block_sum(acc[0]);
        }
        const float rs = rms_rs(ss, cols, eps);                        // N4
        v4u hv[VPT];
        uint32_t ab = 0;
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int idx = i * TPR + t;
            // a slot past the row holds a duplicate of the weight's last vector and rs may be Inf or NaN: its h is zero, not 0 * Inf = NaN (which would be the row's
            // amax).  Zeroed AFTER the arithmetic, the family's dead-slot rule
            hv[i] = rms_h_vec<DT>(sv[i], wv[i], rs);
            if (idx >= nvec) hv[i] = v4u{0u, 0u, 0u, 0u};
            ab = vec_amax_bits<DT>(hv[i], ab);
            if constexpr (WRITE_H) {
                if (active && idx < nvec) store_wt_b128(h_out + row * ldh_bytes + (int64_t)idx * 16, hv[i]);
            }
        }
        reduce_and_encode<DT, VPT, TPR>(hv, ab, t, nvec, active, row, q, ldq, scale);
    }
}

// generic path: every pass walks the elements in the SAME thread order, so a thread only ever reads back the sums it stored itself: the first pass reads x and the
// residual and stores s, the others start from the stored s and never touch x or the residual again (either of them may BE sum_out).
template <int DT, bool QUANT>
__global__ __launch_bounds__(256) void scaled_add_rmsnorm_quant_generic(const void* x, int64_t ldx, const void* res, int64_t ldr, float mult, void* sum_out, int64_t lds,
                                                                        const void* __restrict__ wgt, float eps, int64_t cols, int8_t* __restrict__ q, int64_t ldq,
                                                                        float* __restrict__ scale, void* __restrict__ h_out, int64_t ldh) {
    using S = typename Elem<DT>::store_t;
    const int64_t row = blockIdx.x;
    const S* xr = reinterpret_cast<const S*>(x) + row * ldx;
    const S* rr = reinterpret_cast<const S*>(res) + row * ldr;
    S* sr = reinterpret_cast<S*>(sum_out) + row * lds;
    float acc = 0.0f;
    walk_row<DT, true>(cols, [&](int64_t c) {
        const S s = add_elem<DT>(rr[c], scale_elem<DT>(xr[c], mult));          // S1, A1
        sr[c] = s;
        if constexpr (QUANT) {
            const float f = Elem<DT>::to_f32(s);
            acc = __builtin_fmaf(f, f, acc);
        }
    });
    if constexpr (QUANT) {
        const S* wr = reinterpret_cast<const S*>(wgt);
        const S* in = sr;          // what is normalised
        const float rs = rms_rs(rms_block_sum(acc), (int)cols, eps);
        generic_amax_and_encode<DT, true>(
            row, cols, [&](int64_t c) -> S { return Elem<DT>::from_f32(rms_h<DT>(Elem<DT>::to_f32(in[c]), Elem<DT>::to_f32(wr[c]), rs)); }, q, ldq, scale, h_out, ldh);
    }
}

// wgt == nullptr: K1mo (q, scale and h_out are null as well; pq_api.hip refuses a partly-null group)
template <int DT>
void scaled_add_rmsnorm_quant_dispatch(const void* x, int64_t ldx, const void* res, int64_t ldr, float mult, void* sum_out, int64_t lds, const void* wgt, float eps,
                                       int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale, void* h_out, int64_t ldh, hipStream_t st) {
    const int64_t kb = Elem<DT>::kBytes;
    const bool quant = wgt != nullptr;
    const auto b = [](const void* p) { return reinterpret_cast<const uint8_t*>(p); };
    uint8_t* so = reinterpret_cast<uint8_t*>(sum_out);
    rownorm_dispatch<DT>(
        {{x, ldx}, {res, ldr}, {sum_out, lds}, {wgt, 0}}, rows, cols, quant ? q : nullptr, quant ? ldq : 0, quant ? h_out : nullptr, quant ? ldh : 0,
        [&](auto vpt, auto tpr, auto write_h, dim3 grid, int nvec) {
            constexpr int VPT = decltype(vpt)::value, TPR = decltype(tpr)::value;
            constexpr bool WRITE_H = decltype(write_h)::value;
            if (quant) {
                scaled_add_rmsnorm_quant_rows<DT, VPT, TPR, WRITE_H, true><<<grid, dim3(256), 0, st>>>(b(x), ldx * kb, b(res), ldr * kb, mult, so, lds * kb, b(wgt), eps, (int)cols,
                                                                                                       nvec, rows, q, ldq, scale, reinterpret_cast<uint8_t*>(h_out), ldh * kb);
            } else if constexpr (!WRITE_H) {
                scaled_add_rmsnorm_quant_rows<DT, VPT, TPR, false, false><<<grid, dim3(256), 0, st>>>(b(x), ldx * kb, b(res), ldr * kb, mult, so, lds * kb, nullptr, 0.0f, (int)cols,
                                                                                                      nvec, rows, nullptr, 0, nullptr, nullptr, 0);
            }
        },
        [&](dim3 grid) {
            if (quant) scaled_add_rmsnorm_quant_generic<DT, true><<<grid, dim3(256), 0, st>>>(x, ldx, res, ldr, mult, sum_out, lds, wgt, eps, cols, q, ldq, scale, h_out, ldh);
            else scaled_add_rmsnorm_quant_generic<DT, false><<<grid, dim3(256), 0, st>>>(x, ldx, res, ldr, mult, sum_out, lds, nullptr, 0.0f, cols, nullptr, 0, nullptr, nullptr, 0);
        });
}

template void scaled_add_rmsnorm_quant_dispatch<PQ_BF16>(const void*, int64_t, const void*, int64_t, float, void*, int64_t, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void scaled_add_rmsnorm_quant_dispatch<PQ_FP16>(const void*, int64_t, const void*, int64_t, float, void*, int64_t, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void scaled_add_rmsnorm_quant_dispatch<PQ_F32>(const void*, int64_t, const void*, int64_t, float, void*, int64_t, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);

}  // namespace pq
