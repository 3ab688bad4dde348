// gemma_postnorm_kernels.hip — K1pang and its add-only form K1pa: the sandwich residual flow of Gemma-2 / Gemma-3 in one launch (QSPEC PN1, A1, then NG1-NG6 and
// Q1-Q6):
//   p = GemmaRMSNorm(x; post_weight, post_eps)   rounded to the storage dtype, NEVER stored      (PN1: NG1-NG5 on the sublayer output)
//   s = residual + p                             STORED: the new residual stream                  (A1)
//   K1pang only:  GemmaRMSNorm(s; weight, eps) on the rows of s AS STORED -> int8 codes + row scales (+ the normalised activation when asked for)
// One kernel where a Gemma-2 decoder layer ran the eager GemmaRMSNorm chain, a torch add and K1ng.  Algorithmic traffic for 16-bit rows: 7 B/elem (x and the
// residual read, s and the codes written; the two weight rows are cache-resident) — K1ang's; K1pa 6 B/elem.
// The arithmetic (GemmaGain, add_vec), the lane's sum of squares and the row sum in their pinned order (lane_sumsq, rms_row_sum), rs (rms_rs), the row layouts
// (rownorm_dispatch) and the second half of K1 (reduce_and_encode) are the family's (rownorm_kernels.h).  The row template stays this file's own: its second half is
// K1ang's and its first half OLMo's with another gain, but with either as a shared __forceinline__ function most of the 87 kernels compile to other instructions,
// and they were not timed against their predecessors ("The RMS row kernels on one template").
// Aliasing: sum_out may be exactly x or exactly residual.  A row belongs to one wave or workgroup; rs_p needs the WHOLE of x, so every element of x is read (into
// registers; generic kernel: in a pass of its own, closed by a block barrier) before any element of s is written, and x is never read again once s is stored.
// Registers: x and the residual are in flight together, post_weight with them or once the lane's pass over x is done (3 vectors per slot); p takes x's place and
// post_weight's die, s takes p's place and the residual's die; `weight` is asked for only then (pin_before_loads), before the stores of s, and h makes it 3 per
// slot again — K1ang's peak (s, weight, h).
#include "rownorm_kernels.h"
#include "pq_launch.h"

namespace pq {

// K1pang (QUANT) / K1pa (!QUANT; wgt, q, scale and h_out are null and never touched)
template <int DT, int VPT, int TPR, bool WRITE_H, bool QUANT>
__global__ __launch_bounds__(256) void gemma_postnorm_add_rows(const uint8_t* x, int64_t ldx_bytes, const uint8_t* __restrict__ pwgt, float post_eps, const uint8_t* res,
                                                               int64_t ldr_bytes, uint8_t* sum_out, int64_t lds_bytes, const uint8_t* __restrict__ wgt, float eps, int cols,
                                                               int nvec, int64_t rows, int8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale,
                                                               uint8_t* __restrict__ h_out, int64_t ldh_bytes) {
    static_assert(QUANT || !WRITE_H, "the add-only form stores the sum alone");
    const int t = TPR == 256 ? threadIdx.x : threadIdx.x & 63;
    int64_t row = TPR == 256 ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool active = TPR == 256 || row < rows;          // TPR == 64: a wave past the last row walks a duplicate of the last row and stores nothing
    if constexpr (TPR == 64) row = active ? row : rows - 1;
    const uint8_t* xr = x + row * ldx_bytes;
    const uint8_t* rr = res + row * ldr_bytes;
    v4u sv[VPT];
    {
        float acc[TPR == 64 ? 4 : 1];
        // every load of x and of the residual is issued before the first use.  post_weight (cache-resident): one wave per row, with them; 256 threads per row, once
        // the lane's pass over x is done, while the row sum is under way.  Each layout takes the order in which hipcc allocates fewer registers
        constexpr bool PW_FIRST = TPR == 64;
        v4u rv[VPT], pv[VPT];
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int64_t off = clamped_vec_off(i * TPR + t, nvec);
            sv[i] = *reinterpret_cast<const v4u*>(xr + off);
            rv[i] = *reinterpret_cast<const v4u*>(rr + off);
            if constexpr (PW_FIRST) pv[i] = *reinterpret_cast<const v4u*>(pwgt + off);
        }
        lane_sumsq<DT, VPT, TPR>(sv, t, nvec, acc);                                           // NG2 on x
        if constexpr (!PW_FIRST) {
            pin_before_loads(sv);
#pragma unroll
            for (int i = 0; i < VPT; ++i) pv[i] = *reinterpret_cast<const v4u*>(pwgt + clamped_vec_off(i * TPR + t, nvec));
        }
        const float rs_p = rms_rs(rms_row_sum<TPR>(acc), cols, post_eps);                                  // NG3, NG4
#pragma unroll
        for (int i = 0; i < VPT; ++i) sv[i] = GemmaGain::h_vec<DT>(sv[i], pv[i], rs_p);                     // PN1: p, rounded to the storage dtype, takes the place of x
#pragma unroll
        for (int i = 0; i < VPT; ++i) sv[i] = add_vec<DT>(sv[i], rv[i]);                               // A1: the sum takes the place of p
        pin_before_loads(sv);
    }
    // the weight row, asked for once the residual's and post_weight's registers are free and BEFORE the stores of the sum, so that waiting for it does not wait
    // for them
    [[maybe_unused]] v4u wv[QUANT ? VPT : 1];
    if constexpr (QUANT) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) wv[i] = *reinterpret_cast<const v4u*>(wgt + clamped_vec_off(i * TPR + t, nvec));
    }
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int idx = i * TPR + t;
        if (active && idx < nvec) store_wt_b128(sum_out + row * lds_bytes + (int64_t)idx * 16, sv[i]);
    }
    if constexpr (QUANT) {
        if constexpr (TPR == 256) __syncthreads();                 // row_sum<256>'s four partial sums are one array: everyone has read the first sum
        // NG2-NG4 on s AS STORED (a slot past the row held p = (0 * rs_p) * g + a duplicate of the residual: zeroed in there)
        float acc[TPR == 64 ? 4 : 1];
        lane_sumsq<DT, VPT, TPR>(sv, t, nvec, acc);
        const float rs = rms_rs(rms_row_sum<TPR>(acc), cols, eps);
        v4u hv[VPT];
        uint32_t ab = 0;
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int idx = i * TPR + t;
            hv[i] = GemmaGain::h_vec<DT>(sv[i], wv[i], rs);             // zeroed AFTER the arithmetic, as rmsnorm_quant_rows does
            if (idx >= nvec) hv[i] = v4u{0u, 0u, 0u, 0u};
            ab = vec_amax_bits<DT>(hv[i], ab);
            if constexpr (WRITE_H) {
                if (active && idx < nvec) store_wt_b128(h_out + row * ldh_bytes + (int64_t)idx * 16, hv[i]);
            }
        }
        reduce_and_encode<DT, VPT, TPR>(hv, ab, t, nvec, active, row, q, ldq, scale);
    }
}

// generic path.  Pass 1 reads the whole of x (rs_p); the block barrier of its row sum closes it.  Pass 2 reads x, the residual and post_weight and stores s; every
// pass walks the elements in the SAME thread order, so a thread writes s[c] after it read x[c] and residual[c] itself, and the passes after it start from the stored
// s and never touch x or the residual again (either of them may BE sum_out).
template <int DT, bool QUANT>
__global__ __launch_bounds__(256) void gemma_postnorm_add_generic(const void* x, int64_t ldx, const void* __restrict__ pwgt, float post_eps, const void* res, int64_t ldr,
                                                                  void* sum_out, int64_t lds, const void* __restrict__ wgt, float eps, int64_t cols, int8_t* __restrict__ q,
                                                                  int64_t ldq, float* __restrict__ scale, void* __restrict__ h_out, int64_t ldh) {
    using S = typename Elem<DT>::store_t;
    const int64_t row = blockIdx.x;
    const S* xr = reinterpret_cast<const S*>(x) + row * ldx;
    const S* rr = reinterpret_cast<const S*>(res) + row * ldr;
    S* sr = reinterpret_cast<S*>(sum_out) + row * lds;
    const S* pr = reinterpret_cast<const S*>(pwgt);
    float acc = 0.0f;
    walk_row<DT, true>(cols, [&](int64_t c) {
        const float f = Elem<DT>::to_f32(xr[c]);
        acc = __builtin_fmaf(f, f, acc);
    });
    const float rs_p = rms_rs(rms_block_sum(acc), (int)cols, post_eps);
    acc = 0.0f;
    walk_row<DT, true>(cols, [&](int64_t c) {
        const S p = Elem<DT>::from_f32(GemmaGain::h<DT>(Elem<DT>::to_f32(xr[c]), Elem<DT>::to_f32(pr[c]), rs_p));      // PN1
        const S s = add_elem<DT>(rr[c], p);                                                                   // A1
        sr[c] = s;
        if constexpr (QUANT) {
            const float f = Elem<DT>::to_f32(s);
            acc = __builtin_fmaf(f, f, acc);
        }
    });
    if constexpr (QUANT) {
        const S* wr = reinterpret_cast<const S*>(wgt);
        const S* in = sr;
        __syncthreads();                    // rms_block_sum's partial sums are one array: everyone has read the first sum
        const float rs = rms_rs(rms_block_sum(acc), (int)cols, eps);
        generic_amax_and_encode<DT, true>(
            row, cols, [&](int64_t c) -> S { return Elem<DT>::from_f32(GemmaGain::h<DT>(Elem<DT>::to_f32(in[c]), Elem<DT>::to_f32(wr[c]), rs)); }, q, ldq, scale, h_out, ldh);
    }
}

// wgt == nullptr: the add-only form (q, scale and h_out are null too: pq_api.hip refuses a partly-null group)
template <int DT>
void gemma_postnorm_add_rmsnorm_quant_dispatch(const void* x, int64_t ldx, const void* pwgt, float post_eps, const void* res, int64_t ldr, void* sum_out, int64_t lds,
                                               const void* wgt, float eps, int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale, void* h_out, int64_t ldh,
                                               hipStream_t st) {
    const int64_t kb = Elem<DT>::kBytes;
    rownorm_dispatch_quant_or_sum<DT>(
        {{x, ldx}, {res, ldr}, {sum_out, lds}, {pwgt, 0}, {wgt, 0}}, rows, cols, wgt != nullptr, q, ldq, h_out, ldh,
        [&](auto vpt, auto tpr, auto write_h, auto quant, dim3 grid, int nvec) {
            gemma_postnorm_add_rows<DT, decltype(vpt)::value, decltype(tpr)::value, decltype(write_h)::value, decltype(quant)::value><<<grid, dim3(256), 0, st>>>(
                row_bytes(x), ldx * kb, row_bytes(pwgt), post_eps, row_bytes(res), ldr * kb, row_bytes(sum_out), lds * kb, row_bytes(wgt), eps, (int)cols, nvec, rows, q,
                ldq, scale, row_bytes(h_out), ldh * kb);
        },
        [&](auto quant, dim3 grid) {
            gemma_postnorm_add_generic<DT, decltype(quant)::value><<<grid, dim3(256), 0, st>>>(x, ldx, pwgt, post_eps, res, ldr, sum_out, lds, wgt, eps, cols, q, ldq, scale, h_out,
                                                                                               ldh);
        });
}

PQ_INSTANTIATE_DTYPES(gemma_postnorm_add_rmsnorm_quant_dispatch)

}  // namespace pq
