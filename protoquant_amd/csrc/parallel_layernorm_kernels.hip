// parallel_layernorm_kernels.hip — K1pl and K1l2: the parallel residual of GPT-NeoX / Phi decoders fused into LayerNorm + per-token int8 quantisation
// (QSPEC A2, then L1-L6 and Q1-Q6 per norm):
//   K1pl  t = a + b;  s = t + c  (s stored: the new residual stream; t never is)  ->  LayerNorm(s; w1, b1, eps1) -> codes + row scales
//                                                                                [->  LayerNorm(s; w2, b2, eps2) -> codes + row scales]
//   K1l2  the same without the adds: s = c, nothing stored, two norms (one norm without the adds is K1l and is not instantiated again)
// One kernel where such a block ran two torch adds and the next block K1l once (Phi) or twice on the same tensor (GPT-NeoX).  L1-L3 — the mean and the sum of
// squared differences — belong to the row, not to the norm: they are computed ONCE, on s as stored, and each group applies its own eps (L4), its own affine map
// (L5) and its own quantisation (L6).  Algorithmic traffic for 16-bit rows: K1pl 6 B/elem read + 2 stored + 1 per group (+ 4 B/row per group); K1l2 2 + 2.
// The row layouts, the pinned summation order and the layout decision are the norm family's (rownorm_kernels.h: TPR = 64 / 256, rownorm_dispatch); the row
// template is this file's own, in an object file of its own, so the register allocation of K1l / K1al does not depend on it.
// Registers.  Up to 8 vectors per thread every load of a, b and c is issued before the first add.  At 16 vectors that form would hold 192 VGPRs of addends
// before the first use, so a and b are issued and added first and c is asked for afterwards (128 in flight, then t + c = 128); after that s (64) + weight (64) +
// bias (64), with h taking the place of the weight.  The packed row s survives group 1: group 2's weight and bias are loaded, and its h encoded, after group 1's
// reduce_and_encode.  No instantiation uses scratch (DESIGN.md §4 lists them).
// Aliasing.  sum_out may be exactly one of a, b, c (same base, same leading dimension; pq_api.hip refuses every other overlap).  A row belongs to one wave or
// workgroup and a thread reads its element of all three addends before it writes that element of the sum, so those four pointers carry no __restrict__.  Slots
// past the row's end load a clamped duplicate of the row's last vector, which another thread may be overwriting: they are zeroed before any use.
#include "rownorm_kernels.h"
#include "pq_launch.h"

namespace pq {

// one norm of the launch: its affine parameters, its eps and where its quantisation (and, when asked for, its normalised activation) goes.  Row kernels take the
// leading dimension of h in bytes, the generic kernel in elements.
struct NormGroup {
    const void* wgt;
    const void* bias;
    float eps;
    int8_t* q;
    int64_t ldq;
    float* scale;
    void* h_out;
    int64_t ldh;
};

// L4-L6 of one group on the packed row xv, whose mean and sum of squared differences the caller holds
template <int DT, int VPT, int TPR, bool WRITE_H>
__device__ __forceinline__ void norm_group_rows(const v4u (&xv)[VPT], float mean, float ssd, int cols, const NormGroup& g, int t, int nvec, bool active, int64_t row) {
    const uint8_t* __restrict__ wgt = reinterpret_cast<const uint8_t*>(g.wgt);
    const uint8_t* __restrict__ bias = reinterpret_cast<const uint8_t*>(g.bias);
    uint8_t* __restrict__ h_out = reinterpret_cast<uint8_t*>(g.h_out);
    const bool has_bias = bias != nullptr;
    v4u wv[VPT], bv[VPT];
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int64_t off = clamped_vec_off(i * TPR + t, nvec);
        wv[i] = *reinterpret_cast<const v4u*>(wgt + off);
        bv[i] = has_bias ? *reinterpret_cast<const v4u*>(bias + off) : v4u{0u, 0u, 0u, 0u};
    }
    const float rs = rms_rs(ssd, cols, g.eps);                     // L4
    v4u hv[VPT];
    uint32_t ab = 0;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int idx = i * TPR + t;
        hv[i] = idx < nvec ? ln_h_vec<DT>(xv[i], wv[i], bv[i], mean, rs, has_bias) : v4u{0u, 0u, 0u, 0u};
        ab = vec_amax_bits<DT>(hv[i], ab);
        if constexpr (WRITE_H) {
            if (h_out && active && idx < nvec) store_wt_b128(h_out + row * g.ldh + (int64_t)idx * 16, hv[i]);
        }
    }
    reduce_and_encode<DT, VPT, TPR>(hv, ab, t, nvec, active, row, g.q, g.ldq, g.scale);
}

// K1pl (ADD2) / K1l2 (!ADD2, NORMS == 2).  WRITE_H: at least one group stores its normalised activation (a group whose h_out is null does not).
template <int DT, int VPT, int TPR, bool WRITE_H, bool ADD2, int NORMS>
__global__ __launch_bounds__(256) void parallel_layernorm_quant_rows(const uint8_t* a, int64_t lda_bytes, const uint8_t* b, int64_t ldb_bytes, const uint8_t* c,
                                                                     int64_t ldc_bytes, uint8_t* sum_out, int64_t lds_bytes, NormGroup g1, NormGroup g2, int cols,
                                                                     int nvec, int64_t rows) {
    static_assert(ADD2 || NORMS == 2, "one norm without the adds is K1l (layernorm_kernels.hip)");
    constexpr int NACC = TPR == 64 ? 4 : 1;
    const int t = TPR == 256 ? threadIdx.x : threadIdx.x & 63;
    int64_t row = TPR == 256 ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool active = TPR == 256 || row < rows;          // TPR == 64: a wave past the last row walks a duplicate of the last row and stores nothing
    if constexpr (TPR == 64) row = active ? row : rows - 1;
    const uint8_t* cr = c + row * ldc_bytes;
    v4u xv[VPT];
    if constexpr (ADD2) {
        const uint8_t* ar = a + row * lda_bytes;
        const uint8_t* br = b + row * ldb_bytes;
        v4u rv[VPT];
        if constexpr (VPT <= 8) {
            // every load of the three addends is issued before the first use
            v4u cv[VPT];
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const int64_t off = clamped_vec_off(i * TPR + t, nvec);
                xv[i] = *reinterpret_cast<const v4u*>(ar + off);
                rv[i] = *reinterpret_cast<const v4u*>(br + off);
                cv[i] = *reinterpret_cast<const v4u*>(cr + off);
            }
#pragma unroll
            for (int i = 0; i < VPT; ++i) xv[i] = add_vec<DT>(add_vec<DT>(xv[i], rv[i]), cv[i]);          // A2: (a + b) + c, each sum rounded to the storage dtype
        } else {
            // 16 vectors: a and b, their sum, and only then c (the header comment says why)
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const int64_t off = clamped_vec_off(i * TPR + t, nvec);
                xv[i] = *reinterpret_cast<const v4u*>(ar + off);
                rv[i] = *reinterpret_cast<const v4u*>(br + off);
            }
#pragma unroll
            for (int i = 0; i < VPT; ++i) xv[i] = add_vec<DT>(xv[i], rv[i]);          // A2: t = a + b
            pin_before_loads(xv);
#pragma unroll
            for (int i = 0; i < VPT; ++i) rv[i] = *reinterpret_cast<const v4u*>(cr + clamped_vec_off(i * TPR + t, nvec));
#pragma unroll
            for (int i = 0; i < VPT; ++i) xv[i] = add_vec<DT>(xv[i], rv[i]);          // A2: s = t + c
        }
    } else {
#pragma unroll
        for (int i = 0; i < VPT; ++i) xv[i] = *reinterpret_cast<const v4u*>(cr + clamped_vec_off(i * TPR + t, nvec));
    }
    float acc[NACC] = {};                   // L2 (on s AS STORED): this lane's vectors in increasing v, elements in order
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        if (i * TPR + t >= nvec) xv[i] = v4u{0u, 0u, 0u, 0u};      // past the row: acc + 0 = acc
        acc[i & (NACC - 1)] = ln_sum_vec<DT>(xv[i], acc[i & (NACC - 1)]);
    }
    pin_before_loads(xv);
    if constexpr (ADD2) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int idx = i * TPR + t;
            if (active && idx < nvec) store_wt_b128(sum_out + row * lds_bytes + (int64_t)idx * 16, xv[i]);
        }
    }
    const float mean = ln_mean(row_sum<TPR>(acc), cols);           // L2
#pragma unroll
    for (int gi = 0; gi < NACC; ++gi) acc[gi] = 0.0f;              // L3
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        if (i * TPR + t < nvec) acc[i & (NACC - 1)] = ln_ssd_vec<DT>(xv[i], mean, acc[i & (NACC - 1)]);
    }
    if constexpr (TPR == 256) __syncthreads();                     // row_sum<256>'s four partial sums are one array: everyone has read the first sum
    const float ssd = row_sum<TPR>(acc);                           // L3: the row's, shared by both groups
    norm_group_rows<DT, VPT, TPR, WRITE_H>(xv, mean, ssd, cols, g1, t, nvec, active, row);
    if constexpr (NORMS == 2) {
        pin_before_loads(xv);                                      // group 2's weight and bias are asked for after group 1 is done with its registers
        if constexpr (TPR == 256) __syncthreads();                 // the four partial maxima of the row amax are one array: everyone has read group 1's
        norm_group_rows<DT, VPT, TPR, WRITE_H>(xv, mean, ssd, cols, g2, t, nvec, active, row);
    }
}

// Ragged widths, unaligned bases, odd leading dimensions: one 256-thread block per row, every pass in the order of the specification (vector v on thread v mod 256,
// its elements in order), so a thread only ever reads back the sums it stored itself: the first pass reads a, b and c and stores s, the others start from the
// stored s and never touch the addends again (any one of them may BE sum_out).  The row is read 2 + 2 NORMS times (from cache after the first).
template <int DT, bool ADD2, int NORMS>
__global__ __launch_bounds__(256) void parallel_layernorm_quant_generic(const void* a, int64_t lda, const void* b, int64_t ldb, const void* c, int64_t ldc, void* sum_out,
                                                                        int64_t lds, NormGroup g1, NormGroup g2, int64_t cols) {
    static_assert(ADD2 || NORMS == 2, "one norm without the adds is K1l (layernorm_kernels.hip)");
    using S = typename Elem<DT>::store_t;
    const int64_t row = blockIdx.x;
    const S* ar = reinterpret_cast<const S*>(a) + row * lda;
    const S* br = reinterpret_cast<const S*>(b) + row * ldb;
    const S* cr = reinterpret_cast<const S*>(c) + row * ldc;
    S* sr = reinterpret_cast<S*>(sum_out) + row * lds;
    const S* in = ADD2 ? sr : cr;            // what is normalised
    float acc = 0.0f;
    walk_row<DT, true>(cols, [&](int64_t k) {
        S s;
        if constexpr (ADD2) {
            s = add_elem<DT>(add_elem<DT>(ar[k], br[k]), cr[k]);          // A2
            sr[k] = s;
        } else {
            s = cr[k];
        }
        acc = acc + Elem<DT>::to_f32(s);
    });
    const float mean = ln_mean(rms_block_sum(acc), (int)cols);
    acc = 0.0f;
    walk_row<DT, true>(cols, [&](int64_t k) {
        const float d = Elem<DT>::to_f32(in[k]) - mean;
        acc = __builtin_fmaf(d, d, acc);
    });
    __syncthreads();
    const float ssd = rms_block_sum(acc);
    auto group = [&](const NormGroup& g) {
        const S* wr = reinterpret_cast<const S*>(g.wgt);
        const S* bs = reinterpret_cast<const S*>(g.bias);
        const bool has_bias = bs != nullptr;
        const float rs = rms_rs(ssd, (int)cols, g.eps);
        generic_amax_and_encode<DT, true>(
            row, cols,
            [&](int64_t k) -> S {
                return Elem<DT>::from_f32(ln_h(Elem<DT>::to_f32(in[k]), mean, rs, Elem<DT>::to_f32(wr[k]), has_bias ? Elem<DT>::to_f32(bs[k]) : 0.0f, has_bias));
            },
            g.q, g.ldq, g.scale, g.h_out, g.ldh);
    };
    group(g1);
    if constexpr (NORMS == 2) {
        __syncthreads();                     // the four partial maxima are one array: everyone has read group 1's
        group(g2);
    }
}

template <int DT, bool ADD2, int NORMS>
static void parallel_dispatch_as(const void* a, int64_t lda, const void* b, int64_t ldb, const void* c, int64_t ldc, void* sum_out, int64_t lds, const NormGroup& g1,
                                 const NormGroup& g2, int64_t rows, int64_t cols, hipStream_t st) {
    const int64_t kb = Elem<DT>::kBytes;
    const void* h_any = g1.h_out ? g1.h_out : g2.h_out;
    const int64_t ldh_any = g1.h_out ? g1.ldh : g2.ldh;
    // (the second group's codes and h go through the operand test: a whole number of vectors per row and a 16-byte aligned base — stricter than the codes need)
    rownorm_dispatch<DT>(
        {{a, a ? lda : 0}, {b, b ? ldb : 0}, {c, ldc}, {sum_out, sum_out ? lds : 0}, {g1.wgt, 0}, {g1.bias, 0}, {g2.wgt, 0}, {g2.bias, 0}, {g2.q, g2.q ? g2.ldq : 0},
         {g1.h_out, g1.h_out ? g1.ldh : 0}, {g2.h_out, g2.h_out ? g2.ldh : 0}},
        rows, cols, g1.q, g1.ldq, h_any, ldh_any,
        [&](auto vpt, auto tpr, auto write_h, dim3 grid, int nvec) {
            NormGroup r1 = g1, r2 = g2;
            r1.ldh *= kb;
            r2.ldh *= kb;
            parallel_layernorm_quant_rows<DT, decltype(vpt)::value, decltype(tpr)::value, decltype(write_h)::value, ADD2, NORMS><<<grid, dim3(256), 0, st>>>(
                reinterpret_cast<const uint8_t*>(a), lda * kb, reinterpret_cast<const uint8_t*>(b), ldb * kb, reinterpret_cast<const uint8_t*>(c), ldc * kb,
                reinterpret_cast<uint8_t*>(sum_out), lds * kb, r1, r2, (int)cols, nvec, rows);
        },
        [&](dim3 grid) { parallel_layernorm_quant_generic<DT, ADD2, NORMS><<<grid, dim3(256), 0, st>>>(a, lda, b, ldb, c, ldc, sum_out, lds, g1, g2, cols); });
}

// a == nullptr (then b and sum_out are null too): K1l2, which needs both groups.  wgt2 == nullptr: one norm (q2, scale2, h2 are null as well).
template <int DT>
void parallel_layernorm_quant_dispatch(const void* a, int64_t lda, const void* b, int64_t ldb, const void* c, int64_t ldc, void* sum_out, int64_t lds, const void* wgt1,
                                       const void* bias1, float eps1, const void* wgt2, const void* bias2, float eps2, int64_t rows, int64_t cols, int8_t* q1, int64_t ldq1,
                                       float* scale1, void* h1, int64_t ldh1, int8_t* q2, int64_t ldq2, float* scale2, void* h2, int64_t ldh2, hipStream_t st) {
    const NormGroup g1{wgt1, bias1, eps1, q1, ldq1, scale1, h1, ldh1}, g2{wgt2, bias2, eps2, q2, ldq2, scale2, h2, ldh2};
    if (!a) parallel_dispatch_as<DT, false, 2>(a, lda, b, ldb, c, ldc, sum_out, lds, g1, g2, rows, cols, st);
    else if (wgt2) parallel_dispatch_as<DT, true, 2>(a, lda, b, ldb, c, ldc, sum_out, lds, g1, g2, rows, cols, st);
    else parallel_dispatch_as<DT, true, 1>(a, lda, b, ldb, c, ldc, sum_out, lds, g1, g2, rows, cols, st);
}

template void parallel_layernorm_quant_dispatch<PQ_BF16>(const void*, int64_t, const void*, int64_t, const void*, int64_t, void*, int64_t, const void*, const void*, float, const void*, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void parallel_layernorm_quant_dispatch<PQ_FP16>(const void*, int64_t, const void*, int64_t, const void*, int64_t, void*, int64_t, const void*, const void*, float, const void*, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void parallel_layernorm_quant_dispatch<PQ_F32>(const void*, int64_t, const void*, int64_t, const void*, int64_t, void*, int64_t, const void*, const void*, float, const void*, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);

}  // namespace pq
