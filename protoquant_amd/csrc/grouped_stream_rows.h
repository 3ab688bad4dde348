// grouped_stream_rows.h — what the two weight-streaming GROUPED decode kernels (gemm_s8_grouped_stream.hip: int8 weights; gemm_w4_grouped_stream.hip: int4 weights) share
// in front of their bodies: where activation row i of an expert lies (GroupedRows) and which expert a slot of the grid serves (stream_find_slot).  Both read device data
// nobody has checked — offsets are clamped into [0, M_total] (hi) and [0, hi] (lo), the row index into [0, x_rows): wrong contents give wrong results, never an access
// outside the operands.
#pragma once
#include "pq_common.h"

namespace pq {

// row i of the expert that owns the grouped rows lo .. lo + M - 1 -> where its codes lie
struct GroupedRows {
    const int8_t* X;
    int64_t ldx;
    const int32_t* qrow;
    int x_rows, lo, M;
    __device__ __forceinline__ const int8_t* src_row(int i) const {
        const int gr = lo + (i < M ? i : M - 1);
        int64_t row = gr;
        if (qrow != nullptr) {                                  // (the index is device data nobody has checked)
            const uint32_t s = (uint32_t)qrow[gr];
            row = s < (uint32_t)x_rows ? s : (uint32_t)x_rows - 1u;
        }
        return X + row * ldx;
    }
};

// The expert of slot j: the j-th expert (in expert order) with a non-empty clamped row range.  Every lane of every wave computes the same answer; the caller makes it
// scalar.  Four steps of 64 experts are loaded at a time, so that the offsets of up to 256 experts are one round trip to memory and not four.
struct StreamSlot { int e, lo, hi; };
__device__ __forceinline__ bool stream_find_slot(const int32_t* __restrict__ offsets, int E, int M_total, int j, StreamSlot& g) {
    const int lane = threadIdx.x & 63;
    int run = 0;                                               // live experts before this step
    for (int b0 = 0; b0 < E; b0 += 256) {
        int lo[4], hi[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = b0 + i * 64 + lane;
            lo[i] = 0; hi[i] = 0;
            if (e < E) {
                hi[i] = offsets[e + 1];
                lo[i] = offsets[e];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int h = hi[i] < 0 ? 0 : (hi[i] > M_total ? M_total : hi[i]);
            const int l = lo[i] < 0 ? 0 : (lo[i] > h ? h : lo[i]);
            const bool live = h > l;
            const unsigned long long mask = __ballot(live);
            const int cnt = __popcll(mask);
            if (run + cnt > j) {                               // (wave-uniform)
                const int rank = __popcll(mask & ((1ull << lane) - 1ull));     // exclusive prefix sum of the flags
                const unsigned long long hit = __ballot(live && rank == j - run);
                const int src = __ffsll((long long)hit) - 1;
                g.e = b0 + i * 64 + src;
                g.lo = __shfl(l, src, 64);
                g.hi = __shfl(h, src, 64);
                return true;
            }
            run += cnt;
        }
    }
    return false;
}

}  // namespace pq
