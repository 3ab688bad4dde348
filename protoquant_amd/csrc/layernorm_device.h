// layernorm_device.h — the device helpers of the LayerNorm-family producers (QSPEC L1-L6), shared by K1l (layernorm_kernels.hip) and K1al
// (addlayernorm_kernels.hip): L2 / L3 / L5 on one 16-byte vector, the wave-level sum of the one-wave-per-row layout and the pin that keeps the loads of the weight
// and bias rows behind the first reduction exist once.  Everything is __forceinline__: each kernel file keeps its own templates in its own object.
#pragma once
#include "producer_device.h"

namespace pq {

// L2 on one 16-byte vector: plain adds, elements in order
template <int DT>
__device__ __forceinline__ float ln_sum_vec(const v4u& xv, float acc) {
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    float f[EPV];
    Unpack<DT, EPV>::run(xv, f);
#pragma unroll
    for (int j = 0; j < EPV; ++j) acc = acc + f[j];
    return acc;
}
// L3 on one 16-byte vector: d = x - mean, acc = fma(d, d, acc), elements in order
template <int DT>
__device__ __forceinline__ float ln_ssd_vec(const v4u& xv, float mean, float acc) {
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    float f[EPV];
    Unpack<DT, EPV>::run(xv, f);
#pragma unroll
    for (int j = 0; j < EPV; ++j) {
        const float d = f[j] - mean;
        acc = __builtin_fmaf(d, d, acc);
    }
    return acc;
}
__device__ __forceinline__ float ln_mean(float sum, int cols) { return sum / (float)cols; }

// L5 for one element: ((d * rs) * w) + b, each operation rounded in binary32; the caller rounds to the storage dtype once
__device__ __forceinline__ float ln_h(float x, float mean, float rs, float w, float b, bool has_bias) {
    float y = ((x - mean) * rs) * w;
    if (has_bias) y = y + b;
    return y;
}
// one 16-byte vector of x, of the weight and of the bias -> one 16-byte vector of h (L5), two elements per instruction
template <int DT>
__device__ __forceinline__ v4u ln_h_vec(const v4u& xv, const v4u& wv, const v4u& bv, float mean, float rs, bool has_bias) {
    v4u out;
    if constexpr (DT == PQ_F32) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t xb = xv[j], wb = wv[j], bb = bv[j];      // copies first (hipcc quirk with vector-element lvalues)
            out[j] = __builtin_bit_cast(uint32_t, ln_h(__builtin_bit_cast(float, xb), mean, rs, __builtin_bit_cast(float, wb), __builtin_bit_cast(float, bb), has_bias));
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t xw = xv[j], ww = wv[j], bw = bv[j];
            v2f y = ((Pair<DT>::unpack(xw) - splat(mean)) * splat(rs)) * Pair<DT>::unpack(ww);
            if (has_bias) y = y + Pair<DT>::unpack(bw);
            out[j] = Pair<DT>::pack(y);
        }
    }
    return out;
}

// An empty statement that takes every vector of the row as an operand and clobbers memory: the loads written after it (the weight and bias rows) are issued after
// the first pass over the row has started, not hoisted above the loads of x (addnorm_kernels.hip: pin_before_loads)
template <int VPT>
__device__ __forceinline__ void ln_pin_before_loads(v4u (&xv)[VPT]) {
#pragma unroll
    for (int i = 0; i < VPT; ++i) asm volatile("" : "+v"(xv[i]) : : "memory");
}

// Short rows: one WAVE per row, four rows per block and no block barrier, as rmsnorm_quant_wave — physical lane l holds the virtual lanes l, l + 64, l + 128,
// l + 192 of the specification, one accumulator per group, the xor butterfly on each, the four sums left to right: the same float operations in the same order.
__device__ __forceinline__ float ln_wave_sum(float (&acc)[4]) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int gi = 0; gi < 4; ++gi) acc[gi] = acc[gi] + __shfl_xor(acc[gi], off, 64);
    }
    return ((acc[0] + acc[1]) + acc[2]) + acc[3];
}

}  // namespace pq
