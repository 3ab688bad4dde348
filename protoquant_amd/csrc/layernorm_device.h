// layernorm_device.h — the device helpers of the LayerNorm-family producers (QSPEC L1-L6), for K1l and K1al
// (rownorm_kernels.h): L2 / L3 / L5 on one 16-byte vector.  Everything is __forceinline__.
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

}  // namespace pq
