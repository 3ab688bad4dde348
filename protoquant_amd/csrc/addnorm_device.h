// addnorm_device.h — QSPEC A1 on one 16-byte vector, shared by the residual-fused producers K1a (addnorm_kernels.hip) and K1al (addlayernorm_kernels.hip).
#pragma once
#include "producer_device.h"

namespace pq {

// A1 on one 16-byte vector: one binary32 add per element (residual + x), then the storage rounding
template <int DT>
__device__ __forceinline__ v4u add_vec(const v4u& xv, const v4u& rv) {
    v4u out;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t xw = xv[j], rw = rv[j];      // copies first (hipcc quirk with vector-element lvalues)
        if constexpr (DT == PQ_F32) out[j] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(float, rw) + __builtin_bit_cast(float, xw));
        else out[j] = Pair<DT>::pack(Pair<DT>::unpack(rw) + Pair<DT>::unpack(xw));
    }
    return out;
}

}  // namespace pq
