// addnorm_device.h — QSPEC A1 on one 16-byte vector, for the residual-fused producers K1a and K1al (rownorm_kernels.h).
#pragma once
#include "producer_device.h"

namespace pq {

// A1 for one element: one binary32 add (residual + x), then the storage rounding
template <int DT>
__device__ __forceinline__ typename Elem<DT>::store_t add_elem(typename Elem<DT>::store_t r, typename Elem<DT>::store_t x) {
    return Elem<DT>::from_f32(Elem<DT>::to_f32(r) + Elem<DT>::to_f32(x));
}
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
