// addnorm_device.h — QSPEC A1 on one 16-byte vector, for the residual-fused producers K1a and K1al (rownorm_kernels.h), and S1 (the scaled residual of K1ma / K1mo,
// scaled_addnorm_kernels.hip) in front of it.
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

}  // namespace pq
