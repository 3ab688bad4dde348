// producer_kernels.hip — K1 fused into the op that produces the activation:
//   silu(g) * u           ->  per-token int8 codes + row scales   (K1s: the `down` input of a gated MLP)
//   RMSNorm(x; weight)    ->  per-token int8 codes + row scales   (K1n: the q/k/v and gate/up input of a decoder layer; kernels in rownorm_kernels.h)
// without the bf16 activation ever going to HBM.
// The kernels and the layout decision of K1s are the activation family's (rowmap_kernels.h); this file holds its op and the instantiations.
// Arithmetic follows QSPEC S1-S6: a specified exponential (Cody-Waite + degree-7 Horner with fma),
// IEEE division, storage-dtype rounding after silu and after the product — bit-identical to oracle/qspec_oracle.c.
// Algorithmic traffic: read 2 x elem bytes, write 1 B/elem + 4 B/row (+ elem bytes when h is also requested).
#include "rownorm_kernels.h"
#include "rowmap_kernels.h"
#include "pq_launch.h"

namespace pq {

// K1s: silu(g) * u (QSPEC S1-S5).  The fast-division test and the arithmetic are producer_device.h's.
struct SiluMulOp {
    static constexpr int kInputs = 2;
    static constexpr bool kFastSplit = true, kWideRows = true, kSplitModes = true;
    struct Params {};
    template <int DT> __device__ static __forceinline__ bool fast_ok(uint32_t mn, uint32_t mx, Params) { return silu_fast_div_ok<DT>(mn, mx); }
    template <int DT, bool FASTDIV> __device__ static __forceinline__ v4u vec(const v4u& gv, const v4u& uv, Params) { return silu_mul_vec<DT, FASTDIV>(gv, uv); }
    template <int DT> __device__ static __forceinline__ float spec(float g, float u, Params) {
        return map_one(g, u, [](const auto& ga, const auto& ua, auto& h) { silu_mul_stage<DT, false, 1>(ga, ua, h); });
    }
};
// h = g itself (split modes only): the two halves for a PLAIN column-sharded activation (a rank's heads of the attention output feeding a column-sharded `o`
// projection: pq_quant_rowamax / pq_quant_rowwise_amax).  A copy is not VALU-bound, so its rows of 1025 .. 1536 vectors keep 256 threads x 8.
struct IdentOp {
    static constexpr int kInputs = 1;
    static constexpr bool kFastSplit = false, kWideRows = false, kSplitModes = true;
    struct Params {};
    template <int DT, bool FASTDIV> __device__ static __forceinline__ v4u vec(const v4u& gv, const v4u&, Params) { return gv; }
    template <int DT> __device__ static __forceinline__ float spec(float g, float, Params) { return g; }
};

// dev/test kernel: every 16-bit pattern g of the fast-division domain (0 < |g| <= 86) through the three division forms, u = 1 (so h is the
// stored silu(g)).  out[0] += patterns in the domain, out[1] += patterns whose SHORT result differs from the two-correction form,
// out[2] += patterns whose two-correction form differs from true division.
template <int DT>
__global__ __launch_bounds__(256) void silu_short_check(unsigned long long* __restrict__ out) {
    const uint32_t pat = blockIdx.x * 256u + threadIdx.x;            // 256 blocks x 256 threads = all 65 536 patterns
    const uint32_t mag = pat & 0x7FFFu;
    if (!silu_fast_div_ok<DT>(mag, mag)) return;
    const uint32_t one = DT == PQ_BF16 ? 0x3F80u : 0x3C00u;
    const v4u gv = v4u{pat | (pat << 16), pat | (pat << 16), pat | (pat << 16), pat | (pat << 16)};
    const v4u uv = v4u{one | (one << 16), one | (one << 16), one | (one << 16), one | (one << 16)};
    const v4u a = silu_mul_vec<DT, true, true>(gv, uv), b = silu_mul_vec<DT, true, false>(gv, uv), c = silu_mul_vec<DT, false, false>(gv, uv);
    atomicAdd(&out[0], 1ull);
    if (a[0] != b[0]) atomicAdd(&out[1], 1ull);
    if (b[0] != c[0]) atomicAdd(&out[2], 1ull);
}
void launch_silu_short_check(int dtype, unsigned long long* out, hipStream_t st) {
    if (dtype == PQ_BF16) silu_short_check<PQ_BF16><<<dim3(256), dim3(256), 0, st>>>(out);
    else silu_short_check<PQ_FP16><<<dim3(256), dim3(256), 0, st>>>(out);
}

// the two halves of K1s for a column-sharded intermediate (MODE 1: row amax of these columns -> amax_io; MODE 2: encode against the amax in amax_io).
// Same layouts as the fused kernel (the h vectors are recomputed in MODE 2 — g and u are read twice, from the Infinity Cache the second time — instead of
// parking a 16-bit h in HBM between the two passes: the same 9 bytes per element either way, and no extra buffer).
template <int DT, int MODE, bool IDENT>
void silu_mul_split_dispatch(const void* g, int64_t ldg, const void* u, int64_t ldu, int64_t rows, int64_t cols, uint32_t* amax_io, int8_t* q,
                             int64_t ldq, float* scale, hipStream_t st) {
    static_assert(MODE == 1 || MODE == 2, "split modes");
    using OP = std::conditional_t<IDENT, IdentOp, SiluMulOp>;
    rowmap_dispatch<OP, DT, MODE>(g, ldg, u, ldu, rows, cols, {}, q, ldq, scale, nullptr, 0, amax_io, st);
}

template <int DT>
void silu_mul_quant_dispatch(const void* g, int64_t ldg, const void* u, int64_t ldu, int64_t rows, int64_t cols, int8_t* q,
                             int64_t ldq, float* scale, void* h_out, int64_t ldh, hipStream_t st) {
    rowmap_dispatch<SiluMulOp, DT>(g, ldg, u, ldu, rows, cols, {}, q, ldq, scale, h_out, ldh, nullptr, st);
}

// K1n: the kernels and the layout decision are the norm family's (rownorm_kernels.h), ADD = false
template <int DT>
void rmsnorm_quant_dispatch(const void* x, int64_t ldx, const void* wgt, float eps, int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale,
                            void* h_out, int64_t ldh, hipStream_t st) {
    rmsnorm_rows_dispatch<DT, false, LlamaGain>(x, ldx, nullptr, 0, nullptr, 0, wgt, eps, rows, cols, q, ldq, scale, h_out, ldh, st);
}

PQ_INSTANTIATE_DTYPES(rmsnorm_quant_dispatch)

#define PQ_SPLIT_INST(DT) \
    template void silu_mul_split_dispatch<DT, 1, false>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, uint32_t*, int8_t*, int64_t, float*, hipStream_t); \
    template void silu_mul_split_dispatch<DT, 2, false>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, uint32_t*, int8_t*, int64_t, float*, hipStream_t); \
    template void silu_mul_split_dispatch<DT, 1, true>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, uint32_t*, int8_t*, int64_t, float*, hipStream_t); \
    template void silu_mul_split_dispatch<DT, 2, true>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, uint32_t*, int8_t*, int64_t, float*, hipStream_t);
PQ_SPLIT_INST(PQ_BF16) PQ_SPLIT_INST(PQ_FP16) PQ_SPLIT_INST(PQ_F32)
#undef PQ_SPLIT_INST
template void silu_mul_quant_dispatch<PQ_BF16>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void silu_mul_quant_dispatch<PQ_FP16>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void silu_mul_quant_dispatch<PQ_F32>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);

}  // namespace pq
