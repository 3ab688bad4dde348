// add_gemma_norm_kernels.hip — K1ang: the residual add fused into GemmaRMSNorm + per-token int8 quantisation (QSPEC A1, then NG1-NG6 and Q1-Q6):
//   s = x + residual  (stored: the new residual stream)  ->  GemmaRMSNorm(s; weight)  ->  int8 codes + row scales   (+ the normalised activation when asked for)
// One kernel where a Gemma decoder layer ran a torch add and K1ng.  Algorithmic traffic: K1a's (7 B/elem for 16-bit rows against 9 for the pair).
// The kernels are gemma_rownorm_kernels.h's, ADD = true, and the layout decision is the norm family's (rownorm_dispatch); sum_out may be exactly x or exactly
// residual, as for K1a.  They are instantiated here, in an object file of their own.
#include "gemma_rownorm_kernels.h"
#include "pq_launch.h"

namespace pq {

template <int DT>
void add_gemma_rmsnorm_quant_dispatch(const void* x, int64_t ldx, const void* res, int64_t ldr, void* sum_out, int64_t lds, const void* wgt, float eps, int64_t rows,
                                      int64_t cols, int8_t* q, int64_t ldq, float* scale, void* h_out, int64_t ldh, hipStream_t st) {
    const int64_t kb = Elem<DT>::kBytes;
    rownorm_dispatch<DT>(
        {{x, ldx}, {res, ldr}, {sum_out, lds}, {wgt, 0}}, rows, cols, q, ldq, h_out, ldh,
        [&](auto vpt, auto tpr, auto write_h, dim3 grid, int nvec) {
            gemma_rmsnorm_quant_rows<DT, decltype(vpt)::value, decltype(tpr)::value, decltype(write_h)::value, true><<<grid, dim3(256), 0, st>>>(
                reinterpret_cast<const uint8_t*>(x), ldx * kb, reinterpret_cast<const uint8_t*>(res), ldr * kb, reinterpret_cast<uint8_t*>(sum_out), lds * kb,
                reinterpret_cast<const uint8_t*>(wgt), eps, (int)cols, nvec, rows, q, ldq, scale, reinterpret_cast<uint8_t*>(h_out), ldh * kb);
        },
        [&](dim3 grid) { gemma_rmsnorm_quant_generic<DT, true><<<grid, dim3(256), 0, st>>>(x, ldx, res, ldr, sum_out, lds, wgt, eps, cols, q, ldq, scale, h_out, ldh); });
}

template void add_gemma_rmsnorm_quant_dispatch<PQ_BF16>(const void*, int64_t, const void*, int64_t, void*, int64_t, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void add_gemma_rmsnorm_quant_dispatch<PQ_FP16>(const void*, int64_t, const void*, int64_t, void*, int64_t, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void add_gemma_rmsnorm_quant_dispatch<PQ_F32>(const void*, int64_t, const void*, int64_t, void*, int64_t, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);

}  // namespace pq
