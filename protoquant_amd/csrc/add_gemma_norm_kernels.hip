// add_gemma_norm_kernels.hip — K1ang: the residual add fused into GemmaRMSNorm + per-token int8 quantisation (QSPEC A1, then NG1-NG6 and Q1-Q6):
//   s = x + residual  (stored: the new residual stream)  ->  GemmaRMSNorm(s; weight)  ->  int8 codes + row scales   (+ the normalised activation when asked for)
// One kernel where a Gemma decoder layer ran a torch add and K1ng.  Algorithmic traffic: K1a's (7 B/elem for 16-bit rows against 9 for the pair).
// The kernels are the norm family's (rownorm_kernels.h): rmsnorm_quant_rows / rmsnorm_quant_generic<.., ADD = true, GemmaGain>, K1a with NG5 in N5's place; sum_out
// may be exactly x or exactly residual, as for K1a.  They are instantiated here, in an object file of their own.
#include "rownorm_kernels.h"
#include "pq_launch.h"

namespace pq {

template <int DT>
void add_gemma_rmsnorm_quant_dispatch(const void* x, int64_t ldx, const void* res, int64_t ldr, void* sum_out, int64_t lds, const void* wgt, float eps, int64_t rows,
                                      int64_t cols, int8_t* q, int64_t ldq, float* scale, void* h_out, int64_t ldh, hipStream_t st) {
    rmsnorm_rows_dispatch<DT, true, GemmaGain>(x, ldx, res, ldr, sum_out, lds, wgt, eps, rows, cols, q, ldq, scale, h_out, ldh, st);
}

PQ_INSTANTIATE_DTYPES(add_gemma_rmsnorm_quant_dispatch)

}  // namespace pq
