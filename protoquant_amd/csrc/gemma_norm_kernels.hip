// gemma_norm_kernels.hip — K1ng: GemmaRMSNorm fused into the per-token int8 quantisation (QSPEC NG1-NG6, then Q1-Q6):
//   GemmaRMSNorm(x; weight) = cast((f32(x) * rs) * (1 + f32(weight)))  ->  int8 codes + row scales   (+ the normalised activation when asked for)
// The q/k/v and gate/up input of a Gemma, Gemma-2 or Gemma-3 decoder layer.  Algorithmic traffic: K1n's (read elem bytes, write 1 B/elem + 4 B/row).
// The kernels are the norm family's (rownorm_kernels.h): rmsnorm_quant_rows / rmsnorm_quant_generic<.., ADD = false, GemmaGain>, K1n with NG5 in N5's place.  They
// are instantiated here, in an object file of their own, so no other object's kernel list depends on this file.
#include "rownorm_kernels.h"
#include "pq_launch.h"

namespace pq {

template <int DT>
void gemma_rmsnorm_quant_dispatch(const void* x, int64_t ldx, const void* wgt, float eps, int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale,
                                  void* h_out, int64_t ldh, hipStream_t st) {
    rmsnorm_rows_dispatch<DT, false, GemmaGain>(x, ldx, nullptr, 0, nullptr, 0, wgt, eps, rows, cols, q, ldq, scale, h_out, ldh, st);
}

PQ_INSTANTIATE_DTYPES(gemma_rmsnorm_quant_dispatch)

}  // namespace pq
