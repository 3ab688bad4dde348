// addnorm_kernels.hip — K1a: the residual add fused into RMSNorm + per-token int8 quantisation (QSPEC A1, then N1-N6 and Q1-Q6):
//   s = x + residual  (stored: the new residual stream)  ->  RMSNorm(s; weight)  ->  int8 codes + row scales   (+ the normalised activation when asked for)
// One kernel where a decoder layer ran a torch add and K1n: the residual stream is written once and normalised from the registers that hold it, instead of being
// written by one kernel and read straight back by the next.  Algorithmic traffic: read 2 x elem bytes, write elem bytes + 1 B/elem + 4 B/row (7 B/elem for 16-bit
// rows against 9 for the pair).
// The kernels and the layout decision are the norm family's (rownorm_kernels.h), ADD = true; they are instantiated here, in an object file of their own, so the
// register allocation of K1s / K1n does not depend on this file.
#include "rownorm_kernels.h"
#include "pq_launch.h"

namespace pq {

template <int DT>
void add_rmsnorm_quant_dispatch(const void* x, int64_t ldx, const void* res, int64_t ldr, void* sum_out, int64_t lds, const void* wgt, float eps, int64_t rows,
                                int64_t cols, int8_t* q, int64_t ldq, float* scale, void* h_out, int64_t ldh, hipStream_t st) {
    rmsnorm_rows_dispatch<DT, true, LlamaGain>(x, ldx, res, ldr, sum_out, lds, wgt, eps, rows, cols, q, ldq, scale, h_out, ldh, st);
}

PQ_INSTANTIATE_DTYPES(add_rmsnorm_quant_dispatch)

}  // namespace pq
