// gemma_norm_kernels.hip — K1ng: GemmaRMSNorm fused into the per-token int8 quantisation (QSPEC NG1-NG6, then Q1-Q6):
//   GemmaRMSNorm(x; weight) = cast((f32(x) * rs) * (1 + f32(weight)))  ->  int8 codes + row scales   (+ the normalised activation when asked for)
// The q/k/v and gate/up input of a Gemma, Gemma-2 or Gemma-3 decoder layer.  Algorithmic traffic: K1n's (read elem bytes, write 1 B/elem + 4 B/row).
// The kernels are gemma_rownorm_kernels.h's, ADD = false, and the layout decision is the norm family's (rownorm_dispatch); they are instantiated here, in an
// object file of their own, so no existing object's kernel list or register allocation depends on this file.
#include "gemma_rownorm_kernels.h"
#include "pq_launch.h"

namespace pq {

template <int DT>
void gemma_rmsnorm_quant_dispatch(const void* x, int64_t ldx, const void* wgt, float eps, int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale,
                                  void* h_out, int64_t ldh, hipStream_t st) {
    const int64_t kb = Elem<DT>::kBytes;
    rownorm_dispatch<DT>(
        {{x, ldx}, {wgt, 0}}, rows, cols, q, ldq, h_out, ldh,
        [&](auto vpt, auto tpr, auto write_h, dim3 grid, int nvec) {
            gemma_rmsnorm_quant_rows<DT, decltype(vpt)::value, decltype(tpr)::value, decltype(write_h)::value, false><<<grid, dim3(256), 0, st>>>(
                reinterpret_cast<const uint8_t*>(x), ldx * kb, nullptr, 0, nullptr, 0, reinterpret_cast<const uint8_t*>(wgt), eps, (int)cols, nvec, rows, q, ldq,
                scale, reinterpret_cast<uint8_t*>(h_out), ldh * kb);
        },
        [&](dim3 grid) { gemma_rmsnorm_quant_generic<DT, false><<<grid, dim3(256), 0, st>>>(x, ldx, nullptr, 0, nullptr, 0, wgt, eps, cols, q, ldq, scale, h_out, ldh); });
}

template void gemma_rmsnorm_quant_dispatch<PQ_BF16>(const void*, int64_t, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void gemma_rmsnorm_quant_dispatch<PQ_FP16>(const void*, int64_t, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void gemma_rmsnorm_quant_dispatch<PQ_F32>(const void*, int64_t, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);

}  // namespace pq
