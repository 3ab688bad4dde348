// layernorm_kernels.hip — K1l: LayerNorm (weight, optional bias) fused into the per-token int8 quantisation (QSPEC L1-L6, then Q1-Q6):
//   LayerNorm(x; weight, bias, eps)  ->  int8 codes + row scales   (+ the normalised activation when asked for)
// for the decoders built from LayerNorm and a plain two-linear MLP (GPT-2, StarCoder2, GPT-NeoX, Falcon, Phi, OPT): the normalised activation feeding c_attn /
// q, k, v / c_fc never goes to HBM.  Algorithmic traffic: read elem bytes, write 1 B/elem + 4 B/row (3 B/elem for 16-bit rows against 7 for torch's LayerNorm
// followed by K1); the weight and bias rows come from cache.
// The kernels and the layout decision are the norm family's (rownorm_kernels.h), ADD = false; they are instantiated here, in an object file of their own.
#include "rownorm_kernels.h"
#include "pq_launch.h"

namespace pq {

template <int DT>
void layernorm_quant_dispatch(const void* x, int64_t ldx, const void* wgt, const void* bias, float eps, int64_t rows, int64_t cols, int8_t* q, int64_t ldq,
                              float* scale, void* h_out, int64_t ldh, hipStream_t st) {
    const int64_t kb = Elem<DT>::kBytes;
    rownorm_dispatch<DT>(
        {{x, ldx}, {wgt, 0}, {bias, 0}}, rows, cols, q, ldq, h_out, ldh,
        [&](auto vpt, auto tpr, auto write_h, dim3 grid, int nvec) {
            layernorm_quant_rows<DT, decltype(vpt)::value, decltype(tpr)::value, decltype(write_h)::value, false><<<grid, dim3(256), 0, st>>>(
                reinterpret_cast<const uint8_t*>(x), ldx * kb, nullptr, 0, nullptr, 0, reinterpret_cast<const uint8_t*>(wgt), reinterpret_cast<const uint8_t*>(bias),
                eps, (int)cols, nvec, rows, q, ldq, scale, reinterpret_cast<uint8_t*>(h_out), ldh * kb);
        },
        [&](dim3 grid) {
            layernorm_quant_generic<DT, false><<<grid, dim3(256), 0, st>>>(x, ldx, nullptr, 0, nullptr, 0, wgt, bias, eps, cols, q, ldq, scale, h_out, ldh);
        });
}

template void layernorm_quant_dispatch<PQ_BF16>(const void*, int64_t, const void*, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void layernorm_quant_dispatch<PQ_FP16>(const void*, int64_t, const void*, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void layernorm_quant_dispatch<PQ_F32>(const void*, int64_t, const void*, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);

}  // namespace pq
