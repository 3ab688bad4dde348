// geglu_kernels.hip — K1gg: the tanh-GELU gate of a gated MLP fused into the per-token int8 quantisation (QSPEC GG1-GG3, then Q1-Q6):
//   a = cast(gelu_tanh(g))   (QSPEC U2, stored)      h = cast(a * u)      ->  per-token int8 codes + row scales
// the `down` input of a Gemma, Gemma-2 or Gemma-3 MLP (down(act_fn(gate(x)) * up(x)), act_fn = gelu_pytorch_tanh), without the 16-bit intermediate ever going
// to HBM.  Algorithmic traffic: K1s's — read 2 x elem bytes, write 1 B/elem + 4 B/row (5 B/elem for 16-bit rows against 13 for torch's gelu, mul and K1).
// The kernels and the layout decision are the activation family's (rowmap_kernels.h); the exponential and the quotient are producer_device.h's, the ones K1u's
// GELU (act_kernels.hip) is built from, and tests/test_gpu_geglu.py holds the two gates together on every 16-bit pattern — as rows of 512 sorted by magnitude, where
// whole waves take the division-free quotient on all of its domain, and as wide rows and through the generic kernel, which divide.  This file holds the op's
// instantiations, in an object file of its own; the op's arithmetic and its trait are geglu_device.h's (K1gh shares them).
#include "geglu_device.h"
#include "rowmap_kernels.h"
#include "pq_launch.h"

namespace pq {

template <int DT>
void gelu_mul_quant_dispatch(const void* g, int64_t ldg, const void* u, int64_t ldu, int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale, void* h_out,
                             int64_t ldh, hipStream_t st) {
    rowmap_dispatch<GegluOp, DT>(g, ldg, u, ldu, rows, cols, {}, q, ldq, scale, h_out, ldh, nullptr, st);
}

template void gelu_mul_quant_dispatch<PQ_BF16>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void gelu_mul_quant_dispatch<PQ_FP16>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void gelu_mul_quant_dispatch<PQ_F32>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);

}  // namespace pq
