// scaled_addnorm_kernels.hip — K1ma and its add-only form K1mo: the SCALED residual add of the Granite decoders fused into RMSNorm + per-token int8 quantisation
// (QSPEC S1, A1, then N1-N6 and Q1-Q6).  These decoders compute r1 = x + attn(norm(x)) * m and out = r1 + mlp(norm(r1)) * m with one scalar m per model:
//   p = cast_rne(f32(x) * m)          S1: one binary32 product, one storage rounding (f32 rows: the binary32 product itself); NEVER stored, never fused into the add
//   K1ma:  s = cast_rne(f32(residual) + f32(p))  STORED (A1: the new residual stream)  ->  RMSNorm(s; weight)  ->  int8 codes + row scales   (+ h when asked for)
//   K1mo:  s STORED, nothing else (weight == q == scale == nullptr: the end of a chain)
// which is what `residual + x * m` computes in eager torch — two roundings, where fma(x, m, residual) would round once (and differs in about 15 % of random elements).
// Algorithmic traffic for 16-bit rows: K1ma 7 B/elem (K1a's), K1mo 6; against 13 for the eager multiply, the eager add and K1n.
// The kernels are the norm family's (rownorm_kernels.h): rmsnorm_quant_rows / rmsnorm_quant_generic<.., ADD = true, LlamaGain, QUANT, float>, K1a with one more kernel
// argument (`float mult`, after ldr_bytes) and S1 (scale_vec, addnorm_device.h) in front of the add; QUANT = false is K1mo.  The argument is a parameter pack of the
// templates, empty in K1n / K1a / K1ng / K1ang, so those keep their argument lists: with it every kernel of this object and of theirs compiles to the instructions it had
// when this file held a template of its own.  With `mult` as a trailing argument of every instantiation 78 of the 87 kernels here changed ("The RMS row
// kernels on one template").  They are instantiated here, in an object file of their own.
// Aliasing: sum_out may be exactly x or exactly residual, as for K1a.
#include "rownorm_kernels.h"
#include "pq_launch.h"

namespace pq {

// wgt == nullptr: K1mo (q, scale and h_out are null as well; pq_api.hip refuses a partly-null group)
template <int DT>
void scaled_add_rmsnorm_quant_dispatch(const void* x, int64_t ldx, const void* res, int64_t ldr, float mult, void* sum_out, int64_t lds, const void* wgt, float eps,
                                       int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale, void* h_out, int64_t ldh, hipStream_t st) {
    rmsnorm_rows_dispatch<DT, true, LlamaGain, true>(x, ldx, res, ldr, sum_out, lds, wgt, eps, rows, cols, q, ldq, scale, h_out, ldh, st, mult);
}

PQ_INSTANTIATE_DTYPES(scaled_add_rmsnorm_quant_dispatch)

}  // namespace pq
