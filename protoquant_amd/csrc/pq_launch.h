// pq_launch.h — every host launcher and dispatcher that crosses a translation unit, declared ONCE with named parameters.  Included by pq_api.hip / pq_plan.hip (the
// callers) and by each .hip file that defines one of them: a definition whose return type or default arguments disagree does not compile there, one whose parameter list
// drifts is a different overload and leaves the explicit instantiation in that file (or the link) without a match.  Default arguments live here only; the explicit
// instantiations stay with the definitions.
#pragma once
#include "pq_common.h"

namespace pq {
struct EpiArgs;      // gemm_epilogue.h

// ---- quant_kernels.hip: K1 / K2 / dequantisation and the quotient / encode self-tests
template <int DT> void quant_rowwise_dispatch(const void* x, int64_t rows, int64_t cols, int64_t ldx, int8_t* q, int64_t ldq, float* scale, hipStream_t st);
template <int DT> hipError_t quant_colwise_dispatch(const void* x, int64_t rows, int64_t cols, int64_t ldx, int8_t* q, int64_t ldq, float* scale, hipStream_t st);
template <int ODT> void dequant_dispatch(const int8_t* q, int64_t ldq, const float* scale, int axis, int64_t rows, int64_t cols, void* out, int64_t ldo, hipStream_t st);
void launch_fast_quotient_check(const uint32_t* xb, const uint32_t* sb, int64_t n, unsigned long long* out, hipStream_t st);
void launch_half_encode_check(int dtype, unsigned long long* out, hipStream_t st);

// ---- producer_kernels.hip, glu_kernels.hip, act_kernels.hip and the four norm files: the producer-fused quantisations (K1s, K1g, K1u, K1n, K1a, K1l, K1al)
template <int DT> void silu_mul_quant_dispatch(const void* g, int64_t ldg, const void* u, int64_t ldu, int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale,
                                               void* h_out, int64_t ldh, hipStream_t st);
template <int DT, int MODE, bool IDENT> void silu_mul_split_dispatch(const void* g, int64_t ldg, const void* u, int64_t ldu, int64_t rows, int64_t cols, uint32_t* amax_io,
                                                                     int8_t* q, int64_t ldq, float* scale, hipStream_t st);
void launch_silu_short_check(int dtype, unsigned long long* out, hipStream_t st);
template <int DT> void glu_quant_dispatch(int kind, const void* g, int64_t ldg, const void* u, int64_t ldu, int64_t rows, int64_t cols, float limit, float alpha, int8_t* q,
                                          int64_t ldq, float* scale, void* h_out, int64_t ldh, hipStream_t st);
float glu_limit_in_dtype(int dtype, float limit);
void launch_glu_short_check(int dtype, int kind, float limit, float alpha, unsigned long long* out, hipStream_t st);
template <int DT> void act_quant_dispatch(int kind, const void* x, int64_t ldx, int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale, void* h_out, int64_t ldh,
                                          hipStream_t st);
template <int DT> void rmsnorm_quant_dispatch(const void* x, int64_t ldx, const void* wgt, float eps, int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale,
                                              void* h_out, int64_t ldh, hipStream_t st);
template <int DT> void add_rmsnorm_quant_dispatch(const void* x, int64_t ldx, const void* res, int64_t ldr, void* sum_out, int64_t lds, const void* wgt, float eps,
                                                  int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale, void* h_out, int64_t ldh, hipStream_t st);
template <int DT> void layernorm_quant_dispatch(const void* x, int64_t ldx, const void* wgt, const void* bias, float eps, int64_t rows, int64_t cols, int8_t* q, int64_t ldq,
                                                float* scale, void* h_out, int64_t ldh, hipStream_t st);
template <int DT> void add_layernorm_quant_dispatch(const void* x, int64_t ldx, const void* res, int64_t ldr, void* sum_out, int64_t lds, const void* wgt, const void* bias,
                                                    float eps, int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale, void* h_out, int64_t ldh, hipStream_t st);
// ---- parallel_layernorm_kernels.hip: the parallel residual (K1pl: a, b non-null; K1l2: a, b, sum_out null and both groups; wgt2 == nullptr: one norm, q2 / scale2 / h2 null)
template <int DT> void parallel_layernorm_quant_dispatch(const void* a, int64_t lda, const void* b, int64_t ldb, const void* c, int64_t ldc, void* sum_out, int64_t lds,
                                                         const void* wgt1, const void* bias1, float eps1, const void* wgt2, const void* bias2, float eps2, int64_t rows,
                                                         int64_t cols, int8_t* q1, int64_t ldq1, float* scale1, void* h1, int64_t ldh1, int8_t* q2, int64_t ldq2,
                                                         float* scale2, void* h2, int64_t ldh2, hipStream_t st);
// ---- gemma_norm_kernels.hip, add_gemma_norm_kernels.hip, geglu_kernels.hip, gemma_postnorm_kernels.hip: the Gemma forms (K1ng, K1ang, K1gg, K1pang / K1pa)
template <int DT> void gemma_rmsnorm_quant_dispatch(const void* x, int64_t ldx, const void* wgt, float eps, int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale,
                                                    void* h_out, int64_t ldh, hipStream_t st);
template <int DT> void add_gemma_rmsnorm_quant_dispatch(const void* x, int64_t ldx, const void* res, int64_t ldr, void* sum_out, int64_t lds, const void* wgt, float eps,
                                                        int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale, void* h_out, int64_t ldh, hipStream_t st);
// (wgt == nullptr: the add-only form K1pa — q, scale and h_out are null as well)
template <int DT> void gemma_postnorm_add_rmsnorm_quant_dispatch(const void* x, int64_t ldx, const void* pwgt, float post_eps, const void* res, int64_t ldr, void* sum_out,
                                                                 int64_t lds, const void* wgt, float eps, int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale,
                                                                 void* h_out, int64_t ldh, hipStream_t st);
// ---- olmo_postnorm_kernels.hip: the post-norm flow of OLMo-2 / OLMo-3 (K1oq; q == scale == nullptr: K1oa; res == nullptr as well: K1on, the norm alone)
template <int DT> void olmo_postnorm_add_quant_dispatch(const void* x, int64_t ldx, const void* pwgt, float post_eps, const void* res, int64_t ldr, void* sum_out, int64_t lds,
                                                        int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale, hipStream_t st);
// ---- head_norm_kernels.hip: the per-head norm of q and k (K1hn; gain: PQ_GAIN_LLAMA / PQ_GAIN_GEMMA; operands addressed as base + o * ld_o + i * ld_i + c, in elements)
template <int DT> void head_rmsnorm_dispatch(const void* x, int64_t ld_xo, int64_t ld_xi, const void* wgt, float eps, int gain, int64_t n_outer, int64_t n_inner, int64_t cols,
                                             void* out, int64_t ld_oo, int64_t ld_oi, hipStream_t st);
// ---- scaled_addnorm_kernels.hip: the scaled residual add of the Granite decoders (K1ma; wgt == nullptr: the add-only form K1mo — q, scale and h_out are null as well)
template <int DT> void scaled_add_rmsnorm_quant_dispatch(const void* x, int64_t ldx, const void* res, int64_t ldr, float mult, void* sum_out, int64_t lds, const void* wgt,
                                                         float eps, int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale, void* h_out, int64_t ldh, hipStream_t st);
template <int DT> void gelu_mul_quant_dispatch(const void* g, int64_t ldg, const void* u, int64_t ldu, int64_t rows, int64_t cols, int8_t* q, int64_t ldq, float* scale,
                                               void* h_out, int64_t ldh, hipStream_t st);

// ---- the GEMMs (K3 + K4): gemm_s8_generic.hip, gemm_s8_skinny.hip, gemm_s8_ring.hip, gemm_s8_fast.hip
template <int OUT> void launch_gemm_generic(const int8_t* A, int64_t lda, const int8_t* B, int64_t ldb, const EpiArgs& epi, int64_t M, int64_t N, int64_t K, hipStream_t st);
template <int OUT> void launch_gemm_skinny(const int8_t* A, int64_t lda, const int8_t* B, int64_t ldb, const EpiArgs& epi, int64_t M, int64_t N, int64_t K, hipStream_t st);
template <int OUT> void launch_gemm_ringt(int tile, const int8_t* A, int64_t lda, const int8_t* B, int64_t ldb, const EpiArgs& epi, int64_t M, int64_t N, int64_t K,
                                          hipStream_t st, int64_t a_slab_stride = 0, int64_t a_k_per_slab = 0);
template <int OUT> void launch_gemm_ring128(const int8_t* A, int64_t lda, const int8_t* B, int64_t ldb, const EpiArgs& epi, int64_t M, int64_t N, int64_t K, hipStream_t st,
                                            int64_t a_slab_stride = 0, int64_t a_k_per_slab = 0);
template <int OUT, int TM, int TN> void launch_gemm_fast(const int8_t* A, int64_t lda, const int8_t* B, int64_t ldb, const EpiArgs& epi, int64_t M, int64_t N, int64_t K,
                                                         hipStream_t st);
bool gemm_fast_eligible(const int8_t* A, int64_t lda, const int8_t* B, int64_t ldb, int64_t M, int64_t N, int64_t K);
template <int TM> void launch_gemm_splitk_i32(const int8_t* A, int64_t lda, const int8_t* B, int64_t ldb, int32_t* slabs, int64_t M, int64_t N, int64_t K, int kslices,
                                              hipStream_t st, int nxcd);
template <int OUT> void launch_splitk_reduce(const int32_t* slabs, int kslices, int64_t M, int64_t N, const EpiArgs& epi, hipStream_t st);
template <int OUT> bool launch_gemm_fsk(const int8_t* A, int64_t lda, const int8_t* B, int64_t ldb, const EpiArgs& epi, int64_t M, int64_t N, int64_t K, int kslices,
                                        void* workspace, hipStream_t st, int64_t a_slab_stride = 0, int64_t a_k_per_slab = 0);
bool fsk_kslabs_ok(int64_t K, int64_t k_per_slab, int kslices);
size_t fsk_workspace_bytes(int64_t M, int64_t N, int kslices);
void set_stamp_buffer(unsigned long long* p);

// ---- the grouped GEMMs of a mixture-of-experts layer (gemm_s8_grouped.hip, gemm_s8_grouped_stream.hip) and its routing / combine kernels (moe_kernels.hip)
template <int OUT> void launch_gemm_grouped(int tile, const int8_t* X, int64_t ldx, const int32_t* qrow, int64_t x_rows, const int8_t* W, int64_t ldw, int64_t w_stride,
                                            const EpiArgs& epi, const int32_t* offsets, int E, int64_t M_total, int64_t N, int64_t K, int rot, hipStream_t st);
template <int OUT> void launch_gemm_grouped_stream(const int8_t* X, int64_t ldx, const int32_t* qrow, int64_t x_rows, const int8_t* W, int64_t ldw, int64_t w_stride,
                                                   const EpiArgs& epi, const int32_t* offsets, int E, int64_t M_total, int64_t N, int64_t K, hipStream_t st);
void grouped_stream_plan(int32_t E, int64_t M_total, int64_t N, int64_t K, int* mt_out, int* rb_out, int* ks_out);
const char* grouped_stream_plan_name(int mt, int rb, int ks);
size_t moe_route_workspace_bytes(int64_t npairs, int E);
void launch_moe_route(const void* ids, bool ids_are_int64, int64_t ld_ids, int64_t T, int k, int E, int32_t* offsets, int32_t* row_index, int32_t* rows_of, int32_t* slot_of,
                      const float* xs, float* xs_sorted, void* workspace, hipStream_t st);
template <int DT> void moe_combine_dispatch(const void* y, int64_t ldy, int64_t M_total, const int32_t* rows_of, const int32_t* slot_of, const void* w, int64_t ld_w, int64_t T,
                                            int k, int64_t H, void* out, int64_t ld_out, hipStream_t st);
// ---- moe_topk_kernels.hip: the expert selection behind the router GEMM (K-rt; DT: the logits' dtype; kind: PQ_ROUTER_*; w_dtype: a PQ_* dtype code of its own)
template <int DT> void moe_topk_dispatch(const void* logits, int64_t ld_logits, int64_t T, int E, int k, int kind, int renormalise, void* weights, int w_dtype, int64_t ld_w,
                                         void* ids, bool ids_are_int64, int64_t ld_ids, hipStream_t st);
}  // namespace pq
