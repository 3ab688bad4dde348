// pq_plan.h — the planners of libpq_hip.so (pq_plan.hip): which GEMM variant, which split, which tile a shape gets.  They decide and launch nothing; every switch
// they read comes from the snapshot the C-ABI call in progress pinned (pq::opt(), pq_common.h).
#pragma once
#include "pq_common.h"

namespace pq {

enum Variant { V_AUTO = 0, V_GENERIC, V_SP256_16, V_SP128_16, V_SP128X128, V_RING128, V_SKINNY, V_RING64X128, V_RING64X64, V_RING128X160 };

Variant parse_variant(const char* option);      // a PQ_FORCE_VARIANT string; null, empty or unknown = V_AUTO
Variant forced_variant();
int device_cus();
int device_xcds();

Variant pick_variant(const int8_t* a, int64_t lda, const int8_t* b, int64_t ldb, int64_t M, int64_t N, int64_t K);
int tail_split_plan(int64_t M, int64_t N, int64_t* lead);
int splitk_plan(int64_t M, int64_t N, int64_t K, int* tm_out);
int fsk_plan(int64_t M, int64_t N, int64_t K);
Variant kslabs_in_place(const int8_t* a, int64_t lda, int64_t slab_stride, int64_t kps, const int8_t* b, int64_t ldb, int64_t M, int64_t N, int64_t K);
int kslabs_fsk_in_place(const int8_t* a, int64_t lda, int64_t slab_stride, int64_t kps, const int8_t* b, int64_t ldb, int64_t M, int64_t N, int64_t K);
int grouped_plan(int32_t E, int64_t M_total, int64_t N);

// what pq_gemm_variant_name, pq_kslabs_way_name and pq_grouped_variant_name return (the caller has pinned the snapshot)
const char* gemm_variant_name(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb);
const char* kslabs_way_name(const int8_t* a, int64_t lda, int64_t slab_stride, int64_t k_per_slab, const int8_t* b, int64_t ldb, int64_t M, int64_t N, int64_t K,
                            size_t workspace_bytes);
const char* grouped_variant_name(int32_t E, int64_t M_total, int64_t N);

}  // namespace pq
