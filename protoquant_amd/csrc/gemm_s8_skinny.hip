// gemm_s8_skinny.hip — K3/K4 for decode-like problems (M <= 64 tokens): y[M,N] = dequant(xq[M,K] . wq[N,K]^T).  The DENSE host of the weight-streaming body
// (gemm_stream_body.h; gemm_s8_grouped_stream.hip is its other host).
// With so few tokens the GEMM is a streaming read of the int8 weight matrix — HBM-bound, N*K bytes — and the tiled kernels
// (one 128-row tile per CU, half of every staged K-tile spent on duplicated activation rows, N/128 CUs busy) reach < 1 TB/s.
// Here every wave streams 16 weight rows straight into MFMA fragments, so the weights never touch LDS; the few activation rows come from L2, row-contiguously
// through a wave-private LDS region (STAGE) or, for one token, straight into fragments.  A workgroup = KS waves that split K between them for one 16 RB-row block
// (enough waves in flight to cover HBM latency: KS * U KiB per workgroup), reduce their exact int32 partial tiles through
// LDS and apply QSPEC E1-E4.  Results are bit-identical to every other variant.  This file holds what is the dense kernel's own: where activation row i lies
// (row min(i, M - 1) of X), the epilogue operands with the EPI_* flags, and the launcher; the (RB, KS) of a launch is skinny_plan (pq_plan.hip).
#include <cstdlib>

#include "gemm_stream_body.h"
#include "pq_launch.h"
#include "pq_plan.h"

namespace pq {

struct DenseRows {
    const int8_t* X;
    int64_t ldx;
    int M;
    __device__ __forceinline__ const int8_t* src_row(int i) const { return X + (int64_t)(i < M ? i : M - 1) * ldx; }
};

template <int OUT, int MT, int RB, bool STAGE>       // MT: 16-row tiles of activations (M <= 16 * MT)
__global__ __launch_bounds__(1024) void gemm_s8_skinny(const int8_t* __restrict__ X, int64_t ldx, const int8_t* __restrict__ W,
                                                       int64_t ldw, EpiArgs epi, int M, int N, int K) {
    extern __shared__ __attribute__((aligned(16))) uint8_t sk_smem[];
    stream_body<OUT, MT, RB, STAGE, true>(sk_smem, DenseRows{X, ldx, M}, W, ldw, StreamOut<int32_t>{epi.a_scale, epi.b_scale, epi.bias, epi.y, epi.ldy, epi.flags, 0, M},
                                    (int)blockIdx.x * (16 * RB), N, K);
}

template <int OUT>
void launch_gemm_skinny(const int8_t* A, int64_t lda, const int8_t* B, int64_t ldb, const EpiArgs& epi, int64_t M, int64_t N,
                        int64_t K, hipStream_t st) {
    const int mt = (int)((M + 15) / 16);
    int rb = 1, ks = 1;                                    // (3-4 token tiles x 2 blocks would not fit the register budget: skinny_plan keeps rb = 1 there)
    skinny_plan(M, N, K, &rb, &ks);
    const int64_t blocks = (N + 16 * rb - 1) / (16 * rb);
    const dim3 grid((unsigned)blocks), block((unsigned)(ks * 64));
    const bool stage = opt().skinny_stage && M > 1;       // (one token: its 16 "rows" are one clamped row — the direct loads are already cheap)
    const size_t lds = stream_lds_bytes(ks, mt, rb, stage);
#define PQ_SK(MTv, RBv) stream_launch(stage ? &gemm_s8_skinny<OUT, MTv, RBv, true> : &gemm_s8_skinny<OUT, MTv, RBv, false>, grid, block, lds, st, A, lda, B, ldb, epi, (int)M, (int)N, (int)K)
    if (rb == 2) { if (mt == 1) PQ_SK(1, 2); else PQ_SK(2, 2); }
    else {
        switch (mt) {
            case 1: PQ_SK(1, 1); break;
            case 2: PQ_SK(2, 1); break;
            case 3: PQ_SK(3, 1); break;
            default: PQ_SK(4, 1); break;
        }
    }
#undef PQ_SK
}
template void launch_gemm_skinny<PQ_BF16>(const int8_t*, int64_t, const int8_t*, int64_t, const EpiArgs&, int64_t, int64_t, int64_t, hipStream_t);
template void launch_gemm_skinny<PQ_FP16>(const int8_t*, int64_t, const int8_t*, int64_t, const EpiArgs&, int64_t, int64_t, int64_t, hipStream_t);
template void launch_gemm_skinny<PQ_F32>(const int8_t*, int64_t, const int8_t*, int64_t, const EpiArgs&, int64_t, int64_t, int64_t, hipStream_t);
template void launch_gemm_skinny<OUT_I32>(const int8_t*, int64_t, const int8_t*, int64_t, const EpiArgs&, int64_t, int64_t, int64_t, hipStream_t);

}  // namespace pq
