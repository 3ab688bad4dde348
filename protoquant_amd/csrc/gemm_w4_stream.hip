// gemm_w4_stream.hip — the decode GEMM on int4 weights (M <= 64 tokens): y[M,N] = dequant(xq[M,Kp] . W8[N,Kp]^T) with W8[n][k] = q[n][k] * g[n][k / 128] (QSPEC W1-W4,
// DESIGN.md §2), bit for bit what gemm_s8_skinny gives on the expanded weight (w4_pack_kernels.hip: w4_expand).  With so few tokens the GEMM is a streaming read of the
// weight matrix; here that read is Kp / 2 + Kp / 128 bytes per weight row instead of Kp.
// This is the DENSE host of the int4 weight-streaming body (gemm_w4_stream_body.h, where the work split, the weight movement, the unpack and the multipliers are
// described; gemm_w4_grouped_stream.hip is its grouped host): one matrix, token row i is row i of X, one body per launch — NT token tiles, staged activations for M > 1.
#include "gemm_w4_stream_body.h"
#include "pq_launch.h"

namespace pq {

// token row i of the dense activation matrix, clamped (rows past the last one: the last one again)
struct DenseRows {
    const int8_t* X;
    int64_t ldx;
    int M;
    __device__ __forceinline__ const int8_t* src_row(int i) const { return X + (int64_t)(i < M ? i : M - 1) * ldx; }
};

template <int OUT, int NT, bool STAGE>
__global__ __launch_bounds__(1024) void gemm_w4_stream(const int8_t* __restrict__ X, int64_t ldx, const uint8_t* __restrict__ W4, int64_t ldw4,
                                                       const uint32_t* __restrict__ GS, StreamOut<NoEpiFlags> out, int N, int G) {
    extern __shared__ __attribute__((aligned(16))) uint8_t w4_smem[];
    const StreamOut<NoEpiFlags> all{out.row_scale, out.col_scale, out.bias, out.y, out.ldy, {}, 0, out.rows};      // (first row 0, known to the compiler)
    w4_stream_body<OUT, NT, STAGE>(w4_smem, DenseRows{X, ldx, out.rows}, W4, ldw4, GS, all, (int)blockIdx.x * 16, N, G);
}

template <int OUT>
void launch_gemm_w4_stream(const int8_t* X, int64_t ldx, const uint8_t* W4, int64_t ldw4, const uint8_t* GS, const EpiArgs& epi, int64_t M, int64_t N, int64_t Kp,
                           hipStream_t st) {
    const int nt = (int)((M + 15) / 16), G = (int)(Kp / 128);
    int ks = 1;
    w4_stream_plan(M, N, Kp, &ks);
    const bool stage = M > 1;                              // (one token: its 16 "rows" are one clamped row — direct loads)
    size_t lds = ks > 1 ? (size_t)ks * nt * 64 * sizeof(v4i) : 0;
    if (stage && (size_t)ks * w4_stage_bytes(nt) > lds) lds = (size_t)ks * w4_stage_bytes(nt);
    const dim3 grid((unsigned)((N + 15) / 16)), block((unsigned)(ks * 64));
    const StreamOut<NoEpiFlags> out{epi.a_scale, epi.b_scale, epi.bias, epi.y, epi.ldy, NoEpiFlags{}, 0, (int)M};
    const uint32_t* gs = reinterpret_cast<const uint32_t*>(GS);
#define PQ_W4(NTv, STv) stream_launch(&gemm_w4_stream<OUT, NTv, STv>, grid, block, lds, st, X, ldx, W4, ldw4, gs, out, (int)N, G)
    if (!stage) PQ_W4(1, false);
    else switch (nt) {
        case 1: PQ_W4(1, true); break;
        case 2: PQ_W4(2, true); break;
        case 3: PQ_W4(3, true); break;
        default: PQ_W4(4, true); break;
    }
#undef PQ_W4
}
template void launch_gemm_w4_stream<PQ_BF16>(const int8_t*, int64_t, const uint8_t*, int64_t, const uint8_t*, const EpiArgs&, int64_t, int64_t, int64_t, hipStream_t);
template void launch_gemm_w4_stream<PQ_FP16>(const int8_t*, int64_t, const uint8_t*, int64_t, const uint8_t*, const EpiArgs&, int64_t, int64_t, int64_t, hipStream_t);
template void launch_gemm_w4_stream<PQ_F32>(const int8_t*, int64_t, const uint8_t*, int64_t, const uint8_t*, const EpiArgs&, int64_t, int64_t, int64_t, hipStream_t);
template void launch_gemm_w4_stream<OUT_I32>(const int8_t*, int64_t, const uint8_t*, int64_t, const uint8_t*, const EpiArgs&, int64_t, int64_t, int64_t, hipStream_t);

}  // namespace pq
