// gemm_w4_stream.hip — the decode GEMM on int4 weights (M <= 64 tokens): y[M,N] = dequant(xq[M,Kp] . W8[N,Kp]^T) with W8[n][k] = q[n][k] * g[n][k / 128] (QSPEC W1-W4,
// DESIGN.md §2), bit for bit what gemm_s8_skinny gives on the expanded weight (w4_pack_kernels.hip: w4_expand).  With so few tokens the GEMM is a streaming read of the
// weight matrix; here that read is Kp / 2 + Kp / 128 bytes per weight row instead of Kp.
// Work split: a workgroup = KS waves over one block of 16 weight rows, the waves split the Kp / 128 GROUPS in balanced slices, reduce their exact int32 partial tiles
// through LDS, and wave t finishes token tile t with QSPEC E1-E4 (epi_convert) — the split of the int8 body (gemm_stream_body.h), whose StreamOut / stream_launch this file
// uses; the body itself is not instantiated here.
// Weight movement: lane (r = lane & 15, c = lane >> 4) loads the 16 packed bytes 64 j + 16 c .. + 15 of row n0 + r — ONE load holds its A fragments of the two k-steps of
// group j: the low nibbles are k = 128 j + 16 c .. + 15 (step 2 j), the high nibbles k = 128 j + 64 + 16 c .. (step 2 j + 1).  No LDS; two batches of loads in flight.
// Unpack: hi = v & 0xF0F0F0F0 and lo = (v << 4) & 0xF0F0F0F0 are the signed bytes 16 q — three VALU operations per packed dword, none for the sign.
// Multipliers: the two MFMAs of a group go into a zeroed group accumulator (|16 sum| <= 128 * 128 * 112 < 2^23), then total += (acc >> 4) * g for the lane's four rows
// n0 + 4 c .. + 3, whose multipliers are one dword of gs.  The shift is exact, the product fits 24 bits (v_mad_i32_i24).  `total` is the int32 sum of the int8 GEMM on W8.
// Activations: the same int8 codes; for M > 1 row-contiguous loads into a wave-private padded LDS region and ds_read_b128 fragments (the body's STAGE scheme), for one
// token direct loads.  Nibble 0x8 (reserved, never packed) unpacks to q = -8: a different sum, no address depends on it.
#include "gemm_stream_body.h"
#include "pq_launch.h"
#include "pq_plan.h"

namespace pq {

// bytes of one wave's staging region: nt * 16 rows of a batch (w4_stream_batch groups x 128 bytes of K), row stride padded by 16 B
constexpr int w4_stage_bytes(int nt) { return nt * 16 * (w4_stream_batch(nt) * 128 + 16); }

template <int OUT, int NT, bool STAGE>
__global__ __launch_bounds__(1024) void gemm_w4_stream(const int8_t* __restrict__ X, int64_t ldx, const uint8_t* __restrict__ W4, int64_t ldw4,
                                                       const uint32_t* __restrict__ GS, StreamOut<NoEpiFlags> out, int N, int G) {
    extern __shared__ __attribute__((aligned(16))) uint8_t w4_smem[];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), KS = blockDim.x >> 6;
    const int r = lane & 15, c = lane >> 4;
    const int n0 = (int)blockIdx.x * 16, M = out.rows;
    constexpr int U = w4_stream_batch(NT);

    // this wave's groups: a balanced slice of the G groups (empty when there are more waves than groups)
    const int j0 = (int)((int64_t)G * w / KS), j1 = (int)((int64_t)G * (w + 1) / KS);
    const int nrow = n0 + r < N ? n0 + r : N - 1;                                  // clamp: rows past the edge re-read a valid row
    const uint8_t* wp = W4 + (int64_t)nrow * ldw4 + c * 16;
    const int quads = (N + 3) >> 2, quad = (n0 >> 2) + c < quads ? (n0 >> 2) + c : quads - 1;      // gs holds ceil(N / 4) row quads
    const uint32_t* gp = GS + (int64_t)quad * G;
    const int8_t* xp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) { const int i = t * 16 + r; xp[t] = X + (int64_t)(i < M ? i : M - 1) * ldx + c * 16; }
    v4i total[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) total[t] = v4i{0, 0, 0, 0};

    // one group: two MFMAs per token tile into a zeroed accumulator, then the rescale of the lane's four rows
    auto group = [&](const v4u& v, uint32_t g4, const v4i (&fx)[2][NT]) {
        v4i lo, hi;
#pragma unroll
        for (int d = 0; d < 4; ++d) { hi[d] = (int)(v[d] & 0xF0F0F0F0u); lo[d] = (int)((v[d] << 4) & 0xF0F0F0F0u); }
        const int g[4] = {(int)(g4 & 0xFF), (int)((g4 >> 8) & 0xFF), (int)((g4 >> 16) & 0xFF), (int)(g4 >> 24)};
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            v4i a = __builtin_amdgcn_mfma_i32_16x16x64_i8(lo, fx[0][t], v4i{0, 0, 0, 0}, 0, 0, 0);
            a = __builtin_amdgcn_mfma_i32_16x16x64_i8(hi, fx[1][t], a, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) total[t][i] += __mul24(a[i] >> 4, g[i]);
        }
    };

    // STAGE: a batch is U groups = UPR = 8 U 16-byte units per token row; a load instruction covers 64 / UPR rows
    constexpr int UPR = 8 * U, RPI = 64 / UPR, NLD = NT * 16 / RPI, RSTR = U * 128 + 16;
    uint8_t* const stg = w4_smem + (size_t)w * w4_stage_bytes(NT);
    const int lrow = lane / UPR, lunit = lane % UPR;
    const int8_t* xrow[STAGE ? NLD : 1];
    if constexpr (STAGE) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) { const int m = i * RPI + lrow; xrow[i] = X + (int64_t)(m < M ? m : M - 1) * ldx + lunit * 16; }
    }
    auto load_w = [&](v4u (&fw)[U], uint32_t (&fg)[U], int jb) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            fw[u] = *reinterpret_cast<const v4u*>(wp + (int64_t)(jb + u) * 64);
            fg[u] = gp[jb + u];
        }
    };
    auto compute = [&](const v4u (&fw)[U], const uint32_t (&fg)[U], int jb) {
        v4i fx[U][2][NT];
        if constexpr (!STAGE) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int t = 0; t < NT; ++t) fx[u][h][t] = *reinterpret_cast<const v4i*>(xp[t] + (int64_t)(jb + u) * 128 + h * 64);
        } else {
            v4i xr[NLD];
#pragma unroll
            for (int i = 0; i < NLD; ++i) xr[i] = *reinterpret_cast<const v4i*>(xrow[i] + (int64_t)jb * 128);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                  // the previous batch's fragment reads have returned: its region may be overwritten
#pragma unroll
            for (int i = 0; i < NLD; ++i) *reinterpret_cast<v4i*>(stg + (i * RPI + lrow) * RSTR + lunit * 16) = xr[i];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                  // wave-private region, LDS operations of one wave execute in order: written -> readable
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int t = 0; t < NT; ++t) fx[u][h][t] = *reinterpret_cast<const v4i*>(stg + (t * 16 + r) * RSTR + ((u * 2 + h) * 4 + c) * 16);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) group(fw[u], fg[u], fx[u]);
    };
    int j = j0;
    if (j + U <= j1) {                  // the weights of batch j + U are requested BEFORE the MFMAs of batch j (two register sets)
        v4u fw0[U], fw1[U];
        uint32_t fg0[U], fg1[U];
        load_w(fw0, fg0, j);
        for (;;) {
            const bool more1 = j + 2 * U <= j1;
            if (more1) load_w(fw1, fg1, j + U);
            compute(fw0, fg0, j); j += U;
            if (!more1) break;
            const bool more2 = j + 2 * U <= j1;
            if (more2) load_w(fw0, fg0, j + U);
            compute(fw1, fg1, j); j += U;
            if (!more2) break;
        }
    }
    for (; j < j1; ++j) {               // the groups that do not fill a batch
        v4i fx[2][NT];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int t = 0; t < NT; ++t) fx[h][t] = *reinterpret_cast<const v4i*>(xp[t] + (int64_t)j * 128 + h * 64);
        group(*reinterpret_cast<const v4u*>(wp + (int64_t)j * 64), gp[j], fx);
    }

    // ---- exact reduction of the KS partial tiles through LDS, then E1-E4.  D[row <-> n][col <-> m]: the lane holds n = n0 + 4 c .. + 3 of token 16 t + r.
    v4i* red = reinterpret_cast<v4i*>(w4_smem);
    if (KS > 1) {
        if constexpr (STAGE) __syncthreads();            // the reduction buffer overlays the staging regions of ALL waves
#pragma unroll
        for (int t = 0; t < NT; ++t) red[(w * NT + t) * 64 + lane] = total[t];
        __syncthreads();
    }
    using O = typename OutElem<OUT>::type;
    O* y = reinterpret_cast<O*>(out.y);
    const bool has_bias = (OUT != OUT_I32) && out.bias != nullptr;
    for (int t = w; t < NT; t += KS) {                    // wave w finishes token tiles w, w + KS, ...
        v4i sum = total[0];
        if (KS > 1) {
            sum = v4i{0, 0, 0, 0};
            for (int k = 0; k < KS; ++k) sum += red[(k * NT + t) * 64 + lane];
        } else {
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) if (tt == t) sum = total[tt];
        }
        const int m = t * 16 + r, nb = n0 + c * 4;
        if (m >= M || nb >= N) continue;
        float as = 1.0f;
        if constexpr (OUT != OUT_I32) as = out.row_scale[m];
        O o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = nb + i < N ? nb + i : N - 1;
            float bs = 1.0f, bf = 0.0f;
            if constexpr (OUT != OUT_I32) {
                bs = out.col_scale[n];
                if (has_bias) bf = load_bias<OUT>(out.bias, n);
            }
            o[i] = epi_convert<OUT>(sum[i], as, bs, bf, has_bias, false);
        }
        O* dst = y + (int64_t)m * out.ldy + nb;
        const bool vec = (nb + 3 < N) && ((reinterpret_cast<uintptr_t>(dst) & (4 * sizeof(O) - 1)) == 0);
        if (vec) {
            if constexpr (sizeof(O) == 2) *reinterpret_cast<v2u*>(dst) = *reinterpret_cast<const v2u*>(o);
            else *reinterpret_cast<v4u*>(dst) = *reinterpret_cast<const v4u*>(o);
        } else {                                          // odd N, odd ldy, an unaligned y: element by element
#pragma unroll
            for (int i = 0; i < 4; ++i) if (nb + i < N) dst[i] = o[i];
        }
    }
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
