// gemm_stream_body.h — the ONE weight-streaming GEMM body of the decode kernels: gemm_s8_skinny (gemm_s8_skinny.hip: one dense matrix, M <= 64 tokens) and
// gemm_s8_grouped_stream (gemm_s8_grouped_stream.hip: one expert of a mixture-of-experts layer per workgroup, M_total <= 64 grouped rows) are two hosts of it.
// A workgroup = KS waves that split K between them for one block of 16 RB weight rows.  Every wave streams its weight rows STRAIGHT INTO MFMA FRAGMENTS: lane
// (r = lane & 15, c = lane >> 4) loads the 16 bytes k0 + 16c .. +15 of row n0 + r — exactly the A operand of v_mfma_i32_16x16x64_i8 — so the weights never touch LDS.
// The waves reduce their exact int32 partial tiles through LDS and apply QSPEC E1-E4: bit-identical to every other variant, whatever the plan.
// What differs between the hosts comes in as two small objects passed by value:
//   Rows  src_row(i): where the codes of activation row i lie, already clamped (rows past the last one: the last one again — their products land in accumulator
//         columns nobody stores);
//   Out   StreamOut<Flags>: row scales, column scales, bias, y, ldy, the EPI_* flags, the first row `lo` of y / the row scales and the row count.  The grouped host
//         passes NoEpiFlags — a constant 0, so the EPI_STORE_T / EPI_BIAS_ROWS / EPI_COL_FIRST branches fold away in its instantiations — the dense host lo = 0.
// Neither kernel counts vmcnt and the only inline asm is s_waitcnt lgkmcnt(0): a register allocation that moves changes time, never results.
#pragma once
#include "gemm_epilogue.h"

namespace pq {

// k-steps (64 bytes of K each) per batch, sized so that 16 waves per workgroup stay within 128 VGPRs.  One weight block per wave (RB = 1): TWO batches of weights are in
// registers — the next one is requested before the current one is multiplied, so a wave always has weight bytes in flight (HBM-fed: 1 x 4096 x 4096 7.1 -> 6.7 us,
// 16 x 4096 x 14336 20.5 -> 18.7).  Two blocks per wave (RB = 2): one batch at a time, as in rounds 1-3 — the pipelined form was 7 % SLOWER there (1 x 28672 x 4096).
constexpr int stream_batch(int nt, int rb) { return rb == 1 ? (nt == 1 ? 4 : 2) : (nt * rb == 2 ? 4 : 2); }
// bytes of one wave's staging region for nt token tiles (row stride padded by 16 B: conflict-free both ways)
constexpr int stream_stage_bytes(int nt, int rb) { return nt * 16 * (stream_batch(nt, rb) * 64 + 16); }
// dynamic LDS of a launch: the larger of the reduction buffer and the staging regions of the largest body among 1 .. nt_max token tiles
inline size_t stream_lds_bytes(int ks, int nt_max, int rb, bool stage) {
    size_t lds = ks > 1 ? (size_t)ks * nt_max * rb * 64 * sizeof(v4i) : 0;
    for (int nt = 1; stage && nt <= nt_max; ++nt) {
        const size_t b = (size_t)ks * stream_stage_bytes(nt, rb);
        lds = b > lds ? b : lds;
    }
    return lds;
}
// (the staging regions of 16 waves need up to 147 KiB of dynamic LDS: above the 64-KiB default the limit is raised — per launch, a host-side attribute of the function on
// the CURRENT device, so a process that drives several devices gets it on each)
template <typename... P, typename... A>
void stream_launch(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A... args) {
    if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    kern<<<grid, block, lds, st>>>(args...);
}

struct NoEpiFlags { __device__ constexpr operator int32_t() const { return 0; } };
template <typename Flags>
struct StreamOut {
    const float *row_scale, *col_scale;     // [lo + i], [n]   (unused for OUT_I32)
    const void* bias;                       // in the output dtype, nullable
    void* y;
    int64_t ldy;
    Flags flags;
    int lo, rows;                           // rows lo .. lo + rows - 1 of y and row_scale are this body's rows 0 .. rows - 1 (rows <= 16 NT)
};

// RB: 16-row weight blocks per wave.  The direct-to-fragment access pattern (16 segments of 64 B per instruction) tops out
// near 9.8 TB/s over the whole chip (tools/ubench/l2_ingest), and the activation fragments travel the same path from L2:
// with RB = 1 and one token tile they take half of it.  RB = 2 reuses every activation fragment for two weight blocks.
// STAGE (round 4): the activation fragments no longer come straight from L2 in the MFMA operand layout (16 rows x 64 B per load instruction — the same 16-segment request the
// weight fragments need, on the same vector-memory pipeline: with one weight block per wave HALF of that pipeline's requests were activation re-reads, and 16 tokens ran 15 - 40 %
// slower than 1 token, whose 16 "rows" are one clamped row).  A wave now loads its K-batch of the token rows with row-contiguous requests (2 - 4 rows x 256 - 512 B per
// instruction), parks them in a wave-private LDS region (row stride padded by 16 B: conflict-free both ways) and reads the fragments back with ds_read_b128.  Same values, same
// MFMAs: bit-identical.
// NT: 16-row tiles of activations; `smem`: KS wave-private staging regions (STAGE), reused as [KS][RB * NT][64 lanes] v4i for the reduction; n0: first weight row.
// ILV: the form of the unstaged RB = 2 walk — true: the dense kernel's, requests interleaved k-step by k-step (the form measured in rounds 1-3); false: all weight
// requests of a batch, then the activation requests, as the grouped kernel has always had it for an expert with one row.  One form for both was tried (round 29): with
// the interleaved one the grouped one-row RB = 2 path (PQ_GROUPED_STREAM_RB=2, one token) ran 2.2 % slower on 2 x 28672 x 4096 — 58.8 against 57.5 us, the parent's own
// spread 0.5 % (profiles/r29_stream_body_ab.txt) — so each host keeps its order.  Same integer sums either way.
template <int OUT, int NT, int RB, bool STAGE, bool ILV, typename Rows, typename Out>
__device__ __forceinline__ void stream_body(uint8_t* smem, Rows rows, const int8_t* __restrict__ W, int64_t ldw, Out out, int n0, int N, int K) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), KS = blockDim.x >> 6;
    const int r = lane & 15, c = lane >> 4;
    constexpr int SK_U = stream_batch(NT, RB);

    // this wave's k-steps: a balanced slice of the K / 64 steps (empty when there are more waves than steps)
    const int steps = K >> 6, s0 = (int)((int64_t)steps * w / KS), s1 = (int)((int64_t)steps * (w + 1) / KS);
    const int8_t* wp[RB];
#pragma unroll
    for (int b = 0; b < RB; ++b) {
        const int nrow = n0 + b * 16 + r < N ? n0 + b * 16 + r : N - 1;    // clamp: rows past the edge re-read a valid row
        wp[b] = W + (int64_t)nrow * ldw + c * 16;
    }
    const int8_t* xp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) xp[t] = rows.src_row(t * 16 + r) + c * 16;
    v4i acc[RB][NT];
#pragma unroll
    for (int b = 0; b < RB; ++b)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[b][t] = v4i{0, 0, 0, 0};

    // STAGE: row-contiguous activation loads.  A batch is SK_U k-steps = UPR = 4 SK_U 16-byte units per row; a load instruction covers 64 / UPR rows.
    constexpr int UPR = 4 * SK_U, RPI = 64 / UPR, NLD = NT * 16 / RPI;          // units per row, rows per instruction, instructions per batch
    constexpr int RSTR = SK_U * 64 + 16;                                        // staged row stride (bytes)
    uint8_t* const stg = smem + (size_t)w * stream_stage_bytes(NT, RB);
    const int lrow = lane / UPR, lunit = lane % UPR;
    const int8_t* xrow[STAGE ? NLD : 1];
    if constexpr (STAGE) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) xrow[i] = rows.src_row(i * RPI + lrow) + lunit * 16;
    }
    // one batch: SK_U k-steps.  RB = 1: the weight fragments of batch s + SK_U are requested BEFORE the MFMAs of batch s (two register sets).
    auto load_w = [&](v4i (&fw)[SK_U][RB], int sb) {
#pragma unroll
        for (int u = 0; u < SK_U; ++u)
#pragma unroll
            for (int b = 0; b < RB; ++b) fw[u][b] = *reinterpret_cast<const v4i*>(wp[b] + (int64_t)(sb + u) * 64);
    };
    auto compute = [&](const v4i (&fw)[SK_U][RB], int sb) {
        v4i fx[SK_U][NT];
        if constexpr (!STAGE) {
#pragma unroll
            for (int u = 0; u < SK_U; ++u)
#pragma unroll
                for (int t = 0; t < NT; ++t) fx[u][t] = *reinterpret_cast<const v4i*>(xp[t] + (int64_t)(sb + u) * 64);
        } else {
            v4i xr[NLD];
#pragma unroll
            for (int i = 0; i < NLD; ++i) xr[i] = *reinterpret_cast<const v4i*>(xrow[i] + (int64_t)sb * 64);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                  // the previous batch's fragment reads have returned: its region may be overwritten
#pragma unroll
            for (int i = 0; i < NLD; ++i) *reinterpret_cast<v4i*>(stg + (i * RPI + lrow) * RSTR + lunit * 16) = xr[i];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                  // wave-private region, LDS operations of one wave execute in order: written -> readable
#pragma unroll
            for (int u = 0; u < SK_U; ++u)
#pragma unroll
                for (int t = 0; t < NT; ++t) fx[u][t] = *reinterpret_cast<const v4i*>(stg + (t * 16 + r) * RSTR + (u * 4 + c) * 16);
        }
#pragma unroll
        for (int u = 0; u < SK_U; ++u)
#pragma unroll
            for (int b = 0; b < RB; ++b)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[b][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fw[u][b], fx[u][t], acc[b][t], 0, 0, 0);
    };
    int s = s0;
    if constexpr (RB != 1) {            // (rounds 1-3's loop, weight and activation requests interleaved k-step by k-step when the activations come straight from L2)
        for (; s + SK_U <= s1; s += SK_U) {
            v4i fw[SK_U][RB];
            if constexpr (STAGE || !ILV) {
                load_w(fw, s);
                compute(fw, s);
            } else {
                v4i fx[SK_U][NT];
#pragma unroll
                for (int u = 0; u < SK_U; ++u) {
#pragma unroll
                    for (int b = 0; b < RB; ++b) fw[u][b] = *reinterpret_cast<const v4i*>(wp[b] + (int64_t)(s + u) * 64);
#pragma unroll
                    for (int t = 0; t < NT; ++t) fx[u][t] = *reinterpret_cast<const v4i*>(xp[t] + (int64_t)(s + u) * 64);
                }
#pragma unroll
                for (int u = 0; u < SK_U; ++u)
#pragma unroll
                    for (int b = 0; b < RB; ++b)
#pragma unroll
                        for (int t = 0; t < NT; ++t) acc[b][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fw[u][b], fx[u][t], acc[b][t], 0, 0, 0);
            }
        }
    } else if (s + SK_U <= s1) {
        v4i fw0[SK_U][RB], fw1[SK_U][RB];
        load_w(fw0, s);
        for (;;) {
            const bool more1 = s + 2 * SK_U <= s1;
            if (more1) load_w(fw1, s + SK_U);
            compute(fw0, s); s += SK_U;
            if (!more1) break;
            const bool more2 = s + 2 * SK_U <= s1;
            if (more2) load_w(fw0, s + SK_U);
            compute(fw1, s); s += SK_U;
            if (!more2) break;
        }
    }
    for (; s < s1; ++s) {               // the k-steps that do not fill a batch
        v4i fx[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) fx[t] = *reinterpret_cast<const v4i*>(xp[t] + (int64_t)s * 64);
#pragma unroll
        for (int b = 0; b < RB; ++b) {
            const v4i fw = *reinterpret_cast<const v4i*>(wp[b] + (int64_t)s * 64);
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[b][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fw, fx[t], acc[b][t], 0, 0, 0);
        }
    }

    // ---- exact reduction of the KS partial tiles through LDS, then E1-E4.  D[row <-> n][col <-> m]: the lane holds n = n0 + 16 b + 4 c .. + 3 of this body's row 16 t + r.
    v4i* red = reinterpret_cast<v4i*>(smem);
    constexpr int NTL = RB * NT;                          // output tiles of this workgroup: tile q = b * NT + t
    if (KS > 1) {
        if constexpr (STAGE) __syncthreads();            // the reduction buffer overlays the staging regions of ALL waves (every wave of the workgroup runs this body)
#pragma unroll
        for (int b = 0; b < RB; ++b)
#pragma unroll
            for (int t = 0; t < NT; ++t) red[(w * NTL + b * NT + t) * 64 + lane] = acc[b][t];
        __syncthreads();
    }
    using O = typename OutElem<OUT>::type;
    O* y = reinterpret_cast<O*>(out.y);
    const int32_t flags = out.flags;
    const bool has_bias = (OUT != OUT_I32) && out.bias != nullptr;
    for (int q = w; q < NTL; q += KS) {                   // wave w finishes tiles w, w + KS, ...
        const int b = q / NT, t = q - b * NT;
        v4i sum = acc[0][0];
        if (KS > 1) {
            sum = v4i{0, 0, 0, 0};
            for (int k = 0; k < KS; ++k) sum += red[(k * NTL + q) * 64 + lane];
        } else {
#pragma unroll
            for (int bb = 0; bb < RB; ++bb)
#pragma unroll
                for (int tt = 0; tt < NT; ++tt) if (bb * NT + tt == q) sum = acc[bb][tt];
        }
        const int m = out.lo + t * 16 + r, nb = n0 + b * 16 + c * 4;       // m: the row of y and of the row scales
        if (m >= out.lo + out.rows || nb >= N) continue;
        float as = 1.0f;
        if constexpr (OUT != OUT_I32) as = out.row_scale[m];
        O o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = nb + j < N ? nb + j : N - 1;
            float bs = 1.0f, bf = 0.0f;
            if constexpr (OUT != OUT_I32) {
                bs = out.col_scale[n];
                if (has_bias) bf = load_bias<OUT>(out.bias, (flags & EPI_BIAS_ROWS) ? m : n);
            }
            o[j] = epi_convert<OUT>(sum[j], as, bs, bf, has_bias, flags & EPI_COL_FIRST);
        }
        if (flags & EPI_STORE_T) {                        // y^T[n][m]: four rows of the transposed output, one element each (the whole output is M x N <= 64 x N elements)
#pragma unroll
            for (int j = 0; j < 4; ++j) if (nb + j < N) y[(int64_t)(nb + j) * out.ldy + m] = o[j];
            continue;
        }
        O* dst = y + (int64_t)m * out.ldy + nb;
        const bool vec = (nb + 3 < N) && ((reinterpret_cast<uintptr_t>(dst) & (4 * sizeof(O) - 1)) == 0);
        if (vec) {
            if constexpr (sizeof(O) == 2) *reinterpret_cast<v2u*>(dst) = *reinterpret_cast<const v2u*>(o);
            else *reinterpret_cast<v4u*>(dst) = *reinterpret_cast<const v4u*>(o);
        } else {                                          // odd N, odd ldy, an unaligned y: element by element
#pragma unroll
            for (int j = 0; j < 4; ++j) if (nb + j < N) dst[j] = o[j];
        }
    }
}

}  // namespace pq
