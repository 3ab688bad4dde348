// gemm_w4_stream_body.h — the ONE weight-streaming body of the int4 decode kernels: gemm_w4_stream (gemm_w4_stream.hip: one dense packed matrix, M <= 64 tokens) and
// gemm_w4_grouped_stream (gemm_w4_grouped_stream.hip: one expert of a mixture-of-experts layer per workgroup, M_total <= 64 grouped rows) are two hosts of it, as
// gemm_stream_body.h has two int8 hosts.  y = dequant(x . W8^T) with W8[n][k] = q[n][k] * g[n][k / 128] (QSPEC W1-W4), bit for bit the int8 body on the expanded weight.
// Work split: a workgroup = KS waves over one block of 16 weight rows, the waves split the Kp / 128 GROUPS in balanced slices, reduce their exact int32 partial tiles
// through LDS, and wave t finishes token tile t with QSPEC E1-E4 (epi_convert).
// Weight movement: lane (r = lane & 15, c = lane >> 4) loads the 16 packed bytes 64 j + 16 c .. + 15 of row n0 + r — ONE load holds its A fragments of the two k-steps of
// group j: the low nibbles are k = 128 j + 16 c .. + 15 (step 2 j), the high nibbles k = 128 j + 64 + 16 c .. (step 2 j + 1).  No LDS; two batches of loads in flight.
// Unpack: hi = v & 0xF0F0F0F0 and lo = (v << 4) & 0xF0F0F0F0 are the signed bytes 16 q — three VALU operations per packed dword, none for the sign.
// Multipliers: the two MFMAs of a group go into a zeroed group accumulator (|16 sum| <= 128 * 128 * 112 < 2^23), then total += (acc >> 4) * g for the lane's four rows
// n0 + 4 c .. + 3, whose multipliers are one dword of gs.  The shift is exact, the product fits 24 bits (v_mad_i32_i24).  `total` is the int32 sum of the int8 GEMM on W8.
// Activations: the same int8 codes; STAGE: row-contiguous loads into a wave-private padded LDS region and ds_read_b128 fragments (the int8 body's scheme), otherwise —
// one row, whose 16 "rows" are one address — direct loads.  Nibble 0x8 (reserved, never packed) unpacks to q = -8: a different sum, no address depends on it.
// What differs between the hosts comes in by value, as in the int8 body: Rows (src_row(i): where the codes of activation row i lie, already clamped) and StreamOut
// (scales, bias, y, the first row `lo` of y / the row scales and the row count); W4 and GS are the base of THIS matrix (the grouped host: of its expert).
#pragma once
#include "gemm_stream_body.h"
#include "pq_plan.h"

namespace pq {

// bytes of one wave's staging region: nt * 16 rows of a batch (w4_stream_batch groups x 128 bytes of K), row stride padded by 16 B
constexpr int w4_stage_bytes(int nt) { return nt * 16 * (w4_stream_batch(nt) * 128 + 16); }

// NT: 16-row tiles of activations; `smem`: KS wave-private staging regions (STAGE), reused as [KS][NT][64 lanes] v4i for the reduction; n0: first weight row; G: groups
template <int OUT, int NT, bool STAGE, typename Rows, typename Out>
__device__ __forceinline__ void w4_stream_body(uint8_t* smem, Rows rows, const uint8_t* __restrict__ W4, int64_t ldw4, const uint32_t* __restrict__ GS, Out out, int n0,
                                               int N, int G) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), KS = blockDim.x >> 6;
    const int r = lane & 15, c = lane >> 4;
    constexpr int U = w4_stream_batch(NT);

    // this wave's groups: a balanced slice of the G groups (empty when there are more waves than groups)
    const int j0 = (int)((int64_t)G * w / KS), j1 = (int)((int64_t)G * (w + 1) / KS);
    const int nrow = n0 + r < N ? n0 + r : N - 1;                                  // clamp: rows past the edge re-read a valid row
    const uint8_t* wp = W4 + (int64_t)nrow * ldw4 + c * 16;
    const int quads = (N + 3) >> 2, quad = (n0 >> 2) + c < quads ? (n0 >> 2) + c : quads - 1;      // gs holds ceil(N / 4) row quads
    const uint32_t* gp = GS + (int64_t)quad * G;
    const int8_t* xp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) xp[t] = rows.src_row(t * 16 + r) + c * 16;
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
    uint8_t* const stg = smem + (size_t)w * w4_stage_bytes(NT);
    const int lrow = lane / UPR, lunit = lane % UPR;
    const int8_t* xrow[STAGE ? NLD : 1];
    if constexpr (STAGE) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) xrow[i] = rows.src_row(i * RPI + lrow) + lunit * 16;
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

    // ---- exact reduction of the KS partial tiles through LDS, then E1-E4.  D[row <-> n][col <-> m]: the lane holds n = n0 + 4 c .. + 3 of this body's row 16 t + r.
    v4i* red = reinterpret_cast<v4i*>(smem);
    if (KS > 1) {
        if constexpr (STAGE) __syncthreads();            // the reduction buffer overlays the staging regions of ALL waves (every wave of the workgroup runs this body)
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
        const int m = out.lo + t * 16 + r, nb = n0 + c * 4;                // m: the row of y and of the row scales
        if (m >= out.lo + out.rows || nb >= N) continue;
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

}  // namespace pq
