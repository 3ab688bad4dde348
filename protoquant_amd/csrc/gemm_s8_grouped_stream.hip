// gemm_s8_grouped_stream.hip — K3/K4 for a MIXTURE OF EXPERTS AT DECODE (M_total <= 64 grouped rows): the contract of gemm_s8_grouped.hip — rows sorted by expert,
// `offsets` and the optional row index in device memory and never read on the host, y[r, :] = dequant(xq[src(r), :] . wq[e(r)]^T) — with the body of the weight-streaming
// kernel (gemm_s8_skinny.hip) instead of a 64-row ring tile.  With one or two rows per expert the GEMM is a streaming read of the LIVE experts' weights, N * K bytes
// each: a 64-row tile stages 64 activation rows to use one and leaves most of the chip without a workgroup (Mixtral's down projection at one token: 64 workgroups).
//
//   * grid = ceil(N / (16 RB)) weight blocks (x) times S = min(E, M_total) expert SLOTS (y): no more than M_total experts can own a row, so the grid is known to the host
//     whatever the routing.  Slot j serves the j-th expert whose clamped row range is not empty (stream_find_slot: one lane per expert, 64 experts per step, the wave's
//     prefix sum of the "has a row" flags is a ballot and a population count).  A slot without an expert returns before it touches a weight or an activation.  No
//     workspace, no atomics, no wait on another workgroup: a captured hipGraph stays valid when the CONTENTS of offsets / row index / xs change.
//   * a workgroup = KS waves that split K for ONE 16 RB-row block of ONE expert's weight.  Every wave streams its weight rows straight into the A operand of
//     v_mfma_i32_16x16x64_i8 (lane (r, c) loads bytes k0 + 16 c .. + 15 of row n0 + r), the next batch requested before the current one is multiplied (RB = 1); the
//     expert's token rows come row-contiguously into a wave-private LDS region (STAGE, as in the dense kernel) or, when the expert has ONE row, straight from L2 (its 16
//     "rows" are one address).  Exact int32 reduction of the KS partial tiles through LDS, then QSPEC E1-E4 (epi_convert) with xs[r], ws[e][n], bias[e][n]: every row
//     has the bits pq_qlinear_s8 gives per expert.
//   * token tiles: an expert's row count (1 .. 64) is device data.  The kernel is compiled for MT = 1, 2 or 4 token tiles, chosen by the host from M_total (an expert
//     cannot own more rows than exist), and holds one specialised body per tile count 1 .. MT; a workgroup branches — wave-uniformly, the same way in all its waves — to
//     the body of ITS expert's ceil(rows / 16).  So the weights of a live expert are read once whatever its row count, and an expert with one row of a 64-row step does
//     one tile's MFMAs and activation loads, not four.  Cost: the kernel's register allocation is that of its largest body — 72 VGPRs for MT = 1 and 2 (78 / 82 with
//     RB = 2), 98 for MT = 4, where a one-tile body alone needs 72; every instantiation is launched with up to 16 waves per workgroup, which allows 128, so no
//     occupancy is lost — and MT = 4 carries five bodies of code.  Three or four tiles with two weight
//     blocks per wave would not fit 128 VGPRs (as in the dense kernel): RB = 2 exists for MT <= 2 only.
//   * the row gather is a run-time branch in the prologue (the source row of grouped row r is qrow[r] clamped into [0, x_rows)): it only changes the row pointers.
// Untrusted device data: offsets are clamped into [0, M_total] (hi) and [0, hi] (lo), the row index into [0, x_rows) — wrong contents give wrong results, never an access
// outside the operands; rows >= offsets[E] of y are not written.
// The non-temporal hint on the weight loads is NOT used: it loses when one launch is replayed on cached data, and no A/B of it has been run here.
#include <cstdio>
#include <cstdlib>

#include "gemm_epilogue.h"
#include "pq_launch.h"

namespace pq {

// k-steps (64 bytes of K each) per batch: the dense kernel's table (gemm_s8_skinny.hip: sk_batch), per body — sized so that 16 waves per workgroup stay within 128 VGPRs
constexpr int gs_batch(int nt, int rb) { return rb == 1 ? (nt == 1 ? 4 : 2) : (nt * rb == 2 ? 4 : 2); }
// bytes of one wave's staging region for nt token tiles (row stride padded by 16 B: conflict-free both ways)
constexpr int gs_stage_bytes(int nt, int rb) { return nt * 16 * (gs_batch(nt, rb) * 64 + 16); }

// The expert of slot j: the j-th expert (in expert order) with a non-empty clamped row range.  Every lane of every wave computes the same answer; the caller makes it
// scalar.  Four steps of 64 experts are loaded at a time, so that the offsets of up to 256 experts are one round trip to memory and not four.
struct StreamSlot { int e, lo, hi; };
__device__ __forceinline__ bool stream_find_slot(const int32_t* __restrict__ offsets, int E, int M_total, int j, StreamSlot& g) {
    const int lane = threadIdx.x & 63;
    int run = 0;                                               // live experts before this step
    for (int b0 = 0; b0 < E; b0 += 256) {
        int lo[4], hi[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = b0 + i * 64 + lane;
            lo[i] = 0; hi[i] = 0;
            if (e < E) {
                hi[i] = offsets[e + 1];
                lo[i] = offsets[e];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int h = hi[i] < 0 ? 0 : (hi[i] > M_total ? M_total : hi[i]);
            const int l = lo[i] < 0 ? 0 : (lo[i] > h ? h : lo[i]);
            const bool live = h > l;
            const unsigned long long mask = __ballot(live);
            const int cnt = __popcll(mask);
            if (run + cnt > j) {                               // (wave-uniform)
                const int rank = __popcll(mask & ((1ull << lane) - 1ull));     // exclusive prefix sum of the flags
                const unsigned long long hit = __ballot(live && rank == j - run);
                const int src = __ffsll((long long)hit) - 1;
                g.e = b0 + i * 64 + src;
                g.lo = __shfl(l, src, 64);
                g.hi = __shfl(h, src, 64);
                return true;
            }
            run += cnt;
        }
    }
    return false;
}

// One workgroup's work for one expert with NT token tiles: the body of gemm_s8_skinny with the expert's operands.  W: the expert's weight; ws / bias: the expert's
// column scales / bias (bias nullable); rows [lo, hi) of the grouped order; `smem`: KS wave-private staging regions, reused for the reduction.
template <int OUT, int NT, int RB, bool STAGE>
__device__ __forceinline__ void stream_body(uint8_t* smem, const int8_t* __restrict__ X, int64_t ldx, const int32_t* __restrict__ qrow, int x_rows,
                                            const int8_t* __restrict__ W, int64_t ldw, const float* __restrict__ xs, const float* __restrict__ ws, const void* bias,
                                            void* yv, int64_t ldy, int lo, int hi, int n0, int N, int K) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), KS = blockDim.x >> 6;
    const int r = lane & 15, c = lane >> 4;
    const int M = hi - lo;                                      // this expert's rows: 1 .. 16 NT
    constexpr int SK_U = gs_batch(NT, RB);

    // this wave's k-steps: a balanced slice of the K / 64 steps (empty when there are more waves than steps)
    const int steps = K >> 6, s0 = (int)((int64_t)steps * w / KS), s1 = (int)((int64_t)steps * (w + 1) / KS);
    const int8_t* wp[RB];
#pragma unroll
    for (int b = 0; b < RB; ++b) {
        const int nrow = n0 + b * 16 + r < N ? n0 + b * 16 + r : N - 1;    // clamp: rows past the edge re-read a valid row
        wp[b] = W + (int64_t)nrow * ldw + c * 16;
    }
    // row i of the expert (rows past its last one: its last one again — their products land in accumulator columns nobody stores) -> where its codes lie
    auto src_row = [&](int i) -> const int8_t* {
        const int gr = lo + (i < M ? i : M - 1);
        int64_t row = gr;
        if (qrow != nullptr) {                                  // (the index is device data nobody has checked)
            const uint32_t s = (uint32_t)qrow[gr];
            row = s < (uint32_t)x_rows ? s : (uint32_t)x_rows - 1u;
        }
        return X + row * ldx;
    };
    const int8_t* xp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) xp[t] = src_row(t * 16 + r) + c * 16;
    v4i acc[RB][NT];
#pragma unroll
    for (int b = 0; b < RB; ++b)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[b][t] = v4i{0, 0, 0, 0};

    // STAGE: row-contiguous activation loads.  A batch is SK_U k-steps = UPR = 4 SK_U 16-byte units per row; a load instruction covers 64 / UPR rows.
    constexpr int UPR = 4 * SK_U, RPI = 64 / UPR, NLD = NT * 16 / RPI;
    constexpr int RSTR = SK_U * 64 + 16;
    uint8_t* const stg = smem + (size_t)w * gs_stage_bytes(NT, RB);
    const int lrow = lane / UPR, lunit = lane % UPR;
    const int8_t* xrow[STAGE ? NLD : 1];
    if constexpr (STAGE) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) xrow[i] = src_row(i * RPI + lrow) + lunit * 16;
    }
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
    if constexpr (RB != 1) {            // two weight blocks per wave: one batch at a time (the pipelined form was slower in the dense kernel)
        for (; s + SK_U <= s1; s += SK_U) {
            v4i fw[SK_U][RB];
            load_w(fw, s);
            compute(fw, s);
        }
    } else if (s + SK_U <= s1) {        // one block: the weight fragments of batch s + SK_U are requested BEFORE the MFMAs of batch s (two register sets)
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

    // ---- exact reduction of the KS partial tiles through LDS, then E1-E4.  D[row <-> n][col <-> m]: the lane holds n = n0 + 16 b + 4 c .. + 3 of the expert's row 16 t + r.
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
    O* y = reinterpret_cast<O*>(yv);
    const bool has_bias = (OUT != OUT_I32) && bias != nullptr;
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
        const int m = lo + t * 16 + r, nb = n0 + b * 16 + c * 4;           // m: the row of the grouped order (xs and y)
        if (m >= hi || nb >= N) continue;
        float as = 1.0f;
        if constexpr (OUT != OUT_I32) as = xs[m];
        O o[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int n = nb + jj < N ? nb + jj : N - 1;
            float bs = 1.0f, bf = 0.0f;
            if constexpr (OUT != OUT_I32) {
                bs = ws[n];
                if (has_bias) bf = load_bias<OUT>(bias, n);
            }
            o[jj] = epi_convert<OUT>(sum[jj], as, bs, bf, has_bias, false);
        }
        O* dst = y + (int64_t)m * ldy + nb;
        const bool vec = (nb + 3 < N) && ((reinterpret_cast<uintptr_t>(dst) & (4 * sizeof(O) - 1)) == 0);
        if (vec) {
            if constexpr (sizeof(O) == 2) *reinterpret_cast<v2u*>(dst) = *reinterpret_cast<const v2u*>(o);
            else *reinterpret_cast<v4u*>(dst) = *reinterpret_cast<const v4u*>(o);
        } else {                                          // odd N, odd ldy, an unaligned y: element by element
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) if (nb + jj < N) dst[jj] = o[jj];
        }
    }
}

// blockIdx.x: the 16 RB-row weight block, blockIdx.y: the expert slot.  M_total <= 16 MT (the launcher's choice), so an expert has at most MT token tiles.
template <int OUT, int MT, int RB>
__global__ __launch_bounds__(1024) void gemm_s8_grouped_stream(const int8_t* __restrict__ X, int64_t ldx, const int32_t* __restrict__ qrow, int x_rows,
                                                               const int8_t* __restrict__ W, int64_t ldw, int64_t w_stride, EpiArgs epi,
                                                               const int32_t* __restrict__ offsets, int E, int M_total, int N, int K) {
    extern __shared__ __attribute__((aligned(16))) uint8_t gs_smem[];
    StreamSlot g;
    if (!stream_find_slot(offsets, E, M_total, (int)blockIdx.y, g)) return;        // (wave-uniform, and the same in every wave: nobody is left at a barrier)
    const int e = __builtin_amdgcn_readfirstlane(g.e), lo = __builtin_amdgcn_readfirstlane(g.lo);
    int hi = __builtin_amdgcn_readfirstlane(g.hi);
    if (hi - lo > 16 * MT) hi = lo + 16 * MT;                  // (cannot happen: hi - lo <= M_total <= 16 MT; it bounds the bodies' LDS use by construction)
    using O = typename OutElem<OUT>::type;
    const float* ws = nullptr;
    const void* bias = nullptr;
    if constexpr (OUT != OUT_I32) {
        ws = epi.b_scale + (int64_t)e * N;
        if (epi.bias != nullptr) bias = reinterpret_cast<const O*>(epi.bias) + (int64_t)e * N;
    }
    const int8_t* We = W + (int64_t)e * w_stride;
    const int n0 = (int)blockIdx.x * (16 * RB), rows = hi - lo;
#define PQ_GS_BODY(NT_, STAGE_) stream_body<OUT, NT_, RB, STAGE_>(gs_smem, X, ldx, qrow, x_rows, We, ldw, epi.a_scale, ws, bias, epi.y, epi.ldy, lo, hi, n0, N, K)
    if constexpr (MT >= 4) {
        if (rows > 48) { PQ_GS_BODY(4, true); return; }
        if (rows > 32) { PQ_GS_BODY(3, true); return; }
    }
    if constexpr (MT >= 2) {
        if (rows > 16) { PQ_GS_BODY(2, true); return; }
    }
    if (rows > 1) PQ_GS_BODY(1, true);
    else PQ_GS_BODY(1, false);
#undef PQ_GS_BODY
}

// (MT, RB, KS) of a launch.  MT follows M_total (1, 2 or 4 token tiles).  RB and KS: skinny_plan's rules (gemm_s8_skinny.hip) with the AVERAGE rows of a slot in place of
// M and blocks x slots in place of the blocks of one matrix.  Those constants — ~4096 / 2048 / 768 waves per launch, the N thresholds — were swept for ONE dense N x K
// matrix (profiles/r04_skinny_sweep.txt); for a grid whose slots may be empty and whose live experts lie E * N * K bytes apart they are UNMEASURED.
// PQ_GROUPED_STREAM_RB / PQ_GROUPED_STREAM_KS force either (time only, never bits: tests/test_gpu_grouped_stream.py).
void grouped_stream_plan(int32_t E, int64_t M_total, int64_t N, int64_t K, int* mt_out, int* rb_out, int* ks_out) {
    const int mt = M_total <= 16 ? 1 : (M_total <= 32 ? 2 : 4);
    const int64_t slots = M_total < E ? (M_total < 1 ? 1 : M_total) : E;
    const int64_t avg = M_total < 1 ? 1 : (M_total + slots - 1) / slots;
    int rb = 1, min_ks = 1;
    int64_t target = 4096;
    if (avg == 1) min_ks = 4;
    else if (avg <= 32) {
        if (N <= 4096) target = 2048, min_ks = 2;
        else if (N < 16384) rb = 2, target = 768, min_ks = 2;
        else target = 1, min_ks = avg <= 8 ? 4 : 2;
    }
    if (const int f = opt().grouped_stream_rb; f) rb = f;
    if (mt > 2) rb = 1;                                    // (no two-block body for three or four token tiles)
    const int amt = (int)((avg + 15) / 16);
    const int64_t blocks = (N + 16 * rb - 1) / (16 * rb) * slots, steps = K / 64;
    int ks = 1;
    while (ks < 16 && (blocks * ks < target || ks < min_ks) && steps / (ks * 2) >= gs_batch(amt, rb)) ks <<= 1;
    if (const int f = opt().grouped_stream_ks; f > 0) {    // a forced power of two (<= 16), whatever K: waves without a k-step add zeros
        ks = 1;
        while (ks < f && ks < 16) ks <<= 1;
    }
    *mt_out = mt; *rb_out = rb; *ks_out = ks;
}

// static name of a plan: "gstream_mt<MT>_rb<RB>_ks<KS>_16x16x64"
const char* grouped_stream_plan_name(int mt, int rb, int ks) {
    static const struct Names {
        char s[3][2][5][40];
        Names() {
            const int mts[3] = {1, 2, 4};
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 2; ++b)
                    for (int k = 0; k < 5; ++k) snprintf(s[a][b][k], sizeof(s[a][b][k]), "gstream_mt%d_rb%d_ks%d_16x16x64", mts[a], b + 1, 1 << k);
        }
    } names;
    int k = 0;
    while ((1 << k) < ks && k < 4) ++k;
    return names.s[mt == 1 ? 0 : (mt == 2 ? 1 : 2)][rb == 2 ? 1 : 0][k];
}

template <int OUT>
void launch_gemm_grouped_stream(const int8_t* X, int64_t ldx, const int32_t* qrow, int64_t x_rows, const int8_t* W, int64_t ldw, int64_t w_stride, const EpiArgs& epi,
                                const int32_t* offsets, int E, int64_t M_total, int64_t N, int64_t K, hipStream_t st) {
    int mt = 1, rb = 1, ks = 1;
    grouped_stream_plan(E, M_total, N, K, &mt, &rb, &ks);
    const int64_t slots = M_total < E ? M_total : E;
    const dim3 grid((unsigned)((N + 16 * rb - 1) / (16 * rb)), (unsigned)slots), block((unsigned)(ks * 64));
    // dynamic LDS: the larger of the staging regions (largest body) and the reduction buffer; above the 64-KiB default the limit is raised (per launch, a host-side
    // attribute of the function on the CURRENT device)
    const size_t lds_red = ks > 1 ? (size_t)ks * mt * rb * 64 * sizeof(v4i) : 0;
    size_t lds_stg = 0;
    for (int nt = 1; nt <= mt; ++nt) {
        const size_t b = (size_t)ks * nt * 16 * (gs_batch(nt, rb) * 64 + 16);
        lds_stg = b > lds_stg ? b : lds_stg;
    }
    const size_t lds = lds_red > lds_stg ? lds_red : lds_stg;
    const int xr = (int)x_rows;
#define PQ_GS(MTv, RBv) do { if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_s8_grouped_stream<OUT, MTv, RBv>), \
                                                                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); \
                             gemm_s8_grouped_stream<OUT, MTv, RBv><<<grid, block, lds, st>>>(X, ldx, qrow, xr, W, ldw, w_stride, epi, offsets, E, (int)M_total, (int)N, (int)K); } while (0)
    if (mt == 1) { if (rb == 2) PQ_GS(1, 2); else PQ_GS(1, 1); }
    else if (mt == 2) { if (rb == 2) PQ_GS(2, 2); else PQ_GS(2, 1); }
    else PQ_GS(4, 1);
#undef PQ_GS
}
#define PQ_GS_INST(OUT_) \
    template void launch_gemm_grouped_stream<OUT_>(const int8_t*, int64_t, const int32_t*, int64_t, const int8_t*, int64_t, int64_t, const EpiArgs&, const int32_t*, int, int64_t, int64_t, int64_t, hipStream_t);
PQ_GS_INST(PQ_BF16) PQ_GS_INST(PQ_FP16) PQ_GS_INST(PQ_F32) PQ_GS_INST(OUT_I32)
#undef PQ_GS_INST

}  // namespace pq
