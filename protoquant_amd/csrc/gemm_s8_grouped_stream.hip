// gemm_s8_grouped_stream.hip — K3/K4 for a MIXTURE OF EXPERTS AT DECODE (M_total <= 64 grouped rows): the contract of gemm_s8_grouped.hip — rows sorted by expert,
// `offsets` and the optional row index in device memory and never read on the host, y[r, :] = dequant(xq[src(r), :] . wq[e(r)]^T) — as the GROUPED host of the
// weight-streaming body (gemm_stream_body.h; gemm_s8_skinny.hip is its dense host) instead of a 64-row ring tile.  With one or two rows per expert the GEMM is a
// streaming read of the LIVE experts' weights, N * K bytes
// each: a 64-row tile stages 64 activation rows to use one and leaves most of the chip without a workgroup (Mixtral's down projection at one token: 64 workgroups).
// This file holds what is the grouped kernel's own: the expert's epilogue operands (no EPI_* flags, rows >= hi not stored), the branch over the token-tile count, and
// the launcher; the slot search and where activation row i of an expert lies (GroupedRows) are grouped_stream_rows.h, shared with the int4 grouped kernel; the
// (MT, RB, KS) of a launch is grouped_stream_plan (pq_plan.hip).
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
//     one tile's MFMAs and activation loads, not four.  Cost: the kernel's register allocation is that of its largest body — 72 VGPRs for MT = 1 and 2 (80 with
//     RB = 2), 100 for MT = 4, where a one-tile body alone needs 72; every instantiation is launched with up to 16 waves per workgroup, which allows 128, so no
//     occupancy is lost — and MT = 4 carries five bodies of code.  Three or four tiles with two weight
//     blocks per wave would not fit 128 VGPRs (as in the dense kernel): RB = 2 exists for MT <= 2 only.
//   * the row gather is a run-time branch in the prologue (the source row of grouped row r is qrow[r] clamped into [0, x_rows)): it only changes the row pointers.
// Untrusted device data: offsets are clamped into [0, M_total] (hi) and [0, hi] (lo), the row index into [0, x_rows) — wrong contents give wrong results, never an access
// outside the operands; rows >= offsets[E] of y are not written.
// The non-temporal hint on the weight loads is NOT used: it loses when one launch is replayed on cached data, and no A/B of it has been run here.
#include <cstdlib>

#include "gemm_stream_body.h"
#include "grouped_stream_rows.h"
#include "pq_launch.h"
#include "pq_plan.h"

namespace pq {

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
    const GroupedRows src{X, ldx, qrow, x_rows, lo, rows};
    const StreamOut<NoEpiFlags> out{epi.a_scale, ws, bias, epi.y, epi.ldy, {}, lo, rows};
#define PQ_GS_BODY(NT_, STAGE_) stream_body<OUT, NT_, RB, STAGE_, false>(gs_smem, src, We, ldw, out, n0, N, K)
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

template <int OUT>
void launch_gemm_grouped_stream(const int8_t* X, int64_t ldx, const int32_t* qrow, int64_t x_rows, const int8_t* W, int64_t ldw, int64_t w_stride, const EpiArgs& epi,
                                const int32_t* offsets, int E, int64_t M_total, int64_t N, int64_t K, hipStream_t st) {
    int mt = 1, rb = 1, ks = 1;
    grouped_stream_plan(E, M_total, N, K, &mt, &rb, &ks);
    const int64_t slots = M_total < E ? M_total : E;
    const dim3 grid((unsigned)((N + 16 * rb - 1) / (16 * rb)), (unsigned)slots), block((unsigned)(ks * 64));
    const size_t lds = stream_lds_bytes(ks, mt, rb, true);
#define PQ_GS(MTv, RBv) stream_launch(&gemm_s8_grouped_stream<OUT, MTv, RBv>, grid, block, lds, st, X, ldx, qrow, (int)x_rows, W, ldw, w_stride, epi, offsets, E, (int)M_total, (int)N, (int)K)
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
