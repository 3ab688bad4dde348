// gemm_w4_grouped_stream.hip — the decode GEMM of a MIXTURE OF EXPERTS on int4 weights (M_total <= 64 grouped rows): the contract of gemm_s8_grouped_stream.hip — rows
// sorted by expert, `offsets` and the optional row index in device memory and never read on the host — on the experts' PACKED weights (QSPEC W1-W4):
// y[r, :] = dequant(xq[src(r), :] . W8[e(r)]^T) with W8[e] = w4_expand(w4[e], gs[e]), bit for bit what gemm_s8_grouped_stream gives on the expanded [E, N, Kp] weight.
// A decode step streams the LIVE experts' weights once; here that stream is Kp / 2 + Kp / 128 bytes per weight row instead of Kp.
// This is the GROUPED host of the int4 weight-streaming body (gemm_w4_stream_body.h: 16-byte fragment loads of two k-steps, three-VALU nibble unpack, zeroed group
// accumulator and 24-bit rescale, wave-private activation staging, exact LDS reduction, E1-E4), as gemm_s8_grouped_stream.hip is the grouped host of the int8 one:
//   * grid = ceil(N / 16) weight blocks (x) times S = min(E, M_total) expert SLOTS (y); slot j serves the j-th expert whose clamped row range is not empty
//     (stream_find_slot, grouped_stream_rows.h).  A slot without an expert returns before it touches a weight, a multiplier or an activation.  No workspace, no atomics,
//     no wait on another workgroup: a captured hipGraph stays valid when the CONTENTS of offsets / row index / xs change.
//   * a workgroup = KS waves that split the Kp / 128 groups of ONE 16-row block of ONE expert: w4 + e * w4_stride, gs + e * gs_stride — per expert the W4 v1 layout of
//     its own N rows, so the quad clamp of the body (ceil(N / 4) quads) holds inside every expert whatever N % 4.
//   * token tiles: an expert's row count (1 .. 64) is device data.  Compiled for MT = 1, 2 or 4 token tiles, chosen by the host from M_total; a workgroup branches —
//     wave-uniformly, the same way in all its waves — to the body of ITS expert's ceil(rows / 16): an expert with one row of a 64-row step does one tile's MFMAs and
//     direct activation loads.  The register allocation is that of the largest body (DESIGN.md has the table); all fit 128 VGPRs without scratch.
//   * the row gather is GroupedRows::src_row (row index clamped into [0, x_rows)); epilogue operands xs[lo + m], ws[e][n], bias[e][n]; rows >= offsets[E] are not written.
#include "gemm_w4_stream_body.h"
#include "grouped_stream_rows.h"
#include "pq_launch.h"

namespace pq {

// blockIdx.x: the 16-row weight block, blockIdx.y: the expert slot.  M_total <= 16 MT (the launcher's choice), so an expert has at most MT token tiles.
// w4_stride in bytes, gs_stride in dwords (one dword = the multipliers of a row quad in one group).
template <int OUT, int MT>
__global__ __launch_bounds__(1024) void gemm_w4_grouped_stream(const int8_t* __restrict__ X, int64_t ldx, const int32_t* __restrict__ qrow, int x_rows,
                                                               const uint8_t* __restrict__ W4, int64_t ldw4, int64_t w4_stride, const uint32_t* __restrict__ GS,
                                                               int64_t gs_stride, EpiArgs epi, const int32_t* __restrict__ offsets, int E, int M_total, int N, int G) {
    extern __shared__ __attribute__((aligned(16))) uint8_t w4g_smem[];
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
    const uint8_t* We = W4 + (int64_t)e * w4_stride;
    const uint32_t* Ge = GS + (int64_t)e * gs_stride;
    const int n0 = (int)blockIdx.x * 16, rows = hi - lo;
    const GroupedRows src{X, ldx, qrow, x_rows, lo, rows};
    const StreamOut<NoEpiFlags> out{epi.a_scale, ws, bias, epi.y, epi.ldy, {}, lo, rows};
#define PQ_W4G_BODY(NT_, STAGE_) w4_stream_body<OUT, NT_, STAGE_>(w4g_smem, src, We, ldw4, Ge, out, n0, N, G)
    if constexpr (MT >= 4) {
        if (rows > 48) { PQ_W4G_BODY(4, true); return; }
        if (rows > 32) { PQ_W4G_BODY(3, true); return; }
    }
    if constexpr (MT >= 2) {
        if (rows > 16) { PQ_W4G_BODY(2, true); return; }
    }
    if (rows > 1) PQ_W4G_BODY(1, true);
    else PQ_W4G_BODY(1, false);
#undef PQ_W4G_BODY
}

// dynamic LDS of a launch: the larger of the reduction buffer and the staging regions of the largest body among 1 .. mt token tiles
static size_t w4_grouped_lds_bytes(int ks, int mt) {
    size_t lds = ks > 1 ? (size_t)ks * mt * 64 * sizeof(v4i) : 0;
    for (int nt = 1; nt <= mt; ++nt) {
        const size_t b = (size_t)ks * w4_stage_bytes(nt);
        lds = b > lds ? b : lds;
    }
    return lds;
}

template <int OUT>
void launch_gemm_w4_grouped_stream(const int8_t* X, int64_t ldx, const int32_t* qrow, int64_t x_rows, const uint8_t* W4, int64_t ldw4, int64_t w4_stride, const uint8_t* GS,
                                   int64_t gs_stride, const EpiArgs& epi, const int32_t* offsets, int E, int64_t M_total, int64_t N, int64_t Kp, hipStream_t st) {
    int mt = 1, ks = 1;
    w4_grouped_stream_plan(E, M_total, N, Kp, &mt, &ks);
    const int64_t slots = M_total < E ? M_total : E;
    const dim3 grid((unsigned)((N + 15) / 16), (unsigned)slots), block((unsigned)(ks * 64));
    const size_t lds = w4_grouped_lds_bytes(ks, mt);
    const uint32_t* gs = reinterpret_cast<const uint32_t*>(GS);
#define PQ_W4G(MTv) stream_launch(&gemm_w4_grouped_stream<OUT, MTv>, grid, block, lds, st, X, ldx, qrow, (int)x_rows, W4, ldw4, w4_stride, gs, gs_stride / 4, epi, offsets, E, (int)M_total, (int)N, (int)(Kp / 128))
    if (mt == 1) PQ_W4G(1);
    else if (mt == 2) PQ_W4G(2);
    else PQ_W4G(4);
#undef PQ_W4G
}
#define PQ_W4G_INST(OUT_) \
    template void launch_gemm_w4_grouped_stream<OUT_>(const int8_t*, int64_t, const int32_t*, int64_t, const uint8_t*, int64_t, int64_t, const uint8_t*, int64_t, const EpiArgs&, const int32_t*, int, int64_t, int64_t, int64_t, hipStream_t);
PQ_W4G_INST(PQ_BF16) PQ_W4G_INST(PQ_FP16) PQ_W4G_INST(PQ_F32) PQ_W4G_INST(OUT_I32)
#undef PQ_W4G_INST

}  // namespace pq
