// gemm_s8_grouped.hip — K3/K4 for a MIXTURE OF EXPERTS: y[r, :] = dequant(xq[src(r), :] . wq[e(r)]^T) for the rows r of a token list SORTED BY EXPERT — rows
// offsets[e] .. offsets[e + 1] - 1 belong to expert e — in ONE launch over all experts, instead of one launch of pq_qlinear_s8 per expert on its few rows.
//
//   * `offsets` (int32[E + 1]) lives in DEVICE memory and is read by the kernel only: the host sizes the grid from what it knows — with tile height TM at most
//     ceil(M_total / TM) + E m-tiles exist whatever the split (every expert adds at most one partial tile) — and each workgroup finds its (expert, m-tile) itself
//     (grouped_find_tile: one lane per expert, a wave prefix sum of the experts' tile counts, no prepass kernel, no workspace, no atomics).  A workgroup whose tile does not
//     exist returns before it touches LDS or issues a DMA.  A captured hipGraph therefore stays valid when the CONTENTS of offsets (and of the row index) change.
//   * tile order: the tiles of one expert are consecutive, m fastest inside a weight panel, then the XCD remap — the workgroups that stream one weight panel of one expert
//     are neighbours on one XCD, as in gemm_s8_ringt.
//   * tile body: the loader / consumer ring tile of gemm_s8_ring.hip, instantiated HERE (grouped_tile_body).  Sharing one __forceinline__ body between the two files was
//     tried first: it moved the register allocation of the existing gemm_s8_ringt instantiations (66 -> 63 SGPRs, a different prologue schedule), so gemm_s8_ring.hip stays
//     byte for byte what it was and this file carries its own copy.  A tile of expert e is that tile with the weight base W + e * w_stride, the column scales / bias of
//     expert e and M = offsets[e + 1]: loader rows past the expert's last row re-read a valid row of the same expert, the staged epilogue runs only for wave blocks that lie
//     wholly inside the expert, and the guarded direct stores skip every row >= M — not one byte goes into the next expert's rows.
//   * optional ROW GATHER on the activation operand (GATHER): grouped row r reads its codes at row qrow[r] of X, the un-permuted [T, K] code matrix (a token appears top_k
//     times).  The loader's per-lane 32-bit source offset becomes qrow[r] * ldx + chunk * 16 relative to X itself — the launcher's caller rejects x_rows * ldx >= 2^32 —
//     and nothing else changes.  The row SCALES are always in grouped order.
//   * same MFMA, same integer sums, same epilogue arithmetic as every other variant: bit-identical to pq_qlinear_s8 run once per expert on that expert's row slice.
// Untrusted device data: offsets are clamped into [0, M_total] and the row index into [0, x_rows): wrong contents give wrong results, never an access outside the operands.
#include "gemm_tile_common.h"
#include "pq_launch.h"

namespace pq {

// The tile of m-tile slot q (slots are dealt to the experts in order: expert e owns ceil(rows_e / TM) of them): one lane per expert, 64 experts per step.  Every lane of
// every wave computes the same answer; the results are made scalar by the caller.  false: slot q holds no tile (the grid is the upper bound ceil(M_total / TM) + E).
struct GroupedTile { int e, base, cnt, lo, hi; };      // expert, its first m-tile slot, its m-tile count, its row range [lo, hi)
template <int TM>
__device__ __forceinline__ bool grouped_find_tile(const int32_t* __restrict__ offsets, int E, int M_total, int q, GroupedTile& g) {
    const int lane = threadIdx.x & 63;
    int run = 0;                                               // m-tile slots of the experts before this step
    for (int b = 0; b < E; b += 64) {
        const int e = b + lane;
        int lo = 0, hi = 0;
        if (e < E) {
            hi = offsets[e + 1];
            lo = offsets[e];
            hi = hi < 0 ? 0 : (hi > M_total ? M_total : hi);
            lo = lo < 0 ? 0 : (lo > hi ? hi : lo);
        }
        const int c = (hi - lo + TM - 1) / TM;
        int inc = c;                                           // inclusive prefix sum over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(inc, d, 64);
            if (lane >= d) inc += v;
        }
        const unsigned long long hit = __ballot(run + inc > q);
        if (hit != 0) {
            const int l = __ffsll((long long)hit) - 1;
            g.e = b + l;
            g.base = run + __shfl(inc - c, l, 64);
            g.cnt = __shfl(c, l, 64);
            g.lo = __shfl(lo, l, 64);
            g.hi = __shfl(hi, l, 64);
            return true;
        }
        run += __shfl(inc, 63, 64);
    }
    return false;
}

// ---- the tile body: gemm_s8_ringt's (gemm_s8_ring.hip), with the tile's place and operands handed in by the caller
template <int OUT, int TM, int TN, int NB, int KT, bool GATHER>
__device__ __forceinline__ void grouped_tile_body(uint8_t* smem, const int8_t* __restrict__ X, int64_t ldx, const int8_t* __restrict__ W, int64_t ldw, const EpiArgs& epi,
                                               int M, int N, int K, int m0, int n0, int rsel, int ct, int rot_div,
                                               const int32_t* __restrict__ qrow = nullptr, int x_rows = 0) {
    constexpr int P_OPER = TN * FBK, Q_OPER = TM * FBK, BUF = P_OPER + Q_OPER;
    constexpr int PPW = TN / 32, QPW = TM / 32, PPT = PPW + QPW;      // 1-KiB DMA pieces per loader wave per K-tile: P side, Q side, both
    constexpr int NPI = TN / 32, NQJ = TM / 32;                       // 16 x 16 tiles of a consumer's wave block: along n, along m
    constexpr int NMF = 2 * NPI * NQJ, NRD = 2 * (NPI + NQJ);         // MFMAs and fragment reads per K-tile and consumer wave
    constexpr int RPS = (2 * NRD + NMF - 1) / NMF;                    // fragment reads per MFMA shadow: all of them behind the first half of the MFMAs
    constexpr int SLOT = KT * BUF;
    static_assert(TM % 32 == 0 && TN % 32 == 0 && NB >= 3 && NB * SLOT <= 160 * 1024 && (NB - 1) * KT * PPT <= 63, "ring tile shape");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool loader = wave >= 4;
    const int w = wave & 3, wp = w >> 1, wq = w & 1;

    uint32_t offP[PPW], offQ[QPW];
#pragma unroll
    for (int jj = 0; jj < PPW; ++jj) {
        const int piece = w * PPW + jj, r = piece * 8 + (lane >> 3);
        const int src_chunk = (lane & 7) ^ (((piece & 1) * 4 + (lane >> 4)) & 7);
        const int nl = (n0 + r < N) ? r : (N - 1 - n0);       // clamp: rows past the edge re-read a valid row
        offP[jj] = (uint32_t)nl * (uint32_t)ldw + src_chunk * 16;
    }
#pragma unroll
    for (int jj = 0; jj < QPW; ++jj) {
        const int piece = w * QPW + jj, r = piece * 8 + (lane >> 3);
        const int src_chunk = (lane & 7) ^ (((piece & 1) * 4 + (lane >> 4)) & 7);
        const int ml = (m0 + r < M) ? r : (M - 1 - m0);
        if constexpr (GATHER) {                                // the row's codes lie at row qrow[m] of X (clamped into X: the index is device data nobody has checked)
            const uint32_t src = (uint32_t)qrow[m0 + ml];
            offQ[jj] = (src < (uint32_t)x_rows ? src : (uint32_t)x_rows - 1u) * (uint32_t)ldx + src_chunk * 16;
        } else {
            offQ[jj] = (uint32_t)ml * (uint32_t)ldx + src_chunk * 16;
        }
    }
    const int NT = K / FBK;
    // K rotation in chunks of `ct` K-tiles between the workgroups that stream one weight panel (gemm_s8_ring.hip, "K ROTATION in chunks"): rot_div = 0: none
    auto rot_of = [&](int len) { return rot_div > 0 ? (int)(((int64_t)(rsel % rot_div) * len) / rot_div) : 0; };
    int cbase = 0, clen = ct < NT ? ct : NT;
    int cpos = rot_of(clen), cleft = clen;
    const int8_t* const gP0 = W + (int64_t)n0 * ldw;
    const int8_t* const gQ0 = GATHER ? X : X + (int64_t)m0 * ldx;
    const uint32_t smem_base = (uint32_t)(uintptr_t)(lptr_t)smem;
    auto stage1 = [&](uint32_t la) {                           // this loader wave's pieces of its next K-tile, then the K walk moves on
        const int ktu = __builtin_amdgcn_readfirstlane(cbase + cpos);      // (the rotation's division is vector code; the DMA's base operand must be provably wave-uniform)
        const int8_t* gP = gP0 + ktu * FBK;
        const int8_t* gQ = gQ0 + ktu * FBK;
#pragma unroll
        for (int jj = 0; jj < PPW; ++jj) glds16_sbase(gP, offP[jj], la + (uint32_t)(w * PPW + jj) * 1024u);
#pragma unroll
        for (int jj = 0; jj < QPW; ++jj) glds16_sbase(gQ, offQ[jj], la + P_OPER + (uint32_t)(w * QPW + jj) * 1024u);
        if (++cpos == clen) cpos = 0;
        if (--cleft == 0) {                                    // next chunk
            cbase += clen;
            clen = NT - cbase < ct ? NT - cbase : ct;
            cleft = clen;
            cpos = clen > 0 ? rot_of(clen) : 0;
        }
    };
    const int NS = (NT + KT - 1) / KT;                         // ring slots' worth of K-tiles (the last one may be partly filled)
    auto stage = [&](int s) {                                  // slot s: its KT K-tiles (those that exist)
#pragma unroll
        for (int u = 0; u < KT; ++u)
            if (s * KT + u < NT) stage1(smem_base + (uint32_t)(s % NB) * SLOT + (uint32_t)u * BUF);
    };

    if (loader) {
        // prologue: up to NB slots in flight; then, per slot s: slot s + 1 must have landed (slots s + 2 .. s + NB - 1 may stay in flight: counted in the
        // pieces they really hold), the barrier the consumers share, and the pieces of slot s + NB into the ring slot that slot s has just vacated
        auto fly = [&](int s) {                                // this wave's pieces of the slots behind slot s + 1 that have been issued
            const int t0 = (s + 2) * KT, t1 = (s + NB) * KT < NT ? (s + NB) * KT : NT;
            return t1 > t0 ? (t1 - t0) * PPT : 0;
        };
#pragma unroll 1
        for (int b = 0; b < NB && b < NS; ++b) stage(b);
        {                                                      // slot 0 has landed; slots 1 .. NB - 1 may stay in flight
            const int t1 = NB * KT < NT ? NB * KT : NT;
            wait_vmcnt_lgkm0(t1 > KT ? (t1 - KT) * PPT : 0);
        }
        __builtin_amdgcn_s_barrier();
#pragma unroll 1
        for (int sl = 0; sl < NS; ++sl) {
            if (sl + 1 < NS) {
                wait_vmcnt_lgkm0(fly(sl));
                __builtin_amdgcn_s_barrier();
            }
            if (sl + NB < NS) stage(sl + NB);
        }
        return;
    }

    // ---- consumers.  Fragments: P tile i = rows wp * (TN/2) + 16 i .. + 15, Q tile j = rows wq * (TM/2) + 16 j .. + 15; k-step ks = 64 bytes
    const int frow = lane & 15, fchunk = lane >> 4, fkey = (frow >> 1) & 7;
    uint32_t lP[2], lQ[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int c = ks * 4 + fchunk;
        lP[ks] = (uint32_t)((wp * (TN / 2) + frow) * 128 + ((c ^ fkey) * 16));
        lQ[ks] = (uint32_t)((wq * (TM / 2) + frow) * 128 + ((c ^ fkey) * 16)) + P_OPER;
    }
    // item it < 2 NPI: P tile it % NPI of k-step it / NPI; the others: Q tile (it - 2 NPI) % NQJ of k-step (it - 2 NPI) / NQJ
    v4i fa[NRD], fb[NRD];
    auto read_item = [&](int bufoff, v4i (&f)[NRD], auto ic) {
        constexpr int it = decltype(ic)::value;
        if constexpr (it < 2 * NPI) f[it] = *reinterpret_cast<const v4i*>(smem + bufoff + lP[it / NPI] + (it % NPI) * 16 * 128);
        else f[it] = *reinterpret_cast<const v4i*>(smem + bufoff + lQ[(it - 2 * NPI) / NQJ] + ((it - 2 * NPI) % NQJ) * 16 * 128);
    };
    v4i acc[NPI][NQJ];
#pragma unroll
    for (int i = 0; i < NPI; ++i)
#pragma unroll
        for (int j = 0; j < NQJ; ++j) acc[i][j] = v4i{0, 0, 0, 0};
    __builtin_amdgcn_s_barrier();                              // tile 0 has landed (the loaders waited for it)
    static_for<NRD>([&](auto ic) { read_item(0, fa, ic); });

    auto tile = [&](int kt, v4i (&cur)[NRD], v4i (&nxt)[NRD]) {
        // the next K-tile opens a new slot: that slot must have landed (the loaders waited), and this wave is done with the slot it leaves
        if (kt + 1 < NT && (kt + 1) % KT == 0) {
            __builtin_amdgcn_s_waitcnt(waitcnt_imm(63, 0));    // this wave's fragment reads so far (the loaders wait for the DMA)
            __builtin_amdgcn_s_barrier();
        }
        const int nbuf = (((kt + 1) / KT) % NB) * SLOT + ((kt + 1) % KT) * BUF;
        __builtin_amdgcn_sched_barrier(0);
        static_for<NMF>([&](auto xc) {
            constexpr int x = decltype(xc)::value, ks = x / (NPI * NQJ), i = (x / NQJ) % NPI, j = x % NQJ;
            acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(cur[ks * NPI + i], cur[2 * NPI + ks * NQJ + j], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            static_for<RPS>([&](auto rc) {                     // (last tile: reads a stale slot, values unused)
                constexpr int it = x * RPS + decltype(rc)::value;
                if constexpr (it < NRD) read_item(nbuf, nxt, std::integral_constant<int, it>{});
            });
            __builtin_amdgcn_sched_barrier(0);
        });
    };
    int kt = 0;
    for (; kt + 1 < NT; kt += 2) { tile(kt, fa, fb); tile(kt + 1, fb, fa); }
    if (kt < NT) tile(kt, fa, fb);

    // ---- epilogue: D[row <-> n][col <-> m]; lane holds 4 consecutive n of one m per accumulator
    using O = typename OutElem<OUT>::type;
    constexpr int OB = (int)sizeof(O);
    O* y = reinterpret_cast<O*>(epi.y);
    const bool has_bias = (OUT != OUT_I32) && epi.bias != nullptr;
    const int dcol = lane & 15, drow4 = (lane >> 4) * 4;
    const int wm0 = m0 + wq * (TM / 2), wn0 = n0 + wp * (TN / 2);
    const bool staged = (wm0 + TM / 2 <= M) && (wn0 + TN / 2 <= N) && epi_rows_storable(epi, y, OB) &&
                        (OUT == OUT_I32 || (reinterpret_cast<uintptr_t>(epi.b_scale) & 15) == 0) &&
                        (!has_bias || (reinterpret_cast<uintptr_t>(epi.bias) & (4 * OB - 1)) == 0);
    if (staged) {
        // staging: this wave's quarter of the first K-tile of the ring slot BEHIND the last one: no slot NS exists, so no DMA targets it, its previous
        // tenant (slot NS - NB) was read out long ago, and the last tile's prefetch of "tile NT" reads values nobody uses
        const uint32_t sw_off = (uint32_t)((NS % NB) * SLOT + w * (BUF / 4));
        constexpr int PT_PASS = (NPI * 16 * OB > 256 && NPI % 2 == 0) ? NPI / 2 : NPI;       // (five column tiles — the 128 x 160 tile — stage in one pass of 160 / 320 used bytes per row)
        constexpr int RSTRIDE = PT_PASS * 16 * OB <= 64 ? 64 : PT_PASS * 16 * OB <= 128 ? 128 : PT_PASS * 16 * OB <= 256 ? 256 : 512;      // gemm_epilogue.h: RBY
        constexpr int QT_MAX = (BUF / 4) / (16 * RSTRIDE);
        constexpr int QT_PASS = QT_MAX >= NQJ ? NQJ : 1;
        static_assert(QT_PASS >= 1 && QT_PASS * 16 * RSTRIDE <= BUF / 4, "epilogue staging region");
        auto acc_of = [&](int pt, int qt) -> const v4i& { return acc[pt][qt]; };
        auto as_of = [&](int qt) { return epi.a_scale[wm0 + qt * 16 + dcol]; };
        auto bs_of = [&](int pt) { return *reinterpret_cast<const v4f*>(epi.b_scale + wn0 + pt * 16 + drow4); };
        uint8_t* y_blk = reinterpret_cast<uint8_t*>(y + (int64_t)wm0 * epi.ldy + wn0);
        const void* bias_blk = has_bias ? static_cast<const void*>(reinterpret_cast<const O*>(epi.bias) + ((epi.flags & EPI_BIAS_ROWS) ? wm0 : wn0)) : nullptr;
        PQ_EPI_STAGED_DISPATCH(OUT, NPI, NQJ, QT_PASS, PT_PASS, has_bias, epi.flags, acc_of, as_of, bs_of, bias_blk, smem, sw_off, y_blk, epi.ldy * OB, lane);
        return;
    }
    // direct path (edge tiles / unaligned y): guarded stores from registers, 4 consecutive n at a time when aligned
    const bool vec_ok = ((reinterpret_cast<uintptr_t>(y) & (4 * OB - 1)) == 0) && ((epi.ldy & 3) == 0);
#pragma unroll
    for (int j = 0; j < NQJ; ++j) {
        const int m = wm0 + j * 16 + dcol;
        if (m >= M) continue;
        float as = 1.0f;
        if constexpr (OUT != OUT_I32) as = epi.a_scale[m];
#pragma unroll
        for (int i = 0; i < NPI; ++i) {
            const int nb = wn0 + i * 16 + drow4;
            if (nb >= N) continue;
            O o[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = nb + r < N ? nb + r : N - 1;
                float bs = 1.0f, bf = 0.0f;
                if constexpr (OUT != OUT_I32) {
                    bs = epi.b_scale[n];
                    if (has_bias) bf = load_bias<OUT>(epi.bias, (epi.flags & EPI_BIAS_ROWS) ? m : n);
                }
                o[r] = epi_convert<OUT>(acc[i][j][r], as, bs, bf, has_bias, epi.flags & EPI_COL_FIRST);
            }
            O* dst = y + (int64_t)m * epi.ldy + nb;
            if (nb + 3 < N && vec_ok) {
                if constexpr (OB == 2) *reinterpret_cast<v2u*>(dst) = *reinterpret_cast<const v2u*>(o);
                else *reinterpret_cast<v4u*>(dst) = *reinterpret_cast<const v4u*>(o);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) if (nb + r < N) dst[r] = o[r];
            }
        }
    }
}

// one workgroup = one TM x TN tile of one expert (or nothing).  mt_max = ceil(M_total / TM) + E m-tile slots x tiles_n workgroups are launched.
template <int OUT, int TM, int TN, int NB, int KT, bool GATHER>
__global__ __launch_bounds__(512, 2) void gemm_s8_grouped(const int8_t* __restrict__ X, int64_t ldx, const int32_t* __restrict__ qrow, int x_rows,
                                                          const int8_t* __restrict__ W, int64_t ldw, int64_t w_stride, EpiArgs epi,
                                                          const int32_t* __restrict__ offsets, int E, int M_total, int N, int K, int tiles_n, int mt_max, int ct, int rot) {
    constexpr int SLOT = KT * (TM + TN) * FBK;
    __shared__ __attribute__((aligned(16))) uint8_t smem[NB * SLOT];
    const int t = xcd_remap((int)blockIdx.x, mt_max * tiles_n, epi.nxcd);
    GroupedTile g;
    if (!grouped_find_tile<TM>(offsets, E, M_total, t / tiles_n, g)) return;       // (wave-uniform, and the same in every wave: nobody is left at a barrier)
    const int e = __builtin_amdgcn_readfirstlane(g.e), base = __builtin_amdgcn_readfirstlane(g.base), cnt = __builtin_amdgcn_readfirstlane(g.cnt);
    const int lo = __builtin_amdgcn_readfirstlane(g.lo), hi = __builtin_amdgcn_readfirstlane(g.hi);
    const int tin = t - base * tiles_n;                        // this expert's tiles: m fastest inside a weight panel
    const int tml = tin % cnt, tn = tin / cnt;
    using O = typename OutElem<OUT>::type;
    EpiArgs ee = epi;                                          // expert e's column scales and bias; row scales and y are in grouped order
    if constexpr (OUT != OUT_I32) {
        ee.b_scale = epi.b_scale + (int64_t)e * N;
        if (epi.bias != nullptr) ee.bias = reinterpret_cast<const O*>(epi.bias) + (int64_t)e * N;
    }
    grouped_tile_body<OUT, TM, TN, NB, KT, GATHER>(smem, X, ldx, W + (int64_t)e * w_stride, ldw, ee, hi, N, K, lo + tml * TM, tn * TN, tml, ct,
                                                   rot ? (cnt < 8 ? cnt : 8) : 0, qrow, x_rows);
}

// tile: 0 = 64(m) x 128(n), 3 slots of 2 K-tiles (144 KiB); 1 = 64 x 64, 4 slots of 2 K-tiles (128 KiB) — the two small ring tiles of gemm_s8_ring.hip.
// rot: rotate the K walk between the m-tiles of ONE expert that stream one weight panel (chunk sized for the average expert: the host does not know the split).
template <int OUT>
void launch_gemm_grouped(int tile, const int8_t* X, int64_t ldx, const int32_t* qrow, int64_t x_rows, const int8_t* W, int64_t ldw, int64_t w_stride, const EpiArgs& epi,
                         const int32_t* offsets, int E, int64_t M_total, int64_t N, int64_t K, int rot, hipStream_t st) {
    const int mt_max = (int)((M_total + 63) / 64) + E;
    const int64_t avg_tiles = ((M_total + E - 1) / E + 63) / 64;
    const int sharers = avg_tiles < 1 ? 1 : (avg_tiles > 8 ? 8 : (int)avg_tiles);
    const int xr = (int)x_rows;
#define PQ_GROUPED_LAUNCH(TN_, NB_, GATHER_)                                                                                                                   \
    gemm_s8_grouped<OUT, 64, TN_, NB_, 2, GATHER_><<<dim3((unsigned)(mt_max * tiles_n)), dim3(512), 0, st>>>(X, ldx, qrow, xr, W, ldw, w_stride, epi, offsets, E, \
                                                                                                         (int)M_total, (int)N, (int)K, tiles_n, mt_max, ct, rot)
    if (tile == 0) {
        const int tiles_n = (int)((N + 127) / 128), ct = rot_chunk_ktiles(sharers, 128);
        if (qrow) PQ_GROUPED_LAUNCH(128, 3, true); else PQ_GROUPED_LAUNCH(128, 3, false);
    } else {
        const int tiles_n = (int)((N + 63) / 64), ct = rot_chunk_ktiles(sharers, 64);
        if (qrow) PQ_GROUPED_LAUNCH(64, 4, true); else PQ_GROUPED_LAUNCH(64, 4, false);
    }
#undef PQ_GROUPED_LAUNCH
}
#define PQ_GROUPED_INST(OUT_) \
    template void launch_gemm_grouped<OUT_>(int, const int8_t*, int64_t, const int32_t*, int64_t, const int8_t*, int64_t, int64_t, const EpiArgs&, const int32_t*, int, int64_t, int64_t, int64_t, int, hipStream_t);
PQ_GROUPED_INST(PQ_BF16) PQ_GROUPED_INST(PQ_FP16) PQ_GROUPED_INST(PQ_F32) PQ_GROUPED_INST(OUT_I32)
#undef PQ_GROUPED_INST

}  // namespace pq
