// head_norm_kernels.hip — K1hn: the per-head RMSNorm of an attention's q and k (q_norm / k_norm of Qwen3, Qwen3-MoE and Gemma-3) in one launch, no codes and no
// scales (QSPEC HN1: N1-N5 or NG1-NG5 on rows of head_dim).
//   out[o, i, :] = norm(x[o, i, :]; weight, eps)      o < n_outer, i < n_inner; both operands addressed as base + o * ld_o + i * ld_i + c, ONE weight[cols] for all rows
// The rows are HEADS: 64 .. 256 elements wide, and addressed by two strides (a token stride — the leading dimension of the fused q/k/v output — and a head stride),
// which the row ABI (one leading dimension) cannot express.  Algorithmic traffic for 16-bit rows: 4 B/elem (x read, out written; the weight is cache-resident).
// The gains are the family's tags (rownorm_kernels.h): LlamaGain (N5, Qwen3RMSNorm) and GemmaGain (NG5, Gemma3RMSNorm); rs is rms_rs.
// Vector form: one 16-byte vector per lane, G = the power of two >= nvec (at least 4) lanes per head, 64 / G heads per wave, four waves per block and no block
// barrier.  The order of the specification (N1-N3: vector v on lane v mod 256, an xor butterfly per 64 lanes, the four group sums left to right) on a row of at most
// 64 vectors: lanes past nvec and the three other groups contribute +0 (fma(0, 0, acc) = acc, a + 0 = a: a sum of squares is never -0), so the butterfly over the G
// lanes that hold the head, offsets G/2 .. 1, gives the bits of the pinned order.  Lanes of a group past nvec load a clamped duplicate of the head's last vector and
// are zeroed before use; groups past the last head walk a clamped duplicate of the last head; neither stores anything.  A wave holds ONE group of heads: walking two or
// four groups per wave with every load in front was measured and gains nothing (profiles/r25_head_norm_groups_ab.txt).
// Generic form (a width that is no whole number of vectors or over 1024 bytes, unaligned operands): one wave per head, the same lane layout walked element by
// element with the four group accumulators of the one-wave row layout; the head is read twice (from cache the second time).  Same bits wherever both apply.
// Aliasing: none; out may overlap neither x nor the weight (pq_api.hip refuses it), so every pointer is __restrict__.
#include "rownorm_kernels.h"
#include "pq_launch.h"

namespace pq {

// flat head n -> (outer, inner) index; pq_api.hip holds the number of heads below 2^31, so one 32-bit division serves (the offsets it feeds are 64-bit)
__device__ __forceinline__ void head_index(int64_t n, int64_t n_inner, int64_t& o, int64_t& i) {
    const uint32_t q = n_inner == 1 ? (uint32_t)n : (uint32_t)n / (uint32_t)n_inner;
    o = q;
    i = (int64_t)((uint32_t)n - q * (uint32_t)n_inner);
}

template <int DT, int G, class GAIN>
__global__ __launch_bounds__(256) void head_rmsnorm_vec(const uint8_t* __restrict__ x, int64_t ldxo_bytes, int64_t ldxi_bytes, const uint8_t* __restrict__ wgt, float eps,
                                                        int cols, int nvec, int64_t heads, int64_t n_inner, uint8_t* __restrict__ out, int64_t ldoo_bytes,
                                                        int64_t ldoi_bytes) {
    static_assert(G >= 4 && G <= 64 && (G & (G - 1)) == 0, "G lanes per head: a power of two, 4 .. 64");
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    constexpr int HPW = 64 / G;                                // heads per wave
    const int lane = threadIdx.x & 63, t = lane & (G - 1);
    int64_t head = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * HPW + lane / G;
    const bool active = head < heads;                          // a group past the last head walks a duplicate of the last head and stores nothing
    head = active ? head : heads - 1;
    int64_t o, i;
    head_index(head, n_inner, o, i);
    const int64_t voff = clamped_vec_off(t, nvec);
    v4u xv = *reinterpret_cast<const v4u*>(x + o * ldxo_bytes + i * ldxi_bytes + voff);
    const v4u wv = *reinterpret_cast<const v4u*>(wgt + voff);  // (one weight vector per lane: loaded once per wave)
    const bool live = t < nvec;
    if (!live) xv = v4u{0u, 0u, 0u, 0u};                       // past the head: fma(0, 0, acc) = acc
    float f[EPV];
    Unpack<DT, EPV>::run(xv, f);
    float acc = 0.0f;                                          // N2: the elements of this lane's vector in order
#pragma unroll
    for (int j = 0; j < EPV; ++j) acc = __builtin_fmaf(f[j], f[j], acc);
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);      // N3 on the lanes of this head (xor below G stays inside the group)
    const float rs = rms_rs(acc, cols, eps);                   // N4
    const v4u hv = GAIN::template h_vec<DT>(xv, wv, rs);       // N5 / NG5
    if (active && live) store_wt_b128(out + o * ldoo_bytes + i * ldoi_bytes + (int64_t)t * 16, hv);
}

// one wave per head, four heads per block, no barrier (a wave past the last head leaves at once)
template <int DT, class GAIN>
__global__ __launch_bounds__(256) void head_rmsnorm_generic(const void* __restrict__ x, int64_t ldxo, int64_t ldxi, const void* __restrict__ wgt, float eps, int64_t cols,
                                                            int64_t heads, int64_t n_inner, void* __restrict__ out, int64_t ldoo, int64_t ldoi) {
    using S = typename Elem<DT>::store_t;
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    const int lane = threadIdx.x & 63;
    const int64_t head = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (head >= heads) return;
    int64_t o, i;
    head_index(head, n_inner, o, i);
    const S* xr = reinterpret_cast<const S*>(x) + o * ldxo + i * ldxi;
    const S* wr = reinterpret_cast<const S*>(wgt);
    S* hr = reinterpret_cast<S*>(out) + o * ldoo + i * ldoi;
    const int64_t nvec = (cols + EPV - 1) / EPV;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};                   // N1-N2: vector v belongs to virtual lane v mod 256 = group (v / 64) mod 4, lane v mod 64
    for (int64_t base = 0; base < nvec; base += 256) {
#pragma unroll
        for (int gi = 0; gi < 4; ++gi) {
            const int64_t v = base + gi * 64 + lane;
            if (v < nvec) {
                for (int e = 0; e < EPV && v * EPV + e < cols; ++e) {
                    const float f = Elem<DT>::to_f32(xr[v * EPV + e]);
                    acc[gi] = __builtin_fmaf(f, f, acc[gi]);
                }
            }
        }
    }
    wave_sums(acc);                                            // N3
    const float rs = rms_rs(((acc[0] + acc[1]) + acc[2]) + acc[3], (int)cols, eps);
    for (int64_t c = lane; c < cols; c += 64) hr[c] = Elem<DT>::from_f32(GAIN::template h<DT>(Elem<DT>::to_f32(xr[c]), Elem<DT>::to_f32(wr[c]), rs));
}

// a stride that the kernel multiplies by an index that is always 0 does not have to be a whole number of vectors
static inline bool stride_vec_ok(int64_t ld, int64_t count, int64_t epv) { return count <= 1 || ld % epv == 0; }

template <int DT>
void head_rmsnorm_dispatch(const void* x, int64_t ld_xo, int64_t ld_xi, const void* wgt, float eps, int gain, int64_t n_outer, int64_t n_inner, int64_t cols, void* out,
                           int64_t ld_oo, int64_t ld_oi, hipStream_t st) {
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    const int64_t kb = Elem<DT>::kBytes, heads = n_outer * n_inner;
    const bool vec_ok = cols % EPV == 0 && cols * kb <= 1024 && aligned_to(x, 16) && aligned_to(wgt, 16) && aligned_to(out, 16) && stride_vec_ok(ld_xo, n_outer, EPV) &&
                        stride_vec_ok(ld_xi, n_inner, EPV) && stride_vec_ok(ld_oo, n_outer, EPV) && stride_vec_ok(ld_oi, n_inner, EPV);
    const auto with_gain = [&](auto f) {
        if (gain == PQ_GAIN_GEMMA) f(GemmaGain{});
        else f(LlamaGain{});
    };
    if (!vec_ok) {
        const dim3 grid((unsigned)((heads + 3) / 4));
        with_gain([&](auto g) {
            head_rmsnorm_generic<DT, decltype(g)><<<grid, dim3(256), 0, st>>>(x, ld_xo, ld_xi, wgt, eps, cols, heads, n_inner, out, ld_oo, ld_oi);
        });
        return;
    }
    const int nvec = (int)(cols / EPV);
    int g_lanes = 4;
    while (g_lanes < nvec) g_lanes <<= 1;
    const auto go = [&](auto gl) {
        constexpr int G = decltype(gl)::value;
        constexpr int64_t HPB = 4 * (64 / G);                  // heads per block
        const dim3 grid((unsigned)((heads + HPB - 1) / HPB));
        with_gain([&](auto g) {
            head_rmsnorm_vec<DT, G, decltype(g)><<<grid, dim3(256), 0, st>>>(row_bytes(x), ld_xo * kb, ld_xi * kb, row_bytes(wgt), eps, (int)cols, nvec, heads, n_inner,
                                                                            row_bytes(out), ld_oo * kb, ld_oi * kb);
        });
    };
    switch (g_lanes) {
        case 4: go(std::integral_constant<int, 4>{}); break;
        case 8: go(std::integral_constant<int, 8>{}); break;
        case 16: go(std::integral_constant<int, 16>{}); break;
        case 32: go(std::integral_constant<int, 32>{}); break;
        default: go(std::integral_constant<int, 64>{}); break;
    }
}

PQ_INSTANTIATE_DTYPES(head_rmsnorm_dispatch)

}  // namespace pq
