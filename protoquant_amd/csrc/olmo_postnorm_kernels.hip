// olmo_postnorm_kernels.hip — K1oq and its two shorter forms K1oa and K1on: the post-norm residual flow of OLMo-2 / OLMo-3 in one launch (QSPEC NO1-NO5, PO1, A1,
// Q1-Q6).  These decoders normalise the OUTPUT of a sublayer and nothing else: r1 = x + norm(attn(x)), out = r1 + norm(mlp(r1)).
//   p = OlmoRMSNorm(x; post_weight, post_eps)    cast_rne((f32(x) * rs) * f32(w)): binary32 throughout, ONE storage rounding, gain w     (NO1-NO5)
//   K1oq:  s = residual + p  STORED (A1; p itself NEVER stored: PO1), then Q1-Q6 on the rows of s AS STORED -> int8 codes + row scales
//   K1oa:  s = residual + p  STORED, nothing else (q == scale == nullptr: the end of a chain)
//   K1on:  p STORED to sum_out, nothing else (residual == nullptr as well: the norm alone, q_norm / k_norm)
// Algorithmic traffic for 16-bit rows: K1oq 7 B/elem (x and the residual read, s and the codes written; the weight row is cache-resident), K1oa 6, K1on 4.
// The gain (OlmoGain: NO5), the pinned order of the sum of squares (row_sum), rs (rms_rs), A1 (add_vec), the row layouts (rownorm_dispatch) and the second half of K1
// (reduce_and_encode) are the family's (rownorm_kernels.h).  There is ONE sum of squares and ONE weight row: what is quantised is the stored sum itself, not a second
// norm of it.  The row template stays this file's own, with its steps written out: its first half is K1pang's with another gain and an optional add, but as one
// __forceinline__ function for both, 72 of the 90 kernels here and 67 of K1pang's 87 compile to other instructions, and these kernels were not timed against their
// predecessors ("The RMS row kernels on one template").
// Aliasing: sum_out may be exactly x or exactly residual.  A row belongs to one wave or workgroup; rs needs the WHOLE of x, so every element of x is read (into
// registers; generic kernel: in a pass of its own, closed by a block barrier) before any element of s is written, and x is never read again once s is stored.
// Registers: x, the residual and post_weight are in flight together at the peak (3 vectors per slot; K1on 2); p takes x's place and post_weight's die, s takes p's
// place and the residual's die; the encode works on s in place — strictly less than K1pang holds.
#include "rownorm_kernels.h"
#include "pq_launch.h"

namespace pq {

// K1oq (ADD, QUANT) / K1oa (ADD; q and scale are null and never touched) / K1on (neither; res is null as well)
template <int DT, int VPT, int TPR, bool ADD, bool QUANT>
__global__ __launch_bounds__(256) void olmo_postnorm_rows(const uint8_t* x, int64_t ldx_bytes, const uint8_t* __restrict__ pwgt, float post_eps, const uint8_t* res,
                                                          int64_t ldr_bytes, uint8_t* sum_out, int64_t lds_bytes, int cols, int nvec, int64_t rows,
                                                          int8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale) {
    static_assert(ADD || !QUANT, "what is quantised is the stored sum");
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    constexpr int NACC = TPR == 64 ? 4 : 1;
    const int t = TPR == 256 ? threadIdx.x : threadIdx.x & 63;
    int64_t row = TPR == 256 ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool active = TPR == 256 || row < rows;          // TPR == 64: a wave past the last row walks a duplicate of the last row and stores nothing
    if constexpr (TPR == 64) row = active ? row : rows - 1;
    const uint8_t* xr = x + row * ldx_bytes;
    [[maybe_unused]] const uint8_t* rr = ADD ? res + row * ldr_bytes : nullptr;
    v4u sv[VPT];
    {
        // every load of x and of the residual is issued before the first use.  post_weight (cache-resident): one wave per row, with them; 256 threads per row, once
        // the lane's pass over x is done, while the row sum is under way (the order K1pang measured; DESIGN.md §4 has the registers of both)
        constexpr bool PW_FIRST = TPR == 64;
        [[maybe_unused]] v4u rv[ADD ? VPT : 1];
        v4u pv[VPT];
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int64_t off = clamped_vec_off(i * TPR + t, nvec);
            sv[i] = *reinterpret_cast<const v4u*>(xr + off);
            if constexpr (ADD) rv[i] = *reinterpret_cast<const v4u*>(rr + off);
            if constexpr (PW_FIRST) pv[i] = *reinterpret_cast<const v4u*>(pwgt + off);
        }
        float acc[NACC] = {};                   // NO2: this lane's vectors in increasing v, elements in order
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            if (i * TPR + t >= nvec) sv[i] = v4u{0u, 0u, 0u, 0u};      // past the row: fma(0, 0, acc) = acc
            float f[EPV];
            Unpack<DT, EPV>::run(sv[i], f);
#pragma unroll
            for (int j = 0; j < EPV; ++j) acc[i & (NACC - 1)] = __builtin_fmaf(f[j], f[j], acc[i & (NACC - 1)]);
        }
        if constexpr (!PW_FIRST) {
            pin_before_loads(sv);
#pragma unroll
            for (int i = 0; i < VPT; ++i) pv[i] = *reinterpret_cast<const v4u*>(pwgt + clamped_vec_off(i * TPR + t, nvec));
        }
        const float rs = rms_rs(row_sum<TPR>(acc), cols, post_eps);                                    // NO3, NO4
#pragma unroll
        for (int i = 0; i < VPT; ++i) sv[i] = OlmoGain::h_vec<DT>(sv[i], pv[i], rs);                        // NO5 / PO1: p, rounded to the storage dtype, takes the place of x
        if constexpr (ADD) {
#pragma unroll
            for (int i = 0; i < VPT; ++i) sv[i] = add_vec<DT>(sv[i], rv[i]);                           // A1: the sum takes the place of p
            // the whole sum exists, packed, before the first store and the first step of the amax: 256 threads per row (and one wave at 8 vectors) allocate fewer
            // registers so, one wave per row at 1 - 4 vectors fewer without
            if constexpr (TPR == 256 || VPT == 8) pin_before_loads(sv);
        }
    }
    [[maybe_unused]] uint32_t ab = 0;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int idx = i * TPR + t;
        if (active && idx < nvec) store_wt_b128(sum_out + row * lds_bytes + (int64_t)idx * 16, sv[i]);
        if constexpr (QUANT) {
            // a slot past the row holds (0 * rs) * w + a duplicate of the residual, and rs may be Inf or NaN: zeroed before the amax
            if (idx >= nvec) sv[i] = v4u{0u, 0u, 0u, 0u};
            ab = vec_amax_bits<DT>(sv[i], ab);
        }
    }
    if constexpr (QUANT) reduce_and_encode<DT, VPT, TPR>(sv, ab, t, nvec, active, row, q, ldq, scale);          // Q1-Q6 on s AS STORED
}

// generic path.  Pass 1 reads the whole of x (rs); the block barrier of its row sum closes it.  Pass 2 reads x, the residual and post_weight and stores s; every
// pass walks the elements in the SAME thread order, so a thread writes s[c] after it read x[c] and residual[c] itself, and the passes after it start from the stored
// s and never touch x or the residual again (either of them may BE sum_out).
template <int DT, bool ADD, bool QUANT>
__global__ __launch_bounds__(256) void olmo_postnorm_generic(const void* x, int64_t ldx, const void* __restrict__ pwgt, float post_eps, const void* res, int64_t ldr,
                                                             void* sum_out, int64_t lds, int64_t cols, int8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale) {
    static_assert(ADD || !QUANT, "what is quantised is the stored sum");
    using S = typename Elem<DT>::store_t;
    const int64_t row = blockIdx.x;
    const S* xr = reinterpret_cast<const S*>(x) + row * ldx;
    [[maybe_unused]] const S* rr = ADD ? reinterpret_cast<const S*>(res) + row * ldr : nullptr;
    S* sr = reinterpret_cast<S*>(sum_out) + row * lds;
    const S* pr = reinterpret_cast<const S*>(pwgt);
    float acc = 0.0f;
    walk_row<DT, true>(cols, [&](int64_t c) {
        const float f = Elem<DT>::to_f32(xr[c]);
        acc = __builtin_fmaf(f, f, acc);
    });
    const float rs = rms_rs(rms_block_sum(acc), (int)cols, post_eps);
    walk_row<DT, true>(cols, [&](int64_t c) {
        const S p = Elem<DT>::from_f32(OlmoGain::h<DT>(Elem<DT>::to_f32(xr[c]), Elem<DT>::to_f32(pr[c]), rs));      // NO5 / PO1
        if constexpr (ADD) sr[c] = add_elem<DT>(rr[c], p);                                                 // A1
        else sr[c] = p;
    });
    if constexpr (QUANT) {
        const S* in = sr;          // a thread reads back the sums it stored itself
        generic_amax_and_encode<DT, true>(row, cols, [&](int64_t c) -> S { return in[c]; }, q, ldq, scale, nullptr, 0);
    }
}

// res == nullptr: K1on (q and scale are null too); q == nullptr: K1oa (pq_api.hip refuses a partly-null group and q without res)
template <int DT>
void olmo_postnorm_add_quant_dispatch(const void* x, int64_t ldx, const void* pwgt, float post_eps, const void* res, int64_t ldr, void* sum_out, int64_t lds, int64_t rows,
                                      int64_t cols, int8_t* q, int64_t ldq, float* scale, hipStream_t st) {
    const int64_t kb = Elem<DT>::kBytes;
    const bool add = res != nullptr, quant = q != nullptr;
    // the form as two integral constants (ADD, QUANT), handed to f
    const auto with_form = [&](auto f) {
        if (quant) f(std::true_type{}, std::true_type{});
        else if (add) f(std::true_type{}, std::false_type{});
        else f(std::false_type{}, std::false_type{});
    };
    rownorm_dispatch<DT>(
        {{x, ldx}, {res, add ? ldr : 0}, {sum_out, lds}, {pwgt, 0}}, rows, cols, q, quant ? ldq : 0, nullptr, 0,
        [&](auto vpt, auto tpr, auto write_h, dim3 grid, int nvec) {
            if constexpr (!decltype(write_h)::value) {          // (there is no h_out: s is what is quantised, and it is stored)
                with_form([&](auto a, auto qn) {
                    olmo_postnorm_rows<DT, decltype(vpt)::value, decltype(tpr)::value, decltype(a)::value, decltype(qn)::value><<<grid, dim3(256), 0, st>>>(
                        row_bytes(x), ldx * kb, row_bytes(pwgt), post_eps, row_bytes(res), ldr * kb, row_bytes(sum_out), lds * kb, (int)cols, nvec, rows, q, ldq, scale);
                });
            }
        },
        [&](dim3 grid) {
            with_form([&](auto a, auto qn) {
                olmo_postnorm_generic<DT, decltype(a)::value, decltype(qn)::value><<<grid, dim3(256), 0, st>>>(x, ldx, pwgt, post_eps, res, ldr, sum_out, lds, cols, q, ldq, scale);
            });
        });
}

PQ_INSTANTIATE_DTYPES(olmo_postnorm_add_quant_dispatch)

}  // namespace pq
