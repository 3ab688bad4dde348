// rownorm_kernels.h — the kernels and the dispatch of the norm-into-quantisation family: a normalisation (optionally behind a residual add) fused into the
// per-token int8 quantisation, without the normalised activation ever going to HBM.
//   rmsnorm_quant_rows<.., ADD = false, LlamaGain>        K1n    RMSNorm(x; weight)          -> codes + row scales   (instantiated in producer_kernels.hip)
//   rmsnorm_quant_rows<.., ADD = true, LlamaGain>         K1a    s = x + residual (stored), then K1n on s            (addnorm_kernels.hip)
//   rmsnorm_quant_rows<.., ADD, GemmaGain>                K1ng / K1ang   the same with GemmaRMSNorm's gain 1 + w     (gemma_norm_kernels.hip, add_gemma_norm_kernels.hip)
//   rmsnorm_quant_rows<.., true, LlamaGain, QUANT, float> K1ma / K1mo    s = residual + cast(x * mult) (stored), then K1n on s / nothing more   (scaled_addnorm_kernels.hip)
//   layernorm_quant_rows<.., ADD = false>                 K1l    LayerNorm(x; weight, bias)  -> codes + row scales   (layernorm_kernels.hip)
//   layernorm_quant_rows<.., ADD = true>                  K1al   s = x + residual (stored), then K1l on s            (addlayernorm_kernels.hip)
// and one generic kernel per norm for ragged widths and unaligned operands.  The kernels are templates: a translation unit instantiates those that its
// *_quant_dispatch launches and no others, so each member of the family keeps an object file, and a register allocation, of its own.
// Row layouts (QSPEC N1-N3 / L2-L3 pin the ORDER of the row sums; the layout changes time only, never bits):
//   TPR = 256  one 256-thread block per row, 1-16 vectors of 16 bytes per thread.  The order of the specification IS this layout: vector v on lane v mod 256,
//              the xor butterfly per 64 lanes, the four wave sums left to right.
//   TPR = 64   short rows: one WAVE per row, four rows per block and no block barrier, like K1.  The wave plays all four 64-lane groups of the specification:
//              physical lane l holds the virtual lanes l, l + 64, l + 128, l + 192 (vector v = i * 64 + l belongs to virtual lane v mod 256 = (i mod 4) * 64 + l),
//              keeps one accumulator per group, runs the butterfly on each and adds the four sums left to right — the same float operations in the same order.
//              A wave past the last row walks a clamped duplicate of the last row and stores nothing.
// Aliasing.  Plain kernels: none; q, scale and h_out may not overlap x, the weight, the bias or each other (pq_api.hip refuses it).  ADD kernels: sum_out may be
// exactly x or exactly residual (same base, same leading dimension; pq_api.hip refuses every other overlap).  A row belongs to one wave or workgroup and a thread
// reads every element of x and of residual before it writes that element of the sum, so those three pointers carry no __restrict__ there.  Slots past the row's
// end load a clamped duplicate of the row's last vector, which another thread (or an in-place h_out) may be overwriting: they are zeroed before any use.
// Register allocation.  The bodies are the __global__ templates themselves (a wrapper around an inlined body costs up to 26 VGPRs), their helpers are
// __forceinline__ functions and not lambdas, and the row's arrays are declared in the order x / sum, residual, weight, bias: each of these decides whether hipcc
// gives a kernel the instruction stream it had as a kernel of its own (profiles/r17_rownorm_kernels.txt compares all 228 with their predecessors).  A template
// parameter that leaves an instantiation's body and kernel arguments as they were does not disturb it; a kernel argument added to it, or a step of its body moved
// into a helper, does (profiles/r24_rmsfold_kernels.txt; DESIGN.md §4, "The RMS row kernels on one template").
#pragma once
#include <initializer_list>

#include "addnorm_device.h"
#include "layernorm_device.h"

namespace pq {

// x may alias sum_out in the ADD kernels and nothing in the plain ones
template <bool ADD> using row_in_bytes = std::conditional_t<ADD, const uint8_t*, const uint8_t* __restrict__>;
template <bool ADD> using row_in_void = std::conditional_t<ADD, const void*, const void* __restrict__>;

// An empty statement that takes every vector of the row as an operand and clobbers memory: the loads written after it (the weight and bias rows) are issued after
// what is written before it.  K1a: after the adds, when the residual's registers are free — hipcc otherwise hoists them above the adds and holds x, the residual
// and the weight at once (16 vectors: 256 VGPRs + AGPRs).  K1l / K1al: after the first pass over the row has started, not above the loads of x.
template <int VPT>
__device__ __forceinline__ void pin_before_loads(v4u (&sv)[VPT]) {
#pragma unroll
    for (int i = 0; i < VPT; ++i) asm volatile("" : "+v"(sv[i]) : : "memory");
}

// byte offset of the vector in slot idx of a row of nvec vectors; a slot past the row's end loads a duplicate of the last vector (the loaded value is zeroed
// before any use)
__device__ __forceinline__ int64_t clamped_vec_off(int idx, int nvec) { return (int64_t)(idx < nvec ? idx : nvec - 1) * 16; }

// ---------------------------------------------------------------------------------------------------------------- the gains of the RMS norms
// What a norm does with x * rs and the weight, as a tag of the row kernels: h_vec on one 16-byte vector (two elements per instruction), h on one element (the caller
// rounds to the storage dtype).  A tag leaves the instructions of the instantiations that existed before it as they were (profiles/r24_rmsfold_kernels.txt).
// N5 (Llama): x * rs is rounded to the storage dtype BEFORE the gain w
struct LlamaGain {
    template <int DT> __device__ static __forceinline__ float h(float x, float w, float rs) { return rms_h<DT>(x, w, rs); }
    template <int DT> __device__ static __forceinline__ v4u h_vec(const v4u& xv, const v4u& wv, float rs) { return rms_h_vec<DT>(xv, wv, rs); }
};
// NG5 (Gemma, PLUS_ONE) and NO5 (OLMo): h = (x * rs) * g with g = 1 + w or w, every operation rounded in binary32 (the build has no contraction) and ONE storage
// rounding.  GemmaRMSNorm is ((x.float() * rs) * (1 + w.float())).type_as(x); OLMo's is the same without the `1 +`.
template <bool PLUS_ONE>
struct OneRoundingGain {
    template <int DT> __device__ static __forceinline__ float h(float x, float w, float rs) {
        const float g = PLUS_ONE ? 1.0f + w : w;
        return (x * rs) * g;
    }
    template <int DT> __device__ static __forceinline__ v4u h_vec(const v4u& xv, const v4u& wv, float rs) {
        v4u out;
        if constexpr (DT == PQ_F32) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t xb = xv[j], wb = wv[j];      // copies first (hipcc quirk with vector-element lvalues)
                out[j] = __builtin_bit_cast(uint32_t, h<DT>(__builtin_bit_cast(float, xb), __builtin_bit_cast(float, wb), rs));
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t xw = xv[j], ww = wv[j];
                if constexpr (PLUS_ONE) {
                    const v2f g = splat(1.0f) + Pair<DT>::unpack(ww);
                    out[j] = Pair<DT>::pack((Pair<DT>::unpack(xw) * splat(rs)) * g);
                } else {
                    out[j] = Pair<DT>::pack((Pair<DT>::unpack(xw) * splat(rs)) * Pair<DT>::unpack(ww));          // (the gain unpacked AFTER the product: hipcc keeps the order)
                }
            }
        }
        return out;
    }
};
struct GemmaGain : OneRoundingGain<true> {};
struct OlmoGain : OneRoundingGain<false> {};

// ---------------------------------------------------------------------------------------------------------------- the steps of a row kernel
// A step is a __forceinline__ function here only where a kernel that calls it compiles to the instructions it had with the step written out: hipcc schedules and
// allocates an inlined helper differently from the same statements in the kernel.  The two below are K1pang's.  rmsnorm_quant_rows, olmo_postnorm_rows and the
// first halves of the post-norm kernels keep their steps written out: DESIGN.md §4, "The RMS row kernels on one template", has what was tried and how many kernels
// each step changed.
// this lane's share of the sum of squares of a row held in registers (N2: vectors in increasing v, elements in order; slots past the row are zeroed first:
// fma(0, 0, acc) = acc), one accumulator per 64-lane group of the specification ("Row layouts")
template <int DT, int VPT, int TPR>
__device__ __forceinline__ void lane_sumsq(v4u (&sv)[VPT], int t, int nvec, float (&acc)[TPR == 64 ? 4 : 1]) {
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    constexpr int NACC = TPR == 64 ? 4 : 1;
#pragma unroll
    for (int gi = 0; gi < NACC; ++gi) acc[gi] = 0.0f;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        if (i * TPR + t >= nvec) sv[i] = v4u{0u, 0u, 0u, 0u};
        float f[EPV];
        Unpack<DT, EPV>::run(sv[i], f);
#pragma unroll
        for (int j = 0; j < EPV; ++j) acc[i & (NACC - 1)] = __builtin_fmaf(f[j], f[j], acc[i & (NACC - 1)]);
    }
}

// the row's sum from the lanes' accumulators (N3).  One wave per row: row_sum<64>'s butterfly with its loops written out, as K1pang always had it
template <int TPR>
__device__ __forceinline__ float rms_row_sum(float (&acc)[TPR == 64 ? 4 : 1]) {
    if constexpr (TPR == 64) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
            for (int gi = 0; gi < 4; ++gi) acc[gi] = acc[gi] + __shfl_xor(acc[gi], off, 64);
        }
        return ((acc[0] + acc[1]) + acc[2]) + acc[3];
    } else {
        return rms_block_sum(acc[0]);
    }
}

// the value of a kernel's optional multiplier argument (a pack of no or one float)
__device__ __forceinline__ float the_multiplier(float m) { return m; }

// K1n / K1a, K1ng / K1ang, K1ma / K1mo (QSPEC S1, A1, N1-N6 or NG1-NG6, Q1-Q6).  Reads x (and the residual) once and the weight vector from cache, writes 1 B/elem +
// 4 B/row (+ the sum, + h when asked for).  Registers at 16 vectors, ADD: x + residual + weight in flight (192), then sum + weight + h (192) — the plain kernel's budget.
// GAIN: what the norm does with x * rs and the weight.  MULT: empty, or `float` — then the kernel takes `float mult` after ldr_bytes and adds cast(x * mult) (S1) in x's
// place: the product takes the place of x before the add, so nothing more is live at the peak.  !QUANT: the add-only form, which stops after storing the sum (wgt, q,
// scale and h_out are null and never touched).  An argument that exists only in the instantiations that use it leaves the others their kernel arguments, and every
// instantiation the instructions it had as gemma_rmsnorm_quant_rows / scaled_add_rmsnorm_quant_rows or before GAIN, QUANT and MULT existed (profiles/r24_rmsfold_kernels.txt).
template <int DT, int VPT, int TPR, bool WRITE_H, bool ADD, class GAIN = LlamaGain, bool QUANT = true, class... MULT>
__global__ __launch_bounds__(256) void rmsnorm_quant_rows(row_in_bytes<ADD> x, int64_t ldx_bytes, const uint8_t* res, int64_t ldr_bytes, MULT... mult, uint8_t* sum_out,
                                                          int64_t lds_bytes, const uint8_t* __restrict__ wgt, float eps, int cols, int nvec, int64_t rows,
                                                          int8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale, uint8_t* __restrict__ h_out,
                                                          int64_t ldh_bytes) {
    constexpr bool SCALED = sizeof...(MULT) == 1;
    static_assert((SCALED || sizeof...(MULT) == 0) && (std::is_same_v<MULT, float> && ...), "MULT is empty or one float");
    static_assert(ADD || (QUANT && !SCALED), "the multiplier scales x in front of the add, and the add-only form stores the sum alone");
    static_assert(QUANT || !WRITE_H, "h is the normalised sum: the add-only form has none");
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    constexpr int NACC = TPR == 64 ? 4 : 1;
    const int t = TPR == 256 ? threadIdx.x : threadIdx.x & 63;
    int64_t row = TPR == 256 ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool active = TPR == 256 || row < rows;          // TPR == 64: a wave past the last row walks a duplicate of the last row and stores nothing
    if constexpr (TPR == 64) row = active ? row : rows - 1;
    const uint8_t* xr = x + row * ldx_bytes;
    [[maybe_unused]] const uint8_t* rr = ADD ? res + row * ldr_bytes : nullptr;
    v4u sv[VPT];
    if constexpr (ADD) {
        // every load of x and of the residual is issued before the first use
        v4u rv[VPT];
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int64_t off = clamped_vec_off(i * TPR + t, nvec);
            sv[i] = *reinterpret_cast<const v4u*>(xr + off);
            rv[i] = *reinterpret_cast<const v4u*>(rr + off);
        }
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            if constexpr (SCALED) sv[i] = add_vec<DT>(scale_vec<DT>(sv[i], the_multiplier(mult...)), rv[i]);          // S1, then A1
            else sv[i] = add_vec<DT>(sv[i], rv[i]);                                                                   // A1: the sum takes the place of x
        }
        if constexpr (QUANT) pin_before_loads(sv);
    }
    if constexpr (!QUANT) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int idx = i * TPR + t;
            if (active && idx < nvec) store_wt_b128(sum_out + row * lds_bytes + (int64_t)idx * 16, sv[i]);
        }
        return;
    }
    // the weight row (shared by every workgroup: cache-resident).  Plain: with x, every load before the first use.  ADD: asked for once the residual's registers
    // are free, and BEFORE the stores of the sum, so that waiting for it does not wait for them
    v4u wv[VPT];
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int64_t off = clamped_vec_off(i * TPR + t, nvec);
        if constexpr (!ADD) sv[i] = *reinterpret_cast<const v4u*>(xr + off);
        wv[i] = *reinterpret_cast<const v4u*>(wgt + off);
    }
    if constexpr (ADD) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int idx = i * TPR + t;
            if (active && idx < nvec) store_wt_b128(sum_out + row * lds_bytes + (int64_t)idx * 16, sv[i]);
        }
    }
    float acc[NACC] = {};                   // N2 (on s AS STORED): this lane's vectors in increasing v, elements in order
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        if (i * TPR + t >= nvec) sv[i] = v4u{0u, 0u, 0u, 0u};      // past the row: fma(0, 0, acc) = acc
        float f[EPV];
        Unpack<DT, EPV>::run(sv[i], f);
#pragma unroll
        for (int j = 0; j < EPV; ++j) acc[i & (NACC - 1)] = __builtin_fmaf(f[j], f[j], acc[i & (NACC - 1)]);
    }
    float ss;                               // N3
    if constexpr (TPR == 64) {
        // row_sum<64>'s butterfly, written out: through the helper (which takes the accumulators by reference, as the LayerNorm kernels always did) hipcc orders
        // and allocates the 4- and 8-vector kernels differently, and K1a measured 1-2 % slower at those widths (profiles/r17_rownorm_ab.txt)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
            for (int gi = 0; gi < 4; ++gi) acc[gi] = acc[gi] + __shfl_xor(acc[gi], off, 64);
        }
        ss = ((acc[0] + acc[1]) + acc[2]) + acc[3];
    } else {
        ss = rms_block_sum(acc[0]);
    }
    const float rs = rms_rs(ss, cols, eps);                        // N4
    v4u hv[VPT];
    uint32_t ab = 0;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int idx = i * TPR + t;
        // a slot past the row holds a duplicate of the weight's last vector and rs may be Inf or NaN: its h is zero, not 0 * Inf = NaN (which would be the row's
        // amax).  Zeroed AFTER the arithmetic: selecting before it costs K1ng's 4-vector wave layout four VGPRs and a wave per SIMD (profiles/r22_k1n_dead_slots.txt has
        // the registers and the times of both forms)
        hv[i] = GAIN::template h_vec<DT>(sv[i], wv[i], rs);
        if (idx >= nvec) hv[i] = v4u{0u, 0u, 0u, 0u};
        ab = vec_amax_bits<DT>(hv[i], ab);
        if constexpr (WRITE_H) {
            if (active && idx < nvec) store_wt_b128(h_out + row * ldh_bytes + (int64_t)idx * 16, hv[i]);
        }
    }
    reduce_and_encode<DT, VPT, TPR>(hv, ab, t, nvec, active, row, q, ldq, scale);
}

// K1l / K1al (QSPEC A1, L1-L6, Q1-Q6).  The row sits in registers (packed, as loaded), so mean and variance are a true two-pass computation at no extra traffic:
// L2 sums x, L3 sums (x - mean)^2 with the differences recomputed from the packed row (one subtraction per element instead of 32 more registers per vector pair).
// Registers at 16 vectors: (ADD: x + residual in flight (128), the residual's die at the add, then) x (64) + weight (64) + bias (64); h takes the place of x.
template <int DT, int VPT, int TPR, bool WRITE_H, bool ADD>
__global__ __launch_bounds__(256) void layernorm_quant_rows(row_in_bytes<ADD> x, int64_t ldx_bytes, const uint8_t* res, int64_t ldr_bytes, uint8_t* sum_out,
                                                            int64_t lds_bytes, const uint8_t* __restrict__ wgt, const uint8_t* __restrict__ bias, float eps,
                                                            int cols, int nvec, int64_t rows, int8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale,
                                                            uint8_t* __restrict__ h_out, int64_t ldh_bytes) {
    constexpr int NACC = TPR == 64 ? 4 : 1;
    const int t = TPR == 256 ? threadIdx.x : threadIdx.x & 63;
    int64_t row = TPR == 256 ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool active = TPR == 256 || row < rows;          // TPR == 64: a wave past the last row walks a duplicate of the last row and stores nothing
    if constexpr (TPR == 64) row = active ? row : rows - 1;
    const uint8_t* xr = x + row * ldx_bytes;
    [[maybe_unused]] const uint8_t* rr = ADD ? res + row * ldr_bytes : nullptr;
    const bool has_bias = bias != nullptr;
    v4u xv[VPT];
    // every load of x (and of the residual) is issued before the first use
    if constexpr (ADD) {
        v4u rv[VPT];
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int64_t off = clamped_vec_off(i * TPR + t, nvec);
            xv[i] = *reinterpret_cast<const v4u*>(xr + off);
            rv[i] = *reinterpret_cast<const v4u*>(rr + off);
        }
#pragma unroll
        for (int i = 0; i < VPT; ++i) xv[i] = add_vec<DT>(xv[i], rv[i]);          // A1: the sum takes the place of x
    } else {
#pragma unroll
        for (int i = 0; i < VPT; ++i) xv[i] = *reinterpret_cast<const v4u*>(xr + clamped_vec_off(i * TPR + t, nvec));
    }
    float acc[NACC] = {};                   // L2 (on s AS STORED): this lane's vectors in increasing v, elements in order
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        if (i * TPR + t >= nvec) xv[i] = v4u{0u, 0u, 0u, 0u};      // past the row: acc + 0 = acc
        acc[i & (NACC - 1)] = ln_sum_vec<DT>(xv[i], acc[i & (NACC - 1)]);
    }
    pin_before_loads(xv);
    // the weight and bias rows (shared by every workgroup: cache-resident) are asked for while the first reduction is under way (ADD: once the residual's
    // registers are free, and BEFORE the stores of the sum, so that waiting for them does not wait for the stores)
    v4u wv[VPT], bv[VPT];
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int64_t off = clamped_vec_off(i * TPR + t, nvec);
        wv[i] = *reinterpret_cast<const v4u*>(wgt + off);
        bv[i] = has_bias ? *reinterpret_cast<const v4u*>(bias + off) : v4u{0u, 0u, 0u, 0u};
    }
    if constexpr (ADD) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int idx = i * TPR + t;
            if (active && idx < nvec) store_wt_b128(sum_out + row * lds_bytes + (int64_t)idx * 16, xv[i]);
        }
    }
    const float mean = ln_mean(row_sum<TPR>(acc), cols);           // L2
#pragma unroll
    for (int gi = 0; gi < NACC; ++gi) acc[gi] = 0.0f;              // L3
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        if (i * TPR + t < nvec) acc[i & (NACC - 1)] = ln_ssd_vec<DT>(xv[i], mean, acc[i & (NACC - 1)]);
    }
    if constexpr (TPR == 256) __syncthreads();                     // row_sum<256>'s four partial sums are one array: everyone has read the first sum
    const float rs = rms_rs(row_sum<TPR>(acc), cols, eps);         // L3, L4
    v4u hv[VPT];
    uint32_t ab = 0;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int idx = i * TPR + t;
        hv[i] = idx < nvec ? ln_h_vec<DT>(xv[i], wv[i], bv[i], mean, rs, has_bias) : v4u{0u, 0u, 0u, 0u};
        ab = vec_amax_bits<DT>(hv[i], ab);
        if constexpr (WRITE_H) {
            if (active && idx < nvec) store_wt_b128(h_out + row * ldh_bytes + (int64_t)idx * 16, hv[i]);
        }
    }
    reduce_and_encode<DT, VPT, TPR>(hv, ab, t, nvec, active, row, q, ldq, scale);
}

// ---------------------------------------------------------------------------------------------------------------- generic path
// Ragged widths, unaligned pointers, odd leading dimensions: one 256-thread block per row, the same lane layout walked element by element.
// walk_row calls f(c) for this thread's columns c.  BY_VECTOR: in the order of the specification (vector v on thread v mod 256, its elements in order) — the order
// of the row sums, and the one in which a thread meets exactly the elements it met in every other pass.  Otherwise element by element, 256 apart.
template <int DT, bool BY_VECTOR, class F>
__device__ __forceinline__ void walk_row(int64_t cols, F f) {
    if constexpr (BY_VECTOR) {
        constexpr int EPV = 16 / Elem<DT>::kBytes;
        const int64_t nvec = (cols + EPV - 1) / EPV;
        for (int64_t v = threadIdx.x; v < nvec; v += 256)
            for (int e = 0; e < EPV && v * EPV + e < cols; ++e) f(v * EPV + e);
    } else {
        for (int64_t c = threadIdx.x; c < cols; c += 256) f(c);
    }
}

// the tail of both generic kernels (Q1-Q6): the row amax of h = h_at(c), the scale, and the codes from h recomputed in a second walk
template <int DT, bool BY_VECTOR, class H>
__device__ __forceinline__ void generic_amax_and_encode(int64_t row, int64_t cols, H h_at, int8_t* q, int64_t ldq, float* scale, void* h_out, int64_t ldh) {
    using S = typename Elem<DT>::store_t;
    float amax = 0.0f;
    walk_row<DT, BY_VECTOR>(cols, [&](int64_t c) {
        const S h = h_at(c);
        if (h_out) reinterpret_cast<S*>(h_out)[row * ldh + c] = h;
        amax = amax_step(amax, Elem<DT>::to_f32(h));
    });
    amax = wave_max(amax);
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = amax;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) amax = amax_merge(amax, part[w]);
    const float s = scale_of(amax);
    if (threadIdx.x == 0) scale[row] = s;
    int8_t* qr = q + row * ldq;
    walk_row<DT, BY_VECTOR>(cols, [&](int64_t c) { qr[c] = (int8_t)code_of(Elem<DT>::to_f32(h_at(c)), s); });
}

// ADD: every pass walks the elements in the SAME thread order, so a thread only ever reads back the sums it stored itself: the first pass reads x and the residual
// and stores s, the others start from the stored s and never touch x or the residual again (either of them may BE sum_out).
template <int DT, bool ADD, class GAIN = LlamaGain, bool QUANT = true, class... MULT>
__global__ __launch_bounds__(256) void rmsnorm_quant_generic(row_in_void<ADD> x, int64_t ldx, const void* res, int64_t ldr, MULT... mult, void* sum_out, int64_t lds,
                                                             const void* __restrict__ wgt, float eps, int64_t cols, int8_t* __restrict__ q, int64_t ldq,
                                                             float* __restrict__ scale, void* __restrict__ h_out, int64_t ldh) {
    constexpr bool SCALED = sizeof...(MULT) == 1;
    static_assert(ADD || (QUANT && !SCALED), "the multiplier scales x in front of the add, and the add-only form stores the sum alone");
    using S = typename Elem<DT>::store_t;
    const int64_t row = blockIdx.x;
    const S* xr = reinterpret_cast<const S*>(x) + row * ldx;
    const S* rr = reinterpret_cast<const S*>(res) + row * ldr;
    S* sr = reinterpret_cast<S*>(sum_out) + row * lds;
    float acc = 0.0f;
    walk_row<DT, true>(cols, [&](int64_t c) {
        S s;
        if constexpr (SCALED) s = add_elem<DT>(rr[c], scale_elem<DT>(xr[c], the_multiplier(mult...)));          // S1, A1
        else s = ADD ? add_elem<DT>(rr[c], xr[c]) : xr[c];
        if constexpr (ADD) sr[c] = s;
        if constexpr (QUANT) {
            const float f = Elem<DT>::to_f32(s);
            acc = __builtin_fmaf(f, f, acc);
        }
    });
    if constexpr (QUANT) {
        const S* wr = reinterpret_cast<const S*>(wgt);
        const S* in = ADD ? sr : xr;            // what is normalised
        const float rs = rms_rs(rms_block_sum(acc), (int)cols, eps);
        generic_amax_and_encode<DT, ADD>(
            row, cols, [&](int64_t c) -> S { return Elem<DT>::from_f32(GAIN::template h<DT>(Elem<DT>::to_f32(in[c]), Elem<DT>::to_f32(wr[c]), rs)); }, q, ldq, scale, h_out,
            ldh);
    }
}

// the row is read three times (from cache after the first)
template <int DT, bool ADD>
__global__ __launch_bounds__(256) void layernorm_quant_generic(row_in_void<ADD> x, int64_t ldx, const void* res, int64_t ldr, void* sum_out, int64_t lds,
                                                               const void* __restrict__ wgt, const void* __restrict__ bias, float eps, int64_t cols,
                                                               int8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale, void* __restrict__ h_out,
                                                               int64_t ldh) {
    using S = typename Elem<DT>::store_t;
    const int64_t row = blockIdx.x;
    const S* xr = reinterpret_cast<const S*>(x) + row * ldx;
    const S* rr = reinterpret_cast<const S*>(res) + row * ldr;
    S* sr = reinterpret_cast<S*>(sum_out) + row * lds;
    const S* wr = reinterpret_cast<const S*>(wgt);
    const S* br = reinterpret_cast<const S*>(bias);
    const bool has_bias = bias != nullptr;
    const S* in = ADD ? sr : xr;            // what is normalised
    float acc = 0.0f;
    walk_row<DT, true>(cols, [&](int64_t c) {
        const S s = ADD ? add_elem<DT>(rr[c], xr[c]) : xr[c];
        if constexpr (ADD) sr[c] = s;
        acc = acc + Elem<DT>::to_f32(s);
    });
    const float mean = ln_mean(rms_block_sum(acc), (int)cols);
    acc = 0.0f;
    walk_row<DT, true>(cols, [&](int64_t c) {
        const float d = Elem<DT>::to_f32(in[c]) - mean;
        acc = __builtin_fmaf(d, d, acc);
    });
    __syncthreads();
    const float rs = rms_rs(rms_block_sum(acc), (int)cols, eps);
    generic_amax_and_encode<DT, ADD>(
        row, cols,
        [&](int64_t c) -> S {
            return Elem<DT>::from_f32(ln_h(Elem<DT>::to_f32(in[c]), mean, rs, Elem<DT>::to_f32(wr[c]), has_bias ? Elem<DT>::to_f32(br[c]) : 0.0f, has_bias));
        },
        q, ldq, scale, h_out, ldh);
}

// ---------------------------------------------------------------------------------------------------------------- dispatch (host)
// an operand that is read or written in 16-byte vectors: its base and its leading dimension in elements (0: one vector shared by every row; null: absent)
struct RowOperand {
    const void* p;
    int64_t ld;
};

// The layout decision of the family, once.  Vector path: the width and every leading dimension whole vectors, every operand 16-byte aligned (the codes: a
// vector's worth of them), at most 256 x 16 vectors; anything else is generic().  One wave per row up to PQ_RMS_WAVE_MAX vectors (default 256: 2048 16-bit
// elements; VPT in {1, 2, 4, 8} keeps i & 3 meaningful), else 256 threads x 1 .. 16 vectors (up to 4096 vectors = 32 768 16-bit elements).  Round 1 used the wave
// layout up to 512 vectors (a 4096-wide bf16 hidden state): 118 VGPRs, 4 waves per SIMD.  Measured in round 2 (profiles/r02_k1n_layout.txt): at 512 vectors the
// 256-thread block per row (2 vectors per thread, ~44 VGPRs) is 10 % faster at 4096 rows (15.7 -> 14.2 us) and equal at 16384; at 256 vectors the wave layout
// wins (8.7 vs 9.6 us).
// launch(VPT, TPR, WRITE_H as integral constants, grid, nvec) launches the row kernel; generic(grid) the generic one; blocks are 256 threads.
template <int DT, class Launch, class Generic>
static void rownorm_dispatch(std::initializer_list<RowOperand> operands, int64_t rows, int64_t cols, const int8_t* q, int64_t ldq, const void* h_out, int64_t ldh,
                             Launch&& launch, Generic&& generic) {
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    bool vec_ok = (cols % EPV == 0) && (ldq % EPV == 0) && aligned_to(q, EPV) && cols / EPV <= 256 * 16 && (!h_out || ((ldh % EPV == 0) && aligned_to(h_out, 16)));
    for (const RowOperand& o : operands) vec_ok = vec_ok && (o.ld % EPV == 0) && aligned_to(o.p, 16);
    if (!vec_ok) {
        generic(dim3((unsigned)rows));
        return;
    }
    const int nvec = (int)(cols / EPV);
    const bool wave = nvec <= opt().rms_wave_max;
    int vpt = 1;
    while (vpt * (wave ? 64 : 256) < nvec) vpt <<= 1;
    auto with_vpt = [&](auto tpr) {
        constexpr int TPR = decltype(tpr)::value;
        const dim3 grid((unsigned)((rows + 256 / TPR - 1) / (256 / TPR)));
        auto go = [&](auto v) {
            if (h_out) launch(v, tpr, std::true_type{}, grid, nvec);
            else launch(v, tpr, std::false_type{}, grid, nvec);
        };
        switch (vpt) {
            case 1: go(std::integral_constant<int, 1>{}); break;
            case 2: go(std::integral_constant<int, 2>{}); break;
            case 4: go(std::integral_constant<int, 4>{}); break;
            case 8: go(std::integral_constant<int, 8>{}); break;
            default:
                if constexpr (TPR == 256) go(std::integral_constant<int, 16>{});
                break;
        }
    };
    if (wave) with_vpt(std::integral_constant<int, 64>{});
    else with_vpt(std::integral_constant<int, 256>{});
}

// the three explicit instantiations of a dispatcher that pq_launch.h declares per dtype; the signature is that declaration's
#define PQ_INSTANTIATE_DTYPES(fn)                     \
    template decltype(fn<PQ_BF16>) fn<PQ_BF16>;       \
    template decltype(fn<PQ_FP16>) fn<PQ_FP16>;       \
    template decltype(fn<PQ_F32>) fn<PQ_F32>;

// an operand as the row kernels take it: its base as bytes (the leading dimension goes with it, times Elem<DT>::kBytes)
static inline const uint8_t* row_bytes(const void* p) { return reinterpret_cast<const uint8_t*>(p); }
static inline uint8_t* row_bytes(void* p) { return reinterpret_cast<uint8_t*>(p); }

// rownorm_dispatch for an entry whose quantisation group (weight, q, scale, h_out) is absent as a whole in its add-only form (pq_api.hip refuses a partly-null
// group): launch and generic get QUANT as one more integral constant in front of the grid, and the add-only form has no h_out
template <int DT, class Launch, class Generic>
static void rownorm_dispatch_quant_or_sum(std::initializer_list<RowOperand> operands, int64_t rows, int64_t cols, bool quant, const int8_t* q, int64_t ldq,
                                          const void* h_out, int64_t ldh, Launch&& launch, Generic&& generic) {
    rownorm_dispatch<DT>(
        operands, rows, cols, quant ? q : nullptr, quant ? ldq : 0, quant ? h_out : nullptr, quant ? ldh : 0,
        [&](auto vpt, auto tpr, auto write_h, dim3 grid, int nvec) {
            if (quant) launch(vpt, tpr, write_h, std::true_type{}, grid, nvec);
            else if constexpr (!decltype(write_h)::value) launch(vpt, tpr, write_h, std::false_type{}, grid, nvec);
        },
        [&](dim3 grid) {
            if (quant) generic(std::true_type{}, grid);
            else generic(std::false_type{}, grid);
        });
}

// K1n / K1a / K1ng / K1ang / K1ma: the dispatch of rmsnorm_quant_rows / rmsnorm_quant_generic<.., ADD, GAIN, QUANT, MULT...> (!ADD: res and sum_out are null, their
// leading dimensions 0).  SUM_ONLY_FORM: the entry has an add-only form, wgt == nullptr (K1mo), and its object the kernels of it; mult: the multiplier of K1ma / K1mo
template <int DT, bool ADD, class GAIN, bool SUM_ONLY_FORM = false, class... MULT>
static void rmsnorm_rows_dispatch(const void* x, int64_t ldx, const void* res, int64_t ldr, void* sum_out, int64_t lds, const void* wgt, float eps, int64_t rows,
                                  int64_t cols, int8_t* q, int64_t ldq, float* scale, void* h_out, int64_t ldh, hipStream_t st, MULT... mult) {
    const int64_t kb = Elem<DT>::kBytes;
    rownorm_dispatch_quant_or_sum<DT>(
        {{x, ldx}, {res, ldr}, {sum_out, lds}, {wgt, 0}}, rows, cols, !SUM_ONLY_FORM || wgt != nullptr, q, ldq, h_out, ldh,
        [&](auto vpt, auto tpr, auto write_h, auto quant, dim3 grid, int nvec) {
            constexpr bool QUANT = !SUM_ONLY_FORM || decltype(quant)::value;
            rmsnorm_quant_rows<DT, decltype(vpt)::value, decltype(tpr)::value, decltype(write_h)::value, ADD, GAIN, QUANT, MULT...><<<grid, dim3(256), 0, st>>>(
                row_bytes(x), ldx * kb, row_bytes(res), ldr * kb, mult..., row_bytes(sum_out), lds * kb, row_bytes(wgt), eps, (int)cols, nvec, rows, q, ldq, scale,
                row_bytes(h_out), ldh * kb);
        },
        [&](auto quant, dim3 grid) {
            constexpr bool QUANT = !SUM_ONLY_FORM || decltype(quant)::value;
            rmsnorm_quant_generic<DT, ADD, GAIN, QUANT, MULT...><<<grid, dim3(256), 0, st>>>(x, ldx, res, ldr, mult..., sum_out, lds, wgt, eps, cols, q, ldq, scale, h_out, ldh);
        });
}

}  // namespace pq
