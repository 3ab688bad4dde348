// addnorm_kernels.hip — K1a: the residual add fused into RMSNorm + per-token int8 quantisation (QSPEC A1, then N1-N6 and Q1-Q6):
//   s = x + residual  (stored: the new residual stream)  ->  RMSNorm(s; weight)  ->  int8 codes + row scales   (+ the normalised activation when asked for)
// One kernel where a decoder layer ran a torch add and K1n: the residual stream is written once and normalised from the registers that hold it, instead of being
// written by one kernel and read straight back by the next.  Algorithmic traffic: read 2 x elem bytes, write elem bytes + 1 B/elem + 4 B/row (7 B/elem for 16-bit
// rows against 9 for the pair).
// The skeleton and the three row layouts are K1n's (producer_kernels.hip); the device helpers are CALLED from producer_device.h — the pinned summation order
// N1-N3 exists once — and the kernels here are templates of their own in an object file of their own, so the register allocation of K1s / K1n does not depend on
// this file.
// Aliasing: sum_out may be exactly x or exactly residual (same base, same leading dimension; pq_api.hip refuses every other overlap).  A row belongs to one wave
// or workgroup and a thread reads every element of x and of residual before it writes that element of the sum; the three pointers carry no __restrict__.  Slots
// past the row's end (and the rows of inactive waves) load a clamped duplicate that another thread may be overwriting: they are zeroed before any use.
#include "addnorm_device.h"

namespace pq {

// An empty statement that takes every sum as an operand and clobbers memory: the loads written after it (the weight row) are issued after the adds, when the
// residual's registers are free — hipcc otherwise hoists them above the adds and holds x, the residual and the weight at once (16 vectors: 256 VGPRs + AGPRs).
template <int VPT>
__device__ __forceinline__ void pin_before_loads(v4u (&sv)[VPT]) {
#pragma unroll
    for (int i = 0; i < VPT; ++i) asm volatile("" : "+v"(sv[i]) : : "memory");
}

// 256 threads per row, 1-16 vectors per thread.  Registers at 16 vectors: x + residual + weight in flight (192), then sum + weight + h (192) — K1n's budget.
template <int DT, int VPT, bool WRITE_H>
__global__ __launch_bounds__(256) void add_rmsnorm_quant_vec(const uint8_t* x, int64_t ldx_bytes, const uint8_t* res, int64_t ldr_bytes, uint8_t* sum_out,
                                                             int64_t lds_bytes, const uint8_t* __restrict__ wgt, float eps, int cols, int nvec,
                                                             int8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale, uint8_t* __restrict__ h_out,
                                                             int64_t ldh_bytes) {
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x;
    const uint8_t* xr = x + row * ldx_bytes;
    const uint8_t* rr = res + row * ldr_bytes;
    v4u sv[VPT];
    {
        // every load of x and of the residual is issued before the first use; the sum takes the place of x
        v4u rv[VPT];
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int idx = i * 256 + t;
            const int64_t off = (int64_t)(idx < nvec ? idx : nvec - 1) * 16;
            sv[i] = *reinterpret_cast<const v4u*>(xr + off);
            rv[i] = *reinterpret_cast<const v4u*>(rr + off);
        }
#pragma unroll
        for (int i = 0; i < VPT; ++i) sv[i] = add_vec<DT>(sv[i], rv[i]);
    }
    pin_before_loads(sv);
    // the weight row (shared by every workgroup: cache-resident) is asked for once the residual's registers are free, and BEFORE the stores of the sum, so that
    // waiting for it does not wait for them
    v4u wv[VPT];
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int idx = i * 256 + t;
        wv[i] = *reinterpret_cast<const v4u*>(wgt + (int64_t)(idx < nvec ? idx : nvec - 1) * 16);
    }
    float acc = 0.0f;                       // N2 on s AS STORED: this lane's vectors in increasing v, elements in order
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int idx = i * 256 + t;
        if (idx < nvec) store_wt_b128(sum_out + row * lds_bytes + (int64_t)idx * 16, sv[i]);
    }
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        if (i * 256 + t >= nvec) sv[i] = v4u{0u, 0u, 0u, 0u};      // past the row: fma(0, 0, acc) = acc
        float f[EPV];
        Unpack<DT, EPV>::run(sv[i], f);
#pragma unroll
        for (int j = 0; j < EPV; ++j) acc = __builtin_fmaf(f[j], f[j], acc);
    }
    const float rs = rms_rs(rms_block_sum(acc), cols, eps);        // N3, N4
    v4u hv[VPT];
    uint32_t ab = 0;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        hv[i] = rms_h_vec<DT>(sv[i], wv[i], rs);
        ab = vec_amax_bits<DT>(hv[i], ab);
        if constexpr (WRITE_H) {
            const int idx = i * 256 + t;
            if (idx < nvec) store_wt_b128(h_out + row * ldh_bytes + (int64_t)idx * 16, hv[i]);
        }
    }
    reduce_and_encode<DT, VPT, 256>(hv, ab, t, nvec, true, row, q, ldq, scale);
}

// Short rows: one WAVE per row, four rows per block and no block barrier, as rmsnorm_quant_wave — physical lane l holds the virtual lanes l, l + 64, l + 128,
// l + 192 of the specification, one accumulator per group, the xor butterfly on each, the four sums left to right: the same float operations in the same order.
template <int DT, int VPT, bool WRITE_H>
__global__ __launch_bounds__(256) void add_rmsnorm_quant_wave(const uint8_t* x, int64_t ldx_bytes, const uint8_t* res, int64_t ldr_bytes, uint8_t* sum_out,
                                                              int64_t lds_bytes, const uint8_t* __restrict__ wgt, float eps, int cols, int nvec, int64_t rows,
                                                              int8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale, uint8_t* __restrict__ h_out,
                                                              int64_t ldh_bytes) {
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    const int t = threadIdx.x & 63;
    int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool active = row < rows;
    row = active ? row : rows - 1;
    const uint8_t* xr = x + row * ldx_bytes;
    const uint8_t* rr = res + row * ldr_bytes;
    v4u sv[VPT];
    {
        v4u rv[VPT];
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int idx = i * 64 + t;
            const int64_t off = (int64_t)(idx < nvec ? idx : nvec - 1) * 16;
            sv[i] = *reinterpret_cast<const v4u*>(xr + off);
            rv[i] = *reinterpret_cast<const v4u*>(rr + off);
        }
#pragma unroll
        for (int i = 0; i < VPT; ++i) sv[i] = add_vec<DT>(sv[i], rv[i]);
    }
    pin_before_loads(sv);
    v4u wv[VPT];
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int idx = i * 64 + t;
        wv[i] = *reinterpret_cast<const v4u*>(wgt + (int64_t)(idx < nvec ? idx : nvec - 1) * 16);
    }
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int idx = i * 64 + t;
        if (active && idx < nvec) store_wt_b128(sum_out + row * lds_bytes + (int64_t)idx * 16, sv[i]);
    }
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        if (i * 64 + t >= nvec) sv[i] = v4u{0u, 0u, 0u, 0u};
        float f[EPV];
        Unpack<DT, EPV>::run(sv[i], f);
#pragma unroll
        for (int j = 0; j < EPV; ++j) acc[i & 3] = __builtin_fmaf(f[j], f[j], acc[i & 3]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int gi = 0; gi < 4; ++gi) acc[gi] = acc[gi] + __shfl_xor(acc[gi], off, 64);
    }
    const float rs = rms_rs(((acc[0] + acc[1]) + acc[2]) + acc[3], cols, eps);
    v4u hv[VPT];
    uint32_t ab = 0;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        hv[i] = rms_h_vec<DT>(sv[i], wv[i], rs);
        ab = vec_amax_bits<DT>(hv[i], ab);
        if constexpr (WRITE_H) {
            const int idx = i * 64 + t;
            if (active && idx < nvec) store_wt_b128(h_out + row * ldh_bytes + (int64_t)idx * 16, hv[i]);
        }
    }
    reduce_and_encode<DT, VPT, 64>(hv, ab, t, nvec, active, row, q, ldq, scale);
}

// generic path (ragged widths, unaligned pointers, odd leading dimensions): the same lane layout walked element by element.  All three passes walk the elements
// in the SAME thread order (vector v of the specification on thread v mod 256), so a thread only ever reads back the sums it stored itself: the first pass reads
// x and the residual and stores s, the other two start from the stored s and never touch x or the residual again (either of them may BE sum_out).
template <int DT>
__global__ __launch_bounds__(256) void add_rmsnorm_quant_generic(const void* x, int64_t ldx, const void* res, int64_t ldr, void* sum_out, int64_t lds,
                                                                 const void* __restrict__ wgt, float eps, int64_t cols, int8_t* __restrict__ q, int64_t ldq,
                                                                 float* __restrict__ scale, void* __restrict__ h_out, int64_t ldh) {
    using S = typename Elem<DT>::store_t;
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    const int64_t row = blockIdx.x;
    const S* xr = reinterpret_cast<const S*>(x) + row * ldx;
    const S* rr = reinterpret_cast<const S*>(res) + row * ldr;
    S* sr = reinterpret_cast<S*>(sum_out) + row * lds;
    const S* wr = reinterpret_cast<const S*>(wgt);
    const int64_t nvec = (cols + EPV - 1) / EPV;
    float acc = 0.0f;
    for (int64_t v = threadIdx.x; v < nvec; v += 256)
        for (int e = 0; e < EPV && v * EPV + e < cols; ++e) {
            const int64_t c = v * EPV + e;
            const S s = Elem<DT>::from_f32(Elem<DT>::to_f32(rr[c]) + Elem<DT>::to_f32(xr[c]));      // A1
            sr[c] = s;
            const float f = Elem<DT>::to_f32(s);
            acc = __builtin_fmaf(f, f, acc);
        }
    const float rs = rms_rs(rms_block_sum(acc), (int)cols, eps);
    auto h_at = [&](int64_t c) -> S { return Elem<DT>::from_f32(rms_h<DT>(Elem<DT>::to_f32(sr[c]), Elem<DT>::to_f32(wr[c]), rs)); };
    float amax = 0.0f;
    for (int64_t v = threadIdx.x; v < nvec; v += 256)
        for (int e = 0; e < EPV && v * EPV + e < cols; ++e) {
            const int64_t c = v * EPV + e;
            const S h = h_at(c);
            if (h_out) reinterpret_cast<S*>(h_out)[row * ldh + c] = h;
            amax = amax_step(amax, Elem<DT>::to_f32(h));
        }
    amax = wave_max(amax);
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = amax;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) amax = amax_merge(amax, part[w]);
    const float s = scale_of(amax);
    if (threadIdx.x == 0) scale[row] = s;
    int8_t* qr = q + row * ldq;
    for (int64_t v = threadIdx.x; v < nvec; v += 256)
        for (int e = 0; e < EPV && v * EPV + e < cols; ++e) {
            const int64_t c = v * EPV + e;
            qr[c] = (int8_t)code_of(Elem<DT>::to_f32(h_at(c)), s);
        }
}

static inline bool addnorm_aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// Row layouts as rmsnorm_quant_dispatch: one wave per row up to PQ_RMS_WAVE_MAX vectors (default 256: 2048 16-bit elements), else 256 threads x 1 .. 16 vectors
// (up to 4096 vectors = 32 768 16-bit elements); anything else — ragged width, unaligned pointer or leading dimension of x, the residual, the sum, the codes or
// h — is generic.  The choice changes time only, never bits.
template <int DT>
void add_rmsnorm_quant_dispatch(const void* x, int64_t ldx, const void* res, int64_t ldr, void* sum_out, int64_t lds, const void* wgt, float eps, int64_t rows,
                                int64_t cols, int8_t* q, int64_t ldq, float* scale, void* h_out, int64_t ldh, hipStream_t st) {
    constexpr int EPV = 16 / Elem<DT>::kBytes;
    const bool vec_ok = (cols % EPV == 0) && (ldx % EPV == 0) && (ldr % EPV == 0) && (lds % EPV == 0) && addnorm_aligned_to(x, 16) && addnorm_aligned_to(res, 16) &&
                        addnorm_aligned_to(sum_out, 16) && addnorm_aligned_to(wgt, 16) && (ldq % EPV == 0) && addnorm_aligned_to(q, EPV) && cols / EPV <= 256 * 16 &&
                        (!h_out || ((ldh % EPV == 0) && addnorm_aligned_to(h_out, 16)));
    const dim3 grid((unsigned)rows), block(256);
    if (!vec_ok) {
        add_rmsnorm_quant_generic<DT><<<grid, block, 0, st>>>(x, ldx, res, ldr, sum_out, lds, wgt, eps, cols, q, ldq, scale, h_out, ldh);
        return;
    }
    const int nvec = (int)(cols / EPV);
    const uint8_t* xb = reinterpret_cast<const uint8_t*>(x);
    const uint8_t* rb = reinterpret_cast<const uint8_t*>(res);
    uint8_t* sb = reinterpret_cast<uint8_t*>(sum_out);
    const uint8_t* wb = reinterpret_cast<const uint8_t*>(wgt);
    uint8_t* hb = reinterpret_cast<uint8_t*>(h_out);
    const int64_t kb = Elem<DT>::kBytes;
    if (nvec <= opt().rms_wave_max) {         // one wave per row: VPT in {1, 2, 4, 8} keeps i & 3 meaningful
        const dim3 wgrid((unsigned)((rows + 3) / 4));
#define PQ_ADDW_LAUNCH(V)                                                                                                                                         \
    do {                                                                                                                                                          \
        if (h_out) add_rmsnorm_quant_wave<DT, V, true><<<wgrid, block, 0, st>>>(xb, ldx * kb, rb, ldr * kb, sb, lds * kb, wb, eps, (int)cols, nvec, rows, q, ldq, scale, hb, ldh * kb); \
        else add_rmsnorm_quant_wave<DT, V, false><<<wgrid, block, 0, st>>>(xb, ldx * kb, rb, ldr * kb, sb, lds * kb, wb, eps, (int)cols, nvec, rows, q, ldq, scale, hb, 0);              \
    } while (0)
        if (nvec <= 64) PQ_ADDW_LAUNCH(1);
        else if (nvec <= 128) PQ_ADDW_LAUNCH(2);
        else if (nvec <= 256) PQ_ADDW_LAUNCH(4);
        else PQ_ADDW_LAUNCH(8);
#undef PQ_ADDW_LAUNCH
        return;
    }
    int vpt = 1;
    while (vpt * 256 < nvec) vpt <<= 1;
#define PQ_ADDV_LAUNCH(V)                                                                                                                                    \
    do {                                                                                                                                                     \
        if (h_out) add_rmsnorm_quant_vec<DT, V, true><<<grid, block, 0, st>>>(xb, ldx * kb, rb, ldr * kb, sb, lds * kb, wb, eps, (int)cols, nvec, q, ldq, scale, hb, ldh * kb); \
        else add_rmsnorm_quant_vec<DT, V, false><<<grid, block, 0, st>>>(xb, ldx * kb, rb, ldr * kb, sb, lds * kb, wb, eps, (int)cols, nvec, q, ldq, scale, hb, 0);              \
    } while (0)
    switch (vpt) {
        case 1: PQ_ADDV_LAUNCH(1); break;
        case 2: PQ_ADDV_LAUNCH(2); break;
        case 4: PQ_ADDV_LAUNCH(4); break;
        case 8: PQ_ADDV_LAUNCH(8); break;
        default: PQ_ADDV_LAUNCH(16); break;
    }
#undef PQ_ADDV_LAUNCH
}

template void add_rmsnorm_quant_dispatch<PQ_BF16>(const void*, int64_t, const void*, int64_t, void*, int64_t, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void add_rmsnorm_quant_dispatch<PQ_FP16>(const void*, int64_t, const void*, int64_t, void*, int64_t, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template void add_rmsnorm_quant_dispatch<PQ_F32>(const void*, int64_t, const void*, int64_t, void*, int64_t, const void*, float, int64_t, int64_t, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);

}  // namespace pq
