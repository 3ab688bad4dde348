// hadamard_kernels.hip — K1h: a block-diagonal normalised Hadamard rotation of every row, fused with K1's per-token int8 quantisation (QSPEC H1-H5).
//   h[r, k B .. (k + 1) B) = cast_rne(FWHT_B(f32(x[r, k B .. (k + 1) B))) * c),  c = the binary32 nearest to B^(-1/2);  then Q1-Q6 on the rows of h as stored.
// The fast Walsh-Hadamard transform runs its log2 B stages in ASCENDING stride (stage s: every pair (i, i + 2^s) with bit s of i clear becomes (a + b, a - b), one
// binary32 operation each): every output is one fixed tree of adds, so every layout below gives the same bits.  Algorithmic traffic: K1's (read once, 1 B/elem of codes,
// 4 B/row), plus elem bytes when h_out is asked for; q == scale == nullptr is the transform-only form (the weight rotation: h_out alone).
//
// Wave form (block 64 .. 4096, rows of at most 32 768 elements, 16-byte aligned operands).  Nothing else in this library moves a row's elements across lanes; here a
// lane owns 64 CONSECUTIVE elements and the lane bits are exchanged for register bits ONCE, through LDS:
//   1. unit-stride 16-byte loads (K1's pattern: a wave-instruction reads 1 KiB of whole lines), written raw to LDS and read back as 64 consecutive elements per lane
//      (the alternative, 16-byte loads at a 128-byte lane stride, touches 64 lines per instruction: four times below the worst row of tools/ubench/stream_pattern's table);
//   2. stages 0 .. 5 in registers;
//   3. block > 64: the P = block / 64 lanes of a block write their 64 values (ds_write_b128) and read them back transposed — lane p' of the group gets, from every lane p,
//      the 64 / P values p' 64 / P .. (ds_read_b128 for P <= 16, b64 / b32 for P = 32 / 64); stages 6 .. in registers again, on the p index;
//   4. scale, storage rounding and the row maximum in the transposed layout (a maximum does not care): an xor butterfly over the lanes of the row, across the waves of a
//      long row through LDS as in K1;
//   5. the codes (and h, when asked for) return through LDS as bytes to the unit-stride order, so every global store is 16 bytes and a wave-instruction writes 1 KiB.
// Rows shorter than a wave's 4096 elements are packed 64 / G to a wave (G = the power of two >= cols / 64 lanes), two waves to a workgroup; longer rows take ceil(cols /
// 4096) waves, one row per workgroup.  Every LDS pass is swizzled at 16-byte granularity so that 16 consecutive lanes touch 16 different 16-byte bank groups on both
// sides (swz, tswz below).  No scratch, no atomics, no workspace; one launch.
// Generic form (any other legal block / cols / alignment, rows too long for registers): one workgroup per row, one block at a time transformed in LDS; with codes asked
// for the row is transformed twice (the amax, then the codes: the second read comes from cache).  Same bits.
// Aliasing: none (pq_api.hip refuses every overlap), so every pointer is __restrict__.
//
// K1gh (QSPEC GH1): the same kernels with the gated activation of an MLP as the PRODUCER of the row — h0 = cast(cast(silu(g)) * u) (S1-S5) or the tanh-GELU gate (GG1-GG3)
// AS STORED, then H1-H5 on h0.  The work split, HadMap and the swizzles are K1h's, which is what keeps the rotation's bits.  Wave form: step 1 issues ALL its unit-stride
// 16-byte loads of g and of u (2 NV in flight; each operand has a leading dimension of its own), takes the division-free quotient or `/` once per wave from the min / max
// of the gate bits it loaded (K1s's test; both give the specification's bits), turns every pair of vectors into the stored h0 vector (silu_mul_vec / GegluOp::vec, the
// instruction sequences of K1s / K1gg) and writes THAT to the raw LDS region; from the first barrier on the kernel is K1h.  Only the loaded vectors are live while the
// producer runs, before the 64-float register array exists.  Generic form: the element load becomes the one-element producer (map_one around the same stage, then the
// storage rounding).  h0 is never stored; h_out holds the ROTATED activation.
#include <cmath>
#include <type_traits>
#include "geglu_device.h"
#include "pq_launch.h"

namespace pq {

constexpr int kLaneElems = 64;                            // consecutive elements a lane owns
constexpr int kRegionBytes = kWave * kLaneElems * 4;      // one wave's LDS: its 4096 values as f32
constexpr int kHadMaxWaves = 8;                           // waves per row of the wave form

// the producer in front of the loads: kNoGate is K1h itself (u is never read), PQ_GATE_SILU / PQ_GATE_GELU_TANH are K1gh.  fast_ok: the wave's test on the min / max of
// the |g| bit patterns; vec: one 16-byte vector of g and of u -> one of h0 as stored; one: the specified sequence on one element, before the storage rounding.
constexpr int kNoGate = -1;
template <int ACT> struct Gate;
template <> struct Gate<PQ_GATE_SILU> {
    template <int DT> __device__ static __forceinline__ bool fast_ok(uint32_t mn, uint32_t mx) { return silu_fast_div_ok<DT>(mn, mx); }
    template <int DT, bool FASTDIV> __device__ static __forceinline__ v4u vec(const v4u& gv, const v4u& uv) { return silu_mul_vec<DT, FASTDIV>(gv, uv); }
    template <int DT> __device__ static __forceinline__ float one(float g, float u) {
        return map_one(g, u, [](const auto& ga, const auto& ua, auto& h) { silu_mul_stage<DT, false, 1>(ga, ua, h); });
    }
};
template <> struct Gate<PQ_GATE_GELU_TANH> {
    template <int DT> __device__ static __forceinline__ bool fast_ok(uint32_t mn, uint32_t mx) { return GegluOp::fast_ok<DT>(mn, mx, {}); }
    template <int DT, bool FASTDIV> __device__ static __forceinline__ v4u vec(const v4u& gv, const v4u& uv) { return GegluOp::vec<DT, FASTDIV>(gv, uv, {}); }
    template <int DT> __device__ static __forceinline__ float one(float g, float u) { return GegluOp::spec<DT>(g, u, {}); }
};

// byte offset -> swizzled byte offset in a wave's region seen as 64 lane rows of NV 16-byte granules (NV = 4: codes, 8: 16-bit values, 16: f32).  Granule `col` of row
// `row` lies at column col ^ ((row / (16 / NV)) % NV): 16 consecutive lanes reading (or writing) the same column of their own rows, and 16 consecutive lanes walking
// consecutive granules, both cover every 16-byte group of a 256-byte bank period once.
template <int NV>
__device__ __forceinline__ uint32_t swz(uint32_t off) {
    const uint32_t g = off >> 4, row = g / NV, col = g % NV;
    return ((row * NV + (col ^ ((row / (16 / NV)) & (NV - 1)))) << 4) | (off & 15u);
}
// the f32 transpose: column swizzle of lane row `row` for groups of P lanes — the two fields of row % 16 swapped, so that the readers of one instruction (lane = group * P
// + p', all reading row group * P + p, chunk p' 16 / P + j) land on 16 different columns as well as the writers (16 consecutive rows, one chunk index)
template <int P>
__device__ __forceinline__ uint32_t tswz(uint32_t row) {
    if constexpr (P >= 16) return row & 15u;
    else return ((row & (P - 1)) * (16 / P)) | ((row / P) & (16 / P - 1));
}

// where lane-row `ol` (0 .. 63) of this wave lies: its row of the matrix and its 64-element slot in it
struct HadMap {
    int64_t rows, row0;      // row0: the first row of this wave
    int log_g, slots;        // lanes per row of this wave (2^log_g; a long row: 64 and `t0` counts the waves before), valid slots per row (cols / 64)
    int t0;
    __device__ __forceinline__ void at(int ol, int64_t& row, int& t, bool& valid) const {
        row = row0 + (ol >> log_g);
        t = t0 + (ol & ((1 << log_g) - 1));
        valid = row < rows && t < slots;
    }
};

// the lane's packed results (`words`, in the order of its transposed index i = p RL + r_lo) scattered to their lane rows as runs of RB = NVG 16 / P bytes
template <int NVG, int P, int NWORDS>
__device__ __forceinline__ void scatter_runs(uint8_t* region, int lane, const uint32_t (&words)[NWORDS]) {
    constexpr int RB = NVG * 16 / P;
    static_assert(NWORDS * 4 == NVG * 16, "a lane holds one lane row of results");
    const uint32_t pp = lane & (P - 1), first = lane & ~(P - 1);
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const uint32_t off = (first + p) * (NVG * 16) + pp * RB;
        if constexpr (RB >= 16) {
#pragma unroll
            for (int j = 0; j < RB / 16; ++j) {
                const int w = p * (RB / 4) + 4 * j;
                *reinterpret_cast<v4u*>(region + swz<NVG>(off + 16 * j)) = v4u{words[w], words[w + 1], words[w + 2], words[w + 3]};
            }
        } else if constexpr (RB == 8) {
            *reinterpret_cast<v2u*>(region + swz<NVG>(off)) = v2u{words[2 * p], words[2 * p + 1]};
        } else if constexpr (RB == 4) {
            *reinterpret_cast<uint32_t*>(region + swz<NVG>(off)) = words[p];
        } else if constexpr (RB == 2) {
            *reinterpret_cast<uint16_t*>(region + swz<NVG>(off)) = (uint16_t)(words[p / 2] >> (16 * (p & 1)));
        } else {
            *reinterpret_cast<uint8_t*>(region + swz<NVG>(off)) = (uint8_t)(words[p / 4] >> (8 * (p & 3)));
        }
    }
}

// the region read back in unit-stride order and stored: instruction k stores granule k 64 + lane of the wave (1 KiB per wave-instruction where the rows are contiguous)
template <int NVG>
__device__ __forceinline__ void gather_store(const uint8_t* region, int lane, const HadMap& m, uint8_t* __restrict__ dst, int64_t ld_bytes) {
#pragma unroll
    for (int k = 0; k < NVG; ++k) {
        const int g = k * kWave + lane;
        int64_t row;
        int t;
        bool valid;
        m.at(g / NVG, row, t, valid);
        const v4u v = *reinterpret_cast<const v4u*>(region + swz<NVG>((uint32_t)g * 16u));
        if (valid) store_wt_b128(dst + row * ld_bytes + ((int64_t)t * NVG + g % NVG) * 16, v);
    }
}

// the stages of strides FIRST, 2 FIRST, .. below N on a register array (every index is a constant after unrolling)
template <int FIRST, int N>
__device__ __forceinline__ void fwht_stages(float (&v)[N]) {
    if constexpr (FIRST < N) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if ((i & FIRST) == 0) {
                const float a = v[i], b = v[i + FIRST];
                v[i] = a + b;          // H2: one binary32 operation each (nothing here multiplies, and the build holds -ffp-contract=off)
                v[i + FIRST] = a - b;
            }
        }
        fwht_stages<2 * FIRST>(v);
    }
}

// LOGP: log2(block / 64).  multi: the row spans the waves of the workgroup (one row per workgroup); otherwise every wave holds 64 >> log_g rows of its own.
// ACT: the producer (kNoGate: x is the row, u / ldu_bytes are not read; otherwise x is the gate g).
template <int DT, int LOGP, int ACT>
__global__ __launch_bounds__(64 * kHadMaxWaves) void hadamard_quant_wave(const uint8_t* __restrict__ x, int64_t ldx_bytes, const uint8_t* __restrict__ u, int64_t ldu_bytes,
                                                                          int64_t rows, int slots, int log_g, int multi, float c, int8_t* __restrict__ q, int64_t ldq,
                                                                          float* __restrict__ scale, uint8_t* __restrict__ h_out, int64_t ldh_bytes) {
    constexpr int EB = Elem<DT>::kBytes, EPV = 16 / EB, NV = kLaneElems / EPV;      // NV: 16-byte vectors per lane (8 / 16)
    constexpr int P = 1 << LOGP, RL = kLaneElems / P;
    extern __shared__ v4u had_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    uint8_t* region = reinterpret_cast<uint8_t*>(had_lds) + wave * kRegionBytes;
    HadMap m;
    m.rows = rows; m.slots = slots; m.log_g = log_g;
    if (multi) { m.row0 = blockIdx.x; m.t0 = wave * kWave; }
    else { m.row0 = ((int64_t)blockIdx.x * nwaves + wave) << (6 - log_g); m.t0 = 0; }

    // ---- 1. unit-stride loads (clamped: a lane row past the data reads slot 0 of the last row and is zeroed by its owner), raw through LDS
    v4u raw[NV];
    [[maybe_unused]] v4u uraw[ACT == kNoGate ? 1 : NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int g = k * kWave + lane;
        int64_t row;
        int t;
        bool valid;
        m.at(g / NV, row, t, valid);
        if (!valid) { row = row < rows ? row : rows - 1; t = 0; }
        raw[k] = *reinterpret_cast<const v4u*>(x + row * ldx_bytes + ((int64_t)t * NV + g % NV) * 16);
        if constexpr (ACT != kNoGate) uraw[k] = *reinterpret_cast<const v4u*>(u + row * ldu_bytes + ((int64_t)t * NV + g % NV) * 16);
    }
    if constexpr (ACT != kNoGate) {          // K1gh: raw becomes the stored h0; the quotient's form is the wave's (K1s's test on the gate bits loaded, clamped ones included)
        uint32_t gmn = 0xFFFFFFFFu, gmx = 0u;
#pragma unroll
        for (int k = 0; k < NV; ++k) vec_absminmax_bits<DT>(raw[k], gmn, gmx);
        if (__builtin_amdgcn_ballot_w64(!Gate<ACT>::template fast_ok<DT>(gmn, gmx)) == 0ull) {
#pragma unroll
            for (int k = 0; k < NV; ++k) raw[k] = Gate<ACT>::template vec<DT, true>(raw[k], uraw[k]);
        } else {
#pragma unroll
            for (int k = 0; k < NV; ++k) raw[k] = Gate<ACT>::template vec<DT, false>(raw[k], uraw[k]);
        }
    }
    // K1gh: the lane index from here on is a value of its own, so that the row / slot / validity arithmetic of the stores at the kernel's end is redone there instead of
    // being kept live (and spilled) across the producer, whose 2 NV loaded vectors fill the register file of an f32 row
    int ln = lane;
    if constexpr (ACT != kNoGate) asm volatile("" : "+v"(ln));
#pragma unroll
    for (int k = 0; k < NV; ++k) *reinterpret_cast<v4u*>(region + swz<NV>((uint32_t)(k * kWave + ln) * 16u)) = raw[k];
    __syncthreads();
    int64_t my_row;
    int my_t;
    bool my_valid;
    m.at(ln, my_row, my_t, my_valid);      // (the P lanes of a block are valid together: cols is a multiple of the block)
    float v[kLaneElems];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        v4u r = *reinterpret_cast<const v4u*>(region + swz<NV>((uint32_t)(ln * NV + k) * 16u));
        if (!my_valid) r = v4u{0u, 0u, 0u, 0u};
        float f[EPV];
        Unpack<DT, EPV>::run(r, f);          // H1
#pragma unroll
        for (int j = 0; j < EPV; ++j) v[k * EPV + j] = f[j];
    }
    // ---- 2. stages 0 .. 5
    fwht_stages<1>(v);
    // ---- 3. ln bits <-> register bits, stages 6 ..
    if constexpr (LOGP > 0) {
        __syncthreads();                     // every raw read of this region is done
#pragma unroll
        for (int ch = 0; ch < 16; ++ch)
            *reinterpret_cast<v4f*>(region + ln * 256 + ((ch ^ tswz<P>(ln)) << 4)) = v4f{v[4 * ch], v[4 * ch + 1], v[4 * ch + 2], v[4 * ch + 3]};
        __syncthreads();
        const uint32_t pp = ln & (P - 1), first = ln & ~(P - 1);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const uint32_t row = first + p;
            const uint8_t* src = region + row * 256;
            if constexpr (RL >= 4) {
#pragma unroll
                for (int j = 0; j < RL / 4; ++j) {
                    const v4f t4 = *reinterpret_cast<const v4f*>(src + (((pp * (RL / 4) + j) ^ tswz<P>(row)) << 4));
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[p * RL + 4 * j + e] = t4[e];
                }
            } else if constexpr (RL == 2) {
                const v2f t2 = *reinterpret_cast<const v2f*>(src + (((pp >> 1) ^ tswz<P>(row)) << 4) + (pp & 1) * 8);
                v[2 * p] = t2[0];
                v[2 * p + 1] = t2[1];
            } else {
                v[p] = *reinterpret_cast<const float*>(src + (((pp >> 2) ^ tswz<P>(row)) << 4) + (pp & 3) * 4);
            }
        }
        fwht_stages<RL>(v);      // index p RL + r_lo: the strides RL, 2 RL, .. are the bits of p
    }
    // ---- 4. H3, H4 and the row maximum of |h| as stored
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < kLaneElems; ++i) {
        v[i] = Elem<DT>::to_f32(Elem<DT>::from_f32(v[i] * c));
        amax = amax_step(amax, v[i]);
    }
    __syncthreads();                         // every transposed read is done: the regions are free
    if (q) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
            if (off < (1 << log_g)) amax = amax_merge(amax, __shfl_xor(amax, off, 64));
        if (multi) {
            float* part = reinterpret_cast<float*>(had_lds);
            if (ln == 0) part[wave] = amax;
            __syncthreads();
            for (int w = 0; w < nwaves; ++w) amax = amax_merge(amax, part[w]);
            __syncthreads();
        }
        const float s = scale_of(amax);
        if (my_valid && my_t == 0) scale[my_row] = s;
        uint32_t pk[kLaneElems / 4];
        if (amax == amax && scale_fast_ok(s)) {      // K1's division-free exact encode: h holds storage values and amax is one of them
            fast_encode<kLaneElems, kQuotientSteps<DT>>(v, s, 1.0f / s, pk);
        } else {
#pragma unroll
            for (int j = 0; j < kLaneElems / 4; ++j) pk[j] = pack4(code_of(v[4 * j], s), code_of(v[4 * j + 1], s), code_of(v[4 * j + 2], s), code_of(v[4 * j + 3], s));
        }
        // ---- 5. the codes back to the unit-stride order
        scatter_runs<4, P>(region, ln, pk);
        __syncthreads();
        gather_store<4>(region, ln, m, reinterpret_cast<uint8_t*>(q), ldq);
    }
    if (h_out) {
        if (q) __syncthreads();
        uint32_t hw[kLaneElems * EB / 4];
#pragma unroll
        for (int j = 0; j < kLaneElems * EB / 4; ++j) {
            if constexpr (EB == 4) hw[j] = __builtin_bit_cast(uint32_t, v[j]);
            else hw[j] = (uint32_t)Elem<DT>::from_f32(v[2 * j]) | ((uint32_t)Elem<DT>::from_f32(v[2 * j + 1]) << 16);      // (exact: v holds storage values)
        }
        scatter_runs<NV, P>(region, ln, hw);
        __syncthreads();
        gather_store<NV>(region, ln, m, h_out, ldh_bytes);
    }
}

// one workgroup per row, one block at a time in LDS; thread t owns elements t, t + 256, .. of a block outside the stages
template <int DT, int ACT>
__global__ __launch_bounds__(256) void hadamard_quant_generic(const void* __restrict__ x, int64_t ldx, const void* __restrict__ u, int64_t ldu, int64_t cols, int block,
                                                              int log_b, float c, int8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale, void* __restrict__ h_out,
                                                              int64_t ldh) {
    using S = typename Elem<DT>::store_t;
    __shared__ float buf[4096];
    __shared__ float part[4];
    const int64_t row = blockIdx.x;
    const S* xr = reinterpret_cast<const S*>(x) + row * ldx;
    [[maybe_unused]] const S* ur = reinterpret_cast<const S*>(u) + row * ldu;
    S* hr = h_out ? reinterpret_cast<S*>(h_out) + row * ldh : nullptr;
    const int tid = threadIdx.x;
    const auto transform = [&](int64_t c0) {      // leaves h as stored (widened) in buf; a thread reads back only what it wrote last
        __syncthreads();
        for (int i = tid; i < block; i += 256) {
            if constexpr (ACT == kNoGate) buf[i] = Elem<DT>::to_f32(xr[c0 + i]);
            else buf[i] = Elem<DT>::to_f32(Elem<DT>::from_f32(Gate<ACT>::template one<DT>(Elem<DT>::to_f32(xr[c0 + i]), Elem<DT>::to_f32(ur[c0 + i]))));      // h0 as stored
        }
        __syncthreads();
        for (int s = 0; s < log_b; ++s) {
            for (int idx = tid; idx < block / 2; idx += 256) {
                const int i = ((idx >> s) << (s + 1)) | (idx & ((1 << s) - 1));
                const float a = buf[i], b = buf[i + (1 << s)];
                buf[i] = a + b;
                buf[i + (1 << s)] = a - b;
            }
            __syncthreads();
        }
        for (int i = tid; i < block; i += 256) buf[i] = Elem<DT>::to_f32(Elem<DT>::from_f32(buf[i] * c));
    };
    float amax = 0.0f;
    for (int64_t c0 = 0; c0 < cols; c0 += block) {
        transform(c0);
        for (int i = tid; i < block; i += 256) {
            amax = amax_step(amax, buf[i]);
            if (hr) hr[c0 + i] = Elem<DT>::from_f32(buf[i]);
        }
    }
    if (!q) return;
    amax = wave_max(amax);
    if ((tid & 63) == 0) part[tid >> 6] = amax;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) amax = amax_merge(amax, part[w]);
    const float s = scale_of(amax);
    if (tid == 0) scale[row] = s;
    int8_t* qr = q + row * ldq;
    for (int64_t c0 = 0; c0 < cols; c0 += block) {
        transform(c0);
        for (int i = tid; i < block; i += 256) qr[c0 + i] = (int8_t)code_of(buf[i], s);
    }
}

// the layout decision of K1h and K1gh, made once (u / ldu: K1gh's second operand, null / 0 for K1h)
template <int DT, int ACT>
static hipError_t hadamard_dispatch(const void* x, int64_t ldx, const void* u, int64_t ldu, int64_t rows, int64_t cols, int block, int8_t* q, int64_t ldq, float* scale,
                                    void* h_out, int64_t ldh, hipStream_t st) {
    constexpr int64_t EB = Elem<DT>::kBytes;
    int log_b = 0;
    while ((1 << log_b) < block) ++log_b;
    const float c = (float)(1.0 / std::sqrt((double)block));      // H3: exact for even log2 B, the nearest binary32 otherwise
    const auto rows16 = [&](const void* p, int64_t ld_bytes) { return !p || (aligned_to(p, 16) && (rows == 1 || ld_bytes % 16 == 0)); };
    const bool wave_ok = block >= kLaneElems && cols <= (int64_t)kHadMaxWaves * kWave * kLaneElems && rows16(x, ldx * EB) && rows16(u, ldu * EB) && rows16(q, ldq) && rows16(h_out, ldh * EB);
    if (!wave_ok) {
        hadamard_quant_generic<DT, ACT><<<dim3((unsigned)rows), dim3(256), 0, st>>>(x, ldx, u, ldu, cols, block, log_b, c, q, ldq, scale, h_out, ldh);
        return hipSuccess;
    }
    const int slots = (int)(cols / kLaneElems);
    int log_g = 0;
    while ((1 << log_g) < slots && log_g < 6) ++log_g;
    const bool multi = slots > kWave;
    const int64_t rows_per_wave = multi ? 1 : (kWave >> log_g);
    const int64_t waves = (rows + rows_per_wave - 1) / rows_per_wave;
    const int nwaves = multi ? (slots + kWave - 1) / kWave : (waves < 2 ? 1 : 2);
    const dim3 grid((unsigned)(multi ? rows : (waves + nwaves - 1) / nwaves)), threads(nwaves * kWave);
    const size_t lds = (size_t)nwaves * kRegionBytes;
    hipError_t err = hipSuccess;
    const auto go = [&](auto lp) {
        constexpr int LOGP = decltype(lp)::value;
        auto* kern = hadamard_quant_wave<DT, LOGP, ACT>;
        if (lds >= 64 * 1024) err = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err != hipSuccess) return;
        kern<<<grid, threads, lds, st>>>(reinterpret_cast<const uint8_t*>(x), ldx * EB, reinterpret_cast<const uint8_t*>(u), ldu * EB, rows, slots, log_g, multi ? 1 : 0, c,
                                        q, ldq, scale, reinterpret_cast<uint8_t*>(h_out), ldh * EB);
    };
    switch (log_b - 6) {
        case 0: go(std::integral_constant<int, 0>{}); break;
        case 1: go(std::integral_constant<int, 1>{}); break;
        case 2: go(std::integral_constant<int, 2>{}); break;
        case 3: go(std::integral_constant<int, 3>{}); break;
        case 4: go(std::integral_constant<int, 4>{}); break;
        case 5: go(std::integral_constant<int, 5>{}); break;
        default: go(std::integral_constant<int, 6>{}); break;
    }
    return err;
}

template <int DT>
hipError_t hadamard_quant_dispatch(const void* x, int64_t ldx, int64_t rows, int64_t cols, int block, int8_t* q, int64_t ldq, float* scale, void* h_out, int64_t ldh,
                                   hipStream_t st) {
    return hadamard_dispatch<DT, kNoGate>(x, ldx, nullptr, 0, rows, cols, block, q, ldq, scale, h_out, ldh, st);
}
template <int DT>
hipError_t gated_hadamard_quant_dispatch(const void* g, int64_t ldg, const void* u, int64_t ldu, int64_t rows, int64_t cols, int act, int block, int8_t* q, int64_t ldq,
                                         float* scale, void* h_out, int64_t ldh, hipStream_t st) {
    if (act == PQ_GATE_GELU_TANH) return hadamard_dispatch<DT, PQ_GATE_GELU_TANH>(g, ldg, u, ldu, rows, cols, block, q, ldq, scale, h_out, ldh, st);
    return hadamard_dispatch<DT, PQ_GATE_SILU>(g, ldg, u, ldu, rows, cols, block, q, ldq, scale, h_out, ldh, st);
}

template hipError_t hadamard_quant_dispatch<PQ_BF16>(const void*, int64_t, int64_t, int64_t, int, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template hipError_t hadamard_quant_dispatch<PQ_FP16>(const void*, int64_t, int64_t, int64_t, int, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
template hipError_t hadamard_quant_dispatch<PQ_F32>(const void*, int64_t, int64_t, int64_t, int, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
#define PQ_GH_INST(DT) \
    template hipError_t gated_hadamard_quant_dispatch<DT>(const void*, int64_t, const void*, int64_t, int64_t, int64_t, int, int, int8_t*, int64_t, float*, void*, int64_t, hipStream_t);
PQ_GH_INST(PQ_BF16) PQ_GH_INST(PQ_FP16) PQ_GH_INST(PQ_F32)
#undef PQ_GH_INST

}  // namespace pq
