// w4_pack_kernels.hip — the int4 weight format "W4 v1" (QSPEC W1-W4): a second, integer quantisation level on top of the per-channel int8 weight.
//   W8[n][k] = q[n][k] * g[n][k / 128],   q in [-7, 7] (one nibble),   g in [1, 18] (one byte per 128 k),   |W8| <= 126
//   w4 u8[N][Kp / 2]: byte 64 j + i (i < 64) of row n = q[n][128 j + i] (low nibble) | q[n][128 j + 64 + i] << 4, two's-complement nibbles; Kp = K rounded up to 128
//   gs u8[ceil(N / 4)][Kp / 128][4]: byte ((n >> 2) G + j) 4 + (n & 3) = g[n][j]; rows past N hold 1
// w4_pack makes both from the int8 codes (load time); w4_expand is the format's definition in code and the prefill path: it writes W8, which the int8 tiles then run.
// Everything is integer arithmetic: there is one result.
#include "pq_launch.h"

namespace pq {

namespace {

// W2-W3: the code of w under the group multiplier g — round half away from zero, clamped to [-7, 7]
__device__ __forceinline__ int w4_code(int w, int g) {
    const int a = w < 0 ? -w : w;
    int q = (2 * a + g) / (2 * g);
    q = q > 7 ? 7 : q;
    return w < 0 ? -q : q;
}

// one wave per (row, group): lane i holds k = 128 j + i and k = 128 j + 64 + i, so its two codes are the two nibbles of byte 64 j + i
__global__ __launch_bounds__(256) void w4_pack_kernel(const int8_t* __restrict__ wq, int64_t ldw, int64_t N, int64_t K, int64_t G, uint8_t* __restrict__ w4, int64_t ldw4,
                                                      uint8_t* __restrict__ gs) {
    const int lane = threadIdx.x & 63;
    const int64_t id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n = id / G, j = id - n * G;
    if (n >= ((N + 3) & ~(int64_t)3)) return;                  // (wave-uniform)
    uint8_t* gdst = gs + ((n >> 2) * G + j) * 4 + (n & 3);
    if (n >= N) {                                              // the rows that fill the last quad of gs: multiplier 1, no codes
        if (lane == 0) *gdst = 1;
        return;
    }
    const int64_t k0 = j * 128 + lane, k1 = k0 + 64;
    const int w0 = k0 < K ? wq[n * ldw + k0] : 0, w1 = k1 < K ? wq[n * ldw + k1] : 0;      // zero tail for K < Kp
    int a = (w0 < 0 ? -w0 : w0) > (w1 < 0 ? -w1 : w1) ? (w0 < 0 ? -w0 : w0) : (w1 < 0 ? -w1 : w1);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(a, off, 64); a = o > a ? o : a; }
    int g = (a + 6) / 7;                                       // W1: g = min(18, max(1, ceil(a / 7)))
    g = g < 1 ? 1 : (g > 18 ? 18 : g);
    w4[n * ldw4 + j * 64 + lane] = (uint8_t)((w4_code(w0, g) & 0xF) | ((w4_code(w1, g) & 0xF) << 4));
    if (lane == 0) *gdst = (uint8_t)g;
}

// four signed bytes q * g from the nibbles (bits 4 b + sh .. + 3 of each byte b) of one packed dword
__device__ __forceinline__ uint32_t w4_expand4(uint32_t v, int sh, int g) {
    uint32_t o = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int nib = (int)((v >> (8 * b + sh)) & 0xF), q = (nib ^ 8) - 8;      // two's-complement nibble (0x8, reserved, reads as -8: |q g| <= 144 wraps in the byte, nothing else)
        o |= (uint32_t)((q * g) & 0xFF) << (8 * b);
    }
    return o;
}

// one thread per 16 packed bytes: the 16 codes k = 128 j + 16 c .. + 15 (low nibbles) and k = 128 j + 64 + 16 c .. (high nibbles) of row n, one 16-byte store each
__global__ __launch_bounds__(256) void w4_expand_kernel(const uint8_t* __restrict__ w4, int64_t ldw4, const uint8_t* __restrict__ gs, int64_t N, int64_t G,
                                                        int8_t* __restrict__ w8, int64_t ldw8) {
    const int64_t total = N * G * 4;
    for (int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x; id < total; id += (int64_t)gridDim.x * 256) {
        const int64_t c = id & 3, j = (id >> 2) % G, n = (id >> 2) / G;
        const v4u v = *reinterpret_cast<const v4u*>(w4 + n * ldw4 + j * 64 + c * 16);
        const int g = gs[((n >> 2) * G + j) * 4 + (n & 3)];
        v4u lo, hi;
#pragma unroll
        for (int d = 0; d < 4; ++d) { lo[d] = w4_expand4(v[d], 0, g); hi[d] = w4_expand4(v[d], 4, g); }
        int8_t* dst = w8 + n * ldw8 + j * 128 + c * 16;
        *reinterpret_cast<v4u*>(dst) = lo;
        *reinterpret_cast<v4u*>(dst + 64) = hi;
    }
}

}  // namespace

void launch_w4_pack(const int8_t* wq, int64_t ldw, int64_t N, int64_t K, uint8_t* w4, int64_t ldw4, uint8_t* gs, hipStream_t st) {
    const int64_t G = (K + 127) / 128, waves = ((N + 3) & ~(int64_t)3) * G;
    w4_pack_kernel<<<dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st>>>(wq, ldw, N, K, G, w4, ldw4, gs);
}

void launch_w4_expand(const uint8_t* w4, int64_t ldw4, const uint8_t* gs, int64_t N, int64_t Kp, int8_t* w8, int64_t ldw8, hipStream_t st) {
    const int64_t G = Kp / 128, blocks = (N * G * 4 + 255) / 256;
    w4_expand_kernel<<<dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st>>>(w4, ldw4, gs, N, G, w8, ldw8);
}

}  // namespace pq
