/* pq_hip.h — C-ABI of libpq_hip.so: the MI355X (gfx950) dynamic-int8 linear hot path.
 *
 * This is the drop-in boundary.  The reference's operator interface for this path
 * is the Python API BASELINE.json names (QTensor, quantize(), dequantize(), qlinear); its source is
 * absent from the mount (/root/reference holds only CODE_OF_CONDUCT.md:1-80), so each entry point
 * cites the contract clause / primitive it replaces instead of a reference file:line.
 *
 * Conventions
 *  - plain pointers + sizes; every buffer is CALLER-OWNED DEVICE memory on the current HIP device;
 *    the library never allocates, frees, copies to host or synchronises.
 *  - stream-ordered and asynchronous: work is enqueued on `stream` (a hipStream_t passed as void*;
 *    NULL = the null stream).  Safe to capture into a hipGraph.
 *  - every function returns a pq_status; pq_last_error() gives the thread-local message of the last
 *    failing call on this thread.  Nothing throws across the ABI.
 *  - matrices are row-major with explicit leading dimensions in ELEMENTS.
 *  - the row entries (K1 and its halves, K2, dequant, every K1 fused into a producer or a norm, pq_moe_combine) refuse an output that overlaps another operand —
 *    PQ_ERR_BAD_ARG before any HIP call, pq_last_error naming both ("q overlaps x") — unless the entry's own comment allows it (sum_out being x or residual).
 *    Operands that share a leading dimension (column blocks of one buffer) are told apart by their columns, everything else by its bounding byte range.
 *  - dtype codes: 0 = bf16, 1 = fp16, 2 = f32.
 *  - numeric contract: QSPEC v2.  int32 accumulators are exact; float stages are
 *    IEEE binary32, round-to-nearest-even, no contraction, true division.  A NaN in a token row (weight channel)
 *    PROPAGATES: that row's scale is the canonical quiet NaN 0x7FC00000, its codes are 0 and its qlinear output is NaN —
 *    what the unquantised linear would give; an Inf gives scale = Inf, codes 0 and a NaN output row.
 */
#ifndef PQ_HIP_H
#define PQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PQ_ABI_VERSION 1

typedef enum {
    PQ_OK = 0,
    PQ_ERR_BAD_ARG = 1,        /* null pointer, negative size, ld too small, unknown dtype/axis */
    PQ_ERR_BAD_ALIGN = 2,      /* reserved: every alignment is currently served by a generic path */
    PQ_ERR_LAUNCH = 3,         /* hipGetLastError() after a launch was not hipSuccess */
    PQ_ERR_UNIMPLEMENTED = 4,
    PQ_ERR_WORKSPACE = 5,      /* caller-provided workspace smaller than pq_*_workspace_bytes() */
    PQ_ERR_COMM = 6            /* RCCL error (multi-GPU entry points) */
} pq_status;

enum { PQ_BF16 = 0, PQ_FP16 = 1, PQ_F32 = 2 };

/* ABI version of the loaded library (== PQ_ABI_VERSION it was built with). */
int32_t pq_version(void);
/* Message of the last failing call on the calling thread ("" if none). Valid until the next call. */
const char* pq_last_error(void);
/* Behaviour switches for tests and experiments: PQ_FORCE_VARIANT (generic | sp256_16 | sp128_16 | sp128x128 | ring128 |
 * ring64x128 | ring64x64 | ring128x160 | skinny | "" = auto), PQ_NO_RING160 (1 = never plan the 128 x 160 ring tile: the round-5 dispatch), PQ_NO_KSLABS (1 = stacked codes always take
 * the layout pass), PQ_NO_TAILSPLIT, PQ_NO_SPLITK, PQ_FORCE_SPLITK (slice count: experiments), PQ_FSK (0 = no fused
 * split-K, S = S slices), PQ_FSK_SYMMETRIC and PQ_FSK_FENCED (see pq_qlinear_s8), PQ_NO_MIDM (no 64-row ring tiles), PQ_RING_ROT (0 = no K rotation), PQ_FAKE_CUS (plan as if the device had n CUs),
 * PQ_SKINNY_RB ("" = off / auto), PQ_EPI_ANY_ALIGN (0 = the staged epilogue only for 16-byte aligned output rows; default: any element-aligned row),
 * PQ_K2_BLOCKS_A / PQ_K2_BLOCKS_E (workgroup-count targets of K2's two passes), PQ_GROUPED_TILE / PQ_GROUPED_ROT (see pq_qlinear_s8_grouped), PQ_GROUPED_STREAM_KS / PQ_GROUPED_STREAM_RB (see pq_qlinear_s8_grouped_stream).  The switches that change launch geometry or pick another kernel for the same result are checked bit for bit in
 * tests/test_gpu_switch_paths.py and tests/test_gpu_k_rotation.py.  The environment variables of the same names are read ONCE, at the first call into the
 * library; this call changes a switch afterwards.
 * Threading: the switches live in an immutable snapshot; pq_set_option publishes a modified copy with one atomic pointer
 * swap, and every other entry point pins the snapshot that is live when it is ENTERED and plans and launches under that
 * one — so pq_set_option may race with launches on other host threads (each call sees the old or the new set, never a
 * mixture), and launches from several host threads at once are defined.  There is no other mutable global state in the
 * library (one-time init aside).  A captured hipGraph keeps the choice that was live at capture time. */
int32_t pq_set_option(const char* name, const char* value);

/* K1 — per-token dynamic symmetric int8 quantisation: replaces quantize(x) of the contract for an
 * activation x[rows, cols] (amax over cols).  q[rows, cols] int8, scale[rows] f32.   QSPEC Q1-Q6. */
int32_t pq_quant_rowwise(const void* x, int32_t dtype, int64_t rows, int64_t cols, int64_t ld_x,
                         int8_t* q, int64_t ld_q, float* scale, void* stream);

/* K2 — per-channel quantisation of a row-major matrix along its strided axis (amax over rows):
 * replaces quantize(W) for a [K, N]-stored weight.  scale[cols] f32.  Three stream-ordered graph nodes
 * (a fill kernel, the amax pass, the encode pass: three kernel nodes under capture); `scale` doubles as the amax scratch — no workspace.   QSPEC Q1-Q6. */
int32_t pq_quant_colwise(const void* x, int32_t dtype, int64_t rows, int64_t cols, int64_t ld_x,
                         int8_t* q, int64_t ld_q, float* scale, void* stream);

/* K1 fused into its producer: quantize(F.silu(g) * u) per token in one pass — the activation of the
 * `down` projection of a gated MLP (BASELINE config 3) — so the bf16 product never goes to HBM.  g, u: [rows, cols] of
 * `dtype` with their own leading dimensions (the two column halves of a fused gate+up output qualify: ld = 2*cols).
 * h_out (nullable, ld_h): also store h = silu(g)*u in `dtype`.  Numerics: QSPEC S1-S6 (specified exponential, IEEE
 * division, storage rounding after silu and after the product), then Q1-Q6 on the rows of h. */
int32_t pq_silu_mul_quant_rowwise(const void* g, int64_t ld_g, const void* u, int64_t ld_u, int32_t dtype,
                                  int64_t rows, int64_t cols, int8_t* q, int64_t ld_q, float* scale,
                                  void* h_out, int64_t ld_h, void* stream);

/* K1 fused into the CLAMPED gates of a gated expert MLP: quantize(h) per token in one pass, h by QSPEC G1-G5, L = limit rounded to `dtype`:
 *   kind PQ_GLU_CLAMPED_SILU  (DeepSeek-V4's experts):  h = silu(min(g, L)) * clamp(u, -L, +L)
 *   kind PQ_GLU_ALPHA_SIGMOID (GPT-OSS's experts):      gc = min(g, L);  h = (clamp(u, -L, +L) + 1) * (gc * sigmoid(alpha * gc))
 * with a storage rounding after every step a chain of tensor ops would round at; a NaN in g or u propagates, then Q1-Q6 on the rows of h.  Layouts and argument
 * meaning as pq_silu_mul_quant_rowwise (PQ_SILU_TPR included: time only, never bits; g, u: the two column halves of one [rows, 2 cols] tensor qualify, ld = 2 cols;
 * h_out nullable).  limit must be finite, > 0
 * and must not round to zero in `dtype`; alpha must be finite (it is not read for PQ_GLU_CLAMPED_SILU).  A bad kind / dtype / limit / alpha is PQ_ERR_BAD_ARG before
 * any HIP call; rows == 0 or cols == 0 is a no-op. */
#define PQ_GLU_CLAMPED_SILU 0
#define PQ_GLU_ALPHA_SIGMOID 1
int32_t pq_glu_quant_rowwise(const void* g, int64_t ld_g, const void* u, int64_t ld_u, int32_t dtype, int64_t rows, int64_t cols, int32_t kind, float limit,
                             float alpha, int8_t* q, int64_t ld_q, float* scale, void* h_out, int64_t ld_h, void* stream);

/* The two halves of pq_silu_mul_quant_rowwise for an intermediate whose COLUMNS are sharded over ranks (BASELINE config 5, gate/up and down both
 * column-sharded): a rank holds g, u[rows, cols_local].  The row amax of h = silu(g)*u is an exact max, so
 *   pq_silu_mul_rowamax            -> amax_bits[rows]: the f32 bit pattern of max |h| over the LOCAL columns (non-negative floats and NaNs order as
 *                                     unsigned integers: a NaN propagates, as Q2 says);
 *   all-reduce(max) of amax_bits as uint32 over the ranks (pq_allreduce_max_u32 in pq_rccl.h, or any other exact max);
 *   pq_silu_mul_quant_rowwise_amax -> q[rows, cols_local] and scale[rows] against the GLOBAL amax (h is recomputed: S1-S5 are deterministic)
 * give every rank the column block of the unsharded kernel's codes and the unsharded scale vector, bit for bit; the int8 blocks (1 byte per
 * element instead of 2 x 2 bytes of bf16 g and u) are what travels.  Same numerics, layouts and argument meaning as pq_silu_mul_quant_rowwise.
 * Precondition of the encode half: amax_bits[r] >= the row's local amax (true of any max that includes this block) — the exact encode does not clamp, a smaller
 * amax makes codes wrap. */
int32_t pq_silu_mul_rowamax(const void* g, int64_t ld_g, const void* u, int64_t ld_u, int32_t dtype, int64_t rows, int64_t cols,
                            uint32_t* amax_bits, void* stream);
int32_t pq_silu_mul_quant_rowwise_amax(const void* g, int64_t ld_g, const void* u, int64_t ld_u, int32_t dtype, int64_t rows, int64_t cols,
                                       const uint32_t* amax_bits, int8_t* q, int64_t ld_q, float* scale, void* stream);

/* The same two halves for a PLAIN activation whose columns are sharded over ranks (a rank's heads of the attention output feeding a column-sharded `o`
 * projection): pq_quant_rowamax -> all-reduce(max) -> pq_quant_rowwise_amax give the column block of pq_quant_rowwise's codes on the whole row and its scale
 * vector, bit for bit (QSPEC Q1-Q6; wide rows past 32 768 / 16 384 columns per rank and unaligned operands take the generic kernels). */
int32_t pq_quant_rowamax(const void* x, int32_t dtype, int64_t rows, int64_t cols, int64_t ld_x, uint32_t* amax_bits, void* stream);
int32_t pq_quant_rowwise_amax(const void* x, int32_t dtype, int64_t rows, int64_t cols, int64_t ld_x, const uint32_t* amax_bits, int8_t* q, int64_t ld_q,
                              float* scale, void* stream);

/* K1 fused into RMSNorm: quantize(weight * (x.float() * rsqrt(mean(x.float()^2) + eps)).to(dtype)) per
 * token in one pass — the input of the q/k/v and gate/up projections of a decoder layer.  x: [rows, cols], weight: [cols],
 * both of `dtype`; h_out (nullable, ld_h): also store the normalised activation.  Numerics: QSPEC N1-N6 — the sum of squares
 * is reduced in a pinned order (16-byte vectors dealt to 256 lanes, xor butterfly per 64 lanes, four partial sums left to
 * right), IEEE sqrt and division, storage rounding after x*rs and after the weight product — then Q1-Q6.  cols < 2^24. */
int32_t pq_rmsnorm_quant_rowwise(const void* x, int64_t ld_x, const void* weight, float eps, int32_t dtype,
                                 int64_t rows, int64_t cols, int8_t* q, int64_t ld_q, float* scale,
                                 void* h_out, int64_t ld_h, void* stream);

/* K1a — the residual add fused into pq_rmsnorm_quant_rowwise: s = cast_rne(f32(x) + f32(residual)) is STORED to sum_out (the new residual stream) and its rows
 * AS STORED go through N1-N6 and Q1-Q6 from the registers that hold them.  QSPEC A1: one binary32 add and one storage rounding per element,
 * which is what an eager add of two bf16 / fp16 / f32 tensors computes, so q, scale, sum_out and h_out are those of pq_rmsnorm_quant_rowwise run on residual + x,
 * bit for bit (a NaN propagates; NaNs compare as a class).  Reads 2 x elem bytes, writes elem bytes + 1 B/elem + 4 B/row: 7 B/elem for 16-bit rows against 9 for
 * the add and K1n as two launches.
 * sum_out is required and may BE x or residual (the same pointer AND the same leading dimension): every element is read before it is written.  Any other overlap
 * of sum_out with an input, and any overlap of q, scale or h_out with another operand, returns PQ_ERR_BAD_ARG — as do a null operand, ld < cols, cols >= 2^24, a
 * negative or non-finite eps and an unknown dtype — before any HIP call, with pq_last_error naming the argument.  h_out may be null.  rows == 0 or cols == 0:
 * nothing is read or written, returns PQ_OK.  Row layouts and the PQ_RMS_WAVE_MAX switch as pq_rmsnorm_quant_rowwise (time only, never bits). */
int32_t pq_add_rmsnorm_quant_rowwise(const void* x, int64_t ld_x, const void* residual, int64_t ld_r, void* sum_out, int64_t ld_s, const void* weight, float eps,
                                     int32_t dtype, int64_t rows, int64_t cols, int8_t* q, int64_t ld_q, float* scale, void* h_out, int64_t ld_h, void* stream);

/* K1l — K1 fused into LayerNorm (GPT-2, StarCoder2, GPT-NeoX, Falcon, Phi, OPT and the encoders): quantize(LayerNorm(x; weight, bias, eps)) per token in one pass,
 * the normalised activation never reaching HBM unless h_out asks for it.  x: [rows, cols], weight: [cols], bias: [cols] or NULL (no bias, no add), all of `dtype`.
 * Numerics, QSPEC L1-L6, all binary32, round to nearest even, no contraction: mean = (sum x) / cols and var = (sum (x - mean)^2) / cols, a true
 * two-pass computation, both sums in the pinned order of pq_rmsnorm_quant_rowwise (16-byte vectors dealt to 256 lanes, per lane a plain add resp. an fma per element,
 * xor butterfly per 64 lanes, four partial sums left to right: every row layout gives the same bits); rs = 1 / sqrt(var + eps) with IEEE sqrt and division;
 * h = cast_rne(((x - mean) * rs) * weight + bias), every operation rounded in binary32 and ONE storage rounding (what torch's layer_norm does on a 16-bit tensor;
 * pq_rmsnorm_quant_rowwise rounds twice because transformers' RMSNorm does); then Q1-Q6 on the rows of h.  A NaN or Inf anywhere in a row makes the whole row NaN
 * (scale = the canonical NaN, codes 0).
 * q, scale and h_out may overlap neither x, weight, bias nor each other (PQ_ERR_BAD_ARG: an in-place h_out is not tolerated, the layouts re-read clamped duplicates
 * of x).  A null x / weight / q / scale, ld < cols, cols >= 2^24, a negative or non-finite eps and an unknown dtype are PQ_ERR_BAD_ARG before any HIP call, with
 * pq_last_error naming the argument.  rows == 0 or cols == 0: nothing is read or written, returns PQ_OK.  Row layouts and the PQ_RMS_WAVE_MAX switch as
 * pq_rmsnorm_quant_rowwise (time only, never bits). */
int32_t pq_layernorm_quant_rowwise(const void* x, int64_t ld_x, const void* weight, const void* bias, float eps, int32_t dtype, int64_t rows, int64_t cols,
                                   int8_t* q, int64_t ld_q, float* scale, void* h_out, int64_t ld_h, void* stream);

/* K1al — the residual add that precedes a LayerNorm in a decoder layer, fused into K1l: sum_out = x + residual (QSPEC A1: one binary32 add and one storage rounding
 * per element — what an eager add stores), then pq_layernorm_quant_rowwise on the rows of sum_out AS STORED (L1-L6, Q1-Q6), in one kernel.  Every output holds the
 * bits of the two-launch form.  x, residual, sum_out: [rows, cols] of `dtype` with leading dimensions ld_x, ld_r, ld_s (elements); weight, bias: [cols] of the same
 * dtype, bias nullable.  sum_out is required and may be x or residual themselves (same pointer and leading dimension); any other overlap of sum_out with an input,
 * and any overlap of q, scale or h_out with another operand, returns PQ_ERR_BAD_ARG — as do a null operand (bias and h_out excepted), ld < cols, cols >= 2^24, a
 * negative or non-finite eps and an unknown dtype — before any HIP call, with pq_last_error naming the argument.  rows == 0 or cols == 0: nothing is read or
 * written, returns PQ_OK.  Row layouts and the PQ_RMS_WAVE_MAX switch as pq_rmsnorm_quant_rowwise (time only, never bits). */
int32_t pq_add_layernorm_quant_rowwise(const void* x, int64_t ld_x, const void* residual, int64_t ld_r, void* sum_out, int64_t ld_s, const void* weight, const void* bias,
                                       float eps, int32_t dtype, int64_t rows, int64_t cols, int8_t* q, int64_t ld_q, float* scale, void* h_out, int64_t ld_h, void* stream);

/* K1pl / K1l2 — the parallel residual of a GPT-NeoX (use_parallel_residual) or Phi decoder block, fused into the LayerNorm(s) of the NEXT block:
 *   sum_out = cast_rne(f32(cast_rne(f32(a) + f32(b))) + f32(c))      QSPEC A2: A1 twice, in THIS association; the inner sum is never stored
 * then, on the rows of sum_out AS STORED, the mean and the variance of L1-L3 ONCE, and per norm group g = 1, 2 its own L4 (eps_g), L5 (weight_g, bias_g; bias_g
 * nullable) and L6 = Q1-Q6, in one kernel.  Every output holds the bits of two eager adds in that association followed by pq_layernorm_quant_rowwise per group.
 * Addition commutes, so a and b may be swapped; the three may not be regrouped (the groupings differ in about 30 % of random elements): pass the operands in the order
 * the model adds them.  a, b, c, sum_out: [rows, cols] of `dtype` with leading dimensions in elements; weight_g, bias_g: [cols] of the same dtype.
 *   a and b both null:   no add (K1l2, the "dual norm": c is normalised as it is); sum_out must be null and both groups are required — one norm without an add is
 *                        pq_layernorm_quant_rowwise, and asking for it here is PQ_ERR_BAD_ARG.  Exactly one of a, b null is PQ_ERR_BAD_ARG.
 *   weight2 null:        one norm; bias2, q2, scale2 and h2 must be null as well.
 * sum_out is required with the add and may be exactly one of a, b, c (same pointer and leading dimension); any other overlap of sum_out with an input, and any
 * overlap of q1, scale1, h1, q2, scale2 or h2 with another operand, is PQ_ERR_BAD_ARG — as are a null operand (the biases and h1 / h2 excepted), ld < cols,
 * cols >= 2^24, a negative or non-finite eps1 / eps2 and an unknown dtype — before any HIP call, with pq_last_error naming the argument.  rows == 0 or cols == 0:
 * nothing is read or written, returns PQ_OK.  Row layouts and the PQ_RMS_WAVE_MAX switch as pq_rmsnorm_quant_rowwise (time only, never bits). */
int32_t pq_parallel_layernorm_quant_rowwise(const void* a, int64_t ld_a, const void* b, int64_t ld_b, const void* c, int64_t ld_c, void* sum_out, int64_t ld_s,
                                            const void* weight1, const void* bias1, float eps1, const void* weight2, const void* bias2, float eps2, int32_t dtype,
                                            int64_t rows, int64_t cols, int8_t* q1, int64_t ld_q1, float* scale1, void* h1, int64_t ld_h1, int8_t* q2, int64_t ld_q2,
                                            float* scale2, void* h2, int64_t ld_h2, void* stream);

/* K1u — K1 fused into the unary activation of a plain two-linear MLP (c_proj(act(c_fc(x)))): quantize(act(x)) per token in one pass.  x: [rows, cols] of `dtype`,
 * possibly a column block of a wider tensor (ld_x > cols).  Numerics, QSPEC U1-U4, binary32 throughout and ONE storage rounding of h:
 *   PQ_ACT_RELU       h = x < 0 ? +0 : x                        (a NaN and -0 pass: torch.relu, bit for bit)
 *   PQ_ACT_GELU_TANH  h = x / (1 + exp_spec(-a)), a = x * fma(x * x, K1, K0), K0 = 2 sqrt(2 / pi), K1 = 0.044715 K0   (the tanh GELU without its 1 + tanh
 *                     cancellation: 0.5 x (1 + tanh(u)) = x / (1 + exp(-2 u)))
 *   PQ_ACT_GELU_ERF   h = x * Phi(x), Phi(x) = 0.5 erfc(-x / sqrt 2) from a specified binary32 sequence (a degree-10 polynomial of (t - 4) / (t + 4), t = min(|x|, 12),
 *                     times exp_spec(-t^2 / 8)^4)
 * exp_spec is QSPEC S1-S4.  Both GELUs are within 1 ulp of the storage dtype of the exact value for every bf16 / fp16 input (exact values below 2^-96 become -0);
 * NaN -> NaN, +Inf -> +Inf, -Inf -> -0.  Then Q1-Q6 on the rows of h.  h_out (nullable, ld_h): also store h.
 * q, scale and h_out may overlap neither x nor each other.  An unknown kind or dtype, a null x / q / scale, negative sizes and ld < cols are PQ_ERR_BAD_ARG before any
 * HIP call, with pq_last_error naming the argument.  rows == 0 or cols == 0: nothing is read or written, returns PQ_OK.  Row layouts as pq_silu_mul_quant_rowwise
 * (PQ_SILU_TPR included: time only, never bits). */
#define PQ_ACT_RELU 0
#define PQ_ACT_GELU_TANH 1
#define PQ_ACT_GELU_ERF 2
int32_t pq_act_quant_rowwise(const void* x, int64_t ld_x, int32_t dtype, int64_t rows, int64_t cols, int32_t kind, int8_t* q, int64_t ld_q, float* scale,
                             void* h_out, int64_t ld_h, void* stream);

/* K1ng — K1 fused into GemmaRMSNorm (Gemma, Gemma-2, Gemma-3): quantize(((x.float() * rsqrt(mean(x.float()^2) + eps)) * (1.0 + weight.float())).to(dtype)) per token in
 * one pass.  Arguments, layouts and the PQ_RMS_WAVE_MAX switch as pq_rmsnorm_quant_rowwise; `weight` is the STORED weight w, the gain is 1 + w.  Numerics, QSPEC
 * NG1-NG6: the sum of squares and rs exactly as N1-N4, then g = 1.0f + f32(w) and h = cast_rne((f32(x) * rs) * g), every operation rounded in
 * binary32, no contraction, ONE storage rounding (pq_rmsnorm_quant_rowwise rounds x * rs to the storage dtype first: 1 + w folded into its weight gives other bits);
 * then Q1-Q6 on the rows of h.
 * q, scale and h_out may overlap neither x, weight nor each other.  A null x / weight / q / scale, ld < cols, cols >= 2^24, a negative or non-finite eps and an unknown
 * dtype are PQ_ERR_BAD_ARG before any HIP call, with pq_last_error naming the argument.  rows == 0 or cols == 0: nothing is read or written, returns PQ_OK. */
int32_t pq_gemma_rmsnorm_quant_rowwise(const void* x, int64_t ld_x, const void* weight, float eps, int32_t dtype, int64_t rows, int64_t cols, int8_t* q, int64_t ld_q,
                                       float* scale, void* h_out, int64_t ld_h, void* stream);

/* K1ang — the residual add fused into pq_gemma_rmsnorm_quant_rowwise: sum_out = cast_rne(f32(x) + f32(residual)) is STORED (QSPEC A1) and its rows AS STORED go through
 * NG1-NG6 and Q1-Q6.  Arguments, aliasing (sum_out may BE x or residual: same pointer and leading dimension), checks and no-op cases as pq_add_rmsnorm_quant_rowwise;
 * every output holds the bits of the add followed by pq_gemma_rmsnorm_quant_rowwise. */
int32_t pq_add_gemma_rmsnorm_quant_rowwise(const void* x, int64_t ld_x, const void* residual, int64_t ld_r, void* sum_out, int64_t ld_s, const void* weight, float eps,
                                           int32_t dtype, int64_t rows, int64_t cols, int8_t* q, int64_t ld_q, float* scale, void* h_out, int64_t ld_h, void* stream);

/* K1pang — the sandwich residual flow of Gemma-2 / Gemma-3 in one launch: the post-norm of the sublayer output, the residual add, the next norm and K1.  Per row, with x the
 * sublayer output and residual the residual stream (QSPEC PN1, A1, NG1-NG6, Q1-Q6):
 *   p = cast_rne((f32(x) * rs_p) * (1.0f + f32(post_weight)))   NG1-NG5 on x with post_weight / post_eps; ROUNDED to the storage dtype, never written to memory
 *   sum_out = cast_rne(f32(residual) + f32(p))                  STORED: the new residual stream (A1)
 *   then NG1-NG6 and Q1-Q6 on the rows of sum_out AS STORED, with weight / eps -> q, scale, optionally h_out.
 * Every output holds the bits of pq_gemma_rmsnorm_quant_rowwise(x, post_weight, post_eps) with h_out, a correctly rounded add of its h to residual, and
 * pq_gemma_rmsnorm_quant_rowwise(sum, weight, eps).  post_weight, weight: [cols] of `dtype` (the STORED weights w; the gains are 1 + w).  Row layouts and the
 * PQ_RMS_WAVE_MAX switch as pq_rmsnorm_quant_rowwise (time only, never bits).
 * K1pa, the add-only form: weight == q == scale == h_out == NULL stops after the add and stores sum_out alone (eps is not read).  A partly-null group is PQ_ERR_BAD_ARG
 * naming the missing argument.
 * Aliasing: sum_out may BE x or residual (same pointer and leading dimension; the whole row of x is read before any of sum_out is written); any other overlap of
 * sum_out with an input, and any overlap of q, scale or h_out with an input, sum_out or each other, is refused.  A null x / post_weight / residual / sum_out, ld < cols,
 * cols >= 2^24, a negative or non-finite eps or post_eps and an unknown dtype are PQ_ERR_BAD_ARG before any HIP call, with pq_last_error naming the argument.
 * rows == 0 or cols == 0: nothing is read or written, returns PQ_OK (the scales of empty rows are 1, QSPEC Q3: the caller's). */
int32_t pq_gemma_postnorm_add_rmsnorm_quant_rowwise(const void* x, int64_t ld_x, const void* post_weight, float post_eps, const void* residual, int64_t ld_r, void* sum_out,
                                                    int64_t ld_s, const void* weight, float eps, int32_t dtype, int64_t rows, int64_t cols, int8_t* q, int64_t ld_q, float* scale,
                                                    void* h_out, int64_t ld_h, void* stream);

/* K1oq — the post-norm residual flow of OLMo-2 / OLMo-3 in one launch: the norm of the sublayer output, the residual add and K1 on the sum.  Per row, with x the sublayer
 * output and residual the residual stream (QSPEC NO1-NO5, PO1, A1, Q1-Q6):
 *   p = cast_rne((f32(x) * rs) * f32(post_weight))      NO1-NO5: N1-N4's sum of squares and rs, binary32 throughout, ONE storage rounding, gain w; never written (PO1)
 *   sum_out = cast_rne(f32(residual) + f32(p))          STORED: the new residual stream (A1)
 *   then Q1-Q6 on the rows of sum_out AS STORED -> q, scale (there is no second norm and no h_out: what is quantised is sum_out itself).
 * The three forms, by which operands are null:
 *   K1oq  every operand given.
 *   K1oa  q == scale == NULL: stores sum_out alone (the end of a chain).
 *   K1on  residual == NULL and q == scale == NULL: stores p itself to sum_out (the norm alone: q_norm / k_norm; ld_r is not read).
 * q and scale go together, and q needs residual: a partly-null group is PQ_ERR_BAD_ARG naming the missing argument.  post_weight: [cols] of `dtype`.  Row layouts and the
 * PQ_RMS_WAVE_MAX switch as pq_rmsnorm_quant_rowwise (time only, never bits).
 * Aliasing: sum_out may BE x or residual (same pointer and leading dimension; the whole row of x is read before any of sum_out is written) — with residual == NULL, x
 * alone; any other overlap of sum_out with an input, and any overlap of q or scale with an input, sum_out or each other, is refused.  A null x / post_weight / sum_out,
 * ld < cols, cols >= 2^24, a negative or non-finite post_eps and an unknown dtype are PQ_ERR_BAD_ARG before any HIP call, with pq_last_error naming the argument.
 * rows == 0 or cols == 0: nothing is read or written, returns PQ_OK (the scales of empty rows are 1, QSPEC Q3: the caller's). */
int32_t pq_olmo_postnorm_add_quant_rowwise(const void* x, int64_t ld_x, const void* post_weight, float post_eps, const void* residual, int64_t ld_r, void* sum_out,
                                           int64_t ld_s, int32_t dtype, int64_t rows, int64_t cols, int8_t* q, int64_t ld_q, float* scale, void* stream);

/* K1ma — the SCALED residual add of the Granite decoders (r1 = x + attn(norm(x)) * m, out = r1 + mlp(norm(r1)) * m) fused into pq_rmsnorm_quant_rowwise: K1a with one
 * multiply and one rounding in front of the add.  Per element, with x the sublayer output and residual the residual stream (QSPEC S1, A1):
 *   p = cast_rne(f32(x) * multiplier)                   S1: one binary32 product, one storage rounding (f32 rows: the binary32 product, rounded on its own); never written
 *   sum_out = cast_rne(f32(residual) + f32(p))          STORED: the new residual stream (A1) — two roundings, never fma(x, multiplier, residual)
 *   then N1-N6 and Q1-Q6 on the rows of sum_out AS STORED -> q, scale (and h_out when given).
 * This is what `residual + x * m` computes in eager torch for a Python number m (rounded once to binary32: it crosses this ABI as a float), so q, scale, sum_out and
 * h_out are those of pq_add_rmsnorm_quant_rowwise run on p, bit for bit; multiplier == 1 gives K1a's bits.  7 B/elem for 16-bit rows against 13 for the three launches.
 * K1mo, the add-only form: weight == q == scale == h_out == NULL stops after the add and stores sum_out alone (eps is not read).  A partly-null group is
 * PQ_ERR_BAD_ARG naming the missing argument.
 * Arguments, aliasing (sum_out may BE x or residual: same pointer and leading dimension; every other overlap is refused), checks and no-op cases as
 * pq_add_rmsnorm_quant_rowwise; a NaN or infinite multiplier is PQ_ERR_BAD_ARG naming it.  Row layouts and the PQ_RMS_WAVE_MAX switch as pq_rmsnorm_quant_rowwise (time
 * only, never bits). */
int32_t pq_scaled_add_rmsnorm_quant_rows(const void* x, int64_t ld_x, const void* residual, int64_t ld_r, float multiplier, void* sum_out, int64_t ld_s, const void* weight,
                                         float eps, int32_t dtype, int64_t rows, int64_t cols, int8_t* q, int64_t ld_q, float* scale, void* h_out, int64_t ld_h, void* stream);

/* K1hn — the per-head RMSNorm of an attention's q and k (q_norm / k_norm of Qwen3, Qwen3-MoE, Gemma-3) in one launch; no codes, no scales (QSPEC HN1; DESIGN.md
 * section 2).  The rows are heads of `cols` = head_dim elements, addressed by TWO strides, in elements, for x and for out:
 *   out[o * ld_oo + i * ld_oi + c] = norm(x[o * ld_xo + i * ld_xi + c]; weight, eps)      o < n_outer, i < n_inner, c < cols
 * so the q slice of a fused q/k/v output ([tokens, ld] x [heads, head_dim]) or a transposed view of it is normed where it lies.  weight: ONE [cols] of `dtype` for all
 * rows.  gain: PQ_GAIN_LLAMA — N1-N5, cast_rne(f32(w) * f32(cast_rne(f32(x) * rs))), Qwen3RMSNorm; PQ_GAIN_GEMMA — NG1-NG5, cast_rne((f32(x) * rs) * (1 + f32(w))),
 * Gemma3RMSNorm.  The bits are those h_out of pq_rmsnorm_quant_rowwise / pq_gemma_rmsnorm_quant_rowwise holds for the same rows.  Layouts (time only, never bits): a
 * width of whole 16-byte vectors up to 1024 bytes with 16-byte aligned bases and strides packs 64 / G heads into a wave (G = the power of two >= cols * elem / 16, at
 * least 4); anything else takes one wave per head, element by element.  No switch of its own.
 * There is no in-place form: out may overlap neither x nor weight (told apart by their bounding ranges), and the rows of out may not overlap each other.  A null x /
 * weight / out, a negative size or stride, n_outer * n_inner >= 2^31, cols >= 2^24, ld_xi < cols or ld_oi < cols where n_inner > 1, a negative or non-finite eps and an
 * unknown gain or dtype are PQ_ERR_BAD_ARG before any HIP call, with pq_last_error naming the argument.  n_outer * n_inner == 0 or cols == 0: nothing is read or
 * written, returns PQ_OK. */
#define PQ_GAIN_LLAMA 0
#define PQ_GAIN_GEMMA 1
int32_t pq_head_rmsnorm(const void* x, int64_t ld_xo, int64_t ld_xi, const void* weight, float eps, int32_t gain, int32_t dtype, int64_t n_outer, int64_t n_inner,
                        int64_t cols, void* out, int64_t ld_oo, int64_t ld_oi, void* stream);

/* K1gg— K1 fused into the tanh-GELU gate of a gated MLP (Gemma's down(act_fn(gate(x)) * up(x)), act_fn = gelu_pytorch_tanh): quantize(gelu_tanh(g) * u) per token in
 * one pass.  g, u: [rows, cols] of `dtype` with leading dimensions of their own (the column halves of one fused gate+up output qualify).  Numerics, QSPEC GG1-GG3:
 * a = cast_rne(gelu_tanh(f32(g))) with the tanh GELU of pq_act_quant_rowwise (QSPEC U2: NaN -> NaN, +Inf -> +Inf, -Inf -> -0), h = cast_rne(f32(a) * f32(u)), then Q1-Q6
 * on the rows of h — the eager chain op for op (the activation is stored, then multiplied).  kind: PQ_ACT_GELU_TANH only; anything else is PQ_ERR_BAD_ARG naming `kind`.
 * h_out (nullable, ld_h): also store h.  q, scale and h_out may overlap neither g, u nor each other.  An unknown dtype, a null g / u / q / scale, negative sizes and
 * ld < cols are PQ_ERR_BAD_ARG before any HIP call, with pq_last_error naming the argument.  rows == 0 or cols == 0: nothing is read or written, returns PQ_OK.  Row
 * layouts as pq_silu_mul_quant_rowwise (PQ_SILU_TPR included: time only, never bits). */
int32_t pq_gelu_mul_quant_rowwise(const void* g, int64_t ld_g, const void* u, int64_t ld_u, int32_t dtype, int64_t rows, int64_t cols, int32_t kind, int8_t* q, int64_t ld_q,
                                  float* scale, void* h_out, int64_t ld_h, void* stream);

/* dequantize(): out[r,c] = cast_rne(f32(q[r,c]) * scale[axis==0 ? c : r]).  `axis` is the axis the
 * scale was reduced over (1: one scale per row, 0: one scale per column).   QSPEC D1. */
int32_t pq_dequant(const int8_t* q, int64_t ld_q, const float* scale, int32_t axis,
                   int64_t rows, int64_t cols, void* out, int64_t ld_out, int32_t out_dtype, void* stream);

/* OPERANDS OF THE DENSE GEMM ENTRIES (pq_gemm_s8s8s32, pq_qlinear_s8, pq_qlinear_s8_t, pq_qlinear_s8_kslabs, pq_qlinear_dyn): a[M, K] and b[N, K] are row-major int8
 * with leading dimensions lda, ldb >= K in elements (for stacked codes lda >= k_per_slab), the output has ldy >= N (ldyt >= M); a smaller one is PQ_ERR_BAD_ARG before
 * any HIP call.  Any such operands give the same bits; which kernel runs depends on them.  The MFMA tiles and the weight-streaming kernel need 16-byte aligned bases of
 * a and b, lda and ldb multiples of 16 and below 2^23 (their loaders keep 255 rows x ld in a 32-bit offset), and K a positive multiple of 128: a column window of a
 * wider buffer qualifies when it starts on a 16-byte boundary (no 128- or 256-byte alignment is needed).  Everything else — an odd base or leading dimension, ld >= 2^23,
 * any other K — runs the generic kernel: about 300 TOPS where the tiles do 2000+, and about 50 when the rows are not 16-byte aligned.  pq_gemm_variant_name(M, N, K,
 * lda, ldb) answers for the leading dimensions it is given and ASSUMES 16-byte aligned bases: "generic64" for operands that leave the fast path by their leading
 * dimensions or K (also when PQ_FORCE_VARIANT names a tile); it cannot see a misaligned base.  The workspace queries take no leading dimensions and assume the fast path. */

/* K3 debug/parity twin — c[M,N] = sum_k a[M,k] * b[N,k], exact int32: the drop-in for
 * torch._int_mm(a, b.t()) (aten::_int_mm), which BASELINE.json names as the CPU oracle. */
int32_t pq_gemm_s8s8s32(const int8_t* a, int64_t lda, const int8_t* b, int64_t ldb,
                        int32_t* c, int64_t ldc, int64_t M, int64_t N, int64_t K, void* stream);

/* K3+K4 — int8 GEMM on v_mfma_i32_*_i8 with the fused dequant epilogue:
 *   y[m,n] = cast_rne_out((f32(acc[m,n]) * a_scale[m]) * b_scale[n] (+ f32(bias[n])))   QSPEC E1-E4.
 * bias is nullable and has the output dtype.
 * workspace: optional.  pq_qlinear_workspace_bytes(M,N,K) > 0 marks problems (small M*N, long K) for which a
 * 16-byte aligned device workspace of that size enables split-K — partial int32 sums either in slabs of the whole
 * output + an exact integer reduction pass, or handed over between the workgroups of a tile inside the GEMM kernel
 * (tickets + per-tile slabs; the call re-initialises the tickets itself): results are bit-identical.  The contents need
 * not be initialised or preserved; one workspace must not serve two calls that may run concurrently.  With
 * workspace == NULL the single-pass kernel runs instead.  A workspace of exactly the queried size is enough, a smaller one is
 * PQ_ERR_WORKSPACE before anything is launched, and the query is 0 wherever the call would not look at one (a dispatch that has no
 * split form: M * N < 128^2, at most 64 tokens, a forced variant, a non-positive size): tests/test_gpu_workspace_bounds.py.
 * Liveness of the in-kernel hand-over: the default (ticket) form never waits for a workgroup that may not be running —
 * the workgroups of a tile that finish first store their partial sums and leave, the last one adds them — so it is safe
 * under any placement: several such GEMMs on concurrent streams, CU-masked queues, partitioned devices, a co-running
 * persistent kernel.  It is planned only when tiles x slices <= the CUs the current device reports (a performance rule).
 * Visibility of the handed-over sums rests on write-through (sc1) stores whose acknowledgement (vmcnt) precedes the ticket,
 * and agent-scope (sc1) loads behind a poll + barrier: a sequence measured valid on gfx950 / ROCm 7.2, not
 * an architectural guarantee; PQ_FSK_FENCED=1 adds the documented release / acquire (buffer_wbl2 sc1 / buffer_inv sc1) as
 * a fallback, at ~35 us per launch.
 * PQ_FSK_SYMMETRIC=1 opts into the symmetric exchange for 2 / 4 slices (each workgroup keeps a part of the tile and
 * WAITS for its partners' contributions: 2-5 % faster): the caller then guarantees that every workgroup of the launch
 * can be resident at once — no second fused split-K GEMM in flight on another stream, no CU mask — and the planner
 * additionally refuses it when tiles x slices exceeds the device's CU count.  PQ_FSK_COOP=1 launches those symmetric kernels
 * COOPERATIVELY instead (hipLaunchCooperativeKernel: the runtime guarantees co-residency or refuses, then the ticket form runs) — correct, also under
 * hipGraph capture, but measured 21-24 us slower per launch than the ticket form on ROCm 7.2 (profiles/r05_ab_fsk_coop.txt): opt-in.
 * Output rows that are not 16-byte aligned (an odd ldy, e.g. a 50257-wide vocabulary): the staged epilogue stores its 16-byte pieces at element-aligned addresses,
 * which needs the queue's unaligned-access mode (SH_MEM_CONFIG alignment mode "unaligned" — the default of ROCm compute queues on gfx9, but a platform setting, not an
 * architectural guarantee: some virtual functions and debug configurations run strict).  On such a platform set PQ_EPI_ANY_ALIGN=0 (environment or pq_set_option): those
 * rows then take the slower guarded direct stores; everything else is unaffected. */
int32_t pq_qlinear_s8(const int8_t* a, int64_t lda, const float* a_scale,
                      const int8_t* b, int64_t ldb, const float* b_scale,
                      const void* bias, void* y, int64_t ldy, int32_t out_dtype,
                      int64_t M, int64_t N, int64_t K,
                      void* workspace, size_t workspace_bytes, void* stream);
size_t pq_qlinear_workspace_bytes(int64_t M, int64_t N, int64_t K);

/* The same qlinear with the output TRANSPOSED: yt[N, M] (leading dimension ldyt), yt[n][m] bit-identical to pq_qlinear_s8's
 * y[m][n] (the epilogue keeps QSPEC's order — token scale first — although the tokens are now the GEMM's columns; the bias
 * runs along rows).  For the column-sharded configuration (SURVEY.md §8(e) option 1): the ranks' yt shards [N/G, M] are row
 * blocks of yt, so the all-gather is contiguous and needs no layout pass (pq_allgather_rows_t in pq_rccl.h).
 * Arguments as pq_qlinear_s8 (a, a_scale: activation codes [M, K] and token scales; b, b_scale: weight codes [N, K] and
 * channel scales); workspace per pq_qlinear_t_workspace_bytes(M, N, K).  With few tokens (where pq_qlinear_s8 would run its
 * weight-streaming kernel) the product is computed in the normal orientation and only STORED transposed. */
size_t pq_qlinear_t_workspace_bytes(int64_t M, int64_t N, int64_t K);
int32_t pq_qlinear_s8_t(const int8_t* a, int64_t lda, const float* a_scale, const int8_t* b, int64_t ldb,
                        const float* b_scale, const void* bias, void* yt, int64_t ldyt, int32_t out_dtype, int64_t M,
                        int64_t N, int64_t K, void* workspace, size_t workspace_bytes, void* stream);

/* pq_qlinear_s8 on STACKED activation codes: K-slab s — the columns [s * k_per_slab, (s + 1) * k_per_slab) of the logical a[M, K] — is the row-major
 * block a + s * slab_stride with leading dimension lda (what an all-gather of the ranks' int8 column blocks [M, K / G] leaves: slab_stride = M * K / G).
 * An integer sum has no order: the result is pq_qlinear_s8's on the row-major matrix, bit for bit.  Three ways, in this order:
 *   (1) where pq_qlinear_s8 would run the fused split-K of the 256 x 256 tile (the Llama-70B `down` shard 4096 x 1024 x 28672: four K-slices) AND a workspace of
 *       the hand-over's size is passed AND the slices cover whole slabs (or a slab holds whole slices; >= 512 columns per slab): that kernel walks the slabs in
 *       place — its K-loop's activation cursor jumps at the slab boundaries (round 6);
 *   (2) where the planner picks a ring tile (128 x 128, 64 x 128, 64 x 64: the Llama-70B `o` shard, and the `down` shard when no workspace comes): its loaders walk
 *       the slabs in place — no layout pass, no workspace;
 *   (3) any other shape: ONE layout pass into `workspace` (M * K bytes read and written), then pq_qlinear_s8.
 * K % k_per_slab == 0.  Workspace (256-byte aligned): pq_qlinear_kslabs_workspace_bytes is the size that is ALWAYS enough (way 3's: it knows neither base nor
 * strides); pq_qlinear_kslabs_workspace_bytes_for decides on the very operands of the call (only their alignment is looked at, nothing is read): way 1's hand-over
 * slabs, 0 for way 2, way 3's otherwise.  A workspace smaller than way 1 needs is not an error: ways 2 / 3 follow. */
size_t pq_qlinear_kslabs_workspace_bytes(int64_t M, int64_t N, int64_t K, int64_t k_per_slab);
size_t pq_qlinear_kslabs_workspace_bytes_for(const int8_t* a, int64_t lda, int64_t slab_stride, int64_t k_per_slab, const int8_t* b, int64_t ldb,
                                             int64_t M, int64_t N, int64_t K);
/* which way a call with these operands and a workspace of workspace_bytes takes: "in place: fused split-K x4", "in place: ring128", "layout pass", ... (static string) */
const char* pq_kslabs_way_name(const int8_t* a, int64_t lda, int64_t slab_stride, int64_t k_per_slab, const int8_t* b, int64_t ldb,
                               int64_t M, int64_t N, int64_t K, size_t workspace_bytes);
int32_t pq_qlinear_s8_kslabs(const int8_t* a, int64_t lda, int64_t slab_stride, int64_t k_per_slab, const float* a_scale, const int8_t* b, int64_t ldb,
                             const float* b_scale, const void* bias, void* y, int64_t ldy, int32_t out_dtype, int64_t M, int64_t N, int64_t K,
                             void* workspace, size_t workspace_bytes, void* stream);

/* GROUPED qlinear for mixture-of-experts layers — ONE launch over all E experts (gemm_s8_grouped.hip):
 *   y[r, :] = cast_rne_out((f32(xq[src(r), :] . wq[e(r)]^T) * xs[r]) * ws[e(r)][:] (+ f32(bias[e(r)][:])))      for the rows r of a token list SORTED BY EXPERT:
 * rows offsets[e] .. offsets[e + 1] - 1 belong to expert e.  Every output row has the bits pq_qlinear_s8 gives when it is run once per expert on that expert's row slice
 * (same MFMA, exact integer sums, the same per-element epilogue).
 *  - offsets: int32[E + 1] in DEVICE memory, non-decreasing, offsets[0] = 0, offsets[E] <= M_total.  The host never reads it (no copy, no synchronisation, no allocation):
 *    the grid is sized from E and M_total alone, so a captured hipGraph stays valid when the CONTENTS of offsets (and of a_row_index) change between replays.  Rows
 *    offsets[E] .. M_total - 1 of y are not written.  Values outside [0, M_total] are clamped by the kernel: wrong offsets give wrong results, never a wild access.
 *  - a_row_index (nullable): int32[M_total] in device memory; grouped row r reads its codes from row a_row_index[r] of xq — the un-permuted [x_rows, K] code matrix, where a
 *    token routed to top_k experts appears top_k times in the list — so no permuted copy of the codes is made.  Then x_rows * ldx < 2^32 (the loader's per-lane source
 *    offset is 32 bits); indices are clamped into [0, x_rows).  Without it row r reads row r of xq (x_rows >= M_total).
 *  - xs: row scales in GROUPED order, [M_total] (gathering 4 bytes per row is the caller's job).  wq: [E][N][K] int8, expert e at wq + e * w_expert_stride with leading
 *    dimension ldw; ws: [E][N] column scales; bias: [E][N] in the output dtype, nullable.
 *  - K a multiple of 128, ldx and ldw multiples of 16 (the modules pad K with zeros, as for pq_qlinear_s8's fast tiles), xq and wq 16-byte aligned, 1 <= E <= 1024.
 *    M_total == 0 (or N == 0) is a no-op.  No workspace.
 * Tiles: 64(m) x 128(n) or 64 x 64 loader / consumer ring tiles, chosen from the upper bound ceil(M_total / 64) + E of the m-tiles, N and the device's CU count
 * (pq_grouped_variant_name; PQ_GROUPED_TILE = 64x128 | 64x64 forces one, PQ_GROUPED_ROT=1 rotates the K walk between the m-tiles of one expert — time only, never bits: tests/test_gpu_grouped_edges.py). */
int32_t pq_qlinear_s8_grouped(const int8_t* xq, int64_t ldx, const int32_t* a_row_index, int64_t x_rows, const float* xs,
                              const int8_t* wq, int64_t ldw, int64_t w_expert_stride, const float* ws, const void* bias,
                              const int32_t* offsets, int32_t E, int64_t M_total, int64_t N, int64_t K,
                              void* y, int64_t ldy, int32_t out_dtype, void* stream);
/* ... and its debug / parity twin: acc[r, :] = xq[src(r), :] . wq[e(r)]^T, exact int32 (pq_gemm_s8s8s32 per expert). */
int32_t pq_gemm_s8s8s32_grouped(const int8_t* xq, int64_t ldx, const int32_t* a_row_index, int64_t x_rows,
                                const int8_t* wq, int64_t ldw, int64_t w_expert_stride,
                                const int32_t* offsets, int32_t E, int64_t M_total, int64_t N, int64_t K,
                                int32_t* acc, int64_t ldacc, void* stream);
/* "grouped64x128_16x16x64" | "grouped64x64_16x16x64": the tile the grouped launch would use (static string). */
const char* pq_grouped_variant_name(int32_t E, int64_t M_total, int64_t N, int64_t K);

/* The grouped qlinear AT DECODE — at most 64 grouped rows (gemm_s8_grouped_stream.hip): the contract, operands and bits of pq_qlinear_s8_grouped above, restricted to
 * M_total <= 64 (more is PQ_ERR_BAD_ARG, before any HIP call), served by the weight-streaming kernel instead of a 64-row tile: ceil(N / 16 RB) weight blocks x
 * min(E, M_total) expert slots are launched, slot j finds the j-th expert that owns a row from `offsets` on the device, KS waves per workgroup split K and stream that
 * expert's weight rows straight into MFMA operands — the weights of a live expert are read once, an expert without a row costs nothing but its slot's early exit.  No
 * workspace, no atomics, no wait between workgroups; graph-capturable, a replay is right when only the contents of offsets / a_row_index / xs change.  Entry points of
 * their own: pq_qlinear_s8_grouped and pq_grouped_variant_name keep planning the tile kernels at every M_total.
 * PQ_GROUPED_STREAM_KS (waves per workgroup: a power of two <= 16) and PQ_GROUPED_STREAM_RB (1 | 2 weight blocks per wave; 2 only while M_total <= 32) force the plan —
 * time only, never bits: tests/test_gpu_grouped_stream.py. */
int32_t pq_qlinear_s8_grouped_stream(const int8_t* xq, int64_t ldx, const int32_t* a_row_index, int64_t x_rows, const float* xs,
                                     const int8_t* wq, int64_t ldw, int64_t w_expert_stride, const float* ws, const void* bias,
                                     const int32_t* offsets, int32_t E, int64_t M_total, int64_t N, int64_t K,
                                     void* y, int64_t ldy, int32_t out_dtype, void* stream);
int32_t pq_gemm_s8s8s32_grouped_stream(const int8_t* xq, int64_t ldx, const int32_t* a_row_index, int64_t x_rows,
                                       const int8_t* wq, int64_t ldw, int64_t w_expert_stride,
                                       const int32_t* offsets, int32_t E, int64_t M_total, int64_t N, int64_t K,
                                       int32_t* acc, int64_t ldacc, void* stream);
/* "gstream_mt<1|2|4>_rb<1|2>_ks<1..16>_16x16x64": token tiles the kernel is compiled for, weight blocks per wave and waves per workgroup of that launch (static string). */
const char* pq_grouped_stream_plan_name(int32_t E, int64_t M_total, int64_t N, int64_t K);

/* ROUTING of a mixture-of-experts layer (moe_kernels.hip, kernel R): the (token, slot) pairs of topk_ids[T, k] sorted by expert — a STABLE counting sort of the flat pairs
 * p = t * k + j by topk_ids[t][j].  All outputs int32, in device memory:
 *   offsets[E + 1]   rows offsets[e] .. offsets[e + 1] - 1 of the grouped order belong to expert e (what pq_qlinear_s8_grouped takes as offsets)
 *   row_index[T k]   the token of grouped row r (pq_qlinear_s8_grouped's a_row_index); inside an expert the pairs keep their flat order
 *   rows_of[T, k]    the grouped rows of token t in ascending EXPERT id, ties (one expert twice in a token) by slot
 *   slot_of[T, k]    the slot j of topk_ids[t] each of those rows came from
 *   xs_sorted[T k]   (optional: xs and xs_sorted both given or both NULL) xs_sorted[r] = xs[row_index[r]], the f32 row scales xs[T] in grouped order
 * For ids in [0, E) every output equals protoquant_amd.moe.route_plan(topk_ids, E) element for element, on every run: a pair's place inside its expert is its rank in
 * flat-pair order, never the arrival order of an atomic.
 *  - topk_ids: int32 (ids_are_int64 = 0) or int64 (1) — torch.topk returns int64 —, row stride ld_ids >= k elements.  DEVICE data, never read on the host: an id outside
 *    [0, E) is CLAMPED into the range on its full width (an int64 id is not truncated first: 2^32 + 3 sorts as E - 1) and the result is that of the clamped ids — wrong
 *    ids give a wrong routing, never an access outside the buffers passed in.
 *  - 1 <= E <= 1024, 1 <= k <= 64, T >= 0, T * k < 2^31.  T == 0 writes offsets = zeros and nothing else.
 *  - T * k <= 4096 (every decode step): ONE launch, one workgroup, everything in LDS, no workspace.  Larger: three launches (count per block -> scan -> rank) and a
 *    workspace of pq_moe_route_workspace_bytes(T, k, E) bytes (16-byte aligned; it needs no initialisation and holds nothing between calls).  The size is monotone in T.
 *  - no cooperative launch, no wait on another workgroup, no memset node, no host read, no allocation: capturable into a hipGraph, and a replay is right when only the
 *    CONTENTS of topk_ids (and xs) changed. */
size_t pq_moe_route_workspace_bytes(int64_t T, int32_t k, int32_t E);
int32_t pq_moe_route(const void* topk_ids, int32_t ids_are_int64, int64_t ld_ids, int64_t T, int32_t k, int32_t E,
                     int32_t* offsets, int32_t* row_index, int32_t* rows_of, int32_t* slot_of,
                     const float* xs, float* xs_sorted, void* workspace, size_t workspace_bytes, void* stream);

/* COMBINE of a mixture-of-experts layer (moe_kernels.hip, kernel C): out[t, :] = sum over s = 0 .. k - 1, in that order, of y[rows_of[t, s], :] * w[t, slot_of[t, s]], with
 * the arithmetic of protoquant_amd.moe.combine (an eager loop over the experts that index_adds out_e * w_e into zeros), bit for bit:
 *     acc = +0 (in the dtype of y)
 *     for s:  p   = cast_rne(f32(y[row]) * f32(w))       one binary32 multiply, then the rounding to the dtype
 *             acc = cast_rne(f32(acc) + f32(p))          one binary32 add, then the rounding to the dtype      (no contraction; for f32 the casts are identities)
 * so a token whose only product is -0 gets +0 ((+0) + (-0)), and NaN / Inf rows propagate as the operations above make them.
 *  - y[M_total, H] (leading dimension ldy), out[T, H] (ld_out), topk_w[T, k] (row stride ld_w >= k) all of `dtype`; rows_of, slot_of: int32 [T, k] contiguous, as pq_moe_route
 *    writes them.  They are DEVICE data: rows_of is clamped into [0, M_total), slot_of into [0, k).
 *  - rows of y and out that are 16-byte aligned (base and leading dimension) take 16-byte loads and stores; anything else, and the last H mod (16 / element size)
 *    elements of a row, an element-wise path with the same bits.
 *  - 1 <= k <= 64, T * k < 2^31; T == 0 or H == 0 is a no-op.  One launch, no workspace.  Bandwidth-bound: (k + 1) T H sizeof(dtype) bytes. */
int32_t pq_moe_combine(const void* y, int64_t ldy, int32_t dtype, int64_t M_total, const int32_t* rows_of, const int32_t* slot_of,
                       const void* topk_w, int64_t ld_w, int64_t T, int32_t k, int64_t H, void* out, int64_t ld_out, void* stream);

/* EXPERT SELECTION of a mixture-of-experts router behind its GEMM (moe_topk_kernels.hip, kernel K-rt; QSPEC RT1-RT5): from logits[T, E] the k experts of
 * every token and their routing weights, in ONE launch, where model code runs softmax, topk, a sum, a division and a cast.
 *   ids[t, 0 .. k-1]   the k largest logits of the row, slot 0 the largest (torch.topk(sorted=True)); NaN sorts above +Inf, -0 == +0, EQUAL VALUES GO TO THE LOWER EXPERT
 *                      ID.  Always distinct and in [0, E), whatever the row holds.  The selection compares the logits, not the probabilities.
 *   kind = PQ_ROUTER_SOFTMAX_TOPK (Mixtral, Qwen2-MoE, Qwen3-MoE, OLMoE):  m = l[ids[0]];  x[e] = exp_spec(l[e] - m) (QSPEC S1-S4);  S = the sum of x over the row in the
 *                      pinned order of RT3 (it depends on E alone);  p[j] = x[ids[j]] / S;  with renormalise: s = ((p[0] + p[1]) + ...) in slot order, w[j] = p[j] / s,
 *                      without it w[j] = p[j]
 *   kind = PQ_ROUTER_TOPK_SOFTMAX (GPT-OSS):  x[j] = exp_spec(l[ids[j]] - m);  s = ((x[0] + x[1]) + ...);  w[j] = x[j] / s.  Only the k selected logits decide the
 *                      weights; they sum to one by construction and `renormalise` changes nothing.
 *   weights[t, j] = cast_rne(w[j]) to w_dtype; a NaN weight is the canonical quiet NaN.  Every division is an IEEE binary32 division.  A row whose maximum is NaN or
 *   +-Inf gets NaN weights (inf - inf, as in eager) and the ids above.
 *  - logits: `dtype` (bf16 / fp16 / f32), row stride ld_logits >= E elements; weights: w_dtype (any of the three, independent of `dtype`), row stride ld_w >= k; ids:
 *    int32 (ids_are_int64 = 0) or int64 (1), row stride ld_ids >= k.  Each operand aligned to its element size; the outputs overlap neither each other nor the logits.
 *    The logits are not written.
 *  - 1 <= E <= 1024, 1 <= k <= min(E, 64), T >= 0, T < 2^31.  T == 0 is a no-op.  renormalise: 0 or 1.
 *  - no atomics, no LDS, no workspace, no wait on another workgroup, no host read: capturable into a hipGraph, and a replay is right when only the CONTENTS of the
 *    logits changed.  The bits do not depend on T, on the leading dimensions or on which tokens share a wave. */
#define PQ_ROUTER_SOFTMAX_TOPK 0
#define PQ_ROUTER_TOPK_SOFTMAX 1
int32_t pq_moe_topk(const void* logits, int32_t dtype, int64_t ld_logits, int64_t T, int32_t E, int32_t k, int32_t kind, int32_t renormalise,
                    void* weights, int32_t w_dtype, int64_t ld_w, void* ids, int32_t ids_are_int64, int64_t ld_ids, void* stream);

/* qlinear.forward in ONE call: y[M,N] = qlinear(x[M,K]) with dynamic per-token quantisation of x (K1), the int8 MFMA GEMM
 * and the fused dequant epilogue, output dtype = input dtype.  Scratch (xq, xs, optional split-K slabs) is carved from
 * `workspace` (>= pq_qlinear_dyn_workspace_bytes(M,N,K), 256-byte aligned, caller-owned, reusable across calls on one
 * stream).  Same results, bit for bit, as pq_quant_rowwise followed by pq_qlinear_s8. */
size_t pq_qlinear_dyn_workspace_bytes(int64_t M, int64_t N, int64_t K);
int32_t pq_qlinear_dyn(const void* x, int32_t dtype, int64_t ld_x, const int8_t* w, int64_t ldw, const float* w_scale,
                       const void* bias, void* y, int64_t ldy, int64_t M, int64_t N, int64_t K,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Self-test hook: for n (x, s) fp32 bit-pattern pairs, counts in mismatches[0] the pairs whose division-free
 * code (K1/K2 hot path) differs from clamp(rne(x / s)) and in mismatches[1] the pairs whose rebuilt quotient
 * differs from the IEEE quotient.  mismatches[2] must be zeroed by the caller.  QSPEC Q4. */
int32_t pq_selftest_fast_quotient(const uint32_t* x_bits, const uint32_t* s_bits, int64_t n,
                                  unsigned long long* mismatches, void* stream);

/* Self-test hook: enumerates on the GPU the WHOLE domain of the one-step division-free encode that 16-bit inputs take (dtype 0 = bf16,
 * 1 = fp16): every amax bit pattern whose scale takes the fast path x every magnitude pattern <= amax x both signs.  counts[0] += pairs
 * checked, counts[1] += pairs whose code differs from clamp(rne(x / s)).  counts[2] must be zeroed by the caller.  QSPEC Q4. */
int32_t pq_selftest_half_encode(int32_t dtype, unsigned long long* counts, void* stream);

/* Self-test hook: every 16-bit pattern g with 0 < |g| <= 86 (the domain of the division-free silu of bf16 / fp16 rows) through the
 * one-correction division the producer kernel uses, the two-correction form and true division.  counts[0] += patterns, counts[1] +=
 * patterns whose stored silu(g) differs between the first two, counts[2] += between the last two.  counts[3] zeroed by the caller.  QSPEC S4. */
int32_t pq_selftest_silu_short(int32_t dtype, unsigned long long* counts, void* stream);

/* Self-test hook: every 16-bit pattern g on which pq_glu_quant_rowwise takes its division-free sequence for this (kind, limit, alpha) through that sequence and
 * through the specified one (true division), against two values of u.  counts[0] += patterns, counts[1] += patterns whose stored h differs.  counts[2] zeroed by the
 * caller.  QSPEC G2-G5. */
int32_t pq_selftest_glu_short(int32_t dtype, int32_t kind, float limit, float alpha, unsigned long long* counts, void* stream);

/* Name of the single-pass GEMM kernel variant the dispatcher would pick for this problem (static string); with a workspace
 * (pq_qlinear_workspace_bytes > 0) pq_qlinear_s8 runs a split-K form of the 256 x 256 (or 128 x 256) tile instead. */
const char* pq_gemm_variant_name(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb);

#ifdef __cplusplus
}
#endif
#endif /* PQ_HIP_H */
