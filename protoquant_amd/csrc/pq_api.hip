// pq_api.hip — the C-ABI of libpq_hip.so (include/pq_hip.h): argument validation, launches, status codes; the planners it asks are in pq_plan.hip.
// No allocation, no synchronisation, no host copies: graph-capturable.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <atomic>
#include <mutex>
#include <initializer_list>
#include <type_traits>
#include <utility>

#include "gemm_epilogue.h"
#include "pq_launch.h"
#include "pq_plan.h"

namespace {
using namespace pq;      // (Variant and the planners; the launchers are spelled pq::launch_... at their call sites)

thread_local char g_err[512] = "";

int32_t fail(int32_t code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int32_t check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(PQ_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return PQ_OK;
}

// Behaviour switches (tests / experiments): pq::Options (pq_common.h), one immutable snapshot per state.  The environment is read ONCE, at the
// first call into the library (a getenv per launch is host time on the hot path, and a switch that a captured hipGraph freezes must not look
// live); pq_set_option() publishes a modified copy by one atomic pointer swap.  Every C-ABI entry point pins the live snapshot for its own
// duration (CallScope): planning and launching happen under ONE set of switches, and concurrent calls from several host threads are defined.
std::atomic<const pq::Options*> g_live{nullptr};
std::mutex g_opt_mu;                       // writers only (pq_set_option, the environment pass)
std::once_flag g_opt_once;
thread_local const pq::Options* tl_opt = nullptr;      // the snapshot pinned by the C-ABI call in progress on this thread
thread_local int tl_depth = 0;

// every behaviour switch: its name and what a value does to the snapshot — the ONE table both the environment pass (once) and pq_set_option walk.
// v: the value as given (may be null); set: it is non-empty; iv: atoi(v) when set, else 0.
using O = pq::Options;
const struct OptionRow { const char* name; void (*apply)(O& o, const char* v, bool set, int iv); } kOptions[] = {
    {"PQ_FORCE_VARIANT", [](O& o, const char* v, bool, int) { o.variant = parse_variant(v); }},
    {"PQ_NO_TAILSPLIT", [](O& o, const char*, bool set, int) { o.no_tailsplit = set; }},
    {"PQ_NO_SPLITK", [](O& o, const char*, bool set, int) { o.no_splitk = set; }},
    {"PQ_FORCE_SPLITK", [](O& o, const char*, bool, int iv) { o.force_splitk = iv; }},
    {"PQ_FSK", [](O& o, const char*, bool set, int iv) { o.fsk = set ? iv : -1; }},
    {"PQ_FSK_SYMMETRIC", [](O& o, const char* v, bool set, int) { o.fsk_symmetric = set && *v == '1'; }},
    {"PQ_FSK_FENCED", [](O& o, const char* v, bool set, int) { o.fsk_fenced = set && *v == '1'; }},
    {"PQ_FSK_COOP", [](O& o, const char* v, bool set, int) { o.fsk_coop = set && *v == '1'; }},
    {"PQ_FAKE_CUS", [](O& o, const char*, bool, int iv) { o.fake_cus = iv > 0 ? iv : 0; }},
    {"PQ_NO_MIDM", [](O& o, const char*, bool set, int) { o.no_midm = set; }},
    {"PQ_NO_KSLABS", [](O& o, const char*, bool set, int) { o.no_kslabs = set; }},
    {"PQ_NO_RING160", [](O& o, const char*, bool set, int) { o.no_ring160 = set; }},
    {"PQ_MIDM_CT", [](O& o, const char*, bool, int iv) { o.midm_ct = iv > 0 ? iv : 0; }},
    {"PQ_RMS_WAVE_MAX", [](O& o, const char*, bool set, int iv) { o.rms_wave_max = !set || iv < 0 ? 256 : (iv > 512 ? 512 : iv); }},
    {"PQ_SILU_TPR", [](O& o, const char* v, bool set, int) { o.silu_tpr = set && !strcmp(v, "256") ? 256 : 0; }},
    {"PQ_SP128_LC", [](O& o, const char*, bool set, int iv) { o.sp128_lc = !set || iv < 0 || iv > 2 ? 1 : iv; }},
    {"PQ_SP256_P3", [](O& o, const char* v, bool set, int) { o.sp256_p3 = !(set && *v == '0'); }},
    {"PQ_SP256_ASM", [](O& o, const char*, bool set, int iv) { o.sp256_asm = !set || iv < 0 ? 1 : iv; }},     // "" = default (1)
    {"PQ_SP256_PERSIST", [](O& o, const char* v, bool set, int) { o.sp256_persist = set && *v == '1'; }},
    {"PQ_RING_LC", [](O& o, const char* v, bool set, int) { o.ring_lc = !(set && *v == '0'); }},
    {"PQ_RING_ROT", [](O& o, const char*, bool set, int iv) { o.ring_rot = !set ? 1 : (iv < 0 ? 0 : iv); }},
    {"PQ_K1_LDS", [](O& o, const char*, bool, int iv) { o.k1_lds = iv < 0 ? 0 : (iv > 65536 ? 65536 : iv); }},
    {"PQ_EPI_ANY_ALIGN", [](O& o, const char* v, bool set, int) { o.epi_any_align = !(set && *v == '0'); }},
    {"PQ_K2_BLOCKS_A", [](O& o, const char*, bool, int iv) { o.k2_blocks_a = iv > 0 ? iv : 0; }},
    {"PQ_K2_BLOCKS_E", [](O& o, const char*, bool, int iv) { o.k2_blocks_e = iv > 0 ? iv : 0; }},
    {"PQ_K1_RPW", [](O& o, const char* v, bool set, int) { o.k1_rpw = set && *v == '2' ? 2 : (set && *v == '1' ? 1 : 0); }},
    {"PQ_K1_ST16", [](O& o, const char* v, bool set, int) { o.k1_st16 = set && *v == '1'; }},
    {"PQ_SKINNY_RB", [](O& o, const char* v, bool set, int) { o.skinny_rb = set && *v == '2' ? 2 : (set && *v == '1' ? 1 : 0); }},
    {"PQ_SKINNY_STAGE", [](O& o, const char* v, bool set, int) { o.skinny_stage = !(set && *v == '0'); }},
    {"PQ_SKINNY_KS", [](O& o, const char*, bool, int iv) { o.skinny_ks = iv > 0 ? iv : 0; }},
    {"PQ_GROUPED_TILE", [](O& o, const char* v, bool set, int) { o.grouped_tile = !set ? 0 : (!strcmp(v, "64x128") ? 1 : (!strcmp(v, "64x64") ? 2 : 0)); }},
    {"PQ_GROUPED_ROT", [](O& o, const char* v, bool set, int) { o.grouped_rot = set && *v == '1'; }},
    {"PQ_GROUPED_STREAM_KS", [](O& o, const char*, bool, int iv) { o.grouped_stream_ks = iv > 0 ? iv : 0; }},
    {"PQ_GROUPED_STREAM_RB", [](O& o, const char* v, bool set, int) { o.grouped_stream_rb = set && *v == '2' ? 2 : (set && *v == '1' ? 1 : 0); }},
};
void apply_row(const OptionRow& r, pq::Options& o, const char* value) {
    const bool set = value && *value;
    r.apply(o, value, set, set ? atoi(value) : 0);
}
const pq::Options* live_options() {
    std::call_once(g_opt_once, [] {
        auto* o = new pq::Options();
        for (const OptionRow& r : kOptions)
            if (const char* v = getenv(r.name)) apply_row(r, *o, v);
        if (const char* r = getenv("PQ_ROCTX")) {
            // PQ_ROCTX=1: every C-ABI entry point pushes / pops a roctx range (quant / gemm / ...), so a rocprofv3 --marker-trace
            // timeline shows the path's stages by name.  The marker library is dlopen'ed on first use; absent library = no ranges.
            if (*r && *r != '0') {
                void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
                if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
                if (h) {
                    o->roctx_push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
                    o->roctx_pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
                    if (!o->roctx_push || !o->roctx_pop) o->roctx_push = nullptr, o->roctx_pop = nullptr;
                }
            }
        }
        g_live.store(o, std::memory_order_release);
    });
    return g_live.load(std::memory_order_acquire);
}
const pq::Options& options() { return tl_opt ? *tl_opt : *live_options(); }

// pins the live snapshot for one C-ABI call on this thread (re-entrant: pq_qlinear_dyn calls pq_quant_rowwise and pq_qlinear_s8 under ITS snapshot)
struct CallScope {
    CallScope() { if (tl_depth++ == 0) tl_opt = live_options(); }
    ~CallScope() { if (--tl_depth == 0) tl_opt = nullptr; }
    CallScope(const CallScope&) = delete;
    CallScope& operator=(const CallScope&) = delete;
};

struct Range {      // one C-ABI call: pins the option snapshot (CallScope) and, with PQ_ROCTX, a roctx range (host side: it brackets the asynchronous launches)
    CallScope scope_;
    bool on;
    explicit Range(const char* name) : on(options().roctx_push != nullptr) { if (on) options().roctx_push(name); }
    ~Range() { if (on) options().roctx_pop(); }
    Range(const Range&) = delete;
    Range& operator=(const Range&) = delete;
};

// f(std::integral_constant<int, DT>{}) for the element type a PQ_* code names; the callers have refused codes outside 0 .. 2, so `default` is PQ_F32
template <typename F>
decltype(auto) by_dtype(int32_t dtype, F&& f) {
    switch (dtype) {
        case PQ_BF16: return f(std::integral_constant<int, PQ_BF16>{});
        case PQ_FP16: return f(std::integral_constant<int, PQ_FP16>{});
        default: return f(std::integral_constant<int, PQ_F32>{});
    }
}

int32_t check_dtype(const char* fn, int32_t dtype) { return dtype < 0 || dtype > 2 ? fail(PQ_ERR_BAD_ARG, "%s: unknown dtype %d", fn, dtype) : PQ_OK; }

bool bad_mat(const void* p, int64_t rows, int64_t cols, int64_t ld) {
    return rows < 0 || cols < 0 || ld < cols || (rows > 0 && cols > 0 && p == nullptr);
}

// a caller's workspace: large enough (a missing one counts as 0 bytes), then aligned
int32_t check_workspace(const char* what, const void* p, size_t bytes, size_t need, size_t align) {
    if (!p || bytes < need) return fail(PQ_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", what, p ? bytes : (size_t)0, need);
    if ((reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0) return fail(PQ_ERR_BAD_ALIGN, "%s: workspace must be %zu-byte aligned", what, align);
    return PQ_OK;
}
size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// the epilogue arguments of one launch.  EPI_FULL is what every tile launcher expects.  Two kinds of call site pass less, and have since they were written — kept, not decided
// here: EPI_NXCD (pq_gemm_s8s8s32, the streaming branch of pq_qlinear_s8_t) leaves y_any_align at 0, EPI_BARE (the grouped weight-streaming entries) sets neither field.
enum EpiFill { EPI_BARE, EPI_NXCD, EPI_FULL };
pq::EpiArgs make_epi(const float* a_scale, const float* b_scale, const void* bias, void* y, int64_t ldy, int32_t flags, EpiFill fill = EPI_FULL) {
    pq::EpiArgs e{a_scale, b_scale, bias, y, ldy, flags};
    if (fill == EPI_FULL) e.y_any_align = options().epi_any_align ? 1 : 0;
    if (fill != EPI_BARE) e.nxcd = device_xcds();
    return e;
}

template <int OUT>
void run_gemm(Variant v, const int8_t* a, int64_t lda, const int8_t* b, int64_t ldb, const pq::EpiArgs& epi,
              int64_t M, int64_t N, int64_t K, hipStream_t st) {
    if (!pq::epi_flags_valid(epi.flags, epi.bias != nullptr)) abort();      // internal invariant (gemm_epilogue.h): never reachable from the C-ABI
    if (v == V_SP256_16) pq::launch_gemm_fast<OUT, 256, 256>(a, lda, b, ldb, epi, M, N, K, st);
    else if (v == V_SP128_16) pq::launch_gemm_fast<OUT, 128, 256>(a, lda, b, ldb, epi, M, N, K, st);
    else if (v == V_SP128X128) pq::launch_gemm_fast<OUT, 128, 128>(a, lda, b, ldb, epi, M, N, K, st);
    else if (v == V_RING128) pq::launch_gemm_ring128<OUT>(a, lda, b, ldb, epi, M, N, K, st);
    else if (v == V_SKINNY) pq::launch_gemm_skinny<OUT>(a, lda, b, ldb, epi, M, N, K, st);
    else if (v == V_RING64X128) pq::launch_gemm_ringt<OUT>(0, a, lda, b, ldb, epi, M, N, K, st);
    else if (v == V_RING64X64) pq::launch_gemm_ringt<OUT>(1, a, lda, b, ldb, epi, M, N, K, st);
    else if (v == V_RING128X160) pq::launch_gemm_ringt<OUT>(2, a, lda, b, ldb, epi, M, N, K, st);
    else pq::launch_gemm_generic<OUT>(a, lda, b, ldb, epi, M, N, K, st);
}

// the tail split (pq_plan.hip: tail_split_plan) as two launches: both are plain sub-problems (pointer offsets), results are unchanged bit for bit
template <int OUT>
void run_gemm_auto(Variant v, const int8_t* a, int64_t lda, const int8_t* b, int64_t ldb, const pq::EpiArgs& epi,
                   int64_t M, int64_t N, int64_t K, hipStream_t st) {
    int64_t lead = 0;
    const int axis = (v == V_SP256_16 && forced_variant() == V_AUTO) ? tail_split_plan(M, N, &lead) : 0;
    if (axis == 0) return run_gemm<OUT>(v, a, lda, b, ldb, epi, M, N, K, st);
    using elem_t = typename pq::OutElem<OUT>::type;
    pq::EpiArgs tail = epi;
    if (axis == 1) {
        tail.b_scale = epi.b_scale ? epi.b_scale + lead : nullptr;
        tail.bias = (epi.bias && !(epi.flags & pq::EPI_BIAS_ROWS)) ? static_cast<const elem_t*>(epi.bias) + lead : epi.bias;
        tail.y = static_cast<elem_t*>(epi.y) + lead;
        run_gemm<OUT>(V_SP256_16, a, lda, b, ldb, epi, M, lead, K, st);
        run_gemm<OUT>(V_SP128_16, a, lda, b + lead * ldb, ldb, tail, M, N - lead, K, st);
    } else {
        tail.a_scale = epi.a_scale ? epi.a_scale + lead : nullptr;
        tail.bias = (epi.bias && (epi.flags & pq::EPI_BIAS_ROWS)) ? static_cast<const elem_t*>(epi.bias) + lead : epi.bias;
        tail.y = static_cast<elem_t*>(epi.y) + lead * epi.ldy;
        run_gemm<OUT>(V_SP256_16, a, lda, b, ldb, epi, lead, N, K, st);
        run_gemm<OUT>(V_SP128_16, a + lead * lda, lda, b, ldb, tail, M - lead, N, K, st);
    }
}

// the fused split-K launch shared by qlinear_core and pq_qlinear_s8_kslabs (which passes the slab walk); the caller has checked the workspace
int32_t launch_fsk(const char* what, const int8_t* a, int64_t lda, const int8_t* b, int64_t ldb, const pq::EpiArgs& epi, int32_t out_dtype, int64_t M, int64_t N, int64_t K,
                   int f, void* workspace, hipStream_t st, int64_t slab_stride = 0, int64_t k_per_slab = 0) {
    if (!pq::epi_flags_valid(epi.flags, epi.bias != nullptr)) abort();
    const bool launched = by_dtype(out_dtype, [&](auto dt) { return pq::launch_gemm_fsk<dt>(a, lda, b, ldb, epi, M, N, K, f, workspace, st, slab_stride, k_per_slab); });
    if (!launched) { (void)hipGetLastError(); return fail(PQ_ERR_WORKSPACE, "%s: the split-K workspace could not be initialised (the zeroing launch failed)", what); }
    return check_launch(what);
}

// stacked[s][m][c] (slab stride in bytes, row length lda) -> out[m][s * kps + c], 16 bytes at a time (kps % 16 == 0, aligned bases) or byte by byte: the layout pass of
// pq_qlinear_s8_kslabs (what an all-gather of the ranks' int8 column blocks leaves: [G][M][K / G])
typedef unsigned int v4u_ __attribute__((ext_vector_type(4)));
template <typename V>
__global__ __launch_bounds__(256) void unstack_kslabs_kernel(const uint8_t* __restrict__ a, int64_t lda, int64_t slab_stride, uint8_t* __restrict__ out, int64_t ldo,
                                                             int64_t M, int64_t kps_v, int nslabs) {
    const int64_t total = (int64_t)nslabs * M * kps_v;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t c = i % kps_v, m = (i / kps_v) % M, sl = i / (kps_v * M);
        *reinterpret_cast<V*>(out + m * ldo + (sl * kps_v + c) * (int64_t)sizeof(V)) = *reinterpret_cast<const V*>(a + sl * slab_stride + m * lda + c * (int64_t)sizeof(V));
    }
}

// ---- the row producers with per-argument messages (K1a, K1l, K1al, K1u): each describes its operands, check_row_producer does the rest
// Byte extent of a row-major operand, and the overlap test between two of them.  Operands that share a leading dimension (column
// blocks of one buffer) are told apart by the columns they occupy; everything else by its bounding range.
struct Extent {
    uintptr_t base;
    int64_t ld_bytes, width_bytes, rows;
    uintptr_t end() const { return base + (uintptr_t)((rows - 1) * ld_bytes + width_bytes); }
};
Extent extent_of(const void* p, int64_t ld, int64_t rows, int64_t cols, int64_t elem_bytes) {
    return Extent{reinterpret_cast<uintptr_t>(p), ld * elem_bytes, cols * elem_bytes, rows};
}
bool extents_overlap(const Extent& a, const Extent& b) {
    if (!a.base || !b.base || a.end() <= b.base || b.end() <= a.base) return false;
    if (a.ld_bytes == b.ld_bytes && a.ld_bytes > 0) {      // the same pitch: disjoint when their column intervals, taken modulo the pitch, do not meet
        const int64_t ld = a.ld_bytes;
        const int64_t d = (int64_t)((b.base >= a.base ? b.base - a.base : (uintptr_t)ld - (a.base - b.base) % (uintptr_t)ld) % (uintptr_t)ld);
        if (d >= a.width_bytes && d + b.width_bytes <= ld) return false;
    }
    return true;
}

// The entries that predate check_row_producer (K1 and its halves, K2, K1s, K1g, K1n, dequant, moe_combine) keep their own shape checks and messages; their kernels carry
// __restrict__ on every operand, so an output that overlaps anything else is refused here, by name, before any HIP call.  `v`: the operands in the order of the
// argument list, inputs first; null operands (a nullable h_out) are skipped by extents_overlap.
struct NamedExtent {
    const char* name;
    Extent e;
    bool out;
};
Extent vec_extent(const void* p, int64_t n, int64_t elem_bytes) { return extent_of(p, n, 1, n, elem_bytes); }
int32_t check_disjoint(const char* fn, const NamedExtent* v, int n) {
    for (int o = 0; o < n; ++o) {
        if (!v[o].out) continue;
        for (int j = 0; j < n; ++j)
            if (j != o && (!v[j].out || j > o) && extents_overlap(v[o].e, v[j].e)) return fail(PQ_ERR_BAD_ARG, "%s: %s overlaps %s", fn, v[o].name, v[j].name);
    }
    return PQ_OK;
}

int64_t dtype_bytes(int32_t dtype) { return dtype == PQ_F32 ? 4 : 2; }
// g, u (u null: a one-input entry), the amax vector of the split halves (an output of the first half, an input of the second), q / scale / h_out (each nullable)
int32_t check_gated_disjoint(const char* fn, const void* g, int64_t ld_g, const void* u, int64_t ld_u, int32_t dtype, int64_t rows, int64_t cols, const void* amax_bits,
                             bool amax_is_out, const void* q, int64_t ld_q, const void* scale, const void* h_out, int64_t ld_h) {
    if (cols == 0) return PQ_OK;
    const int64_t eb = dtype_bytes(dtype);
    const NamedExtent ops[] = {{u ? "g" : "x", extent_of(g, ld_g, rows, cols, eb), false}, {"u", extent_of(u, ld_u, rows, cols, eb), false},
                               {"amax_bits", vec_extent(amax_bits, rows, 4), amax_is_out},  {"q", extent_of(q, ld_q, rows, cols, 1), true},
                               {"scale", vec_extent(scale, rows, 4), true},                 {"h_out", extent_of(h_out, ld_h, rows, cols, eb), true}};
    return check_disjoint(fn, ops, 6);
}

enum Role { R_IN, R_INOUT, R_OUT };
struct RowOperand {
    const char* name;
    const void* p;
    Role role;
    const char* ld_name;      // a [rows x cols] matrix with leading dimension `ld`; nullptr: a vector of `ld` elements
    int64_t ld, elem;         // (elem: bytes per element)
    const char* null_note;    // nullptr: may be null; otherwise what follows "<name> is null" in the message
};
const char kSumNote[] = " (the sum is the new residual stream: it is always stored)", kAffineNote[] = " (a LayerNorm without affine parameters is not supported)";

// The checks of a row producer after its dtype (and kind), in this order: shape, eps (`eps` is null for a producer without a norm: no eps, no 2^24 bound on cols; `post_eps`: the second eps of K1pang or K1pl / K1l2, checked after it and named `post_name`; at most 16 operands), the leading
// dimensions in operand order, the empty problem (*empty: nothing to launch), the null pointers in operand order, then the overlaps.  An output may overlap neither an
// input nor another output: the vector layouts load a clamped duplicate of a row's last vector into the slots past its end and the generic kernels read x again in every
// pass, so an in-place h_out is not tolerated.  An in-out operand (sum_out) may BE a matrix input (same base and pitch: every element is read before it is written, by the
// thread that writes it); any other overlap with an input is refused, and for the outputs it counts as the last of the inputs.
int32_t check_row_producer(const char* fn, int64_t rows, int64_t cols, const float* eps, const RowOperand* ops, int n, bool* empty, const float* post_eps = nullptr,
                           const char* post_name = "post_eps") {
    *empty = false;
    if (!eps && (rows < 0 || cols < 0)) return fail(PQ_ERR_BAD_ARG, "%s: bad shape (rows=%lld cols=%lld)", fn, (long long)rows, (long long)cols);
    if (eps && (rows < 0 || cols < 0 || cols >= (1 << 24))) return fail(PQ_ERR_BAD_ARG, "%s: bad shape (rows=%lld cols=%lld; cols < 2^24)", fn, (long long)rows, (long long)cols);
    if (eps && (!(*eps >= 0.0f) || *eps > 3.4028234e38f)) return fail(PQ_ERR_BAD_ARG, "%s: eps must be finite and >= 0 (eps=%g)", fn, (double)*eps);
    if (post_eps && (!(*post_eps >= 0.0f) || *post_eps > 3.4028234e38f))
        return fail(PQ_ERR_BAD_ARG, "%s: %s must be finite and >= 0 (%s=%g)", fn, post_name, post_name, (double)*post_eps);
    for (int i = 0; i < n; ++i)
        if (ops[i].ld_name && (ops[i].null_note || ops[i].p) && ops[i].ld < cols)
            return fail(PQ_ERR_BAD_ARG, "%s: %s %lld < cols %lld", fn, ops[i].ld_name, (long long)ops[i].ld, (long long)cols);
    if (rows == 0 || cols == 0) { *empty = true; return PQ_OK; }
    for (int i = 0; i < n; ++i)
        if (ops[i].null_note && !ops[i].p) return fail(PQ_ERR_BAD_ARG, "%s: %s is null%s", fn, ops[i].name, ops[i].null_note);
    Extent e[16];
    for (int i = 0; i < n; ++i) e[i] = ops[i].ld_name ? extent_of(ops[i].p, ops[i].ld, rows, cols, ops[i].elem) : extent_of(ops[i].p, ops[i].ld, 1, ops[i].ld, ops[i].elem);
    for (int s = 0; s < n; ++s)
        for (int i = 0; i < n && ops[s].role == R_INOUT; ++i) {
            if (ops[i].role != R_IN || (ops[i].ld_name && ops[s].p == ops[i].p && ops[s].ld == ops[i].ld) || !extents_overlap(e[s], e[i])) continue;
            if (!ops[i].ld_name) return fail(PQ_ERR_BAD_ARG, "%s: %s overlaps %s", fn, ops[s].name, ops[i].name);
            return fail(PQ_ERR_BAD_ARG, "%s: %s overlaps %s without being %s (same pointer and leading dimension)", fn, ops[s].name, ops[i].name, ops[i].name);
        }
    int ins[16], nin = 0;      // what an output must stay clear of: the inputs, then the in-out operands, then the outputs after it
    for (const Role r : {R_IN, R_INOUT})
        for (int i = 0; i < n; ++i)
            if (ops[i].role == r) ins[nin++] = i;
    for (int o = 0; o < n; ++o) {
        if (ops[o].role != R_OUT) continue;
        for (int j = 0; j < nin; ++j)
            if (extents_overlap(e[o], e[ins[j]])) return fail(PQ_ERR_BAD_ARG, "%s: %s overlaps %s", fn, ops[o].name, ops[ins[j]].name);
        for (int o2 = o + 1; o2 < n; ++o2)
            if (ops[o2].role == R_OUT && extents_overlap(e[o], e[o2])) return fail(PQ_ERR_BAD_ARG, "%s: %s overlaps %s", fn, ops[o].name, ops[o2].name);
    }
    return PQ_OK;
}

}  // namespace

namespace pq {
const Options& opt() { return options(); }
}  // namespace pq

extern "C" {

int32_t pq_version(void) { return PQ_ABI_VERSION; }

int32_t pq_set_option(const char* name, const char* value) {
    if (!name) return fail(PQ_ERR_BAD_ARG, "pq_set_option: null name");
    std::lock_guard<std::mutex> lock(g_opt_mu);
    const pq::Options* live = live_options();      // (the environment is consumed first, so a later call_once cannot undo this)
    for (const OptionRow& r : kOptions)
        if (!strcmp(name, r.name)) {
            auto* o = new pq::Options(*live);
            apply_row(r, *o, value);
            g_live.store(o, std::memory_order_release);  // calls already in flight keep the snapshot they pinned; the old one is never freed
            return PQ_OK;
        }
    return fail(PQ_ERR_BAD_ARG, "pq_set_option: unknown option %s", name);
}
const char* pq_last_error(void) { return g_err; }

int32_t pq_quant_rowwise(const void* x, int32_t dtype, int64_t rows, int64_t cols, int64_t ld_x, int8_t* q,
                         int64_t ld_q, float* scale, void* stream) {
    Range range_("pq:quant_rowwise (K1)");
    if (const int32_t rc = check_dtype("pq_quant_rowwise", dtype)) return rc;
    if (bad_mat(x, rows, cols, ld_x) || bad_mat(q, rows, cols, ld_q) || (rows > 0 && !scale))
        return fail(PQ_ERR_BAD_ARG, "pq_quant_rowwise: bad matrix (rows=%lld cols=%lld ld_x=%lld ld_q=%lld)", (long long)rows, (long long)cols, (long long)ld_x, (long long)ld_q);
    if (rows == 0) return PQ_OK;
    if (cols > 0) {
        const NamedExtent ops[] = {{"x", extent_of(x, ld_x, rows, cols, dtype_bytes(dtype)), false}, {"q", extent_of(q, ld_q, rows, cols, 1), true}, {"scale", vec_extent(scale, rows, 4), true}};
        if (const int32_t rc = check_disjoint("pq_quant_rowwise", ops, 3)) return rc;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto dt) { pq::quant_rowwise_dispatch<dt>(x, rows, cols, ld_x, q, ld_q, scale, st); });
    return check_launch("pq_quant_rowwise");
}

int32_t pq_quant_colwise(const void* x, int32_t dtype, int64_t rows, int64_t cols, int64_t ld_x, int8_t* q,
                         int64_t ld_q, float* scale, void* stream) {
    Range range_("pq:quant_colwise (K2)");
    if (const int32_t rc = check_dtype("pq_quant_colwise", dtype)) return rc;
    if (bad_mat(x, rows, cols, ld_x) || bad_mat(q, rows, cols, ld_q) || (cols > 0 && !scale))
        return fail(PQ_ERR_BAD_ARG, "pq_quant_colwise: bad matrix (rows=%lld cols=%lld ld_x=%lld ld_q=%lld)", (long long)rows, (long long)cols, (long long)ld_x, (long long)ld_q);
    if (cols == 0) return PQ_OK;
    if (rows > 0) {
        const NamedExtent ops[] = {{"x", extent_of(x, ld_x, rows, cols, dtype_bytes(dtype)), false}, {"q", extent_of(q, ld_q, rows, cols, 1), true}, {"scale", vec_extent(scale, cols, 4), true}};
        if (const int32_t rc = check_disjoint("pq_quant_colwise", ops, 3)) return rc;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const hipError_t e = by_dtype(dtype, [&](auto dt) { return pq::quant_colwise_dispatch<dt>(x, rows, cols, ld_x, q, ld_q, scale, st); });
    if (e != hipSuccess) return fail(PQ_ERR_LAUNCH, "pq_quant_colwise: initialising the amax scratch: %s", hipGetErrorString(e));
    return check_launch("pq_quant_colwise");
}

int32_t pq_silu_mul_quant_rowwise(const void* g, int64_t ld_g, const void* u, int64_t ld_u, int32_t dtype, int64_t rows,
                                  int64_t cols, int8_t* q, int64_t ld_q, float* scale, void* h_out, int64_t ld_h, void* stream) {
    Range range_("pq:silu_mul_quant (K1s)");
    if (const int32_t rc = check_dtype("pq_silu_mul_quant_rowwise", dtype)) return rc;
    if (bad_mat(g, rows, cols, ld_g) || bad_mat(u, rows, cols, ld_u) || bad_mat(q, rows, cols, ld_q) || (rows > 0 && !scale) ||
        (h_out && ld_h < cols))
        return fail(PQ_ERR_BAD_ARG, "pq_silu_mul_quant_rowwise: bad matrix (rows=%lld cols=%lld ld_g=%lld ld_u=%lld ld_q=%lld ld_h=%lld)", (long long)rows, (long long)cols, (long long)ld_g, (long long)ld_u, (long long)ld_q, (long long)ld_h);
    if (rows == 0) return PQ_OK;
    if (const int32_t rc = check_gated_disjoint("pq_silu_mul_quant_rowwise", g, ld_g, u, ld_u, dtype, rows, cols, nullptr, false, q, ld_q, scale, h_out, ld_h)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto dt) { pq::silu_mul_quant_dispatch<dt>(g, ld_g, u, ld_u, rows, cols, q, ld_q, scale, h_out, ld_h, st); });
    return check_launch("pq_silu_mul_quant_rowwise");
}

// kind / dtype / limit / alpha of the clamped gates, shared by the kernel entry and its self-test; nullptr = fine
static const char* glu_bad_params(int32_t dtype, int32_t kind, float limit, float alpha) {
    if (dtype < 0 || dtype > 2) return "unknown dtype";
    if (kind != PQ_GLU_CLAMPED_SILU && kind != PQ_GLU_ALPHA_SIGMOID) return "unknown kind (0 = clamped silu, 1 = alpha sigmoid)";
    if (!(limit > 0.0f) || limit > 3.4028234e38f) return "limit must be finite and > 0";
    if (!(pq::glu_limit_in_dtype(dtype, limit) > 0.0f)) return "limit rounds to zero in the storage dtype";
    if (!(alpha == alpha) || alpha > 3.4028234e38f || alpha < -3.4028234e38f) return "alpha must be finite";
    return nullptr;
}

int32_t pq_glu_quant_rowwise(const void* g, int64_t ld_g, const void* u, int64_t ld_u, int32_t dtype, int64_t rows, int64_t cols, int32_t kind, float limit,
                             float alpha, int8_t* q, int64_t ld_q, float* scale, void* h_out, int64_t ld_h, void* stream) {
    Range range_("pq:glu_quant (K1g)");
    if (const char* why = glu_bad_params(dtype, kind, limit, alpha))
        return fail(PQ_ERR_BAD_ARG, "pq_glu_quant_rowwise: %s (dtype=%d kind=%d limit=%g alpha=%g)", why, dtype, kind, (double)limit, (double)alpha);
    if (bad_mat(g, rows, cols, ld_g) || bad_mat(u, rows, cols, ld_u) || bad_mat(q, rows, cols, ld_q) || (rows > 0 && !scale) || (h_out && ld_h < cols))
        return fail(PQ_ERR_BAD_ARG, "pq_glu_quant_rowwise: bad matrix (rows=%lld cols=%lld ld_g=%lld ld_u=%lld ld_q=%lld ld_h=%lld)", (long long)rows, (long long)cols, (long long)ld_g, (long long)ld_u, (long long)ld_q, (long long)ld_h);
    if (rows == 0 || cols == 0) return PQ_OK;
    if (const int32_t rc = check_gated_disjoint("pq_glu_quant_rowwise", g, ld_g, u, ld_u, dtype, rows, cols, nullptr, false, q, ld_q, scale, h_out, ld_h)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto dt) { pq::glu_quant_dispatch<dt>(kind, g, ld_g, u, ld_u, rows, cols, limit, alpha, q, ld_q, scale, h_out, ld_h, st); });
    return check_launch("pq_glu_quant_rowwise");
}

int32_t pq_silu_mul_rowamax(const void* g, int64_t ld_g, const void* u, int64_t ld_u, int32_t dtype, int64_t rows, int64_t cols,
                            uint32_t* amax_bits, void* stream) {
    Range range_("pq:silu_mul_rowamax (K1s, amax half)");
    if (const int32_t rc = check_dtype("pq_silu_mul_rowamax", dtype)) return rc;
    if (bad_mat(g, rows, cols, ld_g) || bad_mat(u, rows, cols, ld_u) || (rows > 0 && !amax_bits))
        return fail(PQ_ERR_BAD_ARG, "pq_silu_mul_rowamax: bad matrix (rows=%lld cols=%lld ld_g=%lld ld_u=%lld)", (long long)rows, (long long)cols, (long long)ld_g, (long long)ld_u);
    if (rows == 0) return PQ_OK;
    if (const int32_t rc = check_gated_disjoint("pq_silu_mul_rowamax", g, ld_g, u, ld_u, dtype, rows, cols, amax_bits, true, nullptr, 0, nullptr, nullptr, 0)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto dt) { pq::silu_mul_split_dispatch<dt, 1, false>(g, ld_g, u, ld_u, rows, cols, amax_bits, nullptr, 0, nullptr, st); });
    return check_launch("pq_silu_mul_rowamax");
}

int32_t pq_silu_mul_quant_rowwise_amax(const void* g, int64_t ld_g, const void* u, int64_t ld_u, int32_t dtype, int64_t rows, int64_t cols,
                                       const uint32_t* amax_bits, int8_t* q, int64_t ld_q, float* scale, void* stream) {
    Range range_("pq:silu_mul_quant_amax (K1s, encode half)");
    if (const int32_t rc = check_dtype("pq_silu_mul_quant_rowwise_amax", dtype)) return rc;
    if (bad_mat(g, rows, cols, ld_g) || bad_mat(u, rows, cols, ld_u) || bad_mat(q, rows, cols, ld_q) || (rows > 0 && (!scale || !amax_bits)))
        return fail(PQ_ERR_BAD_ARG, "pq_silu_mul_quant_rowwise_amax: bad matrix (rows=%lld cols=%lld ld_g=%lld ld_u=%lld ld_q=%lld)", (long long)rows, (long long)cols, (long long)ld_g, (long long)ld_u, (long long)ld_q);
    if (rows == 0) return PQ_OK;
    if (const int32_t rc = check_gated_disjoint("pq_silu_mul_quant_rowwise_amax", g, ld_g, u, ld_u, dtype, rows, cols, amax_bits, false, q, ld_q, scale, nullptr, 0)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint32_t* ab = const_cast<uint32_t*>(amax_bits);          // (read-only in this mode)
    by_dtype(dtype, [&](auto dt) { pq::silu_mul_split_dispatch<dt, 2, false>(g, ld_g, u, ld_u, rows, cols, ab, q, ld_q, scale, st); });
    return check_launch("pq_silu_mul_quant_rowwise_amax");
}

int32_t pq_quant_rowamax(const void* x, int32_t dtype, int64_t rows, int64_t cols, int64_t ld_x, uint32_t* amax_bits, void* stream) {
    Range range_("pq:quant_rowamax (K1, amax half)");
    if (const int32_t rc = check_dtype("pq_quant_rowamax", dtype)) return rc;
    if (bad_mat(x, rows, cols, ld_x) || (rows > 0 && !amax_bits))
        return fail(PQ_ERR_BAD_ARG, "pq_quant_rowamax: bad matrix (rows=%lld cols=%lld ld_x=%lld)", (long long)rows, (long long)cols, (long long)ld_x);
    if (rows == 0) return PQ_OK;
    if (const int32_t rc = check_gated_disjoint("pq_quant_rowamax", x, ld_x, nullptr, 0, dtype, rows, cols, amax_bits, true, nullptr, 0, nullptr, nullptr, 0)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto dt) { pq::silu_mul_split_dispatch<dt, 1, true>(x, ld_x, nullptr, 0, rows, cols, amax_bits, nullptr, 0, nullptr, st); });
    return check_launch("pq_quant_rowamax");
}

int32_t pq_quant_rowwise_amax(const void* x, int32_t dtype, int64_t rows, int64_t cols, int64_t ld_x, const uint32_t* amax_bits, int8_t* q, int64_t ld_q,
                              float* scale, void* stream) {
    Range range_("pq:quant_rowwise_amax (K1, encode half)");
    if (const int32_t rc = check_dtype("pq_quant_rowwise_amax", dtype)) return rc;
    if (bad_mat(x, rows, cols, ld_x) || bad_mat(q, rows, cols, ld_q) || (rows > 0 && (!scale || !amax_bits)))
        return fail(PQ_ERR_BAD_ARG, "pq_quant_rowwise_amax: bad matrix (rows=%lld cols=%lld ld_x=%lld ld_q=%lld)", (long long)rows, (long long)cols, (long long)ld_x, (long long)ld_q);
    if (rows == 0) return PQ_OK;
    if (const int32_t rc = check_gated_disjoint("pq_quant_rowwise_amax", x, ld_x, nullptr, 0, dtype, rows, cols, amax_bits, false, q, ld_q, scale, nullptr, 0)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint32_t* ab = const_cast<uint32_t*>(amax_bits);          // (read-only in this mode)
    by_dtype(dtype, [&](auto dt) { pq::silu_mul_split_dispatch<dt, 2, true>(x, ld_x, nullptr, 0, rows, cols, ab, q, ld_q, scale, st); });
    return check_launch("pq_quant_rowwise_amax");
}

int32_t pq_rmsnorm_quant_rowwise(const void* x, int64_t ld_x, const void* weight, float eps, int32_t dtype, int64_t rows, int64_t cols,
                                 int8_t* q, int64_t ld_q, float* scale, void* h_out, int64_t ld_h, void* stream) {
    Range range_("pq:rmsnorm_quant (K1n)");
    if (const int32_t rc = check_dtype("pq_rmsnorm_quant_rowwise", dtype)) return rc;
    if (bad_mat(x, rows, cols, ld_x) || bad_mat(q, rows, cols, ld_q) || (rows > 0 && !scale) || (rows > 0 && cols > 0 && !weight) ||
        (h_out && ld_h < cols) || cols >= (1 << 24) || !(eps >= 0.0f))
        return fail(PQ_ERR_BAD_ARG, "pq_rmsnorm_quant_rowwise: bad arguments (rows=%lld cols=%lld ld_x=%lld ld_q=%lld ld_h=%lld eps=%g)", (long long)rows, (long long)cols, (long long)ld_x, (long long)ld_q, (long long)ld_h, (double)eps);
    if (rows == 0) return PQ_OK;
    if (cols > 0) {
        const int64_t eb = dtype_bytes(dtype);
        const NamedExtent ops[] = {{"x", extent_of(x, ld_x, rows, cols, eb), false}, {"weight", vec_extent(weight, cols, eb), false}, {"q", extent_of(q, ld_q, rows, cols, 1), true},
                                   {"scale", vec_extent(scale, rows, 4), true}, {"h_out", extent_of(h_out, ld_h, rows, cols, eb), true}};
        if (const int32_t rc = check_disjoint("pq_rmsnorm_quant_rowwise", ops, 5)) return rc;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (cols == 0) pq::quant_rowwise_dispatch<PQ_F32>(x, rows, 0, 1, q, 1, scale, st);       // nothing to normalise: scale = 1 (QSPEC Q3), no codes
    else by_dtype(dtype, [&](auto dt) { pq::rmsnorm_quant_dispatch<dt>(x, ld_x, weight, eps, rows, cols, q, ld_q, scale, h_out, ld_h, st); });
    return check_launch("pq_rmsnorm_quant_rowwise");
}

int32_t pq_add_rmsnorm_quant_rowwise(const void* x, int64_t ld_x, const void* residual, int64_t ld_r, void* sum_out, int64_t ld_s, const void* weight, float eps,
                                     int32_t dtype, int64_t rows, int64_t cols, int8_t* q, int64_t ld_q, float* scale, void* h_out, int64_t ld_h, void* stream) {
    Range range_("pq:add_rmsnorm_quant (K1a)");
    const char* fn = "pq_add_rmsnorm_quant_rowwise";
    if (const int32_t rc = check_dtype(fn, dtype)) return rc;
    const int64_t eb = dtype == PQ_F32 ? 4 : 2;
    const RowOperand ops[] = {{"x", x, R_IN, "ld_x", ld_x, eb, ""},           {"residual", residual, R_IN, "ld_r", ld_r, eb, ""}, {"sum_out", sum_out, R_INOUT, "ld_s", ld_s, eb, kSumNote},
                              {"weight", weight, R_IN, nullptr, cols, eb, ""}, {"q", q, R_OUT, "ld_q", ld_q, 1, ""},               {"scale", scale, R_OUT, nullptr, rows, 4, ""},
                              {"h_out", h_out, R_OUT, "ld_h", ld_h, eb, nullptr}};
    bool empty;
    if (const int32_t rc = check_row_producer(fn, rows, cols, &eps, ops, 7, &empty); rc || empty) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto dt) { pq::add_rmsnorm_quant_dispatch<dt>(x, ld_x, residual, ld_r, sum_out, ld_s, weight, eps, rows, cols, q, ld_q, scale, h_out, ld_h, st); });
    return check_launch(fn);
}

int32_t pq_gemma_rmsnorm_quant_rowwise(const void* x, int64_t ld_x, const void* weight, float eps, int32_t dtype, int64_t rows, int64_t cols, int8_t* q, int64_t ld_q,
                                       float* scale, void* h_out, int64_t ld_h, void* stream) {
    Range range_("pq:gemma_rmsnorm_quant (K1ng)");
    const char* fn = "pq_gemma_rmsnorm_quant_rowwise";
    if (const int32_t rc = check_dtype(fn, dtype)) return rc;
    const int64_t eb = dtype == PQ_F32 ? 4 : 2;
    const RowOperand ops[] = {{"x", x, R_IN, "ld_x", ld_x, eb, ""},  {"weight", weight, R_IN, nullptr, cols, eb, ""}, {"q", q, R_OUT, "ld_q", ld_q, 1, ""},
                              {"scale", scale, R_OUT, nullptr, rows, 4, ""}, {"h_out", h_out, R_OUT, "ld_h", ld_h, eb, nullptr}};
    bool empty;
    if (const int32_t rc = check_row_producer(fn, rows, cols, &eps, ops, 5, &empty); rc || empty) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto dt) { pq::gemma_rmsnorm_quant_dispatch<dt>(x, ld_x, weight, eps, rows, cols, q, ld_q, scale, h_out, ld_h, st); });
    return check_launch(fn);
}

int32_t pq_add_gemma_rmsnorm_quant_rowwise(const void* x, int64_t ld_x, const void* residual, int64_t ld_r, void* sum_out, int64_t ld_s, const void* weight, float eps,
                                           int32_t dtype, int64_t rows, int64_t cols, int8_t* q, int64_t ld_q, float* scale, void* h_out, int64_t ld_h, void* stream) {
    Range range_("pq:add_gemma_rmsnorm_quant (K1ang)");
    const char* fn = "pq_add_gemma_rmsnorm_quant_rowwise";
    if (const int32_t rc = check_dtype(fn, dtype)) return rc;
    const int64_t eb = dtype == PQ_F32 ? 4 : 2;
    const RowOperand ops[] = {{"x", x, R_IN, "ld_x", ld_x, eb, ""},           {"residual", residual, R_IN, "ld_r", ld_r, eb, ""}, {"sum_out", sum_out, R_INOUT, "ld_s", ld_s, eb, kSumNote},
                              {"weight", weight, R_IN, nullptr, cols, eb, ""}, {"q", q, R_OUT, "ld_q", ld_q, 1, ""},               {"scale", scale, R_OUT, nullptr, rows, 4, ""},
                              {"h_out", h_out, R_OUT, "ld_h", ld_h, eb, nullptr}};
    bool empty;
    if (const int32_t rc = check_row_producer(fn, rows, cols, &eps, ops, 7, &empty); rc || empty) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto dt) { pq::add_gemma_rmsnorm_quant_dispatch<dt>(x, ld_x, residual, ld_r, sum_out, ld_s, weight, eps, rows, cols, q, ld_q, scale, h_out, ld_h, st); });
    return check_launch(fn);
}

int32_t pq_gemma_postnorm_add_rmsnorm_quant_rowwise(const void* x, int64_t ld_x, const void* post_weight, float post_eps, const void* residual, int64_t ld_r, void* sum_out,
                                                    int64_t ld_s, const void* weight, float eps, int32_t dtype, int64_t rows, int64_t cols, int8_t* q, int64_t ld_q, float* scale,
                                                    void* h_out, int64_t ld_h, void* stream) {
    Range range_("pq:gemma_postnorm_add_rmsnorm_quant (K1pang / K1pa)");
    const char* fn = "pq_gemma_postnorm_add_rmsnorm_quant_rowwise";
    if (const int32_t rc = check_dtype(fn, dtype)) return rc;
    const int64_t eb = dtype == PQ_F32 ? 4 : 2;
    const bool add_only = !weight && !q && !scale && !h_out;          // K1pa: the whole quantisation group is absent (then eps is not read)
    const char* group = " (weight, q and scale go together: all three and h_out null is the add-only form)";
    const RowOperand ops[] = {{"x", x, R_IN, "ld_x", ld_x, eb, ""},
                              {"post_weight", post_weight, R_IN, nullptr, cols, eb, ""},
                              {"residual", residual, R_IN, "ld_r", ld_r, eb, ""},
                              {"sum_out", sum_out, R_INOUT, "ld_s", ld_s, eb, kSumNote},
                              {"weight", weight, R_IN, nullptr, cols, eb, group},
                              {"q", q, R_OUT, "ld_q", ld_q, 1, group},
                              {"scale", scale, R_OUT, nullptr, rows, 4, group},
                              {"h_out", h_out, R_OUT, "ld_h", ld_h, eb, nullptr}};
    const float no_eps = 0.0f;
    bool empty;
    if (const int32_t rc = check_row_producer(fn, rows, cols, add_only ? &no_eps : &eps, ops, add_only ? 4 : 8, &empty, &post_eps); rc || empty) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto dt) {
        pq::gemma_postnorm_add_rmsnorm_quant_dispatch<dt>(x, ld_x, post_weight, post_eps, residual, ld_r, sum_out, ld_s, weight, eps, rows, cols, q, ld_q, scale, h_out, ld_h, st);
    });
    return check_launch(fn);
}

int32_t pq_olmo_postnorm_add_quant_rowwise(const void* x, int64_t ld_x, const void* post_weight, float post_eps, const void* residual, int64_t ld_r, void* sum_out,
                                           int64_t ld_s, int32_t dtype, int64_t rows, int64_t cols, int8_t* q, int64_t ld_q, float* scale, void* stream) {
    Range range_("pq:olmo_postnorm_add_quant (K1oq / K1oa / K1on)");
    const char* fn = "pq_olmo_postnorm_add_quant_rowwise";
    if (const int32_t rc = check_dtype(fn, dtype)) return rc;
    const int64_t eb = dtype == PQ_F32 ? 4 : 2;
    const bool quant = q || scale;                 // K1oq: the group is checked as a whole; otherwise K1oa (residual given) or K1on (the norm alone)
    const bool add = quant || residual;
    const char* group = " (q and scale go together: both null is the form that stores sum_out alone)";
    const char* needs = " (q and scale are the codes of residual + p: they need the residual; without q, scale and residual the call is the norm alone)";
    RowOperand ops[6] = {{"x", x, R_IN, "ld_x", ld_x, eb, ""}, {"post_weight", post_weight, R_IN, nullptr, cols, eb, ""}};
    int n = 2;
    if (add) ops[n++] = {"residual", residual, R_IN, "ld_r", ld_r, eb, needs};
    ops[n++] = {"sum_out", sum_out, R_INOUT, "ld_s", ld_s, eb, kSumNote};
    if (quant) {
        ops[n++] = {"q", q, R_OUT, "ld_q", ld_q, 1, group};
        ops[n++] = {"scale", scale, R_OUT, nullptr, rows, 4, group};
    }
    const float no_eps = 0.0f;                     // (the shape checks of a norm — cols < 2^24 — without an eps of that name: the only eps here is post_eps)
    bool empty;
    if (const int32_t rc = check_row_producer(fn, rows, cols, &no_eps, ops, n, &empty, &post_eps); rc || empty) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto dt) { pq::olmo_postnorm_add_quant_dispatch<dt>(x, ld_x, post_weight, post_eps, residual, ld_r, sum_out, ld_s, rows, cols, q, ld_q, scale, st); });
    return check_launch(fn);
}

// elements from the base of a two-stride operand of K1hn to the end of its last row; false: the product does not fit 64 bits
static bool head_span(int64_t n_outer, int64_t ld_o, int64_t n_inner, int64_t ld_i, int64_t cols, int64_t* span) {
    int64_t a, b;
    if (__builtin_mul_overflow(n_outer - 1, ld_o, &a) || __builtin_mul_overflow(n_inner - 1, ld_i, &b) || __builtin_add_overflow(a, b, &a) ||
        __builtin_add_overflow(a, cols, &a) || a > (INT64_MAX >> 2))
        return false;
    *span = a;
    return true;
}

int32_t pq_head_rmsnorm(const void* x, int64_t ld_xo, int64_t ld_xi, const void* weight, float eps, int32_t gain, int32_t dtype, int64_t n_outer, int64_t n_inner,
                        int64_t cols, void* out, int64_t ld_oo, int64_t ld_oi, void* stream) {
    Range range_("pq:head_rmsnorm (K1hn)");
    const char* fn = "pq_head_rmsnorm";
    if (const int32_t rc = check_dtype(fn, dtype)) return rc;
    if (gain != PQ_GAIN_LLAMA && gain != PQ_GAIN_GEMMA) return fail(PQ_ERR_BAD_ARG, "%s: unknown gain %d (0 = Llama: w * round(x * rs), 1 = Gemma: (x * rs) * (1 + w))", fn, gain);
    if (n_outer < 0 || n_inner < 0) return fail(PQ_ERR_BAD_ARG, "%s: bad shape (n_outer=%lld n_inner=%lld)", fn, (long long)n_outer, (long long)n_inner);
    if (n_outer > 0 && n_inner > 0 && n_outer > ((int64_t)INT32_MAX) / n_inner)
        return fail(PQ_ERR_BAD_ARG, "%s: n_outer * n_inner must be < 2^31 (n_outer=%lld n_inner=%lld)", fn, (long long)n_outer, (long long)n_inner);
    const int64_t heads = n_outer * n_inner, eb = dtype == PQ_F32 ? 4 : 2;
    const struct { const char* name; int64_t ld; } lds[] = {{"ld_xo", ld_xo}, {"ld_xi", ld_xi}, {"ld_oo", ld_oo}, {"ld_oi", ld_oi}};
    for (const auto& l : lds)
        if (l.ld < 0) return fail(PQ_ERR_BAD_ARG, "%s: %s %lld < 0", fn, l.name, (long long)l.ld);
    if (cols >= 0 && n_inner > 1 && ld_xi < cols) return fail(PQ_ERR_BAD_ARG, "%s: ld_xi %lld < cols %lld", fn, (long long)ld_xi, (long long)cols);
    if (cols >= 0 && n_inner > 1 && ld_oi < cols) return fail(PQ_ERR_BAD_ARG, "%s: ld_oi %lld < cols %lld", fn, (long long)ld_oi, (long long)cols);
    // the two-stride operands go to the shared checker as their bounding ranges (vectors of `span` elements): the shape, eps, the empty problem, the null pointers
    // and the overlaps of out with x and with weight
    int64_t span_x = 0, span_o = 0;
    if (heads > 0 && cols > 0 && (!head_span(n_outer, ld_xo, n_inner, ld_xi, cols, &span_x) || !head_span(n_outer, ld_oo, n_inner, ld_oi, cols, &span_o)))
        return fail(PQ_ERR_BAD_ARG, "%s: the strides do not fit 64-bit byte offsets (ld_xo=%lld ld_xi=%lld ld_oo=%lld ld_oi=%lld)", fn, (long long)ld_xo, (long long)ld_xi,
                    (long long)ld_oo, (long long)ld_oi);
    const RowOperand ops[] = {{"x", x, R_IN, nullptr, span_x, eb, ""}, {"weight", weight, R_IN, nullptr, cols, eb, ""}, {"out", out, R_OUT, nullptr, span_o, eb, ""}};
    bool empty;
    if (const int32_t rc = check_row_producer(fn, heads, cols, &eps, ops, 3, &empty); rc || empty) return rc;
    // the rows of out among themselves: the axis with the smaller stride holds whole rows, the other whole runs of it (an axis of one index has no stride)
    {
        int64_t s1 = n_inner > 1 ? ld_oi : -1, n1 = n_inner, s2 = n_outer > 1 ? ld_oo : -1, n2 = n_outer;
        if (s2 >= 0 && (s1 < 0 || s2 < s1)) { std::swap(s1, s2); std::swap(n1, n2); }
        if ((s1 >= 0 && s1 < cols) || (s2 >= 0 && s2 < (n1 - 1) * s1 + cols))
            return fail(PQ_ERR_BAD_ARG, "%s: the rows of out overlap each other (ld_oo=%lld ld_oi=%lld n_outer=%lld n_inner=%lld cols=%lld)", fn, (long long)ld_oo,
                        (long long)ld_oi, (long long)n_outer, (long long)n_inner, (long long)cols);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto dt) { pq::head_rmsnorm_dispatch<dt>(x, ld_xo, ld_xi, weight, eps, gain, n_outer, n_inner, cols, out, ld_oo, ld_oi, st); });
    return check_launch(fn);
}

int32_t pq_scaled_add_rmsnorm_quant_rows(const void* x, int64_t ld_x, const void* residual, int64_t ld_r, float multiplier, void* sum_out, int64_t ld_s, const void* weight,
                                         float eps, int32_t dtype, int64_t rows, int64_t cols, int8_t* q, int64_t ld_q, float* scale, void* h_out, int64_t ld_h, void* stream) {
    Range range_("pq:scaled_add_rmsnorm_quant (K1ma / K1mo)");
    const char* fn = "pq_scaled_add_rmsnorm_quant_rows";
    if (const int32_t rc = check_dtype(fn, dtype)) return rc;
    if (!(multiplier >= -3.4028234e38f && multiplier <= 3.4028234e38f)) return fail(PQ_ERR_BAD_ARG, "%s: multiplier must be finite (multiplier=%g)", fn, (double)multiplier);
    const int64_t eb = dtype == PQ_F32 ? 4 : 2;
    const bool add_only = !weight && !q && !scale && !h_out;          // K1mo: the whole quantisation group is absent (then eps is not read)
    const char* group = " (weight, q and scale go together: all three and h_out null is the add-only form)";
    const RowOperand ops[] = {{"x", x, R_IN, "ld_x", ld_x, eb, ""},
                              {"residual", residual, R_IN, "ld_r", ld_r, eb, ""},
                              {"sum_out", sum_out, R_INOUT, "ld_s", ld_s, eb, kSumNote},
                              {"weight", weight, R_IN, nullptr, cols, eb, group},
                              {"q", q, R_OUT, "ld_q", ld_q, 1, group},
                              {"scale", scale, R_OUT, nullptr, rows, 4, group},
                              {"h_out", h_out, R_OUT, "ld_h", ld_h, eb, nullptr}};
    const float no_eps = 0.0f;
    bool empty;
    if (const int32_t rc = check_row_producer(fn, rows, cols, add_only ? &no_eps : &eps, ops, add_only ? 3 : 7, &empty); rc || empty) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto dt) {
        pq::scaled_add_rmsnorm_quant_dispatch<dt>(x, ld_x, residual, ld_r, multiplier, sum_out, ld_s, weight, eps, rows, cols, q, ld_q, scale, h_out, ld_h, st);
    });
    return check_launch(fn);
}

int32_t pq_gelu_mul_quant_rowwise(const void* g, int64_t ld_g, const void* u, int64_t ld_u, int32_t dtype, int64_t rows, int64_t cols, int32_t kind, int8_t* q, int64_t ld_q,
                                  float* scale, void* h_out, int64_t ld_h, void* stream) {
    Range range_("pq:gelu_mul_quant (K1gg)");
    const char* fn = "pq_gelu_mul_quant_rowwise";
    if (const int32_t rc = check_dtype(fn, dtype)) return rc;
    if (kind != PQ_ACT_GELU_TANH) return fail(PQ_ERR_BAD_ARG, "%s: unsupported kind %d (1 = gelu_tanh is the only gated GELU)", fn, kind);
    const int64_t eb = dtype == PQ_F32 ? 4 : 2;
    const RowOperand ops[] = {{"g", g, R_IN, "ld_g", ld_g, eb, ""},          {"u", u, R_IN, "ld_u", ld_u, eb, ""}, {"q", q, R_OUT, "ld_q", ld_q, 1, ""},
                              {"scale", scale, R_OUT, nullptr, rows, 4, ""}, {"h_out", h_out, R_OUT, "ld_h", ld_h, eb, nullptr}};
    bool empty;
    if (const int32_t rc = check_row_producer(fn, rows, cols, nullptr, ops, 5, &empty); rc || empty) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto dt) { pq::gelu_mul_quant_dispatch<dt>(g, ld_g, u, ld_u, rows, cols, q, ld_q, scale, h_out, ld_h, st); });
    return check_launch(fn);
}

int32_t pq_layernorm_quant_rowwise(const void* x, int64_t ld_x, const void* weight, const void* bias, float eps, int32_t dtype, int64_t rows, int64_t cols,
                                   int8_t* q, int64_t ld_q, float* scale, void* h_out, int64_t ld_h, void* stream) {
    Range range_("pq:layernorm_quant (K1l)");
    const char* fn = "pq_layernorm_quant_rowwise";
    if (const int32_t rc = check_dtype(fn, dtype)) return rc;
    const int64_t eb = dtype == PQ_F32 ? 4 : 2;
    const RowOperand ops[] = {{"x", x, R_IN, "ld_x", ld_x, eb, ""},  {"weight", weight, R_IN, nullptr, cols, eb, kAffineNote}, {"bias", bias, R_IN, nullptr, cols, eb, nullptr},
                              {"q", q, R_OUT, "ld_q", ld_q, 1, ""}, {"scale", scale, R_OUT, nullptr, rows, 4, ""},            {"h_out", h_out, R_OUT, "ld_h", ld_h, eb, nullptr}};
    bool empty;
    if (const int32_t rc = check_row_producer(fn, rows, cols, &eps, ops, 6, &empty); rc || empty) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto dt) { pq::layernorm_quant_dispatch<dt>(x, ld_x, weight, bias, eps, rows, cols, q, ld_q, scale, h_out, ld_h, st); });
    return check_launch(fn);
}

int32_t pq_add_layernorm_quant_rowwise(const void* x, int64_t ld_x, const void* residual, int64_t ld_r, void* sum_out, int64_t ld_s, const void* weight, const void* bias,
                                       float eps, int32_t dtype, int64_t rows, int64_t cols, int8_t* q, int64_t ld_q, float* scale, void* h_out, int64_t ld_h, void* stream) {
    Range range_("pq:add_layernorm_quant (K1al)");
    const char* fn = "pq_add_layernorm_quant_rowwise";
    if (const int32_t rc = check_dtype(fn, dtype)) return rc;
    const int64_t eb = dtype == PQ_F32 ? 4 : 2;
    const RowOperand ops[] = {{"x", x, R_IN, "ld_x", ld_x, eb, ""},                    {"residual", residual, R_IN, "ld_r", ld_r, eb, ""}, {"sum_out", sum_out, R_INOUT, "ld_s", ld_s, eb, kSumNote},
                              {"weight", weight, R_IN, nullptr, cols, eb, kAffineNote}, {"bias", bias, R_IN, nullptr, cols, eb, nullptr},   {"q", q, R_OUT, "ld_q", ld_q, 1, ""},
                              {"scale", scale, R_OUT, nullptr, rows, 4, ""},            {"h_out", h_out, R_OUT, "ld_h", ld_h, eb, nullptr}};
    bool empty;
    if (const int32_t rc = check_row_producer(fn, rows, cols, &eps, ops, 8, &empty); rc || empty) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto dt) { pq::add_layernorm_quant_dispatch<dt>(x, ld_x, residual, ld_r, sum_out, ld_s, weight, bias, eps, rows, cols, q, ld_q, scale, h_out, ld_h, st); });
    return check_launch(fn);
}

int32_t pq_parallel_layernorm_quant_rowwise(const void* a, int64_t ld_a, const void* b, int64_t ld_b, const void* c, int64_t ld_c, void* sum_out, int64_t ld_s,
                                            const void* weight1, const void* bias1, float eps1, const void* weight2, const void* bias2, float eps2, int32_t dtype,
                                            int64_t rows, int64_t cols, int8_t* q1, int64_t ld_q1, float* scale1, void* h1, int64_t ld_h1, int8_t* q2, int64_t ld_q2,
                                            float* scale2, void* h2, int64_t ld_h2, void* stream) {
    Range range_("pq:parallel_layernorm_quant (K1pl / K1l2)");
    const char* fn = "pq_parallel_layernorm_quant_rowwise";
    if (const int32_t rc = check_dtype(fn, dtype)) return rc;
    const int64_t eb = dtype == PQ_F32 ? 4 : 2;
    const bool add = a || b, two = weight2 != nullptr;
    if (rows > 0 && cols > 0) {          // which of the three forms is asked for (an empty problem is a no-op whatever its pointers are)
        if (!a != !b)
            return fail(PQ_ERR_BAD_ARG, "%s: %s is null and %s is not (a and b go together: both null is the form without the add)", fn, a ? "b" : "a", a ? "a" : "b");
        if (!add && sum_out) return fail(PQ_ERR_BAD_ARG, "%s: sum_out must be null without the add (a and b are null: nothing is summed or stored)", fn);
        if (!two)
            for (const auto& [name, p] : {std::pair<const char*, const void*>{"bias2", bias2}, {"q2", q2}, {"scale2", scale2}, {"h2", h2}})
                if (p) return fail(PQ_ERR_BAD_ARG, "%s: %s must be null when weight2 is (one norm: the second group is absent as a whole)", fn, name);
        if (!add && !two) return fail(PQ_ERR_BAD_ARG, "%s: neither an add (a, b null) nor a second norm (weight2 null): that is pq_layernorm_quant_rowwise", fn);
    }
    RowOperand ops[14];
    int n = 0;
    if (add) {
        ops[n++] = {"a", a, R_IN, "ld_a", ld_a, eb, ""};
        ops[n++] = {"b", b, R_IN, "ld_b", ld_b, eb, ""};
    }
    ops[n++] = {"c", c, R_IN, "ld_c", ld_c, eb, ""};
    if (add) ops[n++] = {"sum_out", sum_out, R_INOUT, "ld_s", ld_s, eb, kSumNote};
    ops[n++] = {"weight1", weight1, R_IN, nullptr, cols, eb, kAffineNote};
    ops[n++] = {"bias1", bias1, R_IN, nullptr, cols, eb, nullptr};
    if (two) {
        ops[n++] = {"weight2", weight2, R_IN, nullptr, cols, eb, kAffineNote};
        ops[n++] = {"bias2", bias2, R_IN, nullptr, cols, eb, nullptr};
    }
    ops[n++] = {"q1", q1, R_OUT, "ld_q1", ld_q1, 1, ""};
    ops[n++] = {"scale1", scale1, R_OUT, nullptr, rows, 4, ""};
    ops[n++] = {"h1", h1, R_OUT, "ld_h1", ld_h1, eb, nullptr};
    if (two) {
        ops[n++] = {"q2", q2, R_OUT, "ld_q2", ld_q2, 1, ""};
        ops[n++] = {"scale2", scale2, R_OUT, nullptr, rows, 4, ""};
        ops[n++] = {"h2", h2, R_OUT, "ld_h2", ld_h2, eb, nullptr};
    }
    bool empty;
    if (const int32_t rc = check_row_producer(fn, rows, cols, &eps1, ops, n, &empty, two ? &eps2 : nullptr, "eps2"); rc || empty) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto dt) {
        pq::parallel_layernorm_quant_dispatch<dt>(a, ld_a, b, ld_b, c, ld_c, sum_out, ld_s, weight1, bias1, eps1, weight2, bias2, eps2, rows, cols, q1, ld_q1, scale1, h1, ld_h1,
                                                  q2, ld_q2, scale2, h2, ld_h2, st);
    });
    return check_launch(fn);
}

int32_t pq_act_quant_rowwise(const void* x, int64_t ld_x, int32_t dtype, int64_t rows, int64_t cols, int32_t kind, int8_t* q, int64_t ld_q, float* scale,
                             void* h_out, int64_t ld_h, void* stream) {
    Range range_("pq:act_quant (K1u)");
    const char* fn = "pq_act_quant_rowwise";
    if (const int32_t rc = check_dtype(fn, dtype)) return rc;
    if (kind != PQ_ACT_RELU && kind != PQ_ACT_GELU_TANH && kind != PQ_ACT_GELU_ERF)
        return fail(PQ_ERR_BAD_ARG, "%s: unknown kind %d (0 = relu, 1 = gelu_tanh, 2 = gelu_erf)", fn, kind);
    const int64_t eb = dtype == PQ_F32 ? 4 : 2;
    const RowOperand ops[] = {{"x", x, R_IN, "ld_x", ld_x, eb, ""}, {"q", q, R_OUT, "ld_q", ld_q, 1, ""}, {"scale", scale, R_OUT, nullptr, rows, 4, ""}, {"h_out", h_out, R_OUT, "ld_h", ld_h, eb, nullptr}};
    bool empty;
    if (const int32_t rc = check_row_producer(fn, rows, cols, nullptr, ops, 4, &empty); rc || empty) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto dt) { pq::act_quant_dispatch<dt>(kind, x, ld_x, rows, cols, q, ld_q, scale, h_out, ld_h, st); });
    return check_launch(fn);
}

int32_t pq_dequant(const int8_t* q, int64_t ld_q, const float* scale, int32_t axis, int64_t rows, int64_t cols,
                   void* out, int64_t ld_out, int32_t out_dtype, void* stream) {
    Range range_("pq:dequant");
    if (const int32_t rc = check_dtype("pq_dequant", out_dtype)) return rc;
    if (axis != 0 && axis != 1) return fail(PQ_ERR_BAD_ARG, "pq_dequant: axis must be 0 or 1, got %d", axis);
    if (bad_mat(q, rows, cols, ld_q) || bad_mat(out, rows, cols, ld_out) || (rows > 0 && cols > 0 && !scale))
        return fail(PQ_ERR_BAD_ARG, "pq_dequant: bad matrix (rows=%lld cols=%lld)", (long long)rows, (long long)cols);
    if (rows == 0 || cols == 0) return PQ_OK;
    {
        const NamedExtent ops[] = {{"q", extent_of(q, ld_q, rows, cols, 1), false}, {"scale", vec_extent(scale, axis == 0 ? cols : rows, 4), false},
                                   {"out", extent_of(out, ld_out, rows, cols, dtype_bytes(out_dtype)), true}};
        if (const int32_t rc = check_disjoint("pq_dequant", ops, 3)) return rc;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(out_dtype, [&](auto dt) { pq::dequant_dispatch<dt>(q, ld_q, scale, axis, rows, cols, out, ld_out, st); });
    return check_launch("pq_dequant");
}

int32_t pq_gemm_s8s8s32(const int8_t* a, int64_t lda, const int8_t* b, int64_t ldb, int32_t* c, int64_t ldc,
                        int64_t M, int64_t N, int64_t K, void* stream) {
    Range range_("pq:gemm_s8s8s32 (K3)");
    if (M < 0 || N < 0 || K < 0 || bad_mat(a, M, K, lda) || bad_mat(b, N, K, ldb) || bad_mat(c, M, N, ldc))
        return fail(PQ_ERR_BAD_ARG, "pq_gemm_s8s8s32: bad arguments (M=%lld N=%lld K=%lld lda=%lld ldb=%lld ldc=%lld)", (long long)M, (long long)N, (long long)K, (long long)lda, (long long)ldb, (long long)ldc);
    if (M == 0 || N == 0) return PQ_OK;
    const pq::EpiArgs epi = make_epi(nullptr, nullptr, nullptr, c, ldc, 0, EPI_NXCD);      // (y_any_align stays 0 here, as it always has)
    run_gemm_auto<pq::OUT_I32>(pick_variant(a, lda, b, ldb, M, N, K), a, lda, b, ldb, epi, M, N, K, static_cast<hipStream_t>(stream));
    return check_launch("pq_gemm_s8s8s32");
}

size_t pq_qlinear_workspace_bytes(int64_t M, int64_t N, int64_t K) {
    CallScope scope_;
    {   // (alignment of the operands is unknown here: assume the fast path, as pq_gemm_variant_name does)
        const Variant v = pick_variant(reinterpret_cast<const int8_t*>(16), K, reinterpret_cast<const int8_t*>(16), K, M, N, K);
        if (v == V_RING64X128 || v == V_RING64X64 || v == V_RING128X160) return 0;      // the mid-M tiles and the 128 x 160 tile run single-pass
        // qlinear_core's `tiled`: every other dispatch (the generic kernel of M * N < 128^2 or of a non-positive size, the weight-streaming kernel, a forced variant)
        // runs single-pass and never looks at a workspace — the query must not ask for one that the call would not check
        if (!(v == V_SP256_16 || v == V_SP128_16 || v == V_RING128) || forced_variant() != V_AUTO) return 0;
    }
    if (const int f = fsk_plan(M, N, K)) return pq::fsk_workspace_bytes(M, N, f);
    int tm = 256;
    const int s = splitk_plan(M, N, K, &tm);
    return s > 1 ? (size_t)s * (size_t)M * (size_t)N * sizeof(int32_t) : 0;
}

// the GEMM + epilogue of one (M x N x K, A rows x B rows) problem; the scales, bias, y and flags are already in the kernel's orientation
static int32_t qlinear_core(const char* what, const int8_t* a, int64_t lda, const float* a_scale, const int8_t* b, int64_t ldb, const float* b_scale, const void* bias, void* y,
                            int64_t ldy, int32_t flags, int32_t out_dtype, int64_t M, int64_t N, int64_t K, void* workspace, size_t workspace_bytes, void* stream) {
    Range range_("pq:qlinear_s8 (K3+K4)");
    const pq::EpiArgs epi = make_epi(a_scale, b_scale, bias, y, ldy, flags);
    const Variant v = pick_variant(a, lda, b, ldb, M, N, K);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // split-K needs the caller's workspace (pq_qlinear_workspace_bytes); without it the single-pass path runs.
    const bool tiled = (v == V_SP256_16 || v == V_SP128_16 || v == V_RING128) && forced_variant() == V_AUTO;
    if (const int f = tiled ? fsk_plan(M, N, K) : 0; f > 1 && workspace != nullptr) {
        if (const int32_t rc = check_workspace(what, workspace, workspace_bytes, pq::fsk_workspace_bytes(M, N, f), 16)) return rc;
        return launch_fsk(what, a, lda, b, ldb, epi, out_dtype, M, N, K, f, workspace, st);
    }
    int tm = 256;
    const int ks = tiled && fsk_plan(M, N, K) == 0 ? splitk_plan(M, N, K, &tm) : 1;
    if (ks > 1 && workspace != nullptr) {
        if (const int32_t rc = check_workspace(what, workspace, workspace_bytes, (size_t)ks * (size_t)M * (size_t)N * sizeof(int32_t), 16)) return rc;
        int32_t* slabs = static_cast<int32_t*>(workspace);
        if (tm == 128) pq::launch_gemm_splitk_i32<128>(a, lda, b, ldb, slabs, M, N, K, ks, st, epi.nxcd);
        else pq::launch_gemm_splitk_i32<256>(a, lda, b, ldb, slabs, M, N, K, ks, st, epi.nxcd);
        by_dtype(out_dtype, [&](auto dt) { pq::launch_splitk_reduce<dt>(slabs, ks, M, N, epi, st); });
        return check_launch(what);
    }
    by_dtype(out_dtype, [&](auto dt) { run_gemm_auto<dt>(v, a, lda, b, ldb, epi, M, N, K, st); });
    return check_launch(what);
}

int32_t pq_qlinear_s8(const int8_t* a, int64_t lda, const float* a_scale, const int8_t* b, int64_t ldb,
                      const float* b_scale, const void* bias, void* y, int64_t ldy, int32_t out_dtype, int64_t M,
                      int64_t N, int64_t K, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int32_t rc = check_dtype("pq_qlinear_s8", out_dtype)) return rc;
    if (M < 0 || N < 0 || K < 0 || bad_mat(a, M, K, lda) || bad_mat(b, N, K, ldb) || bad_mat(y, M, N, ldy) ||
        (M > 0 && !a_scale) || (N > 0 && !b_scale))
        return fail(PQ_ERR_BAD_ARG, "pq_qlinear_s8: bad arguments (M=%lld N=%lld K=%lld lda=%lld ldb=%lld ldy=%lld)", (long long)M, (long long)N, (long long)K, (long long)lda, (long long)ldb, (long long)ldy);
    if (M == 0 || N == 0) return PQ_OK;
    return qlinear_core("pq_qlinear_s8", a, lda, a_scale, b, ldb, b_scale, bias, y, ldy, 0, out_dtype, M, N, K, workspace, workspace_bytes, stream);
}

// y^T[N, M] of the same qlinear: the kernel's rows are the weight rows (n), its columns the tokens (m); the epilogue applies
// the token (column) scale first and runs the bias along rows, so every value has the bits of pq_qlinear_s8's y[m][n].
size_t pq_qlinear_t_workspace_bytes(int64_t M, int64_t N, int64_t K) { return pq_qlinear_workspace_bytes(N, M, K); }

int32_t pq_qlinear_s8_t(const int8_t* a, int64_t lda, const float* a_scale, const int8_t* b, int64_t ldb,
                        const float* b_scale, const void* bias, void* yt, int64_t ldyt, int32_t out_dtype, int64_t M,
                        int64_t N, int64_t K, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int32_t rc = check_dtype("pq_qlinear_s8_t", out_dtype)) return rc;
    if (M < 0 || N < 0 || K < 0 || bad_mat(a, M, K, lda) || bad_mat(b, N, K, ldb) || bad_mat(yt, N, M, ldyt) ||
        (M > 0 && !a_scale) || (N > 0 && !b_scale))
        return fail(PQ_ERR_BAD_ARG, "pq_qlinear_s8_t: bad arguments (M=%lld N=%lld K=%lld lda=%lld ldb=%lld ldyt=%lld)", (long long)M, (long long)N, (long long)K, (long long)lda, (long long)ldb, (long long)ldyt);
    if (M == 0 || N == 0) return PQ_OK;
    // the workspace arguments are validated the same way on every path (the streaming path below does not use them; error behaviour must not depend on M)
    if (workspace != nullptr && (reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return fail(PQ_ERR_BAD_ALIGN, "pq_qlinear_s8_t: workspace must be 16-byte aligned");
    if (workspace == nullptr && workspace_bytes != 0) return fail(PQ_ERR_BAD_ARG, "pq_qlinear_s8_t: workspace_bytes without a workspace");
    {   // few tokens: the swapped form below would be a 16-column problem for the tile kernels (16 x 4096 x 4096: 23 us); the weight-streaming kernel computes the
        // product in its normal orientation and stores it transposed (5.8 us).  Same arithmetic as pq_qlinear_s8: same bits.
        CallScope scope_;
        const Variant f = forced_variant();
        if ((f == V_AUTO || f == V_SKINNY) && pick_variant(a, lda, b, ldb, M, N, K) == V_SKINNY) {
            Range range_("pq:qlinear_s8_t (K3+K4, streaming)");         // (named only where the streaming kernel really runs: marker traces)
            const pq::EpiArgs e = make_epi(a_scale, b_scale, bias, yt, ldyt, pq::EPI_STORE_T, EPI_NXCD);      // (y_any_align stays 0 on this branch, as it always has)
            hipStream_t st = static_cast<hipStream_t>(stream);
            by_dtype(out_dtype, [&](auto dt) { run_gemm<dt>(V_SKINNY, a, lda, b, ldb, e, M, N, K, st); });
            return check_launch("pq_qlinear_s8_t");
        }
    }
    return qlinear_core("pq_qlinear_s8_t", b, ldb, b_scale, a, lda, a_scale, bias, yt, ldyt, pq::EPI_COL_FIRST | (bias ? pq::EPI_BIAS_ROWS : 0), out_dtype, N, M, K, workspace,
                        workspace_bytes, stream);
}

// ---- qlinear on STACKED activation codes (what an all-gather of the ranks' int8 column blocks leaves: [G][M][K / G]; the planners: pq_plan.hip)
// (the short form knows neither the operand's base nor its strides: it returns what the layout pass needs — always enough, whichever way the call goes)
size_t pq_qlinear_kslabs_workspace_bytes(int64_t M, int64_t N, int64_t K, int64_t k_per_slab) {
    CallScope scope_;
    if (M <= 0 || N <= 0 || K <= 0 || k_per_slab <= 0 || K % k_per_slab != 0) return 0;
    if (K == k_per_slab) return pq_qlinear_workspace_bytes(M, N, K);
    return align256((size_t)M * (size_t)K) + pq_qlinear_workspace_bytes(M, N, K);
}
// the exact form: decides on the operand the call will see (only the ALIGNMENT of `a` and `b` is looked at, nothing is read)
size_t pq_qlinear_kslabs_workspace_bytes_for(const int8_t* a, int64_t lda, int64_t slab_stride, int64_t k_per_slab, const int8_t* b, int64_t ldb, int64_t M, int64_t N, int64_t K) {
    CallScope scope_;
    if (M <= 0 || N <= 0 || K <= 0 || k_per_slab <= 0 || K % k_per_slab != 0) return 0;
    if (K == k_per_slab) return pq_qlinear_workspace_bytes(M, N, K);
    if (const int f = kslabs_fsk_in_place(a, lda, slab_stride, k_per_slab, b, ldb, M, N, K)) return pq::fsk_workspace_bytes(M, N, f);
    if (kslabs_in_place(a, lda, slab_stride, k_per_slab, b, ldb, M, N, K) != V_GENERIC) return 0;
    return align256((size_t)M * (size_t)K) + pq_qlinear_workspace_bytes(M, N, K);
}

const char* pq_kslabs_way_name(const int8_t* a, int64_t lda, int64_t slab_stride, int64_t k_per_slab, const int8_t* b, int64_t ldb, int64_t M, int64_t N, int64_t K,
                               size_t workspace_bytes) {
    CallScope scope_;
    return kslabs_way_name(a, lda, slab_stride, k_per_slab, b, ldb, M, N, K, workspace_bytes);
}

int32_t pq_qlinear_s8_kslabs(const int8_t* a, int64_t lda, int64_t slab_stride, int64_t k_per_slab, const float* a_scale, const int8_t* b, int64_t ldb,
                             const float* b_scale, const void* bias, void* y, int64_t ldy, int32_t out_dtype, int64_t M, int64_t N, int64_t K,
                             void* workspace, size_t workspace_bytes, void* stream) {
    CallScope scope_;
    const char* what = "pq_qlinear_s8_kslabs";
    if (const int32_t rc = check_dtype(what, out_dtype)) return rc;
    if (M < 0 || N < 0 || K < 0 || k_per_slab <= 0 || K % k_per_slab != 0 || bad_mat(a, M, k_per_slab, lda) || bad_mat(b, N, K, ldb) || bad_mat(y, M, N, ldy) ||
        (M > 0 && !a_scale) || (N > 0 && !b_scale) || (K > k_per_slab && slab_stride < (M - 1) * lda + k_per_slab))
        return fail(PQ_ERR_BAD_ARG, "pq_qlinear_s8_kslabs: bad arguments (M=%lld N=%lld K=%lld k_per_slab=%lld lda=%lld slab_stride=%lld ldb=%lld ldy=%lld)", (long long)M, (long long)N,
                    (long long)K, (long long)k_per_slab, (long long)lda, (long long)slab_stride, (long long)ldb, (long long)ldy);
    if (M == 0 || N == 0) return PQ_OK;
    if (K == k_per_slab) return pq_qlinear_s8(a, lda, a_scale, b, ldb, b_scale, bias, y, ldy, out_dtype, M, N, K, workspace, workspace_bytes, stream);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int f = kslabs_fsk_in_place(a, lda, slab_stride, k_per_slab, b, ldb, M, N, K);
        f > 1 && workspace != nullptr && workspace_bytes >= pq::fsk_workspace_bytes(M, N, f) && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0) {
        // (a workspace too small for the hand-over is not an error here, unlike in qlinear_core: the ring tile below walks the slabs without one)
        Range range_("pq:qlinear_s8_kslabs (K3+K4, fused split-K, slabs walked in place)");
        return launch_fsk(what, a, lda, b, ldb, make_epi(a_scale, b_scale, bias, y, ldy, 0), out_dtype, M, N, K, f, workspace, st, slab_stride, k_per_slab);
    }
    if (const Variant v = kslabs_in_place(a, lda, slab_stride, k_per_slab, b, ldb, M, N, K); v != V_GENERIC) {
        Range range_("pq:qlinear_s8_kslabs (K3+K4, slabs walked in place)");
        const pq::EpiArgs epi = make_epi(a_scale, b_scale, bias, y, ldy, 0);
        if (!pq::epi_flags_valid(epi.flags, epi.bias != nullptr)) abort();
        by_dtype(out_dtype, [&](auto dt) {
            if (v == V_RING128) pq::launch_gemm_ring128<dt>(a, lda, b, ldb, epi, M, N, K, st, slab_stride, k_per_slab);
            else pq::launch_gemm_ringt<dt>(v == V_RING64X128 ? 0 : (v == V_RING64X64 ? 1 : 2), a, lda, b, ldb, epi, M, N, K, st, slab_stride, k_per_slab);
        });
        return check_launch(what);
    }
    // any other shape: one layout pass into the caller's workspace (reads + writes M * K bytes), then the planner's own choice on row-major codes
    const size_t need_a = align256((size_t)M * (size_t)K);
    if (const int32_t rc = check_workspace(what, workspace, workspace_bytes, need_a + pq_qlinear_workspace_bytes(M, N, K), 256)) return rc;
    uint8_t* flat = static_cast<uint8_t*>(workspace);
    {
        Range range_("pq:unstack_kslabs");
        const int nslabs = (int)(K / k_per_slab);
        const bool vec = (k_per_slab % 16 == 0) && (lda % 16 == 0) && (slab_stride % 16 == 0) && ((reinterpret_cast<uintptr_t>(a) & 15) == 0);
        const int64_t units = (int64_t)M * K / (vec ? 16 : 1);
        int64_t blocks = (units + 255) / 256;
        blocks = blocks > 256 * 16 ? 256 * 16 : (blocks < 1 ? 1 : blocks);
        if (vec) unstack_kslabs_kernel<v4u_><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(reinterpret_cast<const uint8_t*>(a), lda, slab_stride, flat, K, M, k_per_slab / 16, nslabs);
        else unstack_kslabs_kernel<uint8_t><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(reinterpret_cast<const uint8_t*>(a), lda, slab_stride, flat, K, M, k_per_slab, nslabs);
        const int32_t rc = check_launch("pq_qlinear_s8_kslabs (layout pass)");
        if (rc != PQ_OK) return rc;
    }
    const size_t rest = workspace_bytes - need_a;
    return pq_qlinear_s8(reinterpret_cast<const int8_t*>(flat), K, a_scale, b, ldb, b_scale, bias, y, ldy, out_dtype, M, N, K, rest ? flat + need_a : nullptr, rest, stream);
}

// ---- grouped GEMM over the experts of a mixture-of-experts layer (gemm_s8_grouped.hip; the tile: pq_plan.hip, grouped_plan)
// everything pq_qlinear_s8_grouped and pq_gemm_s8s8s32_grouped have in common; no HIP call is made before the checks are through
static int32_t grouped_check(const char* what, const int8_t* xq, int64_t ldx, const int32_t* a_row_index, int64_t x_rows, const int8_t* wq, int64_t ldw,
                             int64_t w_expert_stride, const int32_t* offsets, int32_t E, int64_t M_total, int64_t N, int64_t K, const void* y, int64_t ldy) {
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (E <= 0 || E > 1024) return fail(PQ_ERR_BAD_ARG, "%s: E = %d (1 .. 1024 experts)", what, E);
    if (M_total < 0 || M_total >= ((int64_t)1 << 30)) return fail(PQ_ERR_BAD_ARG, "%s: M_total = %lld", what, (long long)M_total);
    if (N < 0 || N >= ((int64_t)1 << 30)) return fail(PQ_ERR_BAD_ARG, "%s: N = %lld", what, (long long)N);
    if (K < 128 || K % 128 != 0 || K >= ((int64_t)1 << 30)) return fail(PQ_ERR_BAD_ARG, "%s: K = %lld must be a positive multiple of 128 (pad the codes with zeros)", what, (long long)K);
    if (x_rows < 0 || x_rows >= ((int64_t)1 << 31)) return fail(PQ_ERR_BAD_ARG, "%s: x_rows = %lld", what, (long long)x_rows);
    if (ldx < K || ldx % 16 != 0 || ldx >= (1 << 23)) return fail(PQ_ERR_BAD_ARG, "%s: ldx = %lld (>= K, a multiple of 16, < 2^23)", what, (long long)ldx);
    if (ldw < K || ldw % 16 != 0 || ldw >= (1 << 23)) return fail(PQ_ERR_BAD_ARG, "%s: ldw = %lld (>= K, a multiple of 16, < 2^23)", what, (long long)ldw);
    if (w_expert_stride % 16 != 0 || (N > 0 && w_expert_stride < (N - 1) * ldw + K))
        return fail(PQ_ERR_BAD_ARG, "%s: w_expert_stride = %lld (a multiple of 16, >= (N - 1) * ldw + K)", what, (long long)w_expert_stride);
    if (ldy < N) return fail(PQ_ERR_BAD_ARG, "%s: ldy = %lld < N = %lld", what, (long long)ldy, (long long)N);
    if (!offsets) return fail(PQ_ERR_BAD_ARG, "%s: offsets is null", what);
    if (M_total > 0 && N > 0 && (!xq || !wq || !y)) return fail(PQ_ERR_BAD_ARG, "%s: %s is null", what, !xq ? "xq" : (!wq ? "wq" : "y"));
    if (!al16(xq) || !al16(wq)) return fail(PQ_ERR_BAD_ARG, "%s: %s must be 16-byte aligned", what, !al16(xq) ? "xq" : "wq");
    if (a_row_index) {
        // the loader's per-lane source offset is 32 bits (a_row_index[r] * ldx + 16 * chunk): the address math in the K loop is not widened for larger operands
        if (x_rows < 1) return fail(PQ_ERR_BAD_ARG, "%s: x_rows = %lld with a_row_index", what, (long long)x_rows);
        if (x_rows * ldx >= ((int64_t)1 << 32)) return fail(PQ_ERR_BAD_ARG, "%s: x_rows * ldx = %lld >= 2^32 with a_row_index", what, (long long)(x_rows * ldx));
    } else if (x_rows < M_total) {
        return fail(PQ_ERR_BAD_ARG, "%s: x_rows = %lld < M_total = %lld without a_row_index", what, (long long)x_rows, (long long)M_total);
    }
    return PQ_OK;
}

int32_t pq_qlinear_s8_grouped(const int8_t* xq, int64_t ldx, const int32_t* a_row_index, int64_t x_rows, const float* xs, const int8_t* wq, int64_t ldw,
                              int64_t w_expert_stride, const float* ws, const void* bias, const int32_t* offsets, int32_t E, int64_t M_total, int64_t N, int64_t K,
                              void* y, int64_t ldy, int32_t out_dtype, void* stream) {
    Range range_("pq:qlinear_s8_grouped (K3+K4)");
    if (out_dtype < 0 || out_dtype > 2) return fail(PQ_ERR_BAD_ARG, "pq_qlinear_s8_grouped: unknown out_dtype %d", out_dtype);
    if (const int32_t st = grouped_check("pq_qlinear_s8_grouped", xq, ldx, a_row_index, x_rows, wq, ldw, w_expert_stride, offsets, E, M_total, N, K, y, ldy)) return st;
    if (M_total > 0 && N > 0 && (!xs || !ws)) return fail(PQ_ERR_BAD_ARG, "pq_qlinear_s8_grouped: %s is null", !xs ? "xs" : "ws");
    if (M_total == 0 || N == 0) return PQ_OK;
    const pq::EpiArgs epi = make_epi(xs, ws, bias, y, ldy, 0);
    const int tile = grouped_plan(E, M_total, N), rot = options().grouped_rot ? 1 : 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(out_dtype, [&](auto dt) { pq::launch_gemm_grouped<dt>(tile, xq, ldx, a_row_index, x_rows, wq, ldw, w_expert_stride, epi, offsets, E, M_total, N, K, rot, st); });
    return check_launch("pq_qlinear_s8_grouped");
}

int32_t pq_gemm_s8s8s32_grouped(const int8_t* xq, int64_t ldx, const int32_t* a_row_index, int64_t x_rows, const int8_t* wq, int64_t ldw, int64_t w_expert_stride,
                                const int32_t* offsets, int32_t E, int64_t M_total, int64_t N, int64_t K, int32_t* acc, int64_t ldacc, void* stream) {
    Range range_("pq:gemm_s8s8s32_grouped (K3)");
    if (const int32_t st = grouped_check("pq_gemm_s8s8s32_grouped", xq, ldx, a_row_index, x_rows, wq, ldw, w_expert_stride, offsets, E, M_total, N, K, acc, ldacc)) return st;
    if (M_total == 0 || N == 0) return PQ_OK;
    const pq::EpiArgs epi = make_epi(nullptr, nullptr, nullptr, acc, ldacc, 0);
    pq::launch_gemm_grouped<pq::OUT_I32>(grouped_plan(E, M_total, N), xq, ldx, a_row_index, x_rows, wq, ldw, w_expert_stride, epi, offsets, E, M_total, N, K,
                                         options().grouped_rot ? 1 : 0, static_cast<hipStream_t>(stream));
    return check_launch("pq_gemm_s8s8s32_grouped");
}

const char* pq_grouped_variant_name(int32_t E, int64_t M_total, int64_t N, int64_t K) {
    CallScope scope_;
    (void)K;      // (both tiles step through K in the same 128-byte K-tiles)
    return grouped_variant_name(E, M_total, N);
}

// ---- the grouped GEMM at decode: at most 64 grouped rows, the live experts' weights streamed once (gemm_s8_grouped_stream.hip).  Entry points of their own: the planner
// of pq_qlinear_s8_grouped and pq_grouped_variant_name keep answering for the tile kernels at every M_total.
static int32_t grouped_stream_rows_check(const char* what, int64_t M_total) {
    if (M_total > 64) return fail(PQ_ERR_BAD_ARG, "%s: M_total = %lld (the weight-streaming grouped kernel serves at most 64 grouped rows; use pq_qlinear_s8_grouped)", what, (long long)M_total);
    return PQ_OK;
}

int32_t pq_qlinear_s8_grouped_stream(const int8_t* xq, int64_t ldx, const int32_t* a_row_index, int64_t x_rows, const float* xs, const int8_t* wq, int64_t ldw,
                                     int64_t w_expert_stride, const float* ws, const void* bias, const int32_t* offsets, int32_t E, int64_t M_total, int64_t N, int64_t K,
                                     void* y, int64_t ldy, int32_t out_dtype, void* stream) {
    Range range_("pq:qlinear_s8_grouped_stream (K3+K4)");
    if (out_dtype < 0 || out_dtype > 2) return fail(PQ_ERR_BAD_ARG, "pq_qlinear_s8_grouped_stream: unknown out_dtype %d", out_dtype);
    if (const int32_t st = grouped_check("pq_qlinear_s8_grouped_stream", xq, ldx, a_row_index, x_rows, wq, ldw, w_expert_stride, offsets, E, M_total, N, K, y, ldy)) return st;
    if (const int32_t st = grouped_stream_rows_check("pq_qlinear_s8_grouped_stream", M_total)) return st;
    if (M_total > 0 && N > 0 && (!xs || !ws)) return fail(PQ_ERR_BAD_ARG, "pq_qlinear_s8_grouped_stream: %s is null", !xs ? "xs" : "ws");
    if (M_total == 0 || N == 0) return PQ_OK;
    const pq::EpiArgs epi = make_epi(xs, ws, bias, y, ldy, 0, EPI_BARE);      // (neither nxcd nor y_any_align is passed to this kernel, as it always has been)
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(out_dtype, [&](auto dt) { pq::launch_gemm_grouped_stream<dt>(xq, ldx, a_row_index, x_rows, wq, ldw, w_expert_stride, epi, offsets, E, M_total, N, K, st); });
    return check_launch("pq_qlinear_s8_grouped_stream");
}

int32_t pq_gemm_s8s8s32_grouped_stream(const int8_t* xq, int64_t ldx, const int32_t* a_row_index, int64_t x_rows, const int8_t* wq, int64_t ldw, int64_t w_expert_stride,
                                       const int32_t* offsets, int32_t E, int64_t M_total, int64_t N, int64_t K, int32_t* acc, int64_t ldacc, void* stream) {
    Range range_("pq:gemm_s8s8s32_grouped_stream (K3)");
    if (const int32_t st = grouped_check("pq_gemm_s8s8s32_grouped_stream", xq, ldx, a_row_index, x_rows, wq, ldw, w_expert_stride, offsets, E, M_total, N, K, acc, ldacc)) return st;
    if (const int32_t st = grouped_stream_rows_check("pq_gemm_s8s8s32_grouped_stream", M_total)) return st;
    if (M_total == 0 || N == 0) return PQ_OK;
    const pq::EpiArgs epi = make_epi(nullptr, nullptr, nullptr, acc, ldacc, 0, EPI_BARE);
    pq::launch_gemm_grouped_stream<pq::OUT_I32>(xq, ldx, a_row_index, x_rows, wq, ldw, w_expert_stride, epi, offsets, E, M_total, N, K, static_cast<hipStream_t>(stream));
    return check_launch("pq_gemm_s8s8s32_grouped_stream");
}

const char* pq_grouped_stream_plan_name(int32_t E, int64_t M_total, int64_t N, int64_t K) {
    CallScope scope_;
    int mt = 1, rb = 1, ks = 1;
    pq::grouped_stream_plan(E < 1 ? 1 : E, M_total < 0 ? 0 : (M_total > 64 ? 64 : M_total), N < 0 ? 0 : N, K < 64 ? 64 : K, &mt, &rb, &ks);
    return pq::grouped_stream_plan_name(mt, rb, ks);
}

// ---- routing and combine of a mixture-of-experts layer (moe_kernels.hip): every argument is checked, and the failing one named, before any HIP call
static int32_t moe_dims_check(const char* what, int64_t T, int32_t k, int32_t E, bool with_E) {
    if (with_E && (E <= 0 || E > 1024)) return fail(PQ_ERR_BAD_ARG, "%s: E = %d (1 .. 1024 experts)", what, E);
    if (k <= 0 || k > 64) return fail(PQ_ERR_BAD_ARG, "%s: k = %d (1 .. 64 experts per token)", what, k);
    if (T < 0) return fail(PQ_ERR_BAD_ARG, "%s: T = %lld", what, (long long)T);
    if (T >= ((int64_t)1 << 31) || T * k >= ((int64_t)1 << 31)) return fail(PQ_ERR_BAD_ARG, "%s: T * k = %lld x %d >= 2^31", what, (long long)T, k);
    return PQ_OK;
}

size_t pq_moe_route_workspace_bytes(int64_t T, int32_t k, int32_t E) {
    if (T <= 0 || k <= 0 || k > 64 || E <= 0 || E > 1024 || T >= ((int64_t)1 << 31) || T * k >= ((int64_t)1 << 31)) return 0;
    return pq::moe_route_workspace_bytes(T * k, E);
}

int32_t pq_moe_route(const void* topk_ids, int32_t ids_are_int64, int64_t ld_ids, int64_t T, int32_t k, int32_t E, int32_t* offsets, int32_t* row_index,
                     int32_t* rows_of, int32_t* slot_of, const float* xs, float* xs_sorted, void* workspace, size_t workspace_bytes, void* stream) {
    Range range_("pq:moe_route (R)");
    const char* what = "pq_moe_route";
    if (const int32_t st = moe_dims_check(what, T, k, E, true)) return st;
    if (ids_are_int64 != 0 && ids_are_int64 != 1) return fail(PQ_ERR_BAD_ARG, "%s: ids_are_int64 = %d (0 = int32 ids, 1 = int64 ids)", what, ids_are_int64);
    if (ld_ids < k) return fail(PQ_ERR_BAD_ARG, "%s: ld_ids = %lld < k = %d", what, (long long)ld_ids, k);
    if (!offsets) return fail(PQ_ERR_BAD_ARG, "%s: offsets is null", what);
    if ((xs == nullptr) != (xs_sorted == nullptr)) return fail(PQ_ERR_BAD_ARG, "%s: %s without %s (both or neither)", what, xs ? "xs" : "xs_sorted", xs ? "xs_sorted" : "xs");
    if (T > 0 && (!topk_ids || !row_index || !rows_of || !slot_of))
        return fail(PQ_ERR_BAD_ARG, "%s: %s is null", what, !topk_ids ? "topk_ids" : (!row_index ? "row_index" : (!rows_of ? "rows_of" : "slot_of")));
    if ((reinterpret_cast<uintptr_t>(topk_ids) & (ids_are_int64 ? 7 : 3)) != 0) return fail(PQ_ERR_BAD_ALIGN, "%s: topk_ids is not aligned to its element size", what);
    const size_t need = pq::moe_route_workspace_bytes(T * k, E);
    if (need > 0) {
        if (!workspace) return fail(PQ_ERR_BAD_ARG, "%s: workspace is null (%zu bytes needed: pq_moe_route_workspace_bytes)", what, need);
        if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return fail(PQ_ERR_BAD_ALIGN, "%s: workspace must be 16-byte aligned", what);
        if (workspace_bytes < need) return fail(PQ_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", what, workspace_bytes, need);
    }
    // (T == 0 still launches: the one workgroup writes offsets = zeros)
    pq::launch_moe_route(topk_ids, ids_are_int64 != 0, ld_ids, T, k, E, offsets, row_index, rows_of, slot_of, xs, xs_sorted, workspace, static_cast<hipStream_t>(stream));
    return check_launch(what);
}

int32_t pq_moe_combine(const void* y, int64_t ldy, int32_t dtype, int64_t M_total, const int32_t* rows_of, const int32_t* slot_of, const void* topk_w, int64_t ld_w,
                       int64_t T, int32_t k, int64_t H, void* out, int64_t ld_out, void* stream) {
    Range range_("pq:moe_combine (C)");
    const char* what = "pq_moe_combine";
    if (const int32_t rc = check_dtype(what, dtype)) return rc;
    if (const int32_t st = moe_dims_check(what, T, k, 1, false)) return st;
    if (H < 0 || H >= ((int64_t)1 << 31)) return fail(PQ_ERR_BAD_ARG, "%s: H = %lld", what, (long long)H);
    if (M_total < 0 || M_total >= ((int64_t)1 << 31)) return fail(PQ_ERR_BAD_ARG, "%s: M_total = %lld", what, (long long)M_total);
    if (ldy < H) return fail(PQ_ERR_BAD_ARG, "%s: ldy = %lld < H = %lld", what, (long long)ldy, (long long)H);
    if (ld_out < H) return fail(PQ_ERR_BAD_ARG, "%s: ld_out = %lld < H = %lld", what, (long long)ld_out, (long long)H);
    if (ld_w < k) return fail(PQ_ERR_BAD_ARG, "%s: ld_w = %lld < k = %d", what, (long long)ld_w, k);
    if (T > 0 && H > 0) {
        if (!y || !rows_of || !slot_of || !topk_w || !out)
            return fail(PQ_ERR_BAD_ARG, "%s: %s is null", what, !y ? "y" : (!rows_of ? "rows_of" : (!slot_of ? "slot_of" : (!topk_w ? "topk_w" : "out"))));
        if (M_total < 1) return fail(PQ_ERR_BAD_ARG, "%s: M_total = %lld: no row of y to read for T = %lld tokens", what, (long long)M_total, (long long)T);
        const uintptr_t esz = dtype == PQ_F32 ? 4 : 2;
        if ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(topk_w)) & (esz - 1))
            return fail(PQ_ERR_BAD_ALIGN, "%s: y, out and topk_w must be aligned to their element size", what);
    }
    if (T == 0 || H == 0) return PQ_OK;
    {
        const int64_t eb = dtype_bytes(dtype);
        const NamedExtent ops[] = {{"y", extent_of(y, ldy, M_total, H, eb), false}, {"rows_of", vec_extent(rows_of, T * k, 4), false}, {"slot_of", vec_extent(slot_of, T * k, 4), false},
                                   {"topk_w", extent_of(topk_w, ld_w, T, k, eb), false}, {"out", extent_of(out, ld_out, T, H, eb), true}};
        if (const int32_t rc = check_disjoint(what, ops, 5)) return rc;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto dt) { pq::moe_combine_dispatch<dt>(y, ldy, M_total, rows_of, slot_of, topk_w, ld_w, T, k, H, out, ld_out, st); });
    return check_launch(what);
}

int32_t pq_moe_topk(const void* logits, int32_t dtype, int64_t ld_logits, int64_t T, int32_t E, int32_t k, int32_t kind, int32_t renormalise, void* weights, int32_t w_dtype,
                    int64_t ld_w, void* ids, int32_t ids_are_int64, int64_t ld_ids, void* stream) {
    Range range_("pq:moe_topk (K-rt)");
    const char* what = "pq_moe_topk";
    if (const int32_t rc = check_dtype(what, dtype)) return rc;
    if (w_dtype < 0 || w_dtype > 2) return fail(PQ_ERR_BAD_ARG, "%s: unknown w_dtype %d", what, w_dtype);
    if (kind != PQ_ROUTER_SOFTMAX_TOPK && kind != PQ_ROUTER_TOPK_SOFTMAX)
        return fail(PQ_ERR_BAD_ARG, "%s: unknown kind %d (0 = softmax_topk, 1 = topk_softmax)", what, kind);
    if (renormalise != 0 && renormalise != 1) return fail(PQ_ERR_BAD_ARG, "%s: renormalise = %d (0 or 1)", what, renormalise);
    if (ids_are_int64 != 0 && ids_are_int64 != 1) return fail(PQ_ERR_BAD_ARG, "%s: ids_are_int64 = %d (0 = int32 ids, 1 = int64 ids)", what, ids_are_int64);
    if (const int32_t st = moe_dims_check(what, T, k, E, true)) return st;
    if (k > E) return fail(PQ_ERR_BAD_ARG, "%s: k = %d > E = %d", what, k, E);
    if (ld_logits < E) return fail(PQ_ERR_BAD_ARG, "%s: ld_logits = %lld < E = %d", what, (long long)ld_logits, E);
    if (ld_w < k) return fail(PQ_ERR_BAD_ARG, "%s: ld_w = %lld < k = %d", what, (long long)ld_w, k);
    if (ld_ids < k) return fail(PQ_ERR_BAD_ARG, "%s: ld_ids = %lld < k = %d", what, (long long)ld_ids, k);
    if (T == 0) return PQ_OK;
    if (!logits || !weights || !ids) return fail(PQ_ERR_BAD_ARG, "%s: %s is null", what, !logits ? "logits" : (!weights ? "weights" : "ids"));
    const int64_t eb = dtype_bytes(dtype), wb = dtype_bytes(w_dtype), ib = ids_are_int64 ? 8 : 4;
    if ((reinterpret_cast<uintptr_t>(logits) & (uintptr_t)(eb - 1)) != 0) return fail(PQ_ERR_BAD_ALIGN, "%s: logits is not aligned to its element size", what);
    if ((reinterpret_cast<uintptr_t>(weights) & (uintptr_t)(wb - 1)) != 0) return fail(PQ_ERR_BAD_ALIGN, "%s: weights is not aligned to its element size", what);
    if ((reinterpret_cast<uintptr_t>(ids) & (uintptr_t)(ib - 1)) != 0) return fail(PQ_ERR_BAD_ALIGN, "%s: ids is not aligned to its element size", what);
    {
        const NamedExtent ops[] = {{"logits", extent_of(logits, ld_logits, T, E, eb), false}, {"weights", extent_of(weights, ld_w, T, k, wb), true},
                                   {"ids", extent_of(ids, ld_ids, T, k, ib), true}};
        if (const int32_t rc = check_disjoint(what, ops, 3)) return rc;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto dt) { pq::moe_topk_dispatch<dt>(logits, ld_logits, T, E, k, kind, renormalise, weights, w_dtype, ld_w, ids, ids_are_int64 != 0, ld_ids, st); });
    return check_launch(what);
}

// ---- one-call dynamic qlinear: K1 (x -> xq, xs in the workspace) then pq_qlinear_s8 (with split-K slabs if planned).

size_t pq_qlinear_dyn_workspace_bytes(int64_t M, int64_t N, int64_t K) {
    CallScope scope_;
    if (M <= 0 || N <= 0 || K < 0) return 0;      // (M == 0 or N == 0: pq_qlinear_dyn returns before it looks at the workspace; K == 0 still writes the M row scales)
    return align256((size_t)M * (size_t)K) + align256((size_t)M * sizeof(float)) + pq_qlinear_workspace_bytes(M, N, K);
}

int32_t pq_qlinear_dyn(const void* x, int32_t dtype, int64_t ld_x, const int8_t* w, int64_t ldw, const float* w_scale,
                       const void* bias, void* y, int64_t ldy, int64_t M, int64_t N, int64_t K, void* workspace,
                       size_t workspace_bytes, void* stream) {
    CallScope scope_;           // K1 and the GEMM of this call plan and launch under ONE snapshot
    if (const int32_t rc = check_dtype("pq_qlinear_dyn", dtype)) return rc;
    if (M < 0 || N < 0 || K < 0) return fail(PQ_ERR_BAD_ARG, "pq_qlinear_dyn: negative size");
    // (before the workspace check and before K1 launches: K1 would name itself for ld_x, and would already have run when pq_qlinear_s8 refused ldw or ldy)
    if (bad_mat(x, M, K, ld_x) || bad_mat(w, N, K, ldw) || bad_mat(y, M, N, ldy) || (N > 0 && !w_scale))
        return fail(PQ_ERR_BAD_ARG, "pq_qlinear_dyn: bad arguments (M=%lld N=%lld K=%lld ld_x=%lld ldw=%lld ldy=%lld)", (long long)M, (long long)N, (long long)K, (long long)ld_x, (long long)ldw, (long long)ldy);
    if (M == 0 || N == 0) return PQ_OK;
    if (const int32_t rc = check_workspace("pq_qlinear_dyn", workspace, workspace_bytes, pq_qlinear_dyn_workspace_bytes(M, N, K), 256)) return rc;
    uint8_t* base = static_cast<uint8_t*>(workspace);
    int8_t* xq = reinterpret_cast<int8_t*>(base);
    float* xs = reinterpret_cast<float*>(base + align256((size_t)M * (size_t)K));
    uint8_t* slabs = base + align256((size_t)M * (size_t)K) + align256((size_t)M * sizeof(float));
    const size_t slab_bytes = pq_qlinear_workspace_bytes(M, N, K);
    int32_t st = pq_quant_rowwise(x, dtype, M, K, ld_x, xq, K, xs, stream);
    if (st != PQ_OK) return st;
    return pq_qlinear_s8(xq, K, xs, w, ldw, w_scale, bias, y, ldy, dtype, M, N, K, slab_bytes ? slabs : nullptr, slab_bytes, stream);
}

int32_t pq_selftest_fast_quotient(const uint32_t* x_bits, const uint32_t* s_bits, int64_t n, unsigned long long* mismatches, void* stream) {
    if (!x_bits || !s_bits || !mismatches || n < 0) return fail(PQ_ERR_BAD_ARG, "pq_selftest_fast_quotient: bad arguments");
    pq::launch_fast_quotient_check(x_bits, s_bits, n, mismatches, static_cast<hipStream_t>(stream));
    return check_launch("pq_selftest_fast_quotient");
}

int32_t pq_selftest_half_encode(int32_t dtype, unsigned long long* counts, void* stream) {
    if (!counts || (dtype != PQ_BF16 && dtype != PQ_FP16)) return fail(PQ_ERR_BAD_ARG, "pq_selftest_half_encode: dtype must be bf16 or fp16, counts non-null");
    pq::launch_half_encode_check(dtype, counts, static_cast<hipStream_t>(stream));
    return check_launch("pq_selftest_half_encode");
}

int32_t pq_selftest_silu_short(int32_t dtype, unsigned long long* counts, void* stream) {
    if (!counts || (dtype != PQ_BF16 && dtype != PQ_FP16)) return fail(PQ_ERR_BAD_ARG, "pq_selftest_silu_short: dtype must be bf16 or fp16, counts non-null");
    pq::launch_silu_short_check(dtype, counts, static_cast<hipStream_t>(stream));
    return check_launch("pq_selftest_silu_short");
}

int32_t pq_selftest_glu_short(int32_t dtype, int32_t kind, float limit, float alpha, unsigned long long* counts, void* stream) {
    if (!counts || (dtype != PQ_BF16 && dtype != PQ_FP16)) return fail(PQ_ERR_BAD_ARG, "pq_selftest_glu_short: dtype must be bf16 or fp16, counts non-null");
    if (const char* why = glu_bad_params(dtype, kind, limit, alpha)) return fail(PQ_ERR_BAD_ARG, "pq_selftest_glu_short: %s", why);
    pq::launch_glu_short_check(dtype, kind, limit, alpha, counts, static_cast<hipStream_t>(stream));
    return check_launch("pq_selftest_glu_short");
}

#ifdef PQ_ABLATION_BUILD
void pq_dev_set_stamp_buffer(unsigned long long* p) { pq::set_stamp_buffer(p); }
#endif

const char* pq_gemm_variant_name(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb) {
    CallScope scope_;
    return gemm_variant_name(M, N, K, lda, ldb);
}

}  // extern "C"
