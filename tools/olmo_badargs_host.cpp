// Dev tool (no GPU needed): the argument checks of pq_olmo_postnorm_add_quant_rowwise as a stand-alone host program, for a sanitizer build of pq_api.hip.  Every case
// returns before the first HIP call, so the program runs on a machine without a GPU.  Build pq_api.hip and this file with the host sanitizers and link them with the
// library's other objects (from protoquant_amd/csrc, after `make`):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=off -Xarch_host -fsanitize=address,undefined -c pq_api.hip -o /tmp/pq_api_san.o
//   hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I../../include -c ../../tools/olmo_badargs_host.cpp -o /tmp/olmo_badargs.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o /tmp/olmo_badargs /tmp/olmo_badargs.o /tmp/pq_api_san.o $(ls build/*.o | grep -v -e pq_api.o -e pq_rccl.o) -ldl
//   /tmp/olmo_badargs          # prints one line per case and "N cases, 0 failed"; a sanitizer report ends it with a non-zero status
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "pq_hip.h"

namespace {
struct Args {
    const void* x = reinterpret_cast<const void*>(0x10000);
    int64_t ldx = 128;
    const void* pw = reinterpret_cast<const void*>(0x80000);
    float post_eps = 1e-6f;
    const void* r = reinterpret_cast<const void*>(0x20000);
    int64_t ldr = 128;
    void* s = reinterpret_cast<void*>(0x30000);
    int64_t lds = 128;
    int32_t dtype = 0;
    int64_t rows = 4, cols = 128;
    int8_t* q = reinterpret_cast<int8_t*>(0x50000);
    int64_t ldq = 128;
    float* scale = reinterpret_cast<float*>(0x60000);
};
int32_t call(const Args& a) {
    return pq_olmo_postnorm_add_quant_rowwise(a.x, a.ldx, a.pw, a.post_eps, a.r, a.ldr, a.s, a.lds, a.dtype, a.rows, a.cols, a.q, a.ldq, a.scale, nullptr);
}
Args add_only() { Args a; a.q = nullptr; a.scale = nullptr; return a; }
Args norm_only() { Args a = add_only(); a.r = nullptr; a.ldr = 0; return a; }
template <class T> T* at(uintptr_t v) { return reinterpret_cast<T*>(v); }

int n_cases = 0, n_failed = 0;
void expect(const char* what, const Args& a, int32_t want, const char* named) {
    const int32_t rc = call(a);
    const char* err = pq_last_error();
    const bool ok = rc == want && (want == 0 || (strstr(err, "pq_olmo_postnorm_add_quant_rowwise") && strstr(err, named)));
    ++n_cases;
    if (!ok) ++n_failed;
    printf("%-4s %-44s rc=%d %s\n", ok ? "ok" : "FAIL", what, rc, want ? err : "");
}
}  // namespace

int main() {
    const int64_t ROW = 256, BIG = int64_t(1) << 24;
    for (int form = 0; form < 3; ++form) {
        const Args base = form == 0 ? Args() : form == 1 ? add_only() : norm_only();
        const char* tag = form == 0 ? "K1oq" : form == 1 ? "K1oa" : "K1on";
        char what[96];
        auto name = [&](const char* s) { snprintf(what, sizeof(what), "%s: %s", tag, s); return what; };
        Args a = base; a.x = nullptr; expect(name("null x"), a, 1, "x is null");
        a = base; a.pw = nullptr; expect(name("null post_weight"), a, 1, "post_weight is null");
        a = base; a.s = nullptr; expect(name("null sum_out"), a, 1, "sum_out is null");
        a = base; a.ldx = 64; expect(name("ld_x < cols"), a, 1, "ld_x");
        a = base; a.lds = 127; expect(name("ld_s < cols"), a, 1, "ld_s");
        a = base; a.post_eps = -1e-6f; expect(name("negative post_eps"), a, 1, "post_eps");
        a = base; a.post_eps = NAN; expect(name("NaN post_eps"), a, 1, "post_eps");
        a = base; a.post_eps = INFINITY; expect(name("infinite post_eps"), a, 1, "post_eps");
        a = base; a.dtype = 3; expect(name("unknown dtype 3"), a, 1, "dtype");
        a = base; a.dtype = -1; expect(name("unknown dtype -1"), a, 1, "dtype");
        a = base; a.rows = -1; expect(name("negative rows"), a, 1, "rows");
        a = base; a.cols = -1; expect(name("negative cols"), a, 1, "cols");
        a = base; a.cols = a.ldx = a.ldr = a.lds = a.ldq = BIG; expect(name("cols = 2^24"), a, 1, "cols");
        a = base; a.s = at<void>(0x10000 + 16); expect(name("sum_out 16 bytes into x"), a, 1, "sum_out overlaps x");
        a = base; a.s = at<void>(0x10000 - ROW); expect(name("sum_out one row before x"), a, 1, "sum_out overlaps x");
        a = base; a.s = at<void>(0x10000); a.lds = 256; expect(name("sum_out at x, another pitch"), a, 1, "sum_out overlaps x");
        a = base; a.s = at<void>(0x80000); expect(name("sum_out at post_weight"), a, 1, "sum_out overlaps post_weight");
        a = base; a.rows = 0; expect(name("rows = 0"), a, 0, "");
        a = base; a.cols = 0; a.ldx = a.ldr = a.lds = a.ldq = 0; expect(name("cols = 0"), a, 0, "");
        a = base; a.rows = 0; a.x = a.pw = nullptr; a.s = nullptr; expect(name("rows = 0, null operands"), a, 0, "");
        if (form < 2) {
            a = base; a.ldr = 64; expect(name("ld_r < cols"), a, 1, "ld_r");
            a = base; a.s = at<void>(0x20000 + 2 * ROW); expect(name("sum_out two rows into residual"), a, 1, "sum_out overlaps residual");
            a = base; a.s = at<void>(0x20000); a.lds = 256; expect(name("sum_out at residual, another pitch"), a, 1, "sum_out overlaps residual");
        }
        if (form == 0) {
            a = base; a.q = nullptr; expect(name("q null, scale given"), a, 1, "q is null");
            a = base; a.scale = nullptr; expect(name("scale null, q given"), a, 1, "scale is null");
            a = base; a.r = nullptr; expect(name("q without residual"), a, 1, "residual is null");
            a = base; a.r = nullptr; a.scale = nullptr; expect(name("q alone"), a, 1, "residual is null");
            a = base; a.ldq = 64; expect(name("ld_q < cols"), a, 1, "ld_q");
            a = base; a.q = at<int8_t>(0x10000); expect(name("q at x"), a, 1, "q overlaps x");
            a = base; a.q = at<int8_t>(0x80000 + 8); expect(name("q in post_weight"), a, 1, "q overlaps post_weight");
            a = base; a.q = at<int8_t>(0x20000 + 100); expect(name("q in residual"), a, 1, "q overlaps residual");
            a = base; a.q = at<int8_t>(0x30000 + 64); expect(name("q in sum_out"), a, 1, "q overlaps sum_out");
            a = base; a.scale = at<float>(0x30000); expect(name("scale at sum_out"), a, 1, "scale overlaps sum_out");
            a = base; a.scale = at<float>(0x80000 + 4); expect(name("scale in post_weight"), a, 1, "scale overlaps post_weight");
            a = base; a.scale = at<float>(0x50000 + 128); expect(name("scale in q"), a, 1, "q overlaps scale");
        }
    }
    printf("%d cases, %d failed\n", n_cases, n_failed);
    return n_failed ? 1 : 0;
}
