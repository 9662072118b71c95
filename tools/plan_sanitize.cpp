// Stand-alone AddressSanitizer / UBSan check of the sparse power-flow plan builder (csrc/powerflow_plan.cpp): its own main, linked
// against the builder's translation unit alone (tools/plan_sanitize.sh), no GPU and no Python.  Random trees plus chords with
// parallel lines and self-pairs at several sizes, both modes and the fast-decoupled plan, an exact-size and a too-small buffer, and
// the error paths.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/pfn_hip.h"

namespace pfn {
static char g_error[512];
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}
}  // namespace pfn

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t next_u32() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "plan_sanitize: %s failed (line %d): %s\n", #cond, __LINE__, pfn::g_error); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main() {
    const int sizes[][2] = {{2, 1}, {5, 6}, {14, 20}, {118, 186}, {1100, 1530}, {3000, 4200}};
    for (const auto& sz : sizes) {
        const int n = sz[0], e = sz[1];
        std::vector<int64_t> ei(2 * (size_t)e);
        for (int k = 0; k < e; ++k) {
            int a, b;
            if (k < n - 1) { a = k + 1; b = (int)(next_u32() % (uint32_t)(k + 1)); }          // a random tree first
            else { a = (int)(next_u32() % (uint32_t)n); b = (int)(next_u32() % (uint32_t)n); }   // chords: repeats and self-pairs occur
            ei[k] = a;
            ei[e + k] = b;
        }
        std::vector<int32_t> bt(n);
        for (int i = 0; i < n; ++i) bt[i] = i == 0 ? 0 : (i % 3 == 0 ? 1 : 2);
        for (int mode = 0; mode < 2; ++mode) {
            const size_t need = pfn_powerflow_sparse_plan_bytes(ei.data(), e, bt.data(), n, mode);
            CHECK(need > 0);
            std::vector<unsigned char> blob(need), again(need);                                  // exact size: an overrun is an ASan report
            CHECK(pfn_powerflow_sparse_plan(ei.data(), e, bt.data(), n, mode, blob.data(), need) == PFN_OK);
            CHECK(pfn_powerflow_sparse_plan(ei.data(), e, bt.data(), n, mode, again.data(), need) == PFN_OK);
            CHECK(blob == again);
            CHECK(pfn_powerflow_sparse_plan(ei.data(), e, bt.data(), n, mode, blob.data(), need - 1) == PFN_EINVAL);
            printf("n %d e %d mode %d: plan of %zu bytes\n", n, e, mode, need);
        }
        {                                                                                         // the fast-decoupled plan: two sub-plans in one blob
            const size_t need = pfn_powerflow_sparse_fd_plan_bytes(ei.data(), e, bt.data(), n);
            CHECK(need > 0);
            std::vector<unsigned char> blob(need), again(need);
            CHECK(pfn_powerflow_sparse_fd_plan(ei.data(), e, bt.data(), n, blob.data(), need) == PFN_OK);
            CHECK(pfn_powerflow_sparse_fd_plan(ei.data(), e, bt.data(), n, again.data(), need) == PFN_OK);
            CHECK(blob == again);
            CHECK(pfn_powerflow_sparse_fd_plan(ei.data(), e, bt.data(), n, blob.data(), need - 1) == PFN_EINVAL);
            std::vector<int32_t> no_pq(bt);                                                       // an empty Q half
            for (int i = 1; i < n; ++i) no_pq[i] = 1;
            const size_t need0 = pfn_powerflow_sparse_fd_plan_bytes(ei.data(), e, no_pq.data(), n);
            CHECK(need0 > 0 && need0 <= need);
            std::vector<unsigned char> blob0(need0);
            CHECK(pfn_powerflow_sparse_fd_plan(ei.data(), e, no_pq.data(), n, blob0.data(), need0) == PFN_OK);
            printf("n %d e %d fd: plan of %zu bytes (%zu without a PQ bus)\n", n, e, need, need0);
        }
        for (int mode = 0; mode < 3; ++mode) {                                                    // the single-call entry: 2 is the fast-decoupled plan
            const size_t need = mode == 2 ? pfn_powerflow_sparse_fd_plan_bytes(ei.data(), e, bt.data(), n)
                                          : pfn_powerflow_sparse_plan_bytes(ei.data(), e, bt.data(), n, mode);
            std::vector<unsigned char> want(need), blob(need);                                    // exact size: an overrun is an ASan report
            CHECK((mode == 2 ? pfn_powerflow_sparse_fd_plan(ei.data(), e, bt.data(), n, want.data(), need)
                             : pfn_powerflow_sparse_plan(ei.data(), e, bt.data(), n, mode, want.data(), need)) == PFN_OK);
            size_t needed = 0;
            CHECK(pfn_powerflow_sparse_plan_into(ei.data(), e, bt.data(), n, mode, blob.data(), need, &needed) == PFN_OK && needed == need);
            CHECK(blob == want);
            const size_t small[] = {0, 1, 127, 128, 129, need / 2, need - 16, need - 1};          // every way of being too small
            for (size_t room : small) {
                if (room >= need) continue;
                std::vector<unsigned char> tight(room ? room : 1);
                CHECK(pfn_powerflow_sparse_plan_into(ei.data(), e, bt.data(), n, mode, room ? tight.data() : nullptr, room, &needed) == PFN_ENOSPACE);
                CHECK(needed == need);
            }
            std::vector<unsigned char> roomy(need + 64, 0xAB);
            CHECK(pfn_powerflow_sparse_plan_into(ei.data(), e, bt.data(), n, mode, roomy.data(), roomy.size(), &needed) == PFN_OK && needed == need);
            CHECK(std::vector<unsigned char>(roomy.begin(), roomy.begin() + (long)need) == want && roomy[need] == 0xAB && roomy[need + 63] == 0xAB);
        }
        if (e > 0) {
            std::vector<unsigned char> blob(1 << 16);
            ei[e - 1] = n;
            CHECK(pfn_powerflow_sparse_fd_plan(ei.data(), e, bt.data(), n, blob.data(), blob.size()) == PFN_EINVAL);
            CHECK(pfn_powerflow_sparse_fd_plan_bytes(ei.data(), e, bt.data(), n) == 0);
            ei[e - 1] = n;
            CHECK(pfn_powerflow_sparse_plan(ei.data(), e, bt.data(), n, 0, blob.data(), blob.size()) == PFN_EINVAL);
            ei[e - 1] = -1;
            CHECK(pfn_powerflow_sparse_plan_bytes(ei.data(), e, bt.data(), n, 0) == 0);
            ei[e - 1] = 0;
            bt[n - 1] = 3;
            CHECK(pfn_powerflow_sparse_plan(ei.data(), e, bt.data(), n, 0, blob.data(), blob.size()) == PFN_EINVAL);
            bt[n - 1] = 0;
            CHECK(pfn_powerflow_sparse_plan(ei.data(), e, bt.data(), n, 0, blob.data(), blob.size()) == PFN_EINVAL);
        }
    }
    printf("plan_sanitize: ok\n");
    return 0;
}
