// Per-sample topologies on the sparse power-flow routes (gfx950): pfn_powerflow_cover_map, ONE launch, one workgroup per sample, in
// front of pfn_powerflow_solve_sparse_masked / _fd_masked.  A chunk of samples shares ONE plan, built on a COVER list: a line list
// that holds every line of every sample (utils/powerflow.py cover_plan).  This kernel tells the solver which cover lines a sample
// has -- line_mask -- and lays the sample's line parameters out in cover order -- rx_cover.
//
// THE SLOT RULE (a pure function of the two lists; tests/test_powerflow_cover_host.py restates it in numpy).  A line's key is its
// unordered bus pair, min * n_bus + max.  Sample s's k-th line with key q, in the sample's stored order, takes the k-th cover slot
// with key q, in cover order; a line without such a slot is unplaced, and so is a line that names a bus outside [0, n_bus) or one
// bus twice.  The cover comes as its keys sorted ascending (ties in cover order) with the cover slot of every sorted position, so
// the slot is a binary search and, only where the cover holds the key more than once (parallel lines: rare), the line's rank among
// the sample's own earlier lines of that key -- counted from the sample's keys, held in LDS as far as they fit and formed again
// from the list beyond.  No atomics: lines with different keys land in different runs of the table and counted ranks differ; where
// the shortcut's rank 0 sends two lines of a sample to one place (the sample holds a key twice, the cover once) a claim-and-read-
// back round finds it and those lines count their rank after all, so the result is the rule's on every run.
//
// Every id is tested before it indexes anything; the search never leaves [0, e_cover) whatever the table holds, and a slot number
// outside [0, e_cover) counts as unplaced.
#include "pfn_internal.hpp"

namespace pfn {

struct PcArgs {
    const int64_t* edge_index;                      // [S, 2, e]
    const double* rx;                               // [S, e, 2]
    const int64_t* keys;                            // [e_cover] ascending
    const int32_t* slot;                            // [e_cover]: the cover slot of sorted position i
    uint8_t* line_mask;                             // [S, e_cover]
    double* rx_cover;                               // [S, e_cover, 2]
    int32_t* unplaced;                              // [S]
    int n, e, e_cover, lds_keys;                    // lds_keys: the sample's first keys kept in LDS
};

constexpr int PC_THREADS = 256;

__device__ __forceinline__ int64_t pc_key(const int64_t* ei, int e, int j, int n) {
    const int64_t a = ei[j], b = ei[e + j];
    if ((uint64_t)a >= (uint64_t)n || (uint64_t)b >= (uint64_t)n || a == b) return -1;
    return (a < b ? a : b) * (int64_t)n + (a < b ? b : a);
}

__global__ __launch_bounds__(PC_THREADS) void powerflow_cover_map_kernel(const PcArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pc_smem[];
    __shared__ int s_bad[PC_THREADS / 64];
    int64_t* lkey = reinterpret_cast<int64_t*>(pc_smem);
    const int t = threadIdx.x, s = blockIdx.x;
    const int e = a.e, ec = a.e_cover;
    const int64_t* ei = a.edge_index + (int64_t)s * 2 * e;
    const double2* rx = reinterpret_cast<const double2*>(a.rx) + (int64_t)s * e;
    uint8_t* mask = a.line_mask + (int64_t)s * ec;
    double2* out = reinterpret_cast<double2*>(a.rx_cover) + (int64_t)s * ec;

    for (int j = t; j < a.lds_keys; j += PC_THREADS) lkey[j] = pc_key(ei, e, j, a.n);
    for (int k = t; k < ec; k += PC_THREADS) mask[k] = 0;
    __syncthreads();

    auto key_of = [&](int j) { return j < a.lds_keys ? lkey[j] : pc_key(ei, e, j, a.n); };
    // line j's place by the slot rule, or -1.  counted: the rank is counted whatever the cover holds; else only where the cover
    // holds the key more than once, and a key it holds once gets rank 0 -- right unless the SAMPLE holds that key twice (below)
    auto place_of = [&](int j, bool counted) {
        const int64_t q = key_of(j);
        if (q < 0) return -1;
        int lo = 0, hi = ec;                        // the first sorted position whose key is not below q
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (a.keys[mid] < q) lo = mid + 1; else hi = mid;
        }
        if (lo >= ec || a.keys[lo] != q) return -1;
        int rank = 0;
        if (counted || (lo + 1 < ec && a.keys[lo + 1] == q))
            for (int i = 0; i < j; ++i) rank += key_of(i) == q;
        if (lo + rank >= ec || a.keys[lo + rank] != q) return -1;
        const int place = a.slot[lo + rank];
        return (unsigned)place < (unsigned)ec ? place : -1;
    };
    // ---- a sample that holds a key more often than the shortcut assumed sends two lines to one place.  Found without atomics: every
    // line writes its number into the first word of its place's rx pair (a place that is claimed ends up used, so nothing is written
    // that does not get its rx below), reads it back behind a barrier, and a line that finds another number marks the place (mask
    // 2).  Every line of a marked place then counts its rank after all: the first keeps the place, the others are unplaced -- the
    // rule, whichever claim landed last.
    for (int j = t; j < e; j += PC_THREADS) {
        const int place = place_of(j, false);
        if (place >= 0) *reinterpret_cast<int32_t*>(out + place) = j;
    }
    __syncthreads();
    for (int j = t; j < e; j += PC_THREADS) {
        const int place = place_of(j, false);
        if (place >= 0 && *reinterpret_cast<const int32_t*>(out + place) != j) mask[place] = 2;
    }
    __syncthreads();
    int bad = 0;
    for (int j = t; j < e; j += PC_THREADS) {
        int place = place_of(j, false);
        const bool marked = place >= 0 && mask[place] == 2;     // (a marked place keeps its 2 through this loop: its readers read 2)
        if (marked) place = place_of(j, true);
        if (place >= 0) {
            out[place] = rx[j];
            if (!marked) mask[place] = 1;
        } else {
            ++bad;
        }
    }
    __syncthreads();
    for (int k = t; k < ec; k += PC_THREADS)
        if (mask[k] == 2) mask[k] = 1;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_xor(bad, off);
    if ((t & 63) == 0) s_bad[t >> 6] = bad;
    __syncthreads();
    if (t == 0) {
        int sum = 0;
        for (int w = 0; w < PC_THREADS / 64; ++w) sum += s_bad[w];
        a.unplaced[s] = sum;
    }
}

}  // namespace pfn

using namespace pfn;

extern "C" {

int pfn_powerflow_cover_map(const int64_t* edge_index, int64_t n_lines, const double* rx, int64_t n_samples, int64_t n_bus,
                            const int64_t* cover_keys, const int32_t* cover_slot, int64_t n_cover, uint8_t* line_mask, double* rx_cover,
                            int32_t* unplaced, void* stream) {
    const char* who = "pfn_powerflow_cover_map";
    PFN_CHECK_ARG(n_samples >= 0 && n_samples < (1ll << 29), "%s: bad sample count %lld", who, (long long)n_samples);
    PFN_CHECK_ARG(n_bus >= 1 && n_bus < (1ll << 31) && n_lines >= 0 && n_lines < (1ll << 30) && n_cover >= 0 && n_cover < (1ll << 30),
                  "%s: bad sizes: %lld buses, %lld lines, %lld cover lines", who, (long long)n_bus, (long long)n_lines, (long long)n_cover);
    if (n_samples == 0) return PFN_OK;
    PFN_CHECK_ARG((edge_index && rx) || n_lines == 0, "%s: null edge_index or rx", who);
    PFN_CHECK_ARG((cover_keys && cover_slot && line_mask && rx_cover) || n_cover == 0, "%s: null cover table or output", who);
    PFN_CHECK_ARG(unplaced, "%s: null unplaced", who);
    PFN_CHECK_ARG(((reinterpret_cast<uintptr_t>(rx) | reinterpret_cast<uintptr_t>(rx_cover)) & 15) == 0 &&
                      ((reinterpret_cast<uintptr_t>(edge_index) | reinterpret_cast<uintptr_t>(cover_keys)) & 7) == 0 &&
                      ((reinterpret_cast<uintptr_t>(cover_slot) | reinterpret_cast<uintptr_t>(unplaced)) & 3) == 0,
                  "%s: rx and rx_cover must be 16-byte aligned, edge_index and cover_keys 8-byte, cover_slot and unplaced 4-byte", who);
    static std::atomic<uint64_t> raised{0};
    const int budget = kLdsCuBytes - kLdsReserve;
    PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(powerflow_cover_map_kernel), budget, raised));
    const int lds_keys = (int)std::min<int64_t>(n_lines, budget / 8);
    const PcArgs a{edge_index, rx, cover_keys, cover_slot, line_mask, rx_cover, unplaced, (int)n_bus, (int)n_lines, (int)n_cover, lds_keys};
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope ps("powerflow_cover_map", (double)n_samples * ((double)n_lines * 48.0 + (double)n_cover) + (double)n_cover * 12.0, 0.0, s);
    powerflow_cover_map_kernel<<<(int)n_samples, PC_THREADS, (size_t)lds_keys * 8, s>>>(a);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

}  // extern "C"
