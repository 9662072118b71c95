// Per-bus error analysis on the device (gfx950): WHERE an evaluation split's error is, which pfn_eval_metrics' 31 scalars cannot say.
// pfn_bus_errors_accumulate turns the rows (out, y, pred_mask) of one uniform batch into the de-normalised error and prediction of
// every bus of every sample (written to the sample's row of an [S, n, 4] table) and into running moments per (bus, feature, mask
// group); pfn_bus_errors_histogram bins a finished table per (bus, feature) by np.histogram's rule for explicit edges.  Both are
// pure functions of their inputs: one owner per (bus, feature), a fixed combine order, integer LDS atomics only.
#include <algorithm>

#include "pfn_internal.hpp"
#include "reduce.hpp"

namespace pfn {

// ------------------------------------------------------------------------------------------------- accumulate
// The moments engine of reduce.hpp with a bus as the owner: slice s walks the graphs s, s + MO_SLICES, ..., keeps the 48 moments of
// its bus -- 4 features x {mask != 0, mask == 0} -- in registers and hands them over one feature per round.  6470 buses x 64 graphs:
// 405 workgroups, 4 graphs per thread; 118 x 128: 8 workgroups, 8 graphs per thread in two trips of MO_UNROLL.
struct BusErrScale {
    float std[4], mean[4];
};

// the four "mask != 0" bits of a mask row
__device__ __forceinline__ unsigned be_mask_bits(const void* m, int dtype, int64_t r) {
    if (dtype == 0) {
        const longlong2* p = reinterpret_cast<const longlong2*>(static_cast<const int64_t*>(m) + 4 * r);
        const longlong2 a = p[0], b = p[1];
        return (a.x != 0 ? 1u : 0u) | (a.y != 0 ? 2u : 0u) | (b.x != 0 ? 4u : 0u) | (b.y != 0 ? 8u : 0u);
    }
    const float4 v = ld4(static_cast<const float*>(m) + 4 * r);
    return (v.x != 0.f ? 1u : 0u) | (v.y != 0.f ? 2u : 0u) | (v.z != 0.f ? 4u : 0u) | (v.w != 0.f ? 8u : 0u);
}

// (out - y) * std, every operation rounded on its own, as `denorm` -- the expression of pfn_eval_metrics' de-normalised terms
__device__ __forceinline__ float be_error(float o, float y, float sd) {
#pragma clang fp contract(off)
    const float d = o - y;
    return d * sd;
}

__global__ __launch_bounds__(MO_THREADS) void bus_errors_accumulate_kernel(
    const float* __restrict__ o, const float* __restrict__ y, const void* __restrict__ mask, int mask_dtype, int n_graphs, int n_bus,
    BusErrScale sc, const int64_t* __restrict__ sample_idx, int64_t table_rows, float* __restrict__ err_table,
    float* __restrict__ pred_table, double* __restrict__ moments, int32_t* __restrict__ flags) {
    const int t = threadIdx.x, bl = t & (MO_OWNERS - 1), sl = t / MO_OWNERS;
    const int bus = blockIdx.x * MO_OWNERS + bl;
    const bool live = bus < n_bus;
    Moments6 mo[4][2];                              // [feature][group 0: mask != 0 (predicted), group 1: mask == 0 (given)]
    bool bad_seen = false;
    for (int g0 = sl; g0 < n_graphs; g0 += MO_UNROLL * MO_SLICES) {
        float4 vo[MO_UNROLL], vy[MO_UNROLL];
        unsigned mb[MO_UNROLL];
        int64_t row[MO_UNROLL];
        bool on[MO_UNROLL];
#pragma unroll
        for (int u = 0; u < MO_UNROLL; ++u) {      // every load of the trip is requested before the first row is consumed
            const int g = g0 + u * MO_SLICES;
            on[u] = live && g < n_graphs;
            row[u] = 0;
            vo[u] = vy[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            mb[u] = 0;
            if (on[u]) {
                const int64_t si = sample_idx ? sample_idx[g] : (int64_t)g;
                if (sample_idx && (si < 0 || si >= table_rows)) {      // skipped entirely: tables and moments
                    on[u] = false;
                    bad_seen = true;
                } else {
                    const int64_t r = (int64_t)g * n_bus + bus;
                    row[u] = si * n_bus + bus;
                    vo[u] = ld4(o + 4 * r);
                    vy[u] = ld4(y + 4 * r);
                    mb[u] = be_mask_bits(mask, mask_dtype, r);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < MO_UNROLL; ++u) {
            if (!on[u]) continue;
            const float ov[4] = {vo[u].x, vo[u].y, vo[u].z, vo[u].w}, yv[4] = {vy[u].x, vy[u].y, vy[u].z, vy[u].w};
            float ev[4], pv[4];
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                ev[f] = be_error(ov[f], yv[f], sc.std[f]);
                pv[f] = denorm(ov[f], sc.std[f], sc.mean[f]);
            }
            if (err_table) st4(err_table + 4 * row[u], make_float4(ev[0], ev[1], ev[2], ev[3]));
            if (pred_table) st4(pred_table + 4 * row[u], make_float4(pv[0], pv[1], pv[2], pv[3]));
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const double e = (double)ev[f];
                const bool p = (mb[u] >> f) & 1u;
#pragma unroll
                for (int g = 0; g < 2; ++g) mo[f][g].add_if((g == 0) == p, e);
            }
        }
    }
    if (bad_seen && bl == 0) flags[0] = flags[0] | 1;    // (every writer stores the same bit over the same word)
#pragma unroll
    for (int f = 0; f < 4; ++f) moments_round(mo[f][0], mo[f][1], f, n_bus, 48, moments);      // one feature per round
}

// -------------------------------------------------------------------------------------------------- histogram
// A workgroup owns a tile of `tile` (a power of two <= 32) consecutive buses x 4 features: its nbins counters and its three
// "outside" counters per (bus, feature) live in LDS next to the four edge arrays (float64), it streams the samples -- the tile's
// 16 * tile contiguous bytes of a sample are one coalesced read of `tile` lanes -- and counts with integer LDS atomics, which are
// order-free; then it writes its slab of `hist` / `outside`.  No global atomics.
constexpr int BH_THREADS = 256, BH_UNROLL = 4, BH_MAX_TILE = 32, BH_MAX_BINS = 2048;

__host__ __device__ inline size_t bh_lds_bytes(int tile, int nbins) {
    return (size_t)4 * (nbins + 1) * sizeof(double) + (size_t)tile * 4 * (nbins + 3) * sizeof(uint32_t);
}
// The largest tile that leaves room for a second workgroup on the CU (latency hiding comes from the neighbour: a workgroup's own
// loop is load -> compare -> LDS atomic), else the largest that fits at all.  300 bins: 8 buses (48.4 KB with the 9.6 KB of edges:
// three workgroups per CU; 16 buses + edges = 87.2 KB would be alone on its CU); 2048 bins: 2 buses (131 KB).
static int bh_tile(int nbins) {
    for (int budget : {kLdsCuBytes / 2, kLdsCuBytes - kLdsReserve})
        for (int tile = BH_MAX_TILE; tile >= 1; tile >>= 1)
            if ((int64_t)bh_lds_bytes(tile, nbins) <= budget) return tile;
    return 0;
}

__global__ __launch_bounds__(BH_THREADS) void bus_errors_histogram_kernel(const float* __restrict__ table, int n_samples, int n_bus,
                                                                          const float* __restrict__ scale,
                                                                          const double* __restrict__ edges, int nbins, int tile,
                                                                          uint32_t* __restrict__ hist, uint32_t* __restrict__ outside) {
    extern __shared__ __attribute__((aligned(16))) double bh_lds[];
    double* ed = bh_lds;                                                   // [4][nbins + 1]
    uint32_t* cnt = reinterpret_cast<uint32_t*>(ed + 4 * (nbins + 1));     // [tile][4][nbins]
    uint32_t* out3 = cnt + tile * 4 * nbins;                               // [tile][4][3]: below, above, NaN
    const int t = threadIdx.x;
    const int b0 = blockIdx.x * tile, tb = min(tile, n_bus - b0);
    for (int i = t; i < 4 * (nbins + 1); i += BH_THREADS) ed[i] = edges[i];
    for (int i = t; i < tile * 4 * (nbins + 3); i += BH_THREADS) cnt[i] = 0u;      // (cnt and out3 are adjacent)
    __syncthreads();
    const int bl = t & (tile - 1), sl = t / tile, ss = BH_THREADS / tile;
    const bool live = bl < tb;
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f);
    if (scale && live) sc = ld4(scale + 4 * (int64_t)(b0 + bl));
    const float scv[4] = {sc.x, sc.y, sc.z, sc.w};
    double lo[4], hi[4], inv[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        lo[f] = ed[f * (nbins + 1)];
        hi[f] = ed[f * (nbins + 1) + nbins];
        const double w = hi[f] - lo[f];
        inv[f] = w > 0.0 ? (double)nbins / w : 0.0;
    }
    const float* base = table + 4 * (int64_t)(b0 + bl);
    for (int s0 = sl; s0 < n_samples && live; s0 += BH_UNROLL * ss) {
        float4 v4[BH_UNROLL];
#pragma unroll
        for (int u = 0; u < BH_UNROLL; ++u) {
            const int s = s0 + u * ss;
            v4[u] = s < n_samples ? ld4(base + 4 * (int64_t)s * n_bus) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < BH_UNROLL; ++u) {
            if (s0 + u * ss >= n_samples) continue;
            const float tv[4] = {v4[u].x, v4[u].y, v4[u].z, v4[u].w};
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const float vf = scale ? tv[f] * scv[f] : tv[f];          // ONE fp32 product, then every comparison in float64
                const double v = (double)vf;
                uint32_t* o3 = out3 + (bl * 4 + f) * 3;
                if (v != v) {
                    atomicAdd(o3 + 2, 1u);
                } else if (v < lo[f]) {
                    atomicAdd(o3, 1u);
                } else if (v > hi[f]) {
                    atomicAdd(o3 + 1, 1u);
                } else {
                    // a guess from the uniform spacing, corrected against the ACTUAL edges (np.linspace's are not exactly uniform,
                    // and a value may equal an edge): bin i holds edges[i] <= v < edges[i + 1], the last one also v == edges[nbins]
                    const double* e = ed + f * (nbins + 1);
                    double g = (v - lo[f]) * inv[f];
                    g = g >= 0.0 ? g : 0.0;                                // (also a NaN guess, from an infinite width)
                    int i = g < (double)(nbins - 1) ? (int)g : nbins - 1;
                    while (i > 0 && v < e[i]) --i;
                    while (i < nbins - 1 && v >= e[i + 1]) ++i;
                    atomicAdd(cnt + (bl * 4 + f) * nbins + i, 1u);
                }
            }
        }
    }
    __syncthreads();
    uint32_t* h = hist + (int64_t)b0 * 4 * nbins;
    for (int i = t; i < tb * 4 * nbins; i += BH_THREADS) h[i] = cnt[i];
    uint32_t* os = outside + (int64_t)b0 * 12;
    for (int i = t; i < tb * 12; i += BH_THREADS) os[i] = out3[i];
}

}  // namespace pfn

using namespace pfn;

extern "C" {

int pfn_bus_errors_accumulate(const float* out, const float* y, const void* mask, int mask_dtype, int64_t n_graphs, int64_t n_bus,
                              const float* std4, const float* mean4, const int64_t* sample_idx, int64_t table_rows, float* err_table,
                              float* pred_table, double* moments, int32_t* flags, void* stream) {
    PFN_CHECK_ARG(n_graphs >= 0 && n_bus >= 0 && n_bus < (1ll << 29) && n_graphs < (1ll << 29) && n_graphs * n_bus < (1ll << 29),
                  "pfn_bus_errors_accumulate: bad sizes (%lld graphs of %lld buses)", (long long)n_graphs, (long long)n_bus);
    const bool any = n_graphs > 0 && n_bus > 0;
    PFN_CHECK_ARG(moments && flags && (!any || (out && y && mask)), "pfn_bus_errors_accumulate: null pointer");
    PFN_CHECK_ARG(mask_dtype == 0 || mask_dtype == 1, "pfn_bus_errors_accumulate: mask_dtype must be 0 (int64) or 1 (float32)");
    PFN_CHECK_ARG(!(err_table || pred_table) || (sample_idx && table_rows >= 0 && table_rows < (1ll << 31)),
                  "pfn_bus_errors_accumulate: a table needs sample_idx and 0 <= table_rows < 2^31");
    PFN_CHECK_ARG(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(mask) |
                    reinterpret_cast<uintptr_t>(err_table) | reinterpret_cast<uintptr_t>(pred_table)) & 15) == 0,
                  "pfn_bus_errors_accumulate: out, y, mask and the tables must be 16-byte aligned");
    PFN_CHECK_ARG(((reinterpret_cast<uintptr_t>(moments) | reinterpret_cast<uintptr_t>(sample_idx)) & 7) == 0 &&
                      (reinterpret_cast<uintptr_t>(flags) & 3) == 0,
                  "pfn_bus_errors_accumulate: moments and sample_idx must be 8-byte aligned, flags 4-byte aligned");
    if (!any) return PFN_OK;
    BusErrScale sc;
    for (int f = 0; f < 4; ++f) {
        sc.std[f] = std4 ? std4[f] : 1.f;
        sc.mean[f] = mean4 ? mean4[f] : 0.f;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nb = (int)((n_bus + MO_OWNERS - 1) / MO_OWNERS);
    const double rows = (double)n_graphs * (double)n_bus;
    ProfScope ps("bus_errors_accumulate", rows * (32.0 + (mask_dtype == 0 ? 32.0 : 16.0) + (err_table ? 16.0 : 0.0) + (pred_table ? 16.0 : 0.0)) +
                                              (double)n_bus * 768.0, rows * 64.0, s);
    bus_errors_accumulate_kernel<<<nb, MO_THREADS, 0, s>>>(out, y, mask, mask_dtype, (int)n_graphs, (int)n_bus, sc, sample_idx, table_rows,
                                                           err_table, pred_table, moments, flags);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

int pfn_bus_errors_histogram(const float* table, int64_t n_samples, int64_t n_bus, const float* scale, const double* edges, int nbins,
                             uint32_t* hist, uint32_t* outside, void* stream) {
    PFN_CHECK_ARG(nbins >= 1 && nbins <= BH_MAX_BINS, "pfn_bus_errors_histogram: nbins must be in 1..%d (got %d)", BH_MAX_BINS, nbins);
    PFN_CHECK_ARG(n_samples >= 0 && n_samples < (1ll << 31) && n_bus >= 0 && n_bus < (1ll << 27),
                  "pfn_bus_errors_histogram: bad sizes (%lld samples of %lld buses; counts are uint32)", (long long)n_samples, (long long)n_bus);
    if (n_bus == 0) return PFN_OK;
    PFN_CHECK_ARG(edges && hist && outside && (table || n_samples == 0), "pfn_bus_errors_histogram: null pointer");
    PFN_CHECK_ARG(((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(scale)) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(edges) & 7) == 0 &&
                      ((reinterpret_cast<uintptr_t>(hist) | reinterpret_cast<uintptr_t>(outside)) & 3) == 0,
                  "pfn_bus_errors_histogram: table and scale must be 16-byte aligned, edges 8-byte, hist and outside 4-byte");
    const int tile = bh_tile(nbins);
    PFN_CHECK_ARG(tile >= 1, "pfn_bus_errors_histogram: %d bins do not fit the LDS of a compute unit", nbins);
    static std::atomic<uint64_t> raised{0};
    PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(bus_errors_histogram_kernel), kLdsCuBytes - kLdsReserve, raised));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nb = (int)((n_bus + tile - 1) / tile);
    ProfScope ps("bus_errors_histogram", (double)n_samples * n_bus * 16.0 + (double)n_bus * 4.0 * (nbins + 3) * 4.0,
                 (double)n_samples * n_bus * 4.0, s);
    bus_errors_histogram_kernel<<<nb, BH_THREADS, bh_lds_bytes(tile, nbins), s>>>(table, (int)n_samples, (int)n_bus, scale, edges, nbins,
                                                                                  tile, hist, outside);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

}  // extern "C"
