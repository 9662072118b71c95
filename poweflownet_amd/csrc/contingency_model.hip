// N-1 line-outage screening with the NETWORK's prediction on the device (gfx950): the two launches around a model forward.
// Work item t = s * e + k is scenario s with line k out; a chunk is `chunk` consecutive items from item0[0] (a device word, so that
// a captured chunk is replayed for every chunk of the screen), clamped to the last item: the tail repeats it.
//
// pfn_contingency_model_batch: one workgroup per item of the chunk writes what the dataset (datasets/PowerFlowData.py) plus its
// collate would have produced for the graph "scenario s without line k" -- x, pred_mask, bus_type, the reduced line list with the
// bus ids offset by the item's first row, the normalised (r, x) of the lines that stay.  The dataset's arithmetic in its order,
// every operation rounded on its own: the rows equal the dataset's bit for bit.  A pure streaming kernel: 16-byte stores (a bus
// row of x / pred_mask; two int64 ids, two bus types or two (r, x) pairs where the pair is 16-byte aligned in the collated tensor),
// no LDS, no atomics.
//
// pfn_contingency_model_loadings: one workgroup per item turns the forward's output rows into the screen's three figures.  Per bus
// the row is MERGED -- the de-normalised output where the bus type's mask says "predict", float(spec) where the entry is given -- and
// becomes a rectangular voltage in LDS (bf_phasor_of: one sincosf per bus, 8 bytes per bus); the threads then stride over the e lines
// of the ORIGINAL list, loading_l = bf_line(...).x / rating_l for l != k (branch_line.hpp: branch_flows.hip's text, hence its bits),
// and the workgroup reduces by the one tail of all screens (contingency_monitor.hpp): the maximum with ties to the lowest line, a
// non-finite monitored loading counts as the largest and makes the severity NaN, no monitored line gives (0, -1, 0), overloads are an
// integer count; the same merge serves the wave's shuffles and thread 0's loop over the waves' partials.  Beyond
// BF_LDS_MAX_BUS the phasors are formed per line end (the direct route, same bits).  Every cross-thread reduction is a max or an
// integer sum and every output has one owner: an item's bits are a function of its own inputs, whatever the chunk.  No host sync,
// no allocation (capturable), no float atomics.
#include "branch_line.hpp"
#include "contingency_monitor.hpp"
#include "pfn_internal.hpp"

namespace pfn {

constexpr int CM_THREADS = 256;
constexpr int CM_SCRATCH = 64;                     // dynamic LDS in front of the phasors: the four waves' partial reductions
static_assert(CM_SCRATCH == (CM_THREADS / 64) * sizeof(CtWorst), "a CtWorst per wave");

// PowerFlowData.bus_type_mask as bits (bit f = 1: feature f is predicted): slack (0,0,1,1), PV (0,1,0,1), PQ (1,1,0,0)
__device__ __forceinline__ int cm_mask_bits(int type) { return type <= 0 ? 0xC : (type == 1 ? 0xA : 0x3); }

// two 8-byte values that sit on one 16-byte line of the collated tensor
template <typename T>
struct alignas(16) CmPair {
    T a, b;
};

// dst[g0 + j] = f(j), j in [0, cnt): 8-byte elements of a tensor whose base is 16-byte aligned, written as 16-byte pairs on the even
// GLOBAL indices and as single elements at a ragged end (an item's slice starts at an odd element where chunk position * cnt is odd)
template <typename T, typename F>
__device__ __forceinline__ void cm_put8(T* __restrict__ dst, int64_t g0, int cnt, F f) {
    static_assert(sizeof(T) == 8, "8-byte elements");
    const int odd = (int)(g0 & 1);
    for (int p = threadIdx.x; 2 * p - odd < cnt; p += blockDim.x) {
        const int j0 = 2 * p - odd;
        if (j0 >= 0 && j0 + 1 < cnt) *reinterpret_cast<CmPair<T>*>(dst + g0 + j0) = CmPair<T>{f(j0), f(j0 + 1)};
        else if (j0 >= 0) dst[g0 + j0] = f(j0);
        else if (j0 + 1 < cnt) dst[g0 + j0 + 1] = f(j0 + 1);
    }
}

struct CmStats {
    float div[4], mean[4];                          // x: (v - mean) / div, div = std + 1e-7 formed in fp32 on the host (1, 0: identity)
    float ediv[2], emean[2];                        // edge_attr likewise
};

struct CmBatchArgs {
    const int32_t* bus_type;                        // [n]
    const double* spec;                             // [S, n, 4]
    const int64_t* edge_index;                      // [2, e]
    const double* rx;                               // [S, e, 2]
    const int64_t* item0;                           // [1] on the device
    float* x;                                       // [B n, 4]
    float* pred_mask;                               // [B n, 4]
    int64_t* bus_type_out;                          // [B n]
    int64_t* edge_index_out;                        // [2, B (e - 1)]
    float2* edge_attr;                              // [B (e - 1), 2]
    int32_t* flags;
    int64_t items;                                  // S e
    int n, e, chunk;
    CmStats st;
};

__global__ __launch_bounds__(CM_THREADS) void contingency_model_batch_kernel(const CmBatchArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.x, n = a.n, e = a.e, e1 = a.e - 1;
    const int64_t asked = a.item0[0] + b;
    const int64_t item = asked < 0 ? 0 : (asked < a.items ? asked : a.items - 1);
    const int s = (int)(item / e), k = (int)(item - (int64_t)s * e);
    const double* spec = a.spec + (int64_t)s * 4 * n;
    const double* rx = a.rx + (int64_t)s * 2 * e;
    const int64_t row0 = (int64_t)b * n, edge0 = (int64_t)b * e1;
    // ---- the bus rows: x = (float(spec) * (1 - mask) - mean) / div, the mask, 16 bytes each
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int bits = cm_mask_bits(a.bus_type[i]);
        const double2 lo = *reinterpret_cast<const double2*>(spec + 4 * i), hi = *reinterpret_cast<const double2*>(spec + 4 * i + 2);
        const float y[4] = {(float)lo.x, (float)lo.y, (float)hi.x, (float)hi.y};
        float m[4], v[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            m[f] = (bits >> f) & 1 ? 1.f : 0.f;
            const float keep = 1.0f - m[f];
            const float masked = y[f] * keep;       // (a masked entry is multiplied by 0, as the dataset does: a NaN there stays one)
            const float centred = masked - a.st.mean[f];
            v[f] = centred / a.st.div[f];
        }
        st4(a.x + 4 * (row0 + i), make_float4(v[0], v[1], v[2], v[3]));
        st4(a.pred_mask + 4 * (row0 + i), make_float4(m[0], m[1], m[2], m[3]));
    }
    const int32_t* bt = a.bus_type;
    cm_put8(a.bus_type_out, row0, n, [bt](int i) { return (int64_t)bt[i]; });
    // ---- the lines l != k in stored order: position j of the reduced list is line j + (j >= k)
    const int64_t* ei = a.edge_index;
    const uint64_t nb = (uint64_t)n;
    bool bad_seen = false;
    for (int row = 0; row < 2; ++row) {
        const int64_t* mine = ei + (int64_t)row * e;
        cm_put8(a.edge_index_out, (int64_t)row * a.chunk * e1 + edge0, e1, [&](int j) {
            const int l = j + (j >= k);
            const int64_t u = ei[l], w = ei[e + l];
            const bool ok = (uint64_t)u < nb && (uint64_t)w < nb;      // an id outside [0, n) is written as the local pair (0, 0)
            bad_seen |= !ok;
            return row0 + (ok ? mine[l] : (int64_t)0);
        });
    }
    const float2 emean = make_float2(a.st.emean[0], a.st.emean[1]), ediv = make_float2(a.st.ediv[0], a.st.ediv[1]);
    cm_put8(a.edge_attr, edge0, e1, [&](int j) {
        const int l = j + (j >= k);
        const double2 z = *reinterpret_cast<const double2*>(rx + 2 * l);
        const float cr = (float)z.x - emean.x, cx = (float)z.y - emean.y;
        return make_float2(cr / ediv.x, cx / ediv.y);
    });
    if (bad_seen) a.flags[0] = a.flags[0] | 2;       // (every writer stores the same bit over the same word)
}

struct CmLoadArgs {
    const float* out;                               // [B n, 4], the forward's output for the chunk's batch
    const int32_t* bus_type;                        // [n]
    const double* spec;                             // [S, n, 4]
    const int64_t* edge_index;                      // [2, e]
    const double* rx;                               // [S, e, 2]
    const double* ratings;                          // [e], [S, e] or null (1.0 everywhere)
    const int32_t* islands;                         // [e]
    const int64_t* item0;                           // [1] on the device
    float* severity;                                // [S e]
    int32_t* worst_line;                            // [S e]
    int32_t* overloads;                             // [S e]
    float* loading;                                 // [S e, e] or null
    float* predictions;                             // [S e, n, 4] or null
    int64_t items;
    int n, e, chunk, ratings_per_sample;
    float sd[4], mu[4];                             // denorm: out * sd + mu, sd = std + 1e-7 formed in fp32 on the host (1, 0: identity)
};

// the merged, de-normalised row of bus i: the network's where the mask says "predict", the specification's where it is given
__device__ __forceinline__ float4 cm_merged(const CmLoadArgs& a, const float* __restrict__ out, const double* __restrict__ spec, int i) {
    const int bits = cm_mask_bits(a.bus_type[i]);
    const float4 o = ld4(out + 4 * (int64_t)i);
    const double2 lo = *reinterpret_cast<const double2*>(spec + 4 * i), hi = *reinterpret_cast<const double2*>(spec + 4 * i + 2);
    return make_float4(bits & 1 ? denorm(o.x, a.sd[0], a.mu[0]) : (float)lo.x, bits & 2 ? denorm(o.y, a.sd[1], a.mu[1]) : (float)lo.y,
                       bits & 4 ? denorm(o.z, a.sd[2], a.mu[2]) : (float)hi.x, bits & 8 ? denorm(o.w, a.sd[3], a.mu[3]) : (float)hi.y);
}

template <bool LDS>
__global__ __launch_bounds__(CM_THREADS) void contingency_model_loadings_kernel(const CmLoadArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cm_smem[];
    const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6, nw = nt >> 6;
    const int n = a.n, e = a.e;
    const int64_t item = a.item0[0] + blockIdx.x;
    if (item < 0 || item >= a.items) return;        // the padding of the last chunk (uniform over the workgroup)
    const int s = (int)(item / e), k = (int)(item - (int64_t)s * e);
    const float* out = a.out + (int64_t)blockIdx.x * 4 * n;
    const double* spec = a.spec + (int64_t)s * 4 * n;
    const double* rx = a.rx + (int64_t)s * 2 * e;
    const double* rat = a.ratings ? a.ratings + (a.ratings_per_sample ? (int64_t)s * e : 0) : nullptr;
    float* row = a.loading ? a.loading + item * e : nullptr;
    float* pred = a.predictions ? a.predictions + item * 4 * n : nullptr;
    const float nanv = __builtin_nanf("");
    float2* ph = reinterpret_cast<float2*>(cm_smem + CM_SCRATCH);         // LDS: [n] (e, f)
    // ---- merge, keep the table where asked for, phasors
    if (LDS || pred) {
        for (int i = t; i < n; i += nt) {
            const float4 m = cm_merged(a, out, spec, i);
            if (pred) st4(pred + 4 * (int64_t)i, m);
            if (LDS) ph[i] = bf_phasor_of(m.x, m.y);
        }
    }
    // an islanding outage (or a line list with a bad id: -4): +inf, so that it ranks first, -1, -1 and a NaN row
    if (a.islands[k] != 0) {
        ct_skip(false, row, e, t, nt, a.severity[item], a.worst_line[item], a.overloads[item]);
        return;
    }
    if (LDS) __syncthreads();
    // ---- the lines of the original list: loading; the workgroup's worst (contingency_monitor.hpp)
    const uint64_t nb = (uint64_t)n;
    CtWorst worst = ct_worst_none();
    for (int l = t; l < e; l += nt) {
        if (l == k) {
            if (row) row[l] = nanv;
            continue;
        }
        const int64_t i = a.edge_index[l], j = a.edge_index[e + l];
        const double2 z = *reinterpret_cast<const double2*>(rx + 2 * l);
        const float r = rat ? (float)rat[l] : 1.f;
        float load = nanv;
        if ((uint64_t)i < nb && (uint64_t)j < nb) {                       // (islands is -4 then: never reached, never followed)
            float2 vi, vj;
            if (LDS) {
                vi = ph[(int)i];
                vj = ph[(int)j];
            } else {
                const float4 mi = cm_merged(a, out, spec, (int)i), mj = cm_merged(a, out, spec, (int)j);
                vi = bf_phasor_of(mi.x, mi.y);
                vj = bf_phasor_of(mj.x, mj.y);
            }
            load = bf_line(vi, vj, (float)z.x, (float)z.y).x / r;
        }
        if (row) row[l] = load;
        if (r > 0.f) ct_worst_add(worst, l, load);
    }
    worst = ct_worst_wave(worst);
    CtWorst* part = reinterpret_cast<CtWorst*>(cm_smem);                  // LDS scratch: the waves' partials
    if (lane == 0) part[wave] = worst;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < nw; ++w) ct_worst_merge(worst, part[w]);      // (a max with the lowest line and integer sums: no order to keep)
        ct_store(ct_figures(worst), a.severity[item], a.worst_line[item], a.overloads[item]);
    }
}

static bool cm_sizes_ok(int64_t n_samples, int64_t n_bus, int64_t n_lines, int64_t chunk) {
    return n_samples >= 0 && n_bus >= 2 && n_lines >= 2 && chunk >= 1 && n_samples < (1ll << 29) && n_bus < (1ll << 24) && n_lines < (1ll << 24) &&
           chunk < (1ll << 24) && chunk * n_bus < (1ll << 29) && chunk * (n_lines - 1) < (1ll << 29) && n_samples * n_lines < (1ll << 31);
}

}  // namespace pfn

using namespace pfn;

extern "C" {

int64_t pfn_contingency_model_lds_max_bus(void) { return BF_LDS_MAX_BUS; }

int pfn_contingency_model_batch(const int32_t* bus_type, const double* spec, const int64_t* edge_index, const double* rx, int64_t n_samples,
                                int64_t n_bus, int64_t n_lines, const int64_t* item0, int64_t chunk, const float* div4, const float* mean4,
                                const float* edge_div2, const float* edge_mean2, float* x, float* pred_mask, int64_t* bus_type_out,
                                int64_t* edge_index_out, float* edge_attr, int32_t* flags, void* stream) {
    const char* who = "pfn_contingency_model_batch";
    PFN_CHECK_ARG(cm_sizes_ok(n_samples, n_bus, n_lines, chunk), "%s: bad sizes (%lld scenarios of %lld buses and %lld lines, chunks of %lld items)", who,
                  (long long)n_samples, (long long)n_bus, (long long)n_lines, (long long)chunk);
    if (n_samples == 0) return PFN_OK;
    PFN_CHECK_ARG(bus_type && spec && edge_index && rx && item0 && x && pred_mask && bus_type_out && edge_index_out && edge_attr && flags,
                  "%s: null pointer", who);
    PFN_CHECK_ARG(((reinterpret_cast<uintptr_t>(spec) | reinterpret_cast<uintptr_t>(rx) | reinterpret_cast<uintptr_t>(x) |
                    reinterpret_cast<uintptr_t>(pred_mask) | reinterpret_cast<uintptr_t>(bus_type_out) | reinterpret_cast<uintptr_t>(edge_index_out) |
                    reinterpret_cast<uintptr_t>(edge_attr)) & 15) == 0 &&
                      ((reinterpret_cast<uintptr_t>(edge_index) | reinterpret_cast<uintptr_t>(item0)) & 7) == 0 &&
                      ((reinterpret_cast<uintptr_t>(bus_type) | reinterpret_cast<uintptr_t>(flags)) & 3) == 0,
                  "%s: spec, rx and the batch's tensors must be 16-byte aligned, edge_index and item0 8-byte, bus_type and flags 4-byte", who);
    CmBatchArgs a;
    a.bus_type = bus_type;
    a.spec = spec;
    a.edge_index = edge_index;
    a.rx = rx;
    a.item0 = item0;
    a.x = x;
    a.pred_mask = pred_mask;
    a.bus_type_out = bus_type_out;
    a.edge_index_out = edge_index_out;
    a.edge_attr = reinterpret_cast<float2*>(edge_attr);
    a.flags = flags;
    a.items = n_samples * n_lines;
    a.n = (int)n_bus;
    a.e = (int)n_lines;
    a.chunk = (int)chunk;
    for (int f = 0; f < 4; ++f) {
        a.st.div[f] = div4 ? div4[f] : 1.f;
        a.st.mean[f] = mean4 ? mean4[f] : 0.f;
    }
    for (int f = 0; f < 2; ++f) {
        a.st.ediv[f] = edge_div2 ? edge_div2[f] : 1.f;
        a.st.emean[f] = edge_mean2 ? edge_mean2[f] : 0.f;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double rows = (double)chunk * (double)n_bus, lines = (double)chunk * (double)(n_lines - 1);
    ProfScope ps("contingency_model_batch", rows * (32.0 + 4.0 + 40.0) + lines * (32.0 + 16.0 + 24.0), rows * 12.0 + lines * 4.0, s);
    contingency_model_batch_kernel<<<(int)chunk, CM_THREADS, 0, s>>>(a);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

int pfn_contingency_model_loadings(const float* out, const int32_t* bus_type, const double* spec, const int64_t* edge_index, const double* rx,
                                   const double* ratings, int ratings_per_sample, const int32_t* islands, int64_t n_samples, int64_t n_bus,
                                   int64_t n_lines, const int64_t* item0, int64_t chunk, const float* std4, const float* mean4, int route,
                                   float* severity, int32_t* worst_line, int32_t* overloads, float* loading, float* predictions, void* stream) {
    const char* who = "pfn_contingency_model_loadings";
    PFN_CHECK_ARG(cm_sizes_ok(n_samples, n_bus, n_lines, chunk), "%s: bad sizes (%lld scenarios of %lld buses and %lld lines, chunks of %lld items)", who,
                  (long long)n_samples, (long long)n_bus, (long long)n_lines, (long long)chunk);
    PFN_CHECK_ARG(route >= 0 && route <= 2, "%s: route must be 0 (auto), 1 (LDS) or 2 (direct)", who);
    PFN_CHECK_ARG(route != 1 || n_bus <= BF_LDS_MAX_BUS, "%s: route 1 (LDS): the phasors of %lld buses need %lld bytes of LDS, %d buses fit", who,
                  (long long)n_bus, (long long)(8 * n_bus), BF_LDS_MAX_BUS);
    if (n_samples == 0) return PFN_OK;
    PFN_CHECK_ARG(out && bus_type && spec && edge_index && rx && islands && item0 && severity && worst_line && overloads, "%s: null pointer", who);
    PFN_CHECK_ARG(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(spec) | reinterpret_cast<uintptr_t>(rx) |
                    reinterpret_cast<uintptr_t>(predictions)) & 15) == 0 &&
                      ((reinterpret_cast<uintptr_t>(edge_index) | reinterpret_cast<uintptr_t>(item0) | reinterpret_cast<uintptr_t>(ratings)) & 7) == 0 &&
                      ((reinterpret_cast<uintptr_t>(bus_type) | reinterpret_cast<uintptr_t>(islands) | reinterpret_cast<uintptr_t>(severity) |
                        reinterpret_cast<uintptr_t>(worst_line) | reinterpret_cast<uintptr_t>(overloads) | reinterpret_cast<uintptr_t>(loading)) & 3) == 0,
                  "%s: out, spec, rx and predictions must be 16-byte aligned, int64 and fp64 arrays 8-byte, fp32 and int32 arrays 4-byte", who);
    CmLoadArgs a;
    a.out = out;
    a.bus_type = bus_type;
    a.spec = spec;
    a.edge_index = edge_index;
    a.rx = rx;
    a.ratings = ratings;
    a.islands = islands;
    a.item0 = item0;
    a.severity = severity;
    a.worst_line = worst_line;
    a.overloads = overloads;
    a.loading = loading;
    a.predictions = predictions;
    a.items = n_samples * n_lines;
    a.n = (int)n_bus;
    a.e = (int)n_lines;
    a.chunk = (int)chunk;
    a.ratings_per_sample = ratings_per_sample != 0;
    for (int f = 0; f < 4; ++f) {
        a.sd[f] = std4 ? std4[f] : 1.f;
        a.mu[f] = mean4 ? mean4[f] : 0.f;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double rows = (double)chunk * (double)n_bus, lines = (double)chunk * (double)n_lines;
    ProfScope ps("contingency_model_loadings", rows * (16.0 + 32.0 + 4.0 + (predictions ? 16.0 : 0.0)) + lines * (16.0 + 16.0 + 8.0 + (loading ? 4.0 : 0.0)),
                 rows * 24.0 + lines * 24.0, s);
    const bool lds = route == 1 || (route == 0 && n_bus <= BF_LDS_MAX_BUS);
    return launch_either<contingency_model_loadings_kernel<true>, contingency_model_loadings_kernel<false>>(lds, (int)chunk, CM_THREADS,
                                                                                                            CM_SCRATCH + (size_t)n_bus * 8, CM_SCRATCH, s, a);
}

}  // extern "C"
