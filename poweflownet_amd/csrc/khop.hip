// k-hop locality analysis (gfx950): the device side of utils/explanation.py, the counterpart of the reference's explain_epoch
// (utils/explanation.py:34-114), which reruns the model once per (center bus c, hop radius m, batch) on the edge list cut down to
// the m-hop ball around c (PyG k_hop_subgraph(directed=False) over _make_bidirectional(edge_index)).  Here every ball is packed
// as a small graph of its own, so a few forwards over batches of balls replace thousands of whole-batch forwards.
//
// All three entry points work on a graph_ws that pfn_graph_build made in mode 1 (always undirect) from ONE graph's edge list:
// the by-destination CSR (rowptr_in / in_src) then holds every stored edge in both directions, whatever the list held.
//   khop_dist_kernel   one workgroup per center: level-synchronous BFS over the CSR, the distance row in LDS while it fits
//                      (else in the caller's global row), eccentricity from one reduction at the end
//   khop_hist_kernel   one workgroup per center: node / edge histograms over the distance row -> cumulative ball sizes
//   khop_pack_kernel   one workgroup per instance: ballot + popcount stream compaction of the ball's nodes (ascending id, the
//                      old -> new id map in LDS) and of its edges (ascending id of the bidirectional list), deterministic
#include "pfn_internal.hpp"

namespace pfn {

constexpr int KHOP_THREADS = 256;
constexpr int KHOP_WAVES = KHOP_THREADS / 64;
constexpr uint16_t KHOP_INF = 0xFFFF;
constexpr int KHOP_LDS_CAP = 150 * 1024;   // dynamic LDS a khop kernel may ask for (160 KiB per CU, statics kept clear)

// ------------------------------------------------------------------------------------------ distances
// Frontier of level L = the nodes whose distance is L (no queue): each level scans the row once and relaxes the neighbours of its
// frontier.  A relaxed node is written the same value L + 1 by every thread that finds it, so the races are benign; `grew` is
// triple-buffered so that the slot a level writes is cleared two barriers before anyone writes it again.
__global__ __launch_bounds__(KHOP_THREADS) void khop_dist_kernel(const int* __restrict__ rowptr, const int* __restrict__ nbr, int n,
                                                                 const int* __restrict__ centers, int max_hops, int lds_row,
                                                                 uint16_t* __restrict__ dist, int* __restrict__ ecc) {
    extern __shared__ __attribute__((aligned(16))) uint16_t kd_row[];
    __shared__ int grew[3];
    __shared__ int red_cnt[KHOP_WAVES], red_max[KHOP_WAVES];
    const int c = blockIdx.x, tid = threadIdx.x;
    uint16_t* row = lds_row ? kd_row : dist + (size_t)c * n;
    const int src = centers[c];
    for (int v = tid; v < n; v += KHOP_THREADS) row[v] = (v == src) ? 0 : KHOP_INF;
    if (tid < 3) grew[tid] = 0;
    __syncthreads();
    for (int level = 0; level < max_hops; ++level) {
        int any = 0;
        for (int v = tid; v < n; v += KHOP_THREADS) {
            if (row[v] != level) continue;
            for (int k = rowptr[v], k1 = rowptr[v + 1]; k < k1; ++k) {
                const int u = nbr[k];
                if (row[u] == KHOP_INF) {
                    row[u] = (uint16_t)(level + 1);
                    any = 1;
                }
            }
        }
        if (any) grew[level % 3] = 1;
        __syncthreads();
        const int go = grew[level % 3];
        if (tid == 0) grew[(level + 2) % 3] = 0;
        if (!go) break;
    }
    int cnt = 0, mx = 0;
    for (int v = tid; v < n; v += KHOP_THREADS) {
        const int d = row[v];
        if (d != KHOP_INF) {
            ++cnt;
            mx = d > mx ? d : mx;
        }
        if (lds_row && dist) dist[(size_t)c * n + v] = (uint16_t)d;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        cnt += __shfl_xor(cnt, off);
        const int o = __shfl_xor(mx, off);
        mx = o > mx ? o : mx;
    }
    if ((tid & 63) == 0) {
        red_cnt[tid >> 6] = cnt;
        red_max[tid >> 6] = mx;
    }
    __syncthreads();
    if (tid == 0) {
        int tc = 0, tm = 0;
        for (int w = 0; w < KHOP_WAVES; ++w) {
            tc += red_cnt[w];
            tm = red_max[w] > tm ? red_max[w] : tm;
        }
        ecc[c] = (tc == n) ? tm : -1;
    }
}

// ----------------------------------------------------------------------------------------- histograms
// node_count[c][r] = |{v : dist <= r}|, edge_count[c][r] = |{bidirectional edges (u, v) : max(dist u, dist v) <= r}|.  Every
// by-destination slot of the CSR is one edge of the bidirectional list, so each is counted exactly once.
__global__ __launch_bounds__(KHOP_THREADS) void khop_hist_kernel(const int* __restrict__ rowptr, const int* __restrict__ nbr, int n,
                                                                 const uint16_t* __restrict__ dist, int R, int* __restrict__ node_count,
                                                                 int* __restrict__ edge_count) {
    extern __shared__ __attribute__((aligned(16))) int kh_hist[];   // [R + 1] nodes | [R + 1] edges
    const int c = blockIdx.x, tid = threadIdx.x, nr = R + 1;
    int* hn = kh_hist;
    int* he = kh_hist + nr;
    for (int r = tid; r < 2 * nr; r += KHOP_THREADS) kh_hist[r] = 0;
    __syncthreads();
    const uint16_t* row = dist + (size_t)c * n;
    for (int v = tid; v < n; v += KHOP_THREADS) {
        const int d = row[v];
        if (d > R) continue;                      // (KHOP_INF > R always)
        atomicAdd(&hn[d], 1);
        for (int k = rowptr[v], k1 = rowptr[v + 1]; k < k1; ++k) {
            const int du = row[nbr[k]];
            const int m = du > d ? du : d;
            if (m <= R) atomicAdd(&he[m], 1);
        }
    }
    __syncthreads();
    if (tid == 0) {                               // cumulative sums: R is the graph's diameter at most, a few hundred
        int an = 0, ae = 0;
        for (int r = 0; r < nr; ++r) {
            an += hn[r];
            ae += he[r];
            node_count[(size_t)c * nr + r] = an;
            edge_count[(size_t)c * nr + r] = ae;
        }
    }
}

// ---------------------------------------------------------------------------------------------- pack
// Stable workgroup compaction of one tile of KHOP_THREADS predicates: returns this thread's rank among the set predicates of the
// tile (valid where pred), adds the tile's total to `base` (every thread).  Two barriers.
__device__ __forceinline__ int khop_tile_rank(bool pred, int* wtot /* [KHOP_WAVES] */, int& base) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(pred);
    int rank = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[wave] = __popcll(b);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < KHOP_WAVES; ++w) {
        before += (w < wave) ? wtot[w] : 0;
        total += wtot[w];
    }
    __syncthreads();                              // wtot is rewritten by the next tile
    rank += base + before;
    base += total;
    return rank;
}

struct KhopPackArgs {
    int n, e;                        // graph 0: nodes, stored edges
    const int64_t* ei;               // [2][e] graph 0's stored list (the one graph_ws was built from)
    const int* graph_flags;          // GraphView::flags: [2] != 0 = the build found an id outside [0, n)
    const int* centers;              // [rows] node id of each distance row
    const uint16_t* dist;            // [rows][n]
    const int* inst_row;             // [I] distance row (= center) of each instance
    const int* inst_radius;          // [I]
    const int* inst_sample;          // [I] batch position s: node ids are s * n + v
    const int64_t* node_off;         // [I + 1] exclusive offsets of the instances' nodes in the packed batch
    const int64_t* edge_off;         // [I + 1] ... and of their edges
    int64_t total_edges;             // edge_off[I]: row stride of edge_index_out
    int64_t* node_ids;               // [node_off[I]]
    int64_t* edge_index_out;         // [2][total_edges] relabelled to packed rows
    int64_t* edge_ids;               // [total_edges] id in graph 0's bidirectional list (< e: stored edge, >= e: its reverse)
    int64_t* center_pos;             // [I] packed row of each instance's center
    int* err;                        // set to 1 when an instance's size disagrees with its offsets (nothing is written past them)
};

__global__ __launch_bounds__(KHOP_THREADS) void khop_pack_kernel(KhopPackArgs a) {
    extern __shared__ __attribute__((aligned(16))) int kp_map[];     // [n] old id -> new id, -1 outside the ball
    __shared__ int wtot[KHOP_WAVES];
    const int i = blockIdx.x, tid = threadIdx.x, n = a.n, e = a.e;
    if (a.graph_flags[2] != 0) {                  // ids out of range: the CSR and the stored list disagree
        if (tid == 0) atomicOr(a.err, 1);
        return;
    }
    const int m = a.inst_radius[i], s = a.inst_sample[i];
    const uint16_t* row = a.dist + (size_t)a.inst_row[i] * n;
    const int64_t n0 = a.node_off[i], ncap = a.node_off[i + 1] - n0;
    const int64_t e0 = a.edge_off[i], ecap = a.edge_off[i + 1] - e0;
    int base = 0;
    for (int t = 0; t < n; t += KHOP_THREADS) {
        const int v = t + tid;
        const bool in = v < n && (int)row[v] <= m;
        const int r = khop_tile_rank(in, wtot, base);
        if (v < n) kp_map[v] = in ? r : -1;
        if (in && r < ncap) a.node_ids[n0 + r] = (int64_t)s * n + v;
    }
    if (tid == 0 && base != ncap) atomicOr(a.err, 1);
    __syncthreads();                              // kp_map complete
    if (tid == 0) {
        const int ctr = a.centers[a.inst_row[i]];
        a.center_pos[i] = n0 + ((ctr >= 0 && ctr < n) ? kp_map[ctr] : 0);
    }
    // bidirectional list of _make_bidirectional: k < e -> (ei[0][k], ei[1][k]); k >= e -> (ei[1][k - e], ei[0][k - e]),
    // i.e. source ei[k] and destination ei[k < e ? e + k : k - e] of the flat [2][e] array
    base = 0;
    for (int t = 0; t < 2 * e; t += KHOP_THREADS) {
        const int k = t + tid;
        int ma = -1, mb = -1;
        if (k < 2 * e) {
            const int64_t u = a.ei[k], w = a.ei[k < e ? e + k : k - e];
            if (u >= 0 && u < n && w >= 0 && w < n) {
                ma = kp_map[u];
                mb = kp_map[w];
            }
        }
        const bool in = ma >= 0 && mb >= 0;
        const int r = khop_tile_rank(in, wtot, base);
        if (in && r < ecap) {
            a.edge_index_out[e0 + r] = n0 + ma;
            a.edge_index_out[a.total_edges + e0 + r] = n0 + mb;
            a.edge_ids[e0 + r] = k;
        }
    }
    if (tid == 0 && base != ecap) atomicOr(a.err, 1);
}

static std::atomic<uint64_t> lds_raised_dist{0}, lds_raised_hist{0}, lds_raised_pack{0};

}  // namespace pfn

using namespace pfn;

extern "C" {

int pfn_khop_distances(const void* graph_ws, int64_t n, int64_t e, const int32_t* centers, int64_t n_centers, int32_t max_hops,
                       uint16_t* dist, int32_t* ecc, void* stream) {
    PFN_CHECK_ARG(graph_ws && ecc && (n_centers == 0 || centers), "pfn_khop_distances: null pointer");
    PFN_CHECK_ARG(n > 0 && n < (1ll << 30) && e >= 0 && n_centers >= 0 && n_centers < (1ll << 31),
                  "pfn_khop_distances: bad sizes (n %lld, centers %lld)", (long long)n, (long long)n_centers);
    PFN_CHECK_ARG(max_hops >= 0 && max_hops < KHOP_INF, "pfn_khop_distances: max_hops %d outside [0, 65534]", (int)max_hops);
    const size_t row_bytes = (size_t)round_up(n * 2, 16);
    const int lds_row = row_bytes <= (size_t)KHOP_LDS_CAP;
    PFN_CHECK_ARG(lds_row || dist, "pfn_khop_distances: %lld nodes do not fit in LDS; pass a distance buffer", (long long)n);
    if (n_centers == 0) return PFN_OK;
    GraphView g = graph_view(const_cast<void*>(graph_ws), n, e);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int lds = lds_row ? (int)row_bytes : 0;
    if (lds > 64 * 1024) PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(khop_dist_kernel), KHOP_LDS_CAP, lds_raised_dist));
    khop_dist_kernel<<<(unsigned)n_centers, KHOP_THREADS, lds, s>>>(g.rowptr_in, g.in_src, (int)n, centers, max_hops, lds_row, dist, ecc);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

int pfn_khop_histograms(const void* graph_ws, int64_t n, int64_t e, const uint16_t* dist, int64_t n_centers, int32_t max_radius,
                        int32_t* node_count, int32_t* edge_count, void* stream) {
    PFN_CHECK_ARG(graph_ws && node_count && edge_count && (n_centers == 0 || dist), "pfn_khop_histograms: null pointer");
    PFN_CHECK_ARG(n > 0 && n < (1ll << 30) && e >= 0 && n_centers >= 0 && n_centers < (1ll << 31), "pfn_khop_histograms: bad sizes");
    const int64_t lds = (int64_t)2 * (max_radius + 1) * 4;
    PFN_CHECK_ARG(max_radius >= 0 && max_radius < KHOP_INF && lds <= KHOP_LDS_CAP, "pfn_khop_histograms: max_radius %d too large",
                  (int)max_radius);
    if (n_centers == 0) return PFN_OK;
    GraphView g = graph_view(const_cast<void*>(graph_ws), n, e);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (lds > 64 * 1024) PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(khop_hist_kernel), KHOP_LDS_CAP, lds_raised_hist));
    khop_hist_kernel<<<(unsigned)n_centers, KHOP_THREADS, (size_t)lds, s>>>(g.rowptr_in, g.in_src, (int)n, dist, max_radius,
                                                                            node_count, edge_count);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

int pfn_khop_pack(const void* graph_ws, int64_t n, int64_t e, const int64_t* edge_index, const int32_t* centers,
                  const uint16_t* dist, const int32_t* inst_row, const int32_t* inst_radius, const int32_t* inst_sample,
                  const int64_t* node_off, const int64_t* edge_off, int64_t n_inst, int64_t total_edges, int64_t* node_ids,
                  int64_t* edge_index_out, int64_t* edge_ids, int64_t* center_pos, int32_t* err, void* stream) {
    PFN_CHECK_ARG(n > 0 && n < (1ll << 30) && e >= 0 && e < (1ll << 29) && n_inst >= 0 && n_inst < (1ll << 31) && total_edges >= 0,
                  "pfn_khop_pack: bad sizes");
    PFN_CHECK_ARG(graph_ws && centers && dist && inst_row && inst_radius && inst_sample && node_off && edge_off && node_ids &&
                      center_pos && err && (e == 0 || edge_index) && (total_edges == 0 || (edge_index_out && edge_ids)),
                  "pfn_khop_pack: null pointer");
    const int64_t lds = round_up(n * 4, 16);
    PFN_CHECK_ARG(lds <= KHOP_LDS_CAP, "pfn_khop_pack: %lld nodes do not fit the LDS id map", (long long)n);
    if (n_inst == 0) return PFN_OK;
    GraphView g = graph_view(const_cast<void*>(graph_ws), n, e);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (lds > 64 * 1024) PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(khop_pack_kernel), KHOP_LDS_CAP, lds_raised_pack));
    KhopPackArgs a;
    a.n = (int)n;
    a.e = (int)e;
    a.ei = edge_index;
    a.graph_flags = g.flags;
    a.centers = centers;
    a.dist = dist;
    a.inst_row = inst_row;
    a.inst_radius = inst_radius;
    a.inst_sample = inst_sample;
    a.node_off = node_off;
    a.edge_off = edge_off;
    a.total_edges = total_edges;
    a.node_ids = node_ids;
    a.edge_index_out = edge_index_out;
    a.edge_ids = edge_ids;
    a.center_pos = center_pos;
    a.err = err;
    khop_pack_kernel<<<(unsigned)n_inst, KHOP_THREADS, (size_t)lds, s>>>(a);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

}  // extern "C"
