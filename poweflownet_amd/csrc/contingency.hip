// N-1 line-outage screening on the device (gfx950): which single line outages overload the rest of the grid?  Two launches.
//
// pfn_contingency_islands: one workgroup per outage k asks topology_reach.hpp's reach routine which buses the slack still reaches
// over the base list with line k skipped (a keep flag per line in LDS: no [e, 2, e - 1] lists exist anywhere).  islands[k] > 0 is a
// bridge; it is decided combinatorially, from the line list alone, never from a small denominator.  The N-2 screen's
// pfn_contingency_pair_islands (described in contingency_pairs.hip) lives here too: one LDS layout, one staging, one set of checks.
//
// pfn_contingency_dc: one workgroup per scenario, the DC model of powerflow.hip's mode 1 and the classical line outage
// distribution factors.  With X = B'^-1 (zeros at the slack) and the outage of line k = (i -> j):
//     w_k = X[:, i] - X[:, j]      phi_{l,k} = (w_k[a] - w_k[b]) / x_l  for line l = (a -> b)      den_k = 1 - phi_{k,k}
//     f_l^(k) = f_l + phi_{l,k} / den_k * f_k   (l != k),   f_k^(k) = 0
// -- one inverse per scenario and e^2 multiply-adds where the brute-force path factorises e matrices.
//   PHASE A, the whole workgroup, once (contingency_base.hpp ct_base_solve, shared with the N-2 screen's base launch): the lines are
//   staged in LDS, B' is built in fp32 (row-major, ld = m | 1, m = n - 1) by the row owners in stored order exactly as the
//   fast-decoupled modes build theirs and inverted in place by THEIR Gauss-Jordan (powerflow_dense.hpp); theta is refined,
//   theta -= X F, under the fp64 residual F = B' theta + P of mode 1 to tol / max_iter (status = the refinement solves used); the base
//   flows f_l = (theta_a - theta_b) / x_l are fp64.
//   PHASE B, no workgroup barrier: wave w takes the outages w, w + nw, ...  Its lanes form w_k into the wave's own fp32 vector [n]
//   (contingency_base.hpp ct_column: two column walks of X, stride ld, odd, so conflict-free), then stride over the lines: phi,
//   post-outage flow, loading |f| / rating.  The wave reduces and lane 0 writes severity, worst line and overload count of (s, k) by
//   the one tail of all screens (contingency_monitor.hpp: the maximum with ties to the lowest line, an integer sum, what a skipped
//   item carries); the full table row, where asked for, is written coalesced by the lanes.
// The per-line expression is compiled without contraction (as branch_flows.hip's), every cross-thread reduction is a max or an
// integer sum, one owner per output: a scenario's bits are a pure function of its own inputs, whatever the batch, the workgroup
// size or the route.  LDS route: X sits behind the scenario's vectors in LDS; global route: in a per-scenario slab of the caller's
// workspace, same code.  No host sync, no allocation (capturable), no float atomics.
#include "contingency_base.hpp"
#include "contingency_line.hpp"
#include "contingency_monitor.hpp"
#include "topology_reach.hpp"

namespace pfn {

// ------------------------------------------------------------------------------------------------------ islands
// Both islands launches (N-1: a workgroup per outage; N-2: a workgroup per first candidate, contingency_pairs.hip has the screen):
// dynamic LDS of a workgroup: ID from[e] | ID to[e] | uint8 keep[e] | uint8 reached[n]
__host__ __device__ inline size_t ct_islands_lds_bytes(int n, int e) {
    const size_t id = n <= 65536 ? 2 : 4;
    return tp_align4(2 * id * (size_t)e) + tp_align4((size_t)e) + tp_align4((size_t)n);
}
template <typename ID>
struct CtIslandsLds {
    ID* from;
    ID* to;
    uint8_t* keep;
    uint8_t* reached;
};
// the layout, and the line ends staged where the ids are good (returns that): thread t stages the lines t, t + nt, ... -- those it
// flags in `keep` and walks in tp_unreached.  An id outside [0, n) is never followed: every item of such a list reports it.
template <typename ID>
__device__ __forceinline__ bool ct_islands_stage(unsigned char* smem, const int64_t* __restrict__ ei, int n, int e, CtIslandsLds<ID>& v) {
    v.from = reinterpret_cast<ID*>(smem);
    v.to = v.from + e;
    v.keep = smem + tp_align4(2 * sizeof(ID) * (size_t)e);
    v.reached = v.keep + tp_align4((size_t)e);
    if (tp_bad_lines(ei, e, n)) return false;
    for (int l = threadIdx.x; l < e; l += blockDim.x) {
        v.from[l] = (ID)ei[l];
        v.to[l] = (ID)ei[e + l];
    }
    return true;
}

template <typename ID>
__global__ __launch_bounds__(1024) void contingency_islands_kernel(const int64_t* __restrict__ ei, int n, int e, int root,
                                                                   int32_t* __restrict__ islands) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ct_smem[];
    __shared__ int s_count;
    const int t = threadIdx.x, nt = blockDim.x;
    const int k = blockIdx.x;
    CtIslandsLds<ID> v;
    int count = PF_BAD_LINE;
    if (ct_islands_stage(ct_smem, ei, n, e, v)) {
        for (int l = t; l < e; l += nt) v.keep[l] = l != k;
        count = tp_unreached<ID>(v.from, v.to, v.keep, e, n, root, v.reached, &s_count);
    }
    if (t == 0) islands[k] = count;
}

// pair p = (lines[i], lines[j]), i < j: workgroup i loops over j > i with BOTH keep flags cleared
template <typename ID>
__global__ __launch_bounds__(1024) void contingency_pair_islands_kernel(const int64_t* __restrict__ ei, int n, int e, int root,
                                                                        const int32_t* __restrict__ lines, int c, int32_t* __restrict__ islands) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ct_smem[];
    __shared__ int s_count;
    const int t = threadIdx.x, nt = blockDim.x;
    const int i = blockIdx.x;
    CtIslandsLds<ID> v;
    const bool bad = !ct_islands_stage(ct_smem, ei, n, e, v);
    const int a = lines[i];
    int32_t* out = islands + cp_first_pair(i, c);
    for (int j = i + 1; j < c; ++j) {
        const int b = lines[j];
        int count = PF_BAD_LINE;                    // (also a candidate that is no line: the pair is never computed)
        if (!bad && (unsigned)a < (unsigned)e && (unsigned)b < (unsigned)e) {
            for (int l = t; l < e; l += nt) v.keep[l] = l != a && l != b;
            count = tp_unreached<ID>(v.from, v.to, v.keep, e, n, root, v.reached, &s_count);
        }
        if (t == 0) out[j - i - 1] = count;
    }
}

// ----------------------------------------------------------------------------------------------------------- DC
using CtArgs = CtCommon;

// (the scenario's vectors, ct_vec_bytes / ct_vecs, the workgroup-size and LDS-fit rules and PHASE A itself: contingency_base.hpp)

// (den_k and the post-outage flow of line l, ct_den and ct_post: contingency_line.hpp, shared with the sparse route)

template <bool LDS>
__global__ __launch_bounds__(PF_BIG_THREADS) void contingency_dc_kernel(const CtArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ct_smem[];
    const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6, nw = nt >> 6;
    const int s = blockIdx.x;
    const int n = a.n, e = a.e, m = n - 1, ld = pf_ld(m);
    const CtVecs v = ct_vecs(ct_smem, n, e, nw);
    const double* flow = v.flow;
    const float* x32 = v.x32;
    const float* rat = v.rat;
    float* wk = v.wk;
    const int* aidx = v.aidx;
    const uint16_t* la = v.la;
    const uint16_t* lb = v.lb;
    float* X;
    if constexpr (LDS) X = reinterpret_cast<float*>(ct_smem + ct_vec_bytes(n, e, nw));
    else X = static_cast<float*>(a.ws) + (size_t)s * pf_mat_floats(m);

    // ================================================================================================ PHASE A
    const int code = ct_base_solve(ct_base_in(a, s), v, X);

    // ================================================================================================ PHASE B
    float* w = wk + (size_t)wave * n;
    for (int k = wave; k < e; k += nw) {
        const int64_t o = (int64_t)s * e + k;
        float* row = a.post_flow ? a.post_flow + o * e : nullptr;
        if (code != 0 || a.islands[k] != 0) {       // a failed scenario, an islanding outage
            ct_skip(code != 0, row, e, lane, 64, a.severity[o], a.worst_line[o], a.overloads[o]);
            continue;
        }
        const int bi = la[k], bj = lb[k];
        ct_column<false>(w, X, ld, aidx, n, aidx[bi], aidx[bj], lane, 64);
        __syncwarp();                               // (the wave's own LDS vector: written by its lanes, gathered by its lanes)
        const float den = ct_den(w[bi], w[bj], x32[k]);
        const float fk = (float)flow[k];
        // ---- the lines: post-outage flow, loading; the wave's worst (contingency_monitor.hpp)
        CtWorst worst = ct_worst_none();
        for (int l = lane; l < e; l += 64) {
            const float post = l == k ? 0.f : ct_post(w[la[l]], w[lb[l]], x32[l], den, (float)flow[l], fk);
            if (row) row[l] = post;
            const float r = rat[l];
            if (l != k && r > 0.f) ct_worst_add(worst, l, ct_loading(post, r));
        }
        worst = ct_worst_wave(worst);
        if (lane == 0) ct_store(ct_figures(worst), a.severity[o], a.worst_line[o], a.overloads[o]);
        __syncwarp();                               // (the next outage overwrites the vector)
    }
}

// Both islands entries: their checks in their order, then the 16-bit-id or the 32-bit-id instantiation.  `pairs`: the N-2 entry,
// with its candidates.
static int ct_islands_entry(const char* who, bool pairs, const int64_t* edge_index, int64_t n_lines, int64_t n_bus, int64_t root,
                            const int32_t* lines, int64_t n_candidates, int32_t* islands, void* stream) {
    PFN_CHECK_ARG(n_bus >= 1 && n_lines >= 0 && n_lines < (1ll << 24) && n_bus < (1ll << 24), "%s: bad sizes (%lld buses and %lld lines)", who,
                  (long long)n_bus, (long long)n_lines);
    PFN_CHECK_ARG(!pairs || (n_candidates >= 0 && n_candidates <= n_lines), "%s: %lld candidates among %lld lines", who, (long long)n_candidates,
                  (long long)n_lines);
    PFN_CHECK_ARG(root >= 0 && root < n_bus, "%s: root %lld is outside [0, %lld)", who, (long long)root, (long long)n_bus);
    const int n = (int)n_bus, e = (int)n_lines, c = (int)n_candidates;
    const size_t bytes = ct_islands_lds_bytes(n, e);
    PFN_CHECK_ARG(bytes <= (size_t)(kLdsCuBytes - kLdsReserve), "%s: %d buses and %d lines need %zu bytes of LDS, %d are there", who, n, e, bytes,
                  kLdsCuBytes - kLdsReserve);
    if (pairs ? c < 2 : e == 0) return PFN_OK;
    PFN_CHECK_ARG(edge_index && islands && (lines || !pairs), "%s: null pointer", who);
    PFN_CHECK_ARG((reinterpret_cast<uintptr_t>(edge_index) & 7) == 0 && ((reinterpret_cast<uintptr_t>(islands) | reinterpret_cast<uintptr_t>(lines)) & 3) == 0,
                  "%s: edge_index must be 8-byte aligned, %sislands 4-byte", who, pairs ? "lines and " : "");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool id16 = n <= 65536;
    const int threads = tp_threads(n, e);
    if (pairs) {
        ProfScope ps("contingency_pair_islands", (double)(c - 1) * 16.0 * (double)e + 0.5 * (double)c * (double)(c - 1) * 4.0, 0.0, s);
        return launch_either<contingency_pair_islands_kernel<uint16_t>, contingency_pair_islands_kernel<uint32_t>>(
            id16, c - 1, threads, bytes, bytes, s, edge_index, n, e, (int)root, lines, c, islands);
    }
    ProfScope ps("contingency_islands", (double)n_lines * (16.0 * (double)n_lines + 4.0), 0.0, s);
    return launch_either<contingency_islands_kernel<uint16_t>, contingency_islands_kernel<uint32_t>>(id16, e, threads, bytes, bytes, s, edge_index, n, e,
                                                                                                    (int)root, islands);
}

}  // namespace pfn

using namespace pfn;

extern "C" {

int pfn_contingency_islands(const int64_t* edge_index, int64_t n_lines, int64_t n_bus, int64_t root, int32_t* islands, void* stream) {
    return ct_islands_entry("pfn_contingency_islands", false, edge_index, n_lines, n_bus, root, nullptr, 0, islands, stream);
}

int pfn_contingency_pair_islands(const int64_t* edge_index, int64_t n_lines, int64_t n_bus, int64_t root, const int32_t* lines,
                                 int64_t n_candidates, int32_t* islands, void* stream) {
    return ct_islands_entry("pfn_contingency_pair_islands", true, edge_index, n_lines, n_bus, root, lines, n_candidates, islands, stream);
}

size_t pfn_contingency_workspace_bytes(int64_t n_samples, int64_t n_bus, int64_t n_lines, int route) {
    if (n_samples <= 0 || n_bus < 2 || n_bus > PF_MAX_UNKNOWNS + 1 || n_lines < 0 || n_lines >= (1ll << 24)) return 0;
    if (route == 1 || (route != 2 && ct_fits_lds((int)n_bus, (int)n_lines))) return 0;
    return (size_t)n_samples * pf_mat_floats((int)n_bus - 1) * sizeof(float);
}

int pfn_contingency_dc(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                       const double* ratings, int ratings_per_sample, const int32_t* islands, int64_t n_samples, int64_t n_bus,
                       int64_t n_pv, int64_t n_pq, double tol, int max_iter, int route, float* severity, int32_t* worst_line,
                       int32_t* overloads, double* base_flow, int32_t* status, float* post_flow, int32_t* flags, void* ws,
                       size_t ws_bytes, void* stream) {
    const char* who = "pfn_contingency_dc";
    PFN_CHECK_ARG(n_samples >= 0 && n_bus >= 2 && n_lines >= 0 && n_samples < (1ll << 29) && n_lines < (1ll << 24) && n_bus < (1ll << 24),
                  "%s: bad sizes (%lld scenarios of %lld buses and %lld lines)", who, (long long)n_samples, (long long)n_bus, (long long)n_lines);
    PFN_CHECK_ARG(n_pv >= 0 && n_pq >= 0 && n_pv + n_pq == n_bus - 1, "%s: %lld PV and %lld PQ buses do not leave exactly one slack among %lld buses",
                  who, (long long)n_pv, (long long)n_pq, (long long)n_bus);
    PFN_CHECK_ARG(route >= 0 && route <= 2, "%s: route must be 0 (auto), 1 (LDS) or 2 (global)", who);
    PFN_CHECK_ARG(max_iter >= 0 && tol > 0.0, "%s: max_iter must be >= 0 and tol > 0", who);
    PFN_CHECK_ARG(n_bus - 1 <= PF_MAX_UNKNOWNS,
                  "%s: %lld unknowns per scenario exceed the dense screen's %d; the sparse route is not built", who, (long long)(n_bus - 1),
                  PF_MAX_UNKNOWNS);
    const int n = (int)n_bus, e = (int)n_lines, m = n - 1;
    const int threads = ct_threads(m);
    const size_t vec = ct_vec_bytes(n, e, threads >> 6);
    PFN_CHECK_ARG(vec <= (size_t)(kLdsCuBytes - kLdsReserve), "%s: the vectors of %d buses and %d lines need %zu bytes of LDS, %d are there", who, n, e,
                  vec, kLdsCuBytes - kLdsReserve);
    const bool fits = ct_fits_lds(n, e);
    PFN_CHECK_ARG(route != 1 || fits, "%s: route 1 (LDS): %d unknowns of %d buses and %d lines need %zu bytes of LDS, %d are there", who, m, n, e,
                  ct_lds_bytes(n, e), kLdsCuBytes - kLdsReserve);
    if (n_samples == 0 || n_lines == 0) return PFN_OK;
    PFN_CHECK_ARG(edge_index && rx && bus_type && spec && islands && severity && worst_line && overloads && base_flow && status && flags,
                  "%s: null pointer", who);
    const CtArgs a{edge_index, rx, bus_type, spec, ratings, islands, severity, worst_line, overloads, base_flow, status, post_flow, flags, ws, tol, n, e,
                   max_iter, (int)n_pv, (int)n_pq, ratings_per_sample != 0};
    PFN_TRY(ct_check_aligned(who, a, nullptr));
    const bool lds = route == 1 || (route == 0 && fits);
    if (!lds) {
        const size_t need = (size_t)n_samples * pf_mat_floats(m) * sizeof(float);
        if (!ws || ws_bytes < need) {
            set_error("%s: the global route needs a workspace of %zu bytes (got %zu)", who, need, ws ? ws_bytes : (size_t)0);
            return PFN_ENOSPACE;
        }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double mm = (double)m, ee = (double)e;
    ProfScope ps("contingency_dc", (double)n_samples * (ee * (16.0 + 8.0 + 12.0 + 8.0 + (post_flow ? 4.0 * ee : 0.0)) + (double)n * 32.0),
                 (double)n_samples * (2.0 * mm * mm * mm + 6.0 * mm * mm + ee * (2.0 * mm + 8.0 * ee)), s);
    return launch_either<contingency_dc_kernel<true>, contingency_dc_kernel<false>>(lds, (int)n_samples, threads, vec + pf_mat_floats(m) * 4, vec, s, a);
}

}  // extern "C"
