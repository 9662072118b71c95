// N-1 line-outage screening on the device (gfx950): which single line outages overload the rest of the grid?  Two launches.
//
// pfn_contingency_islands: one workgroup per outage k asks topology_reach.hpp's reach routine which buses the slack still reaches
// over the base list with line k skipped (a keep flag per line in LDS: no [e, 2, e - 1] lists exist anywhere).  islands[k] > 0 is a
// bridge; it is decided combinatorially, from the line list alone, never from a small denominator.
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
//   (two column walks of X: stride ld, odd, so conflict-free), then stride over the lines: phi, post-outage flow, loading
//   |f| / rating.  The wave reduces by max (ties to the lowest line) and by an integer sum; lane 0 writes severity, worst line and
//   overload count of (s, k); the full table row, where asked for, is written coalesced by the lanes.
// The per-line expression is compiled without contraction (as branch_flows.hip's), every cross-thread reduction is a max or an
// integer sum, one owner per output: a scenario's bits are a pure function of its own inputs, whatever the batch, the workgroup
// size or the route.  LDS route: X sits behind the scenario's vectors in LDS; global route: in a per-scenario slab of the caller's
// workspace, same code.  No host sync, no allocation (capturable), no float atomics.
#include "contingency_base.hpp"
#include "contingency_line.hpp"
#include "topology_reach.hpp"

namespace pfn {

// ------------------------------------------------------------------------------------------------------ islands
// dynamic LDS of one outage: ID from[e] | ID to[e] | uint8 keep[e] | uint8 reached[n]
__host__ __device__ inline size_t ct_islands_lds_bytes(int n, int e) {
    const size_t id = n <= 65536 ? 2 : 4;
    return tp_align4(2 * id * (size_t)e) + tp_align4((size_t)e) + tp_align4((size_t)n);
}

template <typename ID>
__global__ __launch_bounds__(1024) void contingency_islands_kernel(const int64_t* __restrict__ ei, int n, int e, int root,
                                                                   int32_t* __restrict__ islands) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ct_smem[];
    __shared__ int s_count;
    const int t = threadIdx.x, nt = blockDim.x;
    const int k = blockIdx.x;
    ID* from = reinterpret_cast<ID*>(ct_smem);
    ID* to = from + e;
    uint8_t* keep = ct_smem + tp_align4(2 * sizeof(ID) * (size_t)e);
    uint8_t* reached = keep + tp_align4((size_t)e);
    int count = PF_BAD_LINE;                        // (an id outside [0, n) is never followed: every outage reports it)
    if (!tp_bad_lines(ei, e, n)) {
        for (int j = t; j < e; j += nt) {           // (a thread stages and flags the lines it will walk: tp_unreached's ownership)
            from[j] = (ID)ei[j];
            to[j] = (ID)ei[e + j];
            keep[j] = j != k;
        }
        count = tp_unreached<ID>(from, to, keep, e, n, root, reached, &s_count);
    }
    if (t == 0) islands[k] = count;
}

// ----------------------------------------------------------------------------------------------------------- DC
struct CtArgs {
    const int64_t* edge_index;                      // [2, e], one list for all scenarios
    const double* rx;                               // [S, e, 2]
    const int32_t* bus_type;                        // [n]
    const double* spec;                             // [S, n, 4]
    const double* ratings;                          // [e], [S, e] or null (1.0 everywhere)
    const int32_t* islands;                         // [e], pfn_contingency_islands' output
    float* severity;                                // [S, e]
    int32_t* worst_line;                            // [S, e]
    int32_t* overloads;                             // [S, e]
    double* base_flow;                              // [S, e]
    int32_t* status;                                // [S]
    float* post_flow;                               // [S, e, e] or null
    int32_t* flags;
    void* ws;                                       // the global route's fp32 slabs or null
    double tol;
    int n, e, max_iter, n_pv, n_pq, ratings_per_sample;
};

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
    const CtBaseIn in{a.edge_index, a.rx + (int64_t)s * 2 * e, a.bus_type, a.spec + (int64_t)s * 4 * n,
                      a.ratings ? a.ratings + (a.ratings_per_sample ? (int64_t)s * e : 0) : nullptr, a.base_flow + (int64_t)s * e, a.status + s,
                      a.flags, a.tol, n, e, a.max_iter, a.n_pv, a.n_pq};
    const int code = ct_base_solve(in, v, X);

    // ================================================================================================ PHASE B
    const float nanv = __builtin_nanf(""), infv = __builtin_inff();
    float* w = wk + (size_t)wave * n;
    for (int k = wave; k < e; k += nw) {
        const int64_t o = (int64_t)s * e + k;
        float* row = a.post_flow ? a.post_flow + o * e : nullptr;
        // a failed scenario: NaN and -1; an islanding outage: +inf, so that it ranks first, -1, -1 and a NaN row
        if (code != 0 || a.islands[k] != 0) {
            if (row)
                for (int l = lane; l < e; l += 64) row[l] = nanv;
            if (lane == 0) {
                a.severity[o] = code ? nanv : infv;
                a.worst_line[o] = -1;
                a.overloads[o] = -1;
            }
            continue;
        }
        // ---- w_k = X[:, i] - X[:, j], zero at the slack; a column of X at the slack is zero
        const int bi = la[k], bj = lb[k], ci = aidx[bi], cj = aidx[bj];
        for (int b = lane; b < n; b += 64) {
            const int r = aidx[b];
            float v = 0.f;
            if (r >= 0) {
                const float xi = ci >= 0 ? X[r * ld + ci] : 0.f;
                const float xj = cj >= 0 ? X[r * ld + cj] : 0.f;
                v = xi - xj;
            }
            w[b] = v;
        }
        __syncwarp();                               // (the wave's own LDS vector: written by its lanes, gathered by its lanes)
        const float den = ct_den(w[bi], w[bj], x32[k]);
        const float fk = (float)flow[k];
        // ---- the lines: post-outage flow, loading; per lane the largest loading with the lowest line, and the overload count
        float best = -1.f;                          // (a loading is >= 0; a non-finite one counts as +inf and poisons the severity)
        int arg = 0x7fffffff, cnt = 0, wild = 0;
        for (int l = lane; l < e; l += 64) {
            const float post = l == k ? 0.f : ct_post(w[la[l]], w[lb[l]], x32[l], den, (float)flow[l], fk);
            if (row) row[l] = post;
            const float r = rat[l];
            if (l != k && r > 0.f) {                // (a rating that is not > 0 -- zero, negative, NaN -- is unmonitored)
                const float load = fabsf(post) / r;
                const bool finite = load < infv;
                const float key = finite ? load : infv;
                wild |= !finite;
                cnt += load > 1.f;
                if (key > best) { best = key; arg = l; }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ob = __shfl_xor(best, off);
            const int oa = __shfl_xor(arg, off);
            if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
            cnt += __shfl_xor(cnt, off);
            wild |= __shfl_xor(wild, off);
        }
        if (lane == 0) {
            const bool none = arg == 0x7fffffff;
            a.severity[o] = none ? 0.f : (wild ? nanv : best);
            a.worst_line[o] = none ? -1 : arg;
            a.overloads[o] = cnt;
        }
        __syncwarp();                               // (the next outage overwrites the vector)
    }
}

}  // namespace pfn

using namespace pfn;

extern "C" {

int pfn_contingency_islands(const int64_t* edge_index, int64_t n_lines, int64_t n_bus, int64_t root, int32_t* islands, void* stream) {
    PFN_CHECK_ARG(n_bus >= 1 && n_lines >= 0 && n_lines < (1ll << 24) && n_bus < (1ll << 24),
                  "pfn_contingency_islands: bad sizes (%lld buses and %lld lines)", (long long)n_bus, (long long)n_lines);
    PFN_CHECK_ARG(root >= 0 && root < n_bus, "pfn_contingency_islands: root %lld is outside [0, %lld)", (long long)root, (long long)n_bus);
    const int n = (int)n_bus, e = (int)n_lines;
    const size_t bytes = ct_islands_lds_bytes(n, e);
    PFN_CHECK_ARG(bytes <= (size_t)(kLdsCuBytes - kLdsReserve), "pfn_contingency_islands: %d buses and %d lines need %zu bytes of LDS, %d are there",
                  n, e, bytes, kLdsCuBytes - kLdsReserve);
    if (n_lines == 0) return PFN_OK;
    PFN_CHECK_ARG(edge_index && islands, "pfn_contingency_islands: null pointer");
    PFN_CHECK_ARG((reinterpret_cast<uintptr_t>(edge_index) & 7) == 0 && (reinterpret_cast<uintptr_t>(islands) & 3) == 0,
                  "pfn_contingency_islands: edge_index must be 8-byte aligned, islands 4-byte");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope ps("contingency_islands", (double)n_lines * (16.0 * (double)n_lines + 4.0), 0.0, s);
    static std::atomic<uint64_t> raised16{0}, raised32{0};
    if (n <= 65536) {
        PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(contingency_islands_kernel<uint16_t>), kLdsCuBytes - kLdsReserve, raised16));
        contingency_islands_kernel<uint16_t><<<e, tp_threads(n, e), bytes, s>>>(edge_index, n, e, (int)root, islands);
    } else {
        PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(contingency_islands_kernel<uint32_t>), kLdsCuBytes - kLdsReserve, raised32));
        contingency_islands_kernel<uint32_t><<<e, tp_threads(n, e), bytes, s>>>(edge_index, n, e, (int)root, islands);
    }
    PFN_CHECK_LAUNCH();
    return PFN_OK;
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
    PFN_CHECK_ARG(((reinterpret_cast<uintptr_t>(ws)) & 15) == 0 &&
                      ((reinterpret_cast<uintptr_t>(edge_index) | reinterpret_cast<uintptr_t>(rx) | reinterpret_cast<uintptr_t>(spec) |
                        reinterpret_cast<uintptr_t>(ratings) | reinterpret_cast<uintptr_t>(base_flow)) & 7) == 0 &&
                      ((reinterpret_cast<uintptr_t>(bus_type) | reinterpret_cast<uintptr_t>(islands) | reinterpret_cast<uintptr_t>(severity) |
                        reinterpret_cast<uintptr_t>(worst_line) | reinterpret_cast<uintptr_t>(overloads) | reinterpret_cast<uintptr_t>(status) |
                        reinterpret_cast<uintptr_t>(post_flow) | reinterpret_cast<uintptr_t>(flags)) & 3) == 0,
                  "%s: the workspace must be 16-byte aligned, fp64 and int64 arrays 8-byte, fp32 and int32 arrays 4-byte", who);
    const bool lds = route == 1 || (route == 0 && fits);
    if (!lds) {
        const size_t need = (size_t)n_samples * pf_mat_floats(m) * sizeof(float);
        if (!ws || ws_bytes < need) {
            set_error("%s: the global route needs a workspace of %zu bytes (got %zu)", who, need, ws ? ws_bytes : (size_t)0);
            return PFN_ENOSPACE;
        }
    }
    CtArgs a{edge_index, rx, bus_type, spec, ratings, islands, severity, worst_line, overloads, base_flow, status, post_flow, flags, ws, tol,
             n, e, max_iter, (int)n_pv, (int)n_pq, ratings_per_sample != 0};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double mm = (double)m, ee = (double)e;
    ProfScope ps("contingency_dc", (double)n_samples * (ee * (16.0 + 8.0 + 12.0 + 8.0 + (post_flow ? 4.0 * ee : 0.0)) + (double)n * 32.0),
                 (double)n_samples * (2.0 * mm * mm * mm + 6.0 * mm * mm + ee * (2.0 * mm + 8.0 * ee)), s);
    static std::atomic<uint64_t> raised{0};
    if (lds) {
        PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(contingency_dc_kernel<true>), kLdsCuBytes - kLdsReserve, raised));
        contingency_dc_kernel<true><<<(int)n_samples, threads, vec + pf_mat_floats(m) * 4, s>>>(a);
    } else {
        static std::atomic<uint64_t> raised_g{0};
        PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(contingency_dc_kernel<false>), kLdsCuBytes - kLdsReserve, raised_g));
        contingency_dc_kernel<false><<<(int)n_samples, threads, vec, s>>>(a);
    }
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

}  // extern "C"
