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
//   PHASE A, the whole workgroup, once: the lines are staged in LDS, B' is built in fp32 (row-major, ld = m | 1, m = n - 1) by the
//   row owners in stored order exactly as the fast-decoupled modes build theirs and inverted in place by THEIR Gauss-Jordan
//   (powerflow_dense.hpp); theta is refined, theta -= X F, under the fp64 residual F = B' theta + P of mode 1 to tol / max_iter
//   (status = the refinement solves used); the base flows f_l = (theta_a - theta_b) / x_l are fp64.
//   PHASE B, no workgroup barrier: wave w takes the outages w, w + nw, ...  Its lanes form w_k into the wave's own fp32 vector [n]
//   (two column walks of X: stride ld, odd, so conflict-free), then stride over the lines: phi, post-outage flow, loading
//   |f| / rating.  The wave reduces by max (ties to the lowest line) and by an integer sum; lane 0 writes severity, worst line and
//   overload count of (s, k); the full table row, where asked for, is written coalesced by the lanes.
// The per-line expression is compiled without contraction (as branch_flows.hip's), every cross-thread reduction is a max or an
// integer sum, one owner per output: a scenario's bits are a pure function of its own inputs, whatever the batch, the workgroup
// size or the route.  LDS route: X sits behind the scenario's vectors in LDS; global route: in a per-scenario slab of the caller's
// workspace, same code.  No host sync, no allocation (capturable), no float atomics.
#include "contingency_line.hpp"
#include "powerflow_dense.hpp"
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

// the scenario's vectors: double th [n], F [m], flow [e], bl [e]; float x32 [e], rat [e], wk [nw][n]; int aidx [n];
// uint16 la [e], lb [e] (n <= PF_MAX_UNKNOWNS + 1); rounded to 16 bytes
__host__ __device__ inline size_t ct_vec_bytes(int n, int e, int nw) {
    return ((size_t)8 * ((size_t)n + (n - 1) + 2 * (size_t)e) + (size_t)4 * (2 * (size_t)e + (size_t)nw * n + n) + (size_t)4 * e + 15) & ~(size_t)15;
}
static inline int ct_threads(int m) { return m > PF_BIG_M ? PF_BIG_THREADS : PF_SMALL_THREADS; }
static inline size_t ct_lds_bytes(int n, int e) { return ct_vec_bytes(n, e, ct_threads(n - 1) >> 6) + pf_mat_floats(n - 1) * 4; }
static inline bool ct_fits_lds(int n, int e) { return ct_lds_bytes(n, e) <= (size_t)(kLdsCuBytes - kLdsReserve); }

// (den_k and the post-outage flow of line l, ct_den and ct_post: contingency_line.hpp, shared with the sparse route)

template <bool LDS>
__global__ __launch_bounds__(PF_BIG_THREADS) void contingency_dc_kernel(const CtArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ct_smem[];
    __shared__ double s_red[16];
    __shared__ int s_ok, s_slack;
    const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6, nw = nt >> 6;
    const int s = blockIdx.x;
    const int n = a.n, e = a.e, m = n - 1, ld = pf_ld(m);
    double* th = reinterpret_cast<double*>(ct_smem);
    double* F = th + n;
    double* flow = F + m;
    double* bl = flow + e;                          // -1 / x_l, the DC end's b
    float* x32 = reinterpret_cast<float*>(bl + e);
    float* rat = x32 + e;
    float* wk = rat + e;
    int* aidx = reinterpret_cast<int*>(wk + (size_t)nw * n);
    uint16_t* la = reinterpret_cast<uint16_t*>(aidx + n);
    uint16_t* lb = la + e;
    float* X;
    if constexpr (LDS) X = reinterpret_cast<float*>(ct_smem + ct_vec_bytes(n, e, nw));
    else X = static_cast<float*>(a.ws) + (size_t)s * pf_mat_floats(m);
    const int64_t* ei = a.edge_index;
    const double* rx = a.rx + (int64_t)s * 2 * e;
    const double* spec = a.spec + (int64_t)s * 4 * n;
    const double* rat_in = a.ratings ? a.ratings + (a.ratings_per_sample ? (int64_t)s * e : 0) : nullptr;
    int code = 0;                                   // (uniform over the workgroup wherever it is tested)

    // ---- the lines name buses of the grid?  (an id outside [0, n) is never followed)
    int bad = 0;
    for (int k = t; k < e; k += nt) bad |= (uint64_t)ei[k] >= (uint64_t)n || (uint64_t)ei[e + k] >= (uint64_t)n;
    // ---- unknown numbering; the host's n_pv / n_pq against the device bus types, as the solver does
    if (t == 0) {
        int na = 0, ns = 0, npv = 0, npq = 0, odd = 0, slack = 0;
        for (int i = 0; i < n; ++i) {
            const int ty = a.bus_type[i];
            int ia = -1;
            if (ty == 0) { ++ns; slack = i; }
            else if (ty == 1) { ++npv; ia = na++; }
            else if (ty == 2) { ++npq; ia = na++; }
            else odd = 1;
            aidx[i] = ia;
        }
        s_slack = slack;
        s_ok = !odd && ns == 1 && npv == a.n_pv && npq == a.n_pq;
    }
    bad = __syncthreads_or(bad);
    if (!s_ok) {
        code = PF_BAD_TYPES;
        if (t == 0) a.flags[0] = a.flags[0] | 1;    // (every writer stores the same bit over the same word)
    } else if (bad) {
        code = PF_BAD_LINE;
    }

    // ================================================================================================ PHASE A
    int it = 0;
    if (code == 0) {
        const double th0 = spec[4 * s_slack + 1] * PF_RAD;
        for (int k = t; k < e; k += nt) {
            const double x = rx[2 * k + 1];
            la[k] = (uint16_t)ei[k];
            lb[k] = (uint16_t)ei[e + k];
            bl[k] = -1.0 / x;
            x32[k] = (float)x;
            rat[k] = rat_in ? (float)rat_in[k] : 1.f;
        }
        for (int i = t; i < n; i += nt) th[i] = th0;
        __syncthreads();
        for (;; ++it) {
            // ---- F = B' theta + P at the non-slack buses: bus i's lines in stored order, the stored direction, then the reverse
            for (int i = t; i < n; i += nt) {
                const int ra = aidx[i];
                if (ra < 0) continue;
                const double ti = th[i];
                double sP = 0.0;
                for (int k = 0; k < e; ++k) {
                    const int ka = la[k], kb = lb[k];
                    if (ka != i && kb != i) continue;
                    const double b = bl[k];
                    if (ka == i) sP += b * (ti - th[kb]);
                    if (kb == i) sP += b * (ti - th[ka]);
                }
                F[ra] = spec[4 * i + 2] - sP;
            }
            __syncthreads();
            double mx = 0.0;
            for (int k = t; k < m; k += nt) mx = fmax(mx, pf_abs_clamped(F[k]));
            const double res = pf_block_max(mx, s_red, nw);
            const int stop = pf_stop(res, a.tol, it, a.max_iter);
            if (stop < 0) { code = stop; break; }
            if (it == 0) {
                // ---- B', once: the Laplacian of 1 / x over the stored lines (parallel lines add, a self-loop cancels), bus i's row
                //      by bus i in stored order, the diagonal summed in fp64 and added last; then inverted in place.  A scenario
                //      that starts converged still needs X: the outages do.
                for (int k = t; k < (int)pf_mat_floats(m); k += nt) X[k] = 0.f;
                __syncthreads();
                for (int i = t; i < n; i += nt) {
                    const int ra = aidx[i];
                    if (ra < 0) continue;
                    double dp = 0.0;
                    for (int k = 0; k < e; ++k) {
                        const int ka = la[k], kb = lb[k];
                        if (ka != i && kb != i) continue;
                        const double w = -bl[k];
#pragma unroll 1
                        for (int side = 0; side < 2; ++side) {
                            if ((side ? kb : ka) != i) continue;
                            const int ca = aidx[side ? ka : kb];
                            dp += w;
                            if (ca >= 0) X[ra * ld + ca] += (float)(-w);
                        }
                    }
                    X[ra * ld + ra] += (float)dp;
                }
                __syncthreads();
                if (!pf_invert_in_place(X, m, ld)) { code = PF_SINGULAR; break; }
            }
            if (stop) break;
            // ---- theta -= X F: a row by its owner, fp64 sum in column order
            for (int i = t; i < n; i += nt) {
                const int r = aidx[i];
                if (r < 0) continue;
                const float* row = X + r * ld;
                double acc = 0.0;
                for (int c = 0; c < m; ++c) acc += (double)row[c] * F[c];
                th[i] -= acc;
            }
            __syncthreads();
        }
    }
    // ---- the base flows (fp64) and the scenario's status
    double* bf = a.base_flow + (int64_t)s * e;
    for (int k = t; k < e; k += nt) {
        double f = __builtin_nan("");
        if (code == 0) {
            f = (th[la[k]] - th[lb[k]]) / rx[2 * k + 1];
            flow[k] = f;
        }
        bf[k] = f;
    }
    if (t == 0) a.status[s] = code ? code : it;
    __syncthreads();

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
