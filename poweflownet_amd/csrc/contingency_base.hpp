// The base solve of the dense contingency screens, spelled once: PHASE A of contingency.hip's N-1 kernel and the base launch of
// contingency_pairs.hip's N-2 screen are this one routine -- the type check, the staging of the lines in LDS, B' in fp32 (row-major,
// ld = m | 1, m = n - 1) by the row owners in stored order exactly as the fast-decoupled modes build theirs, THEIR Gauss-Jordan in
// place (powerflow_dense.hpp), theta refined, theta -= X F, under the fp64 residual F = B' theta + P of mode 1 to tol / max_iter
// (status = the refinement solves used), the fp64 base flows f_l = (theta_a - theta_b) / x_l and the scenario's status.  A scenario's
// base flows and status are the same bits from either kernel.  Beside it, what else the two dense screens share: the entries' common
// argument block (CtCommon, with the CtBaseIn of a scenario and the pointer-alignment check) and the sensitivity column
// w = X[:, i] - X[:, j] (ct_column, row-major or transposed storage).
#pragma once
#include "powerflow_dense.hpp"

namespace pfn {

// the scenario's vectors: double th [n], F [m], flow [e], bl [e]; float x32 [e], rat [e], wk [nw][n]; int aidx [n];
// uint16 la [e], lb [e] (n <= PF_MAX_UNKNOWNS + 1); rounded to 16 bytes
__host__ __device__ inline size_t ct_vec_bytes(int n, int e, int nw) {
    return ((size_t)8 * ((size_t)n + (n - 1) + 2 * (size_t)e) + (size_t)4 * (2 * (size_t)e + (size_t)nw * n + n) + (size_t)4 * e + 15) & ~(size_t)15;
}
static inline int ct_threads(int m) { return m > PF_BIG_M ? PF_BIG_THREADS : PF_SMALL_THREADS; }
static inline size_t ct_lds_bytes(int n, int e) { return ct_vec_bytes(n, e, ct_threads(n - 1) >> 6) + pf_mat_floats(n - 1) * 4; }
static inline bool ct_fits_lds(int n, int e) { return ct_lds_bytes(n, e) <= (size_t)(kLdsCuBytes - kLdsReserve); }

// the vectors of ct_vec_bytes in a workgroup's dynamic LDS, `nw` per-wave vectors wk between rat and aidx
struct CtVecs {
    double* th;
    double* F;
    double* flow;
    double* bl;                                     // -1 / x_l, the DC end's b
    float* x32;
    float* rat;
    float* wk;
    int* aidx;
    uint16_t* la;
    uint16_t* lb;
};
__device__ __forceinline__ CtVecs ct_vecs(unsigned char* smem, int n, int e, int nw) {
    CtVecs v;
    v.th = reinterpret_cast<double*>(smem);
    v.F = v.th + n;
    v.flow = v.F + (n - 1);
    v.bl = v.flow + e;
    v.x32 = reinterpret_cast<float*>(v.bl + e);
    v.rat = v.x32 + e;
    v.wk = v.rat + e;
    v.aidx = reinterpret_cast<int*>(v.wk + (size_t)nw * n);
    v.la = reinterpret_cast<uint16_t*>(v.aidx + n);
    v.lb = v.la + e;
    return v;
}

// one scenario's inputs and per-scenario outputs
struct CtBaseIn {
    const int64_t* ei;                              // [2, e], one list for all scenarios
    const double* rx;                               // [e, 2] of the scenario
    const int32_t* bus_type;                        // [n]
    const double* spec;                             // [n, 4] of the scenario
    const double* rat_in;                           // [e] of the scenario or null (1.0 everywhere)
    double* base_flow;                              // [e] of the scenario
    int32_t* status;                                // the scenario's word
    int32_t* flags;
    double tol;
    int n, e, max_iter, n_pv, n_pq;
};

// What the two dense entries take alike (pfn_contingency_dc: items = outages; pfn_contingency_pairs: items = pairs).  It IS the N-1
// kernel's argument block; the pair kernels' block (contingency_pairs.hip CpArgs) repeats these names with its own fields among them
// in the order it has always had -- the order of a kernel's arguments decides which of them the base solve keeps in scalar registers,
// and the pair base launch measured 1.5 to 3 % slower with its fields moved behind a shared prefix --, so the two helpers below
// take either block by its field names.
struct CtCommon {
    const int64_t* edge_index;                      // [2, e], one list for all scenarios
    const double* rx;                               // [S, e, 2]
    const int32_t* bus_type;                        // [n]
    const double* spec;                             // [S, n, 4]
    const double* ratings;                          // [e], [S, e] or null (1.0 everywhere)
    const int32_t* islands;                         // [items], the islands launch's output
    float* severity;                                // [S, items]
    int32_t* worst_line;                            // [S, items]
    int32_t* overloads;                             // [S, items]
    double* base_flow;                              // [S, e]
    int32_t* status;                                // [S]
    float* post_flow;                               // [S, items, e] or null
    int32_t* flags;
    void* ws;                                       // the global route's fp32 slabs or null
    double tol;
    int n, e, max_iter, n_pv, n_pq, ratings_per_sample;
};
template <typename Args>
__device__ __forceinline__ CtBaseIn ct_base_in(const Args& a, int s) {
    return CtBaseIn{a.edge_index, a.rx + (int64_t)s * 2 * a.e, a.bus_type, a.spec + (int64_t)s * 4 * a.n,
                    a.ratings ? a.ratings + (a.ratings_per_sample ? (int64_t)s * a.e : 0) : nullptr, a.base_flow + (int64_t)s * a.e, a.status + s,
                    a.flags, a.tol, a.n, a.e, a.max_iter, a.n_pv, a.n_pq};
}
// the alignment of their pointers (null is aligned: ratings, post_flow, the N-1 entry's lines)
template <typename Args>
static inline int ct_check_aligned(const char* who, const Args& a, const int32_t* lines) {
    const auto at = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    PFN_CHECK_ARG((at(a.ws) & 15) == 0 && ((at(a.edge_index) | at(a.rx) | at(a.spec) | at(a.ratings) | at(a.base_flow)) & 7) == 0 &&
                      ((at(a.bus_type) | at(a.islands) | at(a.severity) | at(a.worst_line) | at(a.overloads) | at(a.status) | at(a.post_flow) |
                        at(a.flags) | at(lines)) & 3) == 0,
                  "%s: the workspace must be 16-byte aligned, fp64 and int64 arrays 8-byte, fp32 and int32 arrays 4-byte", who);
    return PFN_OK;
}

// w = X[:, i] - X[:, j], the sensitivity column of the outage of a line whose ends have the unknowns ci and cj (-1: the slack, whose
// column of X is zero), by the threads first, first + step, ... into w [n], zero at the slack.  TRANSPOSED: the matrix is kept as
// XT[c * ld + r] = X[r][c] (the pair screen's slab) -- a template flag, so that the compiler sees the one address expression.
template <bool TRANSPOSED>
__device__ __forceinline__ void ct_column(float* w, const float* X, int ld, const int* aidx, int n, int ci, int cj, int first, int step) {
    for (int b = first; b < n; b += step) {
        const int r = aidx[b];
        float v = 0.f;
        if (r >= 0) {
            const float xi = ci >= 0 ? (TRANSPOSED ? X[ci * ld + r] : X[r * ld + ci]) : 0.f;
            const float xj = cj >= 0 ? (TRANSPOSED ? X[cj * ld + r] : X[r * ld + cj]) : 0.f;
            v = xi - xj;
        }
        w[b] = v;
    }
}

// Every thread of the workgroup calls it with the same arguments.  Returns the scenario's code (0, or the negative status), uniform;
// on 0 the vectors hold the staged lines, the unknown numbering, theta and the fp64 base flows, and X (mm x mm, ld = m | 1; LDS or
// global) holds B'^-1.  Ends behind a barrier.
__device__ __forceinline__ int ct_base_solve(const CtBaseIn& a, const CtVecs& v, float* X) {
    __shared__ double s_red[16];
    __shared__ int s_ok, s_slack;
    const int t = threadIdx.x, nt = blockDim.x, nw = nt >> 6;
    const int n = a.n, e = a.e, m = n - 1, ld = pf_ld(m);
    double* th = v.th;
    double* F = v.F;
    double* flow = v.flow;
    double* bl = v.bl;
    float* x32 = v.x32;
    float* rat = v.rat;
    int* aidx = v.aidx;
    uint16_t* la = v.la;
    uint16_t* lb = v.lb;
    const int64_t* ei = a.ei;
    const double* rx = a.rx;
    const double* spec = a.spec;
    const double* rat_in = a.rat_in;
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
    for (int k = t; k < e; k += nt) {
        double f = __builtin_nan("");
        if (code == 0) {
            f = (th[la[k]] - th[lb[k]]) / rx[2 * k + 1];
            flow[k] = f;
        }
        a.base_flow[k] = f;
    }
    if (t == 0) a.status[0] = code ? code : it;
    __syncthreads();
    return code;
}

}  // namespace pfn
