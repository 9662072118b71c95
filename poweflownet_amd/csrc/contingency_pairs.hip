// N-2 line-pair outage screening on the dense DC route (gfx950): which PAIRS of line outages overload the rest of the grid?  The
// pairs are those of `c` candidate lines (strictly increasing ids): pair p = (lines[i], lines[j]), i < j, row-major in (i, j),
// P = c (c - 1) / 2; all e lines stay monitored.  Three launches.
//
// pfn_contingency_pair_islands (contingency.hip, beside the N-1 islands kernel whose LDS layout, staging and entry checks it shares):
// one workgroup per first candidate i loops over the second candidates j > i and asks topology_reach.hpp's reach routine which buses
// the slack still reaches with BOTH lines skipped (two keep flags cleared in LDS: no [P, 2, e - 2] lists exist anywhere).
// islands[p] > 0 is an islanding pair -- also where neither line is a bridge; it is decided combinatorially, from the line list
// alone, never from a small determinant.
//
// pfn_contingency_pairs, two kernels.  With X = B'^-1 (zeros at the slack), w_k and phi_{l,k} as in contingency.hip:
//     M = [[1 - phi_aa, -phi_ab], [-phi_ba, 1 - phi_bb]]      t = M^-1 (f_a, f_b)
//     f_l^(a,b) = f_l + phi_la t_a + phi_lb t_b   (l != a, b),   f_a^(a,b) = f_b^(a,b) = 0
// -- a rank-2 update of the one inverse per scenario, where the brute-force path factorises P matrices.
//   BASE, one workgroup per scenario: contingency_base.hpp's ct_base_solve, the N-1 kernel's PHASE A (the same base flows and status,
//   bit for bit), with X in LDS where the N-1 screen would keep it there, else in the scenario's slab.  It leaves in the slab
//   XT = X TRANSPOSED (XT[c * ld + r] = X[r][c]: the column walk that forms w_k becomes a row walk, coalesced from global memory and
//   free of bank conflicts from LDS; the element read is X[r][c], the N-1 kernel's -- the fp32 inverse is not bitwise symmetric) and
//   behind it the staged per-line vectors: float f [e] (the fp64 base flows rounded once), x [e], rating [e]; int aidx [n];
//   uint16 la [e], lb [e].
//   PAIRS, one workgroup per (scenario, first candidate i), so that a single scenario still fills the machine: the vectors come from
//   the slab, XT too where it fits LDS beside them (full-width loads; "lds") -- else it is read from the slab ("global"), same code,
//   same bits.  The workgroup forms w_a once; wave w takes the second candidates i + 1 + w, i + 1 + w + nw, ...: w_b into the wave's
//   own vector (both by contingency_base.hpp's ct_column), the four phi of M, t by Cramer's rule, then the lanes stride over the
//   lines: post-pair flow, loading |f| / rating.  The wave reduces and lane 0 writes severity, worst line and overload count of
//   (s, p) by the one tail of all screens (contingency_monitor.hpp); the table row, where asked for, is written coalesced by the lanes.
// The per-line and 2 x 2 arithmetic is contingency_line.hpp's ct_pair_*, compiled without contraction; every cross-thread reduction
// is a max or an integer sum, one owner per output: the bits of (scenario, a, b) are a pure function of the scenario's inputs and
// the two lines, whatever the batch, the candidate list, the workgroup size or count, or the route.  No host sync, no allocation
// (capturable), no float atomics.
#include "contingency_base.hpp"
#include "contingency_line.hpp"
#include "contingency_monitor.hpp"

namespace pfn {

// ------------------------------------------------------------------------------------------------------------ DC
struct CpArgs {                                     // (contingency_base.hpp CtCommon's names, and the pair screen's own among them)
    const int64_t* edge_index;                      // [2, e], one list for all scenarios
    const double* rx;                               // [S, e, 2]
    const int32_t* bus_type;                        // [n]
    const double* spec;                             // [S, n, 4]
    const double* ratings;                          // [e], [S, e] or null (1.0 everywhere)
    const int32_t* lines;                           // [c] candidates
    const int32_t* islands;                         // [P], pfn_contingency_pair_islands' output
    float* severity;                                // [S, P]
    int32_t* worst_line;                            // [S, P]
    int32_t* overloads;                             // [S, P]
    double* base_flow;                              // [S, e]
    int32_t* status;                                // [S]
    float* post_flow;                               // [S, P, e] or null
    int32_t* flags;
    unsigned char* ws;                              // the scenarios' slabs
    double tol;
    size_t slab;                                    // bytes per scenario
    int64_t P;
    int n, e, c, max_iter, n_pv, n_pq, ratings_per_sample;
};

// a scenario's slab: XT | float f [e], x [e], rating [e] | int aidx [n] | uint16 la [e], lb [e]; rounded to 16 bytes
__host__ __device__ inline size_t cp_staged_bytes(int n, int e) { return (size_t)16 * e + (size_t)4 * n; }
__host__ __device__ inline size_t cp_slab_bytes(int n, int e) { return (pf_mat_floats(n - 1) * 4 + cp_staged_bytes(n, e) + 15) & ~(size_t)15; }
// the pair kernel's vectors in LDS: the staged ones | float wa [n] | float wb [nw][n]; rounded to 16 bytes; XT behind them ("lds")
__host__ __device__ inline size_t cp_vec_bytes(int n, int e, int nw) { return (cp_staged_bytes(n, e) + (size_t)4 * n * (1 + nw) + 15) & ~(size_t)15; }
static inline size_t cp_lds_bytes(int n, int e) { return cp_vec_bytes(n, e, ct_threads(n - 1) >> 6) + pf_mat_floats(n - 1) * 4; }
static inline bool cp_fits_lds(int n, int e) { return cp_lds_bytes(n, e) <= (size_t)(kLdsCuBytes - kLdsReserve); }

template <bool LDS>
__global__ __launch_bounds__(PF_BIG_THREADS) void contingency_pairs_base_kernel(const CpArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cp_smem[];
    const int t = threadIdx.x, nt = blockDim.x;
    const int s = blockIdx.x;
    const int n = a.n, e = a.e, m = n - 1, ld = pf_ld(m);
    const CtVecs v = ct_vecs(cp_smem, n, e, 0);
    unsigned char* slab = a.ws + (size_t)s * a.slab;
    float* XT = reinterpret_cast<float*>(slab);
    float* X;
    if constexpr (LDS) X = reinterpret_cast<float*>(cp_smem + ct_vec_bytes(n, e, 0));
    else X = XT;
    if (ct_base_solve(ct_base_in(a, s), v, X) != 0) return;   // (a failed scenario's slab is never read)
    // ---- the staged vectors, for the pair launch
    float* f32 = XT + pf_mat_floats(m);
    float* x32 = f32 + e;
    float* rat = x32 + e;
    int* aidx = reinterpret_cast<int*>(rat + e);
    uint16_t* la = reinterpret_cast<uint16_t*>(aidx + n);
    uint16_t* lb = la + e;
    for (int k = t; k < e; k += nt) {
        f32[k] = (float)v.flow[k];
        x32[k] = v.x32[k];
        rat[k] = v.rat[k];
        la[k] = v.la[k];
        lb[k] = v.lb[k];
    }
    for (int i = t; i < n; i += nt) aidx[i] = v.aidx[i];
    // ---- XT[c][r] = X[r][c]
    if constexpr (LDS) {
        const int total = (int)pf_mat_floats(m);
        for (int k = t; k < total; k += nt) {       // (consecutive lanes: consecutive r -- LDS stride ld, odd; global stride 1)
            const int c = k / ld, r = k - c * ld;
            XT[k] = c < m && r < m ? X[r * ld + c] : 0.f;
        }
    } else {
        for (int k = t; k < m * m; k += nt) {       // in place: a pair of elements by one owner (the padding stays zero)
            const int r = k / m, c = k - r * m;
            if (r < c) {
                const float u = X[r * ld + c];
                X[r * ld + c] = X[c * ld + r];
                X[c * ld + r] = u;
            }
        }
    }
}

template <bool LDS>
__global__ __launch_bounds__(PF_BIG_THREADS) void contingency_pairs_kernel(const CpArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cp_smem[];
    const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6, nw = nt >> 6;
    const int n = a.n, e = a.e, c = a.c, m = n - 1, ld = pf_ld(m);
    const int s = blockIdx.x / (c - 1), i = blockIdx.x - s * (c - 1);
    const unsigned char* slab = a.ws + (size_t)s * a.slab;
    float* f32 = reinterpret_cast<float*>(cp_smem);
    float* x32 = f32 + e;
    float* rat = x32 + e;
    int* aidx = reinterpret_cast<int*>(rat + e);
    uint16_t* la = reinterpret_cast<uint16_t*>(aidx + n);
    uint16_t* lb = la + e;
    float* wa = reinterpret_cast<float*>(cp_smem + cp_staged_bytes(n, e));
    float* wb = wa + n + (size_t)wave * n;
    const float* XT = reinterpret_cast<const float*>(slab);
    const int failed = a.status[s] < 0;             // (uniform: the base launch's word)
    const int la_id = a.lines[i];
    const bool a_ok = (unsigned)la_id < (unsigned)e;   // (a candidate that is no line: its pairs carry islands -4 and are never computed)
    if (!failed && a_ok) {
        // ---- the staged vectors, and XT where it fits
        const uint32_t* src = reinterpret_cast<const uint32_t*>(XT + pf_mat_floats(m));
        uint32_t* dst = reinterpret_cast<uint32_t*>(cp_smem);
        const int words = (int)(cp_staged_bytes(n, e) >> 2);
        for (int k = t; k < words; k += nt) dst[k] = src[k];
        if constexpr (LDS) {
            float4* xl = reinterpret_cast<float4*>(cp_smem + cp_vec_bytes(n, e, nw));
            const float4* xg = reinterpret_cast<const float4*>(XT);
            const int quads = (int)(pf_mat_floats(m) >> 2);
            for (int k = t; k < quads; k += nt) xl[k] = xg[k];
            XT = reinterpret_cast<const float*>(xl);
        }
        __syncthreads();
        ct_column<true>(wa, XT, ld, aidx, n, aidx[la[la_id]], aidx[lb[la_id]], t, nt);   // w_a, once per workgroup
        __syncthreads();
    }

    const int64_t p0 = cp_first_pair(i, c);
    for (int j = i + 1 + wave; j < c; j += nw) {
        const int64_t p = p0 + (j - i - 1);
        const int64_t o = (int64_t)s * a.P + p;
        float* row = a.post_flow ? a.post_flow + o * e : nullptr;
        const int lb_id = a.lines[j];
        if (failed || !a_ok || (unsigned)lb_id >= (unsigned)e || a.islands[p] != 0) {   // a failed scenario, an islanding pair
            ct_skip(failed, row, e, lane, 64, a.severity[o], a.worst_line[o], a.overloads[o]);
            continue;
        }
        ct_column<true>(wb, XT, ld, aidx, n, aidx[la[lb_id]], aidx[lb[lb_id]], lane, 64);   // w_b, into the wave's own vector
        __syncwarp();                               // (the wave's own LDS vector: written by its lanes, gathered by its lanes)
        const int aa = la[la_id], ab = lb[la_id], ba = la[lb_id], bb = lb[lb_id];
        const float xa = x32[la_id], xb = x32[lb_id];
        float ta, tb;
        ct_pair_solve(ct_pair_phi(wa[aa], wa[ab], xa), ct_pair_phi(wb[aa], wb[ab], xa), ct_pair_phi(wa[ba], wa[bb], xb),
                      ct_pair_phi(wb[ba], wb[bb], xb), f32[la_id], f32[lb_id], &ta, &tb);
        // ---- the lines: post-pair flow, loading; the wave's worst (contingency_monitor.hpp)
        CtWorst worst = ct_worst_none();
        for (int l = lane; l < e; l += 64) {
            const bool out = l == la_id || l == lb_id;
            const int fa = la[l], fb = lb[l];
            const float post = out ? 0.f : ct_pair_post(ct_pair_phi(wa[fa], wa[fb], x32[l]), ct_pair_phi(wb[fa], wb[fb], x32[l]), f32[l], ta, tb);
            if (row) row[l] = post;
            const float r = rat[l];
            if (!out && r > 0.f) ct_worst_add(worst, l, ct_loading(post, r));
        }
        worst = ct_worst_wave(worst);
        if (lane == 0) ct_store(ct_figures(worst), a.severity[o], a.worst_line[o], a.overloads[o]);
        __syncwarp();                               // (the next pair overwrites the vector)
    }
}

static bool cp_sizes_ok(int64_t S, int64_t n, int64_t e, int64_t c) {
    return S >= 0 && n >= 2 && e >= 0 && c >= 0 && S < (1ll << 29) && e < (1ll << 24) && n < (1ll << 24) && c <= e &&
           (c < 2 || S * (c - 1) < (1ll << 31));
}

}  // namespace pfn

using namespace pfn;

extern "C" {

size_t pfn_contingency_pairs_workspace_bytes(int64_t n_samples, int64_t n_bus, int64_t n_lines, int64_t n_candidates, int route) {
    if (n_samples <= 0 || !cp_sizes_ok(n_samples, n_bus, n_lines, n_candidates) || n_bus > PF_MAX_UNKNOWNS + 1 || route < 0 || route > 2) return 0;
    const int n = (int)n_bus, e = (int)n_lines;
    if (ct_vec_bytes(n, e, 0) > (size_t)(kLdsCuBytes - kLdsReserve) || cp_vec_bytes(n, e, ct_threads(n - 1) >> 6) > (size_t)(kLdsCuBytes - kLdsReserve))
        return 0;
    if (route == 1 && !cp_fits_lds(n, e)) return 0;
    return (size_t)n_samples * cp_slab_bytes(n, e);
}

int pfn_contingency_pairs(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                          const double* ratings, int ratings_per_sample, const int32_t* lines, int64_t n_candidates,
                          const int32_t* islands, int64_t n_samples, int64_t n_bus, int64_t n_pv, int64_t n_pq, double tol, int max_iter,
                          int route, float* severity, int32_t* worst_line, int32_t* overloads, double* base_flow, int32_t* status,
                          float* post_flow, int32_t* flags, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "pfn_contingency_pairs";
    PFN_CHECK_ARG(cp_sizes_ok(n_samples, n_bus, n_lines, n_candidates), "%s: bad sizes (%lld scenarios of %lld buses and %lld lines, %lld candidates)",
                  who, (long long)n_samples, (long long)n_bus, (long long)n_lines, (long long)n_candidates);
    PFN_CHECK_ARG(n_pv >= 0 && n_pq >= 0 && n_pv + n_pq == n_bus - 1, "%s: %lld PV and %lld PQ buses do not leave exactly one slack among %lld buses",
                  who, (long long)n_pv, (long long)n_pq, (long long)n_bus);
    PFN_CHECK_ARG(route >= 0 && route <= 2, "%s: route must be 0 (auto), 1 (LDS) or 2 (global)", who);
    PFN_CHECK_ARG(max_iter >= 0 && tol > 0.0, "%s: max_iter must be >= 0 and tol > 0", who);
    PFN_CHECK_ARG(n_bus - 1 <= PF_MAX_UNKNOWNS, "%s: %lld unknowns per scenario exceed the dense screen's %d; pfn_contingency_pairs_sparse goes beyond it", who,
                  (long long)(n_bus - 1), PF_MAX_UNKNOWNS);
    const int n = (int)n_bus, e = (int)n_lines, c = (int)n_candidates, m = n - 1;
    const int threads = ct_threads(m), nw = threads >> 6;
    const size_t lds_max = (size_t)(kLdsCuBytes - kLdsReserve);
    const size_t vec_base = ct_vec_bytes(n, e, 0), vec = cp_vec_bytes(n, e, nw), mat = pf_mat_floats(m) * 4;
    PFN_CHECK_ARG(vec_base <= lds_max && vec <= lds_max, "%s: the vectors of %d buses and %d lines need %zu bytes of LDS, %zu are there", who, n, e,
                  vec_base > vec ? vec_base : vec, lds_max);
    const bool fits = cp_fits_lds(n, e);
    PFN_CHECK_ARG(route != 1 || fits, "%s: route 1 (LDS): %d unknowns of %d buses and %d lines need %zu bytes of LDS, %zu are there", who, m, n, e,
                  cp_lds_bytes(n, e), lds_max);
    if (n_samples == 0 || n_lines == 0) return PFN_OK;
    PFN_CHECK_ARG(edge_index && rx && bus_type && spec && base_flow && status && flags && ws, "%s: null pointer", who);
    PFN_CHECK_ARG(c < 2 || (lines && islands && severity && worst_line && overloads), "%s: null pointer", who);
    const size_t slab = cp_slab_bytes(n, e), need = (size_t)n_samples * slab;
    const int64_t P = (int64_t)c * (c - 1) / 2;
    const CpArgs a{edge_index, rx, bus_type, spec, ratings, lines, islands, severity, worst_line, overloads, base_flow, status, post_flow, flags,
                   static_cast<unsigned char*>(ws), tol, slab, P, n, e, c, max_iter, (int)n_pv, (int)n_pq, ratings_per_sample != 0};
    PFN_TRY(ct_check_aligned(who, a, lines));
    if (ws_bytes < need) {
        set_error("%s: needs a workspace of %zu bytes (got %zu)", who, need, ws_bytes);
        return PFN_ENOSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double ss = (double)n_samples, mm = (double)m, ee = (double)e, pp = (double)P;
    {
        ProfScope ps("contingency_pairs_base", ss * (ee * 44.0 + (double)n * 36.0 + mm * mm * 4.0), ss * (2.0 * mm * mm * mm + 6.0 * mm * mm), s);
        // (the N-1 screen's rule: the inverse is formed in LDS where it fits there)
        PFN_TRY((launch_either<contingency_pairs_base_kernel<true>, contingency_pairs_base_kernel<false>>(ct_fits_lds(n, e), (int)n_samples, threads,
                                                                                                          vec_base + mat, vec_base, s, a)));
    }
    if (c < 2) return PFN_OK;
    {
        const bool lds = route == 1 || (route == 0 && fits);
        ProfScope ps("contingency_pairs", ss * ((double)(c - 1) * (lds ? (double)mat : 0.0) + pp * (8.0 * mm + 12.0 + (post_flow ? 4.0 * ee : 0.0))),
                     ss * pp * (2.0 * mm + 12.0 * ee), s);
        PFN_TRY((launch_either<contingency_pairs_kernel<true>, contingency_pairs_kernel<false>>(lds, (int)(n_samples * (c - 1)), threads, vec + mat, vec, s, a)));
    }
    return PFN_OK;
}

}  // extern "C"
