// The AC N-1 screen beyond the dense cap (gfx950): compensated 1P1Q on the sparse route.  pfn_contingency_ac_sparse, two launches
// behind pfn_contingency_islands, for grids whose B' and B'' are kept as sparse fp32 FACTORS under the fast-decoupled plan of the
// sparse power-flow route (powerflow_plan.hpp, mode "fd") where contingency_ac.hip keeps their dense inverses.  Same definitions,
// same outputs, same statuses as pfn_contingency_ac, plus -6 where the device line list is not the plan's -- because a bus's
// mismatch, 1 / c_k - a^T w, the per-bus and per-line tails, the stores and the fill values are contingency_ac_core.hpp's, one text
// for both routes; this file keeps the substitutions, the serial w . g and the lane's loops.
//
// BASE launch: powerflow_sparse_fd.hip's kernel through its exported call (powerflow_sparse_fd.hpp pfd_solve) -- base table, status
// and residual are pfn_powerflow_solve_sparse_fd's bits because they are its launch.  The sample's slab of the workspace then holds
// what the outages read: the fp64 base state (vm, th [n]) and both factors (pf_sample_bytes' layout).
//
// OUTAGE launch: a LANE per outage, a one-wave workgroup per tile of 64 consecutive outages of a scenario (contingency_sparse.hip's
// mapping); workgroup g of G takes the items (scenario, tile) g, g + G, ...; an item's arithmetic does not know G.  The lane's fp64
// vectors are columns of one block [2 n + 2 mmax][64] (a row is 512 contiguous bytes; mmax = max(m_p, m_q)):
//     TH, VM [n]     the state, by bus
//     G  [mmax]      the half's scaled mismatch, then -- substituted in place -- X g, by the half's unknown in plan order
//     W  [mmax]      w = X a of the half, a = e_i - e_j restricted to the matrix's buses: formed anew in every half, so that four
//                    vectors do (with the classical two halves each w is formed exactly once anyway)
// in LDS where the whole block fits, else in the workgroup's block of the workspace: the same code, the same bits.  Per half h:
//     W = a, substituted through the half's factor (pfc_substitute's expression and column order, the diagonal division of
//     pfc_solution); den = 1 / c_k - a^T w;
//     the fp64 mismatch of the grid without line k at (TH, VM): every bus's line ends in stored order over the plan's per-bus list,
//     pf_ac_end per end, line k skipped; G = dP / Vm over the angle buses (even h, every h without a PQ bus) or dQ / Vm over the PQ
//     buses (odd h);
//     w . g, ONE serial fp64 sum in ascending unknown order; G substituted; x -= G + W (w . g) / den over the half's buses.
// Then max |F| once more, the fp32 state, the phasors (bf_phasor_of; they take the place of G and W), the currents of the lines
// l != k in ascending order (bf_line), the lane's worst under strict > -- contingency_monitor.hpp's accumulator and stores; a lane per
// outage, so nothing is merged -- and the voltage figures over the PQ buses in ascending order.
// Everything the lanes share -- column bounds, row ids, factor values, the per-bus line ends, rx, spec, the base state, the line
// list -- comes in through const __restrict__ pointers and does not depend on the lane; the block's rows are the only per-lane
// traffic besides the outputs.  No barrier, no shuffle, no atomic; a lane whose outage islands buses, whose scenario failed or whose
// tile slot is past e runs nothing and writes its fill values.  No host read, no allocation: capturable.
#include <algorithm>

#include "contingency_ac_core.hpp"
#include "contingency_sparse_core.hpp"
#include "powerflow_sparse_fd.hpp"

namespace pfn {

constexpr int CAS_GROUPS_PER_CU = 4;                // groups = 0: min(items, this many one-wave workgroups per compute unit): the sweep of DESIGN 7za

// an outage block: theta, Vm [n] and g, w [mmax], 64 doubles to a row
__host__ __device__ inline size_t cas_block_bytes(int n, int mmax) { return (size_t)512 * (2 * (size_t)n + 2 * (size_t)mmax); }
static inline bool cas_block_fits_lds(int n, int mmax) { return cas_block_bytes(n, mmax) <= (size_t)(kLdsCuBytes - kLdsReserve); }
static inline int64_t cas_groups(int64_t n_samples, int64_t e, int groups) {
    const int64_t items = n_samples * cs_tiles(e);
    const int64_t want = groups > 0 ? (int64_t)groups : (int64_t)CAS_GROUPS_PER_CU * device_cus();
    return items < want ? items : want;
}

// ---- the lane's column of a vector V [rows][64] (V points at the lane's word of row 0) through one factor, fp64 on fp32 entries:
// V[r] -= (double)fac * y for the B entries at i of one column; the rows of a column are distinct, so the B loads go out together
template <int B>
__device__ __forceinline__ void cas_update(double* __restrict__ V, const uint32_t* __restrict__ row32, const float* __restrict__ fac, int i, double y) {
    size_t r[B];
    float f[B];
    double w[B];
#pragma unroll
    for (int u = 0; u < B; ++u) {
        r[u] = cs_row(row32, i + u);
        f[u] = fac[i + u];
    }
#pragma unroll
    for (int u = 0; u < B; ++u) w[u] = V[r[u]];
#pragma unroll
    for (int u = 0; u < B; ++u) V[r[u]] = w[u] - (double)f[u] * y;
}
__device__ __forceinline__ void cas_column(double* __restrict__ V, const uint32_t* __restrict__ row32, const float* __restrict__ fac, int cb, int ce,
                                           double y) {
    int i = cb;
    for (; i + 4 <= ce; i += 4) cas_update<4>(V, row32, fac, i, y);
    for (; i < ce; ++i) cas_update<1>(V, row32, fac, i, y);
}
// L y = V, U x = y by columns, ascending then descending; V becomes x (the division by the diagonal is pfc_solution's)
__device__ __forceinline__ void cas_substitute(double* __restrict__ V, const int32_t* __restrict__ colptr, const int32_t* __restrict__ diag,
                                               const uint32_t* __restrict__ row32, const float* __restrict__ fac, int m) {
    if (m <= 0) return;
    int lb = diag[0] + 1, le = colptr[1];
    for (int j = 0; j < m; ++j) {
        const int cb = lb, ce = le;
        if (j + 1 < m) {
            lb = diag[j + 1] + 1;
            le = colptr[j + 2];
        }
        if (cb >= ce) continue;
        cas_column(V, row32, fac, cb, ce, V[(size_t)j * 64]);
    }
    int ub = colptr[m - 1], ue = diag[m - 1];
    for (int j = m - 1; j >= 0; --j) {
        const int cb = ub, ce = ue;
        if (j > 0) {
            ub = colptr[j - 1];
            ue = diag[j - 1];
        }
        const double x = V[(size_t)j * 64] / (double)fac[ce];
        V[(size_t)j * 64] = x;
        cas_column(V, row32, fac, cb, ce, x);
    }
}

// ---- the fp64 mismatch of the grid without line k at the lane's state: buses ascending, a bus's line ends in stored order.
// mode 0: G = dP / Vm by the angle unknown; mode 1: G = dQ / Vm by the PQ unknown; mode 2: nothing stored.  Returns max |F| over
// both kinds of equation (a non-finite entry counts as +inf).
__device__ __forceinline__ double cas_mismatch(const double* TH, const double* VM, double* G, const int32_t* __restrict__ adjptr,
                                               const int2* __restrict__ adj, const int32_t* __restrict__ uap, const int32_t* __restrict__ uaq,
                                               const double* __restrict__ rx, const double* __restrict__ spec, int n, int k, int mode) {
    double mx = 0.0;
    int q = adjptr[0];
    for (int i = 0; i < n; ++i) {
        const int q1 = adjptr[i + 1];
        const int ra = uap[i], rq = uaq[i];
        if (ra >= 0) mx = ca_bus_mismatch<64, 1>(mx, TH, VM, G, adj, q, q1, rx, spec, i, ra, rq, k, mode);       // (the slack: no equation)
        q = q1;
    }
    return mx;
}

// ------------------------------------------------------------------------------------------------------ outages
template <bool LDS>
__global__ __launch_bounds__(64) void contingency_ac_sparse_outages_kernel(
    const unsigned char* __restrict__ plan, const unsigned char* __restrict__ slabs, double* __restrict__ blocks, const int64_t* __restrict__ ei,
    const double* __restrict__ rx_all, const double* __restrict__ spec_all, const double* __restrict__ ratings, const int32_t* __restrict__ status,
    const int32_t* __restrict__ islands, const CaOut out, size_t ws_stride, int n, int e, int mmax, int n_samples, int halves, int bx,
    int ratings_per_sample, float v_lo, float v_hi) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cas_smem[];
    const int lane = threadIdx.x;
    // ---- the two halves of the plan (every section is wave-uniform)
    const int32_t* H = reinterpret_cast<const int32_t*>(plan);
    const unsigned char* pp = plan + H[PFD_H_OFF_P];
    const unsigned char* pq = plan + H[PFD_H_OFF_Q];
    const int32_t* HP = reinterpret_cast<const int32_t*>(pp);
    const int32_t* HQ = reinterpret_cast<const int32_t*>(pq);
    const int m_q = HQ[PFP_H_M];
    const int32_t* __restrict__ uap = reinterpret_cast<const int32_t*>(pp + HP[PFP_H_OFF_UA]);
    const int32_t* __restrict__ uaq = reinterpret_cast<const int32_t*>(pq + HQ[PFP_H_OFF_UA]);
    const int32_t* __restrict__ adjptr = reinterpret_cast<const int32_t*>(pp + HP[PFP_H_OFF_ADJPTR]);
    const int2* __restrict__ adj = reinterpret_cast<const int2*>(pp + HP[PFP_H_OFF_ADJ]);

    // ---- the lane's columns of the block
    double* blk;
    if constexpr (LDS) blk = reinterpret_cast<double*>(cas_smem) + lane;
    else blk = blocks + (size_t)blockIdx.x * (cas_block_bytes(n, mmax) / 8) + lane;
    double* TH = blk;
    double* VM = TH + (size_t)n * 64;
    double* G = VM + (size_t)n * 64;
    double* W = G + (size_t)mmax * 64;
    float2* PH = reinterpret_cast<float2*>(G);     // (n phasors of 8 bytes in the place of G and W: 2 mmax >= n rows)

    const int tiles = (e + 63) >> 6;
    const int64_t items = (int64_t)n_samples * tiles;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int s = (int)(item / tiles);
        const int k = (int)(item - (int64_t)s * tiles) * 64 + lane;
        if (k >= e) continue;                       // (lanes past e in the last tile are idle)
        const int64_t o = (int64_t)s * e + k;
        float* crow = out.post_current ? out.post_current + o * e : nullptr;
        float* srow = out.post_state ? out.post_state + o * 2 * n : nullptr;
        const bool failed = status[s] < 0;
        if (failed || islands[k] != 0) {            // a failed scenario, an islanding outage: the fill values
            ca_skip(failed, out, o, crow, srow, e, n, 0, 1);
            continue;
        }
        // ---- the scenario's inputs and its slab as the base launch left it
        const double* __restrict__ rx = rx_all + (int64_t)s * 2 * e;
        const double* __restrict__ spec = spec_all + (int64_t)s * 4 * n;
        const double* __restrict__ svm = reinterpret_cast<const double*>(slabs + (size_t)s * ws_stride);
        const double* __restrict__ sth = svm + n;
        const float* __restrict__ fac_p = reinterpret_cast<const float*>(svm + 4 * (size_t)n + mmax);
        for (int b = 0; b < n; ++b) {
            TH[(size_t)b * 64] = sth[b];
            VM[(size_t)b * 64] = svm[b];
        }
        const int bi = (int)ei[k], bj = (int)ei[e + k];
        const double2 ck = ca_weights(rx[2 * k], rx[2 * k + 1]);

        double mx;
        for (int h = 0;; ++h) {
            const bool last = h == halves;
            const bool qhalf = m_q != 0 && (h & 1);
            mx = cas_mismatch(TH, VM, G, adjptr, adj, uap, uaq, rx, spec, n, k, last ? 2 : (qhalf ? 1 : 0));
            if (last) break;
            // (the half's sections are looked up here, not kept across the loop: fewer live scalar registers)
            const unsigned char* ph = qhalf ? pq : pp;
            const int32_t* HH = reinterpret_cast<const int32_t*>(ph);
            const int32_t* __restrict__ colptr = reinterpret_cast<const int32_t*>(ph + HH[PFP_H_OFF_COLPTR]);
            const int32_t* __restrict__ diag = reinterpret_cast<const int32_t*>(ph + HH[PFP_H_OFF_DIAG]);
            const uint32_t* __restrict__ row32 = reinterpret_cast<const uint32_t*>(ph + HH[PFP_H_OFF_ROWIDX]);
            const int32_t* __restrict__ ua = qhalf ? uaq : uap;
            const float* __restrict__ fac = fac_p + (qhalf ? HP[PFP_H_NNZ] : 0);
            const int m = HH[PFP_H_M];
            double* X = qhalf ? VM : TH;
            // ---- w = X a: the right-hand side e_i - e_j in plan order (an end outside the matrix adds nothing), substituted
            for (int r = 0; r < m; ++r) W[(size_t)r * 64] = 0.0;
            const int pi = ua[bi], pj = ua[bj];
            if (pi >= 0) W[(size_t)pi * 64] += 1.0;
            if (pj >= 0) W[(size_t)pj * 64] -= 1.0;
            cas_substitute(W, colptr, diag, row32, fac, m);
            // ---- 1 / c_k - a^T w (c: the line's weight in the half's matrix)
            const double den = ca_den(ck, bx != 0, qhalf, (pi >= 0 ? W[(size_t)pi * 64] : 0.0) - (pj >= 0 ? W[(size_t)pj * 64] : 0.0));
            // ---- w . g, one sum in ascending unknown order; then G = X g
            double dot = 0.0;
            for (int r = 0; r < m; ++r) dot += W[(size_t)r * 64] * G[(size_t)r * 64];
            const double scale = dot / den;
            cas_substitute(G, colptr, diag, row32, fac, m);
            // ---- x -= X g + w (w . g) / den over the half's buses
            for (int b = 0; b < n; ++b) {
                const int r = ua[b];
                if (r < 0) continue;
                X[(size_t)b * 64] -= G[(size_t)r * 64] + W[(size_t)r * 64] * scale;
            }
        }

        // ---- the fp32 state, the phasors and the voltage figures over the PQ buses, ascending: strict < keeps the lowest bus
        CaLow low = ca_low_none();
        for (int b = 0; b < n; ++b) ca_bus_tail<64>(low, TH, VM, PH, srow, spec, b, uap[b] < 0, uaq[b] >= 0, v_lo, v_hi);
        // ---- the currents of the lines l != k in ascending order, their loadings, the lane's worst (contingency_monitor.hpp)
        const double* __restrict__ rat = ratings ? ratings + (ratings_per_sample ? (int64_t)s * e : 0) : nullptr;
        CtWorst worst = ct_worst_none();
        for (int l = 0; l < e; ++l) ca_line_tail<64>(worst, PH, ei, rx, rat, crow, e, l, k);
        ca_store(out, o, worst, low, mx);
    }
}

// counts that contradict the plan's (n_pq is not its m_q): what pfn_contingency_ac reports for counts that contradict bus_type --
// every scenario -5 with NaN rows and bit 0 of flags[0]; the base solve does not run
__global__ __launch_bounds__(64) void contingency_ac_sparse_bad_counts_kernel(double* table, int32_t* status, double* residual, int32_t* flags, int n) {
    const int s = blockIdx.x;
    for (int q = threadIdx.x; q < 4 * n; q += 64) table[(int64_t)s * 4 * n + q] = __builtin_nan("");
    if (threadIdx.x == 0) {
        status[s] = PF_BAD_TYPES;
        residual[s] = __builtin_nan("");
        flags[0] = flags[0] | 1;                    // (every writer stores the same bit over the same word)
    }
}

// the header, the sizes and the options of a call: what the size functions and the entry share
static int cas_check_shape(const char* who, const int32_t* h, int64_t n_samples, int64_t n_lines, int block_route, int groups) {
    PFN_TRY(pfd_check_header(h, who));
    PFN_CHECK_ARG(n_samples >= 0 && n_samples < (1ll << 29) && n_lines >= 0 && n_lines < (1ll << 24), "%s: bad sizes (%lld scenarios of %lld lines)", who,
                  (long long)n_samples, (long long)n_lines);
    PFN_CHECK_ARG(h[PFP_H_N] >= 2 && h[PFP_H_M] == h[PFP_H_N] - 1, "%s: the plan header is inconsistent", who);
    PFN_CHECK_ARG(h[PFP_H_E] == n_lines, "%s: the plan is for %d buses and %d lines; the call has %lld lines", who, (int)h[PFP_H_N], (int)h[PFP_H_E],
                  (long long)n_lines);
    PFN_CHECK_ARG(block_route >= 0 && block_route <= 2, "%s: block_route must be 0 (auto), 1 (LDS) or 2 (global)", who);
    PFN_CHECK_ARG(groups >= 0, "%s: groups must be 0 (the default) or the number of one-wave workgroups", who);
    return PFN_OK;
}

}  // namespace pfn

using namespace pfn;

extern "C" {

size_t pfn_contingency_ac_sparse_block_bytes(const void* plan_header) {
    const int32_t* h = static_cast<const int32_t*>(plan_header);
    if (pfd_check_header(h, "pfn_contingency_ac_sparse_block_bytes") != PFN_OK) return 0;
    return cas_block_bytes(h[PFP_H_N], std::max(h[PFP_H_M], h[PFD_H_M_Q]));
}

size_t pfn_contingency_ac_sparse_workspace_bytes(int64_t n_samples, int64_t n_lines, const void* plan_header, int block_route, int groups) {
    const int32_t* h = static_cast<const int32_t*>(plan_header);
    if (n_samples <= 0 || n_lines < 1 || cas_check_shape("pfn_contingency_ac_sparse_workspace_bytes", h, n_samples, n_lines, block_route, groups) != PFN_OK)
        return 0;
    const int n = h[PFP_H_N], mmax = std::max(h[PFP_H_M], h[PFD_H_M_Q]);
    const bool fits = cas_block_fits_lds(n, mmax);
    if (block_route == 1 && !fits) return 0;
    const bool lds = block_route == 1 || (block_route == 0 && fits);
    return (size_t)n_samples * pf_sample_bytes(n, mmax, h[PFP_H_NNZ]) + (lds ? 0 : (size_t)cas_groups(n_samples, n_lines, groups) * cas_block_bytes(n, mmax));
}

int pfn_contingency_ac_sparse(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                              const double* init, const double* ratings, int ratings_per_sample, const int32_t* islands, int64_t n_samples,
                              int64_t n_bus, int64_t n_pv, int64_t n_pq, int variant, int halves, float v_lo, float v_hi, double tol, int max_iter,
                              const void* plan_header, const void* plan_dev, int threads, int block_route, int groups, float* severity,
                              int32_t* worst_line, int32_t* overloads, float* vm_min, int32_t* vm_min_bus, int32_t* v_violations, double* mismatch,
                              double* base_table, int32_t* status, double* residual, float* post_current, float* post_state, int32_t* flags, void* ws,
                              size_t ws_bytes, void* stream) {
    const char* who = "pfn_contingency_ac_sparse";
    const int32_t* h = static_cast<const int32_t*>(plan_header);
    PFN_TRY(cas_check_shape(who, h, n_samples, n_lines, block_route, groups));
    PFN_CHECK_ARG(h[PFP_H_N] == n_bus, "%s: the plan is for %d buses and %d lines; the call has %lld and %lld", who, (int)h[PFP_H_N], (int)h[PFP_H_E],
                  (long long)n_bus, (long long)n_lines);
    PFN_TRY(ca_check_options(who, n_bus, n_pv, n_pq, variant, halves, v_lo, v_hi, tol, max_iter));
    const int n = h[PFP_H_N], e = (int)n_lines, m_q = h[PFD_H_M_Q], mmax = std::max(h[PFP_H_M], m_q);
    PFN_TRY(pf_check_sparse_launch(who, threads, nullptr, n_samples, h, mmax));
    const bool fits = cas_block_fits_lds(n, mmax);
    PFN_CHECK_ARG(block_route != 1 || fits, "%s: block_route 1 (LDS): an outage block of %d buses needs %zu bytes of LDS, %d are there", who, n,
                  cas_block_bytes(n, mmax), kLdsCuBytes - kLdsReserve);
    if (n_samples == 0 || n_lines == 0) return PFN_OK;
    const CaOut out{severity, worst_line, overloads, vm_min, vm_min_bus, v_violations, mismatch, post_current, post_state};
    PFN_TRY(ca_check_pointers(who, edge_index, rx, bus_type, spec, init, ratings, islands, out, base_table, status, residual, flags, ws, true, plan_dev));
    const bool lds = block_route == 1 || (block_route == 0 && fits);
    const size_t stride = pf_sample_bytes(n, mmax, h[PFP_H_NNZ]), slabs = (size_t)n_samples * stride, block = cas_block_bytes(n, mmax);
    const int64_t G = cas_groups(n_samples, e, groups);
    PFN_TRY(pf_check_workspace(who, ws, ws_bytes, slabs + (lds ? 0 : (size_t)G * block)));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_pq != m_q) {
        contingency_ac_sparse_bad_counts_kernel<<<(int)n_samples, 64, 0, s>>>(base_table, status, residual, flags, n);
        PFN_CHECK_LAUNCH();
    } else {
        PFN_TRY(pfd_solve(who, edge_index, n_lines, rx, nullptr, nullptr, bus_type, spec, init, n_samples, n_bus, 2 + variant, tol, max_iter, plan_header,
                          plan_dev, threads, base_table, status, residual, flags, ws, ws_bytes, stream));
    }
    const double ss = (double)n_samples, ee = (double)e, nn = (double)n, nz = (double)h[PFP_H_NNZ], hh = (double)halves, tl = (double)cs_tiles(e);
    ProfScope ps("contingency_ac_sparse_outages",
                 ss * (tl * ((hh + 1.0) * (ee * 48.0 + nn * 40.0) + hh * nz * 6.0) + ee * (28.0 + (post_current ? 4.0 * ee : 0.0) + (post_state ? 8.0 * nn : 0.0))),
                 ss * tl * 64.0 * (hh * (2.0 * nz + 4.0 * nn) + (hh + 1.0) * 120.0 * ee + 30.0 * ee), s);
    return launch_either<contingency_ac_sparse_outages_kernel<true>, contingency_ac_sparse_outages_kernel<false>>(
        lds, (int)G, 64, block, 0, s, static_cast<const unsigned char*>(plan_dev), static_cast<const unsigned char*>(ws),
        lds ? static_cast<double*>(nullptr) : reinterpret_cast<double*>(static_cast<unsigned char*>(ws) + slabs), edge_index, rx, spec, ratings,
        static_cast<const int32_t*>(status), islands, out, stride, n, e, mmax, (int)n_samples, halves, variant, ratings_per_sample != 0, v_lo, v_hi);
}

}  // extern "C"
