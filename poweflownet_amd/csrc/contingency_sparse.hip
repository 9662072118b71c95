// The N-1 line-outage screen beyond the dense cap (gfx950): pfn_contingency_sparse, two launches behind pfn_contingency_islands, for
// grids whose B' is kept as a sparse fp32 FACTOR under the host plan of the sparse power-flow route (mode 1, powerflow_plan.hpp)
// where contingency.hip keeps its dense inverse.  Same model, same definitions, same statuses as pfn_contingency_dc.
//
// contingency_sparse_base_kernel: one workgroup per scenario, the DC solve of powerflow_sparse.hip's mode 1 through the shared pieces
// (powerflow_common.hpp, powerflow_sparse_core.hpp).  F = B' theta + P in fp64 first -- so a NaN in P or x = 0 is -3, never a pivot
// failure --, then, once, B' at the planned positions in fp32 (bus i's line ends in stored order, the diagonal summed in fp64 and
// added last) and its left-looking factorisation; theta -= B'^-1 F by the column substitutions under the fp64 residual to tol /
// max_iter.  It leaves in the scenario's workspace slab the FACTOR and what the outages read per line: the base flow and x in fp32,
// the fp32 rating, and the plan-order unknown of either end (m at the slack: row m of an outage block is zero).
//
// contingency_sparse_outages_kernel: a lane per outage, a one-wave workgroup per tile of 64 consecutive outages.  The tile's 64
// right-hand sides e_i - e_j live in one block W [m + 1][64] fp32 (row = unknown in plan order, column = lane): every access is one
// 256-byte row, a lane reads and writes its own column only, so there is no barrier, no shuffle and no atomic.  Forward by columns
// ascending (W[r] = fma(-L_rj, W[j], W[r])), backward descending (W[j] /= U_jj, W[r] = fma(-U_rj, W[j], W[r])): the column bounds,
// row ids and factor values do not depend on the lane and are loaded once per wave.  Then den_k from two gathers and ONE loop over
// the lines in ascending order with contingency.hip's per-line expression (contingency_line.hpp): the lane keeps the largest loading
// under strict > (ties to the lowest line), the overload count and the non-finite flag in registers and writes its three outputs --
// the accumulator and the stores of every screen's tail (contingency_monitor.hpp); a lane per outage, so nothing is merged.
// Workgroup g of G takes the items (scenario, tile) g, g + G, ...; an item's arithmetic does not know G.  W sits in LDS where
// 256 (m + 1) bytes fit, else in the workgroup's block of the workspace: the same code, the same bits.
#include "contingency_line.hpp"
#include "contingency_monitor.hpp"
#include "contingency_sparse_core.hpp"

namespace pfn {

// ------------------------------------------------------------------------------------------------------ launch 1
template <int THREADS>
__global__ __launch_bounds__(THREADS) void contingency_sparse_base_kernel(const CsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cs_smem[];
    __shared__ double s_red[THREADS / 64];
    const int t = threadIdx.x;
    constexpr int nt = THREADS;
    const int s = blockIdx.x;
    const PfProblem& p = a.p;
    const int n = p.n, e = p.e, m = a.m, nnz = a.nnz;
    const PfPlanView v = pf_plan_view(reinterpret_cast<const unsigned char*>(a.plan));
    const int32_t* ua = v.ua;
    const int32_t* uv = v.uv;
    const PfcMatrix A{v.A.colptr, v.A.diag, v.A.row, m};
    const CsSlab b = cs_slab(p.ws, a.ws_stride, s, n, m, nnz, e);
    double* th = b.th;
    float* slab = b.factor;
    float* w = reinterpret_cast<float*>(cs_smem);
    double* F = a.f_in_lds ? reinterpret_cast<double*>(cs_smem + pf_w_bytes(m)) : b.F;
    const int64_t* ei = p.edge_index;
    const double* rx = p.rx + (int64_t)s * 2 * e;
    const double* spec = p.spec + (int64_t)s * 4 * n;
    const double* rat_in = a.ratings ? a.ratings + (a.ratings_per_sample ? (int64_t)s * e : 0) : nullptr;
    const PfSample sm{nullptr, rx, spec, nullptr};

    // ---- the lines name buses of the grid?  the host's PV count against the device bus types?  the device arrays against the plan?
    // code is uniform over the workgroup wherever it is tested
    int bad = 0, pv = 0;
    for (int k = t; k < e; k += nt) bad |= (uint64_t)ei[k] >= (uint64_t)n || (uint64_t)ei[e + k] >= (uint64_t)n;
    for (int i0 = 0; i0 < n; i0 += nt) pv += __syncthreads_count(i0 + t < n && p.bus_type[i0 + t] == 1);
    bad = __syncthreads_or(bad);
    int code = pf_check_plan(p, v, nt, 0, [&](int i, int ty, int&) { return (ty != 0) != (ua[i] >= 0) || uv[i] >= 0; });
    if (code != PF_BAD_TYPES && pv != a.n_pv) {
        code = PF_BAD_TYPES;
        if (t == 0) p.flags[0] = p.flags[0] | 1;    // (every writer stores the same bit over the same word)
    }
    if (code != PF_BAD_TYPES && bad) code = PF_BAD_LINE;
    if (code == 0 && pf_start_state(p, sm, p.bus_type, a.plan[PFP_H_SLACK], true, nt, b.vm, th)) code = PF_NON_FINITE;
    int it = 0;
    if (code == 0) {
        for (;; ++it) {
            // ---- F = B' theta + P at the non-slack buses: bus i's line ends in stored order
            for (int i = t; i < n; i += nt) {
                const int ra = ua[i];
                if (ra < 0) continue;
                const double ti = th[i];
                double sP = 0.0;
                const int q1 = v.adjptr[i + 1];
                for (int q = v.adjptr[i]; q < q1; ++q) {
                    const int2 lj = v.adj[q];
                    pf_dc_end(rx[2 * (lj.x >> 1) + 1], ti, th[lj.y], sP);
                }
                F[ra] = spec[4 * i + 2] - sP;
            }
            __syncthreads();
            double mx = 0.0;
            for (int k = t; k < m; k += nt) mx = fmax(mx, pf_abs_clamped(F[k]));
            const double res = pf_block_max(mx, s_red, THREADS / 64);
            const int stop = pf_stop(res, p.tol, it, p.max_iter);
            if (stop < 0) { code = stop; break; }
            if (it == 0) {
                // ---- B', once: the Laplacian of 1 / x at the planned positions (parallel lines add), the diagonal summed in fp64 and
                //      added last; then factored in place.  A scenario that starts converged still needs the factor: the outages do.
                for (int k = t; k < nnz; k += nt) slab[k] = 0.f;
                __syncthreads();
                for (int i = t; i < n; i += nt) {
                    if (ua[i] < 0) continue;
                    double dp = 0.0;
                    const int q1 = v.adjptr[i + 1];
                    for (int q = v.adjptr[i]; q < q1; ++q) {
                        const int pos = v.adjpos[q].x;
                        const double wl = 1.0 / rx[2 * (v.adj[q].x >> 1) + 1];
                        dp += wl;
                        if (pos >= 0) slab[pos] += (float)(-wl);
                    }
                    slab[v.buspos[i].x] += (float)dp;
                }
                __syncthreads();
                if (!pfc_factor<THREADS>(A, slab, w)) { code = PF_SINGULAR; break; }
            }
            if (stop) break;
            // ---- theta -= B'^-1 F: L y = F, U d = y by columns on the fp64 right-hand side
            pfc_substitute<THREADS>(A, slab, F);
            for (int i = t; i < n; i += nt) {
                const int ia = ua[i];
                if (ia >= 0) th[i] -= pfc_solution(A, slab, F, ia);
            }
            __syncthreads();
        }
    }
    // ---- the base flows (fp64), what the outages read per line, and the scenario's status
    double* bf = a.base_flow + (int64_t)s * e;
    for (int k = t; k < e; k += nt) {
        double f = __builtin_nan("");
        if (code == 0) {
            const int la = (int)ei[k], lb = (int)ei[e + k];
            const double x = rx[2 * k + 1];
            f = (th[la] - th[lb]) / x;
            b.f32[k] = (float)f;
            b.x32[k] = (float)x;
            b.rat[k] = rat_in ? (float)rat_in[k] : 1.f;
            b.pa[k] = ua[la] >= 0 ? ua[la] : m;
            b.pb[k] = ua[lb] >= 0 ? ua[lb] : m;
        }
        bf[k] = f;
    }
    if (t == 0) p.status[s] = code ? code : it;
}

// ------------------------------------------------------------------------------------------------------ launch 2
// (what the launch reads but never writes comes in through its own const __restrict__ arguments: contingency_sparse_core.hpp)
template <bool LDS>
__global__ __launch_bounds__(64) void contingency_sparse_outages_kernel(const unsigned char* __restrict__ plan, const unsigned char* __restrict__ slabs,
                                                                        float* __restrict__ blocks, const int32_t* __restrict__ status,
                                                                        const int32_t* __restrict__ islands, float* __restrict__ severity,
                                                                        int32_t* __restrict__ worst_line, int32_t* __restrict__ overloads,
                                                                        float* __restrict__ post_flow, size_t ws_stride, int n, int e, int m, int nnz,
                                                                        int n_samples) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cs_smem[];
    const int lane = threadIdx.x;
    const int32_t* H = reinterpret_cast<const int32_t*>(plan);
    const int32_t* __restrict__ colptr = reinterpret_cast<const int32_t*>(plan + H[PFP_H_OFF_COLPTR]);
    const int32_t* __restrict__ diag = reinterpret_cast<const int32_t*>(plan + H[PFP_H_OFF_DIAG]);
    const uint32_t* __restrict__ row32 = reinterpret_cast<const uint32_t*>(plan + H[PFP_H_OFF_ROWIDX]);
    float* __restrict__ W;                          // [m + 1][64]; this lane's column is W[r * 64], r = 0 .. m
    if constexpr (LDS) W = reinterpret_cast<float*>(cs_smem) + lane;
    else W = blocks + (size_t)blockIdx.x * 64 * ((size_t)m + 1) + lane;
    const int tiles = (e + 63) >> 6;
    const int64_t items = (int64_t)n_samples * tiles;
    W[(size_t)m * 64] = 0.f;                        // (the slack's row: no column of the factor reaches it)

    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int s = (int)(item / tiles);
        const int k = (int)(item - (int64_t)s * tiles) * 64 + lane;
        const bool live = k < e;                    // (lanes past e in the last tile are idle)
        const int kc = live ? k : e - 1;
        const int64_t o = (int64_t)s * e + kc;
        float* out_row = post_flow ? post_flow + o * e : nullptr;
        // a failed scenario: NaN and -1, no substitution
        if (status[s] < 0) {
            if (live) {
                if (out_row)
                    for (int l = 0; l < e; ++l) out_row[l] = __builtin_nanf("");
                ct_store(ct_figures_skipped(true), severity[o], worst_line[o], overloads[o]);
            }
            continue;
        }
        // the scenario's slab as the base launch left it
        const CsLines v = cs_lines(slabs, ws_stride, s, n, m, nnz, e);
        const float* __restrict__ fac = v.fac;
        const float* __restrict__ f32 = v.f32;
        const float* __restrict__ x32 = v.x32;
        const float* __restrict__ rat = v.rat;
        const int32_t* __restrict__ pa = v.pa;
        const int32_t* __restrict__ pb = v.pb;
        // an islanding outage keeps a zero right-hand side: +inf, -1, -1 and a NaN row in the end
        const bool run = live && islands[kc] == 0;
        const int pi = pa[kc], pj = pb[kc];
        cs_substitute(W, colptr, diag, row32, fac, m, run, pi, pj);
        // ---- den_k from two gathers, then the lines in ascending order: post-outage flow, loading, the lane's worst
        //      (contingency_monitor.hpp: a lane per outage, so nothing is merged)
        const float den = ct_den(W[(size_t)pi * 64], W[(size_t)pj * 64], x32[kc]);
        const float fk = f32[kc];
        CtWorst worst = ct_worst_none();
        for (int l = 0; l < e; ++l) {
            const float post = l == k ? 0.f : ct_post(W[(size_t)pa[l] * 64], W[(size_t)pb[l] * 64], x32[l], den, f32[l], fk);
            if (out_row && live) out_row[l] = run ? post : __builtin_nanf("");
            const float r = rat[l];
            if (l != k && r > 0.f) ct_worst_add(worst, l, ct_loading(post, r));
        }
        if (live) ct_store(run ? ct_figures(worst) : ct_figures_skipped(false), severity[o], worst_line[o], overloads[o]);
    }
}

int cs_check_header(const int32_t* h, const char* who) {
    PFN_TRY(pf_check_plan_header(who, h));
    PFN_CHECK_ARG(h[PFP_H_MODE] == 1, "%s: the screen takes a mode-1 (\"dc\") plan; this one has mode %d", who, (int)h[PFP_H_MODE]);
    PFN_CHECK_ARG(h[PFP_H_N] >= 2 && h[PFP_H_M] == h[PFP_H_N] - 1, "%s: the plan header is inconsistent", who);
    return PFN_OK;
}

int cs_check_call(const char* who, const CsCall& c, PfProblem* p, size_t* base_lds) {
    const int32_t* h = static_cast<const int32_t*>(c.plan_header);
    PFN_TRY(cs_check_header(h, who));
    PFN_CHECK_ARG(c.n_bus >= 2 && c.n_lines >= 0 && c.n_lines < (1ll << 24) && c.n_bus < (1ll << 24),
                  "%s: bad sizes (%lld scenarios of %lld buses and %lld lines)", who, (long long)c.n_samples, (long long)c.n_bus, (long long)c.n_lines);
    PFN_CHECK_ARG(c.n_pv >= 0 && c.n_pq >= 0 && c.n_pv + c.n_pq == c.n_bus - 1,
                  "%s: %lld PV and %lld PQ buses do not leave exactly one slack among %lld buses", who, (long long)c.n_pv, (long long)c.n_pq,
                  (long long)c.n_bus);
    PFN_CHECK_ARG(h[PFP_H_N] == c.n_bus && h[PFP_H_E] == c.n_lines, "%s: the plan is for %d buses and %d lines; the call has %lld and %lld", who,
                  (int)h[PFP_H_N], (int)h[PFP_H_E], (long long)c.n_bus, (long long)c.n_lines);
    PFN_CHECK_ARG(c.block_route >= 0 && c.block_route <= 2, "%s: block_route must be 0 (auto), 1 (LDS) or 2 (global)", who);
    PFN_CHECK_ARG(c.groups >= 0, "%s: groups must be 0 (the default) or the number of one-wave workgroups", who);
    const int n = h[PFP_H_N], m = h[PFP_H_M], e = (int)c.n_lines;
    PFN_TRY(pf_check_sparse_launch(who, c.threads, nullptr, c.n_samples, h, m));
    // (the screen writes no table and no residual: pf_check_call looks at a stand-in and at base_flow in their places)
    static double table_stand_in[4] __attribute__((aligned(32)));
    *p = PfProblem{c.edge_index, c.rx, c.bus_type, c.spec, nullptr, table_stand_in, c.status, c.base_flow, c.flags, c.ws, c.tol, n, e, c.max_iter,
                   nullptr, nullptr};
    PFN_TRY(pf_check_call(who, *p, c.n_samples, &c.plan_dev, "the workspace and the plan 16-byte"));
    p->table = nullptr;
    p->residual = nullptr;
    PFN_CHECK_ARG(c.block_route != 1 || cs_block_fits_lds(m), "%s: block_route 1 (LDS): an outage block of %d unknowns needs %zu bytes of LDS, %d are there",
                  who, m, cs_block_bytes(m), kLdsCuBytes - kLdsReserve);
    *base_lds = pf_lds_bytes(m);
    PFN_CHECK_ARG(*base_lds <= (size_t)(kLdsCuBytes - kLdsReserve), "%s: a work vector of %d unknowns needs %zu bytes of LDS, %d are there", who, m,
                  *base_lds, kLdsCuBytes - kLdsReserve);
    return PFN_OK;
}

int cs_launch_base(const CsArgs& a, const int32_t* h, int threads, int64_t n_samples, size_t base_lds, hipStream_t s) {
    const double madds = (double)(((int64_t)h[PFP_H_MADDS_HI] << 32) | (uint32_t)h[PFP_H_MADDS_LO]);
    const double ss = (double)n_samples, ee = (double)a.p.e, nz = (double)a.nnz;
    ProfScope ps("contingency_sparse_base", ss * (ee * 44.0 + (double)a.p.n * 32.0 + nz * 4.0) + (double)h[PFP_H_BYTES], ss * 2.0 * (madds + 4.0 * nz), s);
    return pf_launch_sparse<2>(contingency_sparse_base_kernel<64>, contingency_sparse_base_kernel<256>, threads, h[PFP_H_MAX_COL], n_samples, base_lds,
                               s, a);
}

}  // namespace pfn

using namespace pfn;

extern "C" {

size_t pfn_contingency_sparse_workspace_bytes(int64_t n_samples, int64_t n_lines, const void* plan_header, int block_route, int groups) {
    const char* who = "pfn_contingency_sparse_workspace_bytes";
    const int32_t* h = static_cast<const int32_t*>(plan_header);
    if (n_samples <= 0 || n_samples >= (1ll << 29) || cs_check_header(h, who) != PFN_OK) return 0;
    if (n_lines < 1 || n_lines != h[PFP_H_E] || block_route < 0 || block_route > 2 || groups < 0) return 0;
    const int n = h[PFP_H_N], m = h[PFP_H_M], nnz = h[PFP_H_NNZ], e = (int)n_lines;
    const bool lds = block_route == 1 || (block_route == 0 && cs_block_fits_lds(m));
    return (size_t)n_samples * cs_sample_bytes(n, m, nnz, e) + (lds ? 0 : (size_t)cs_groups(n_samples, e, groups) * cs_block_bytes(m));
}

int pfn_contingency_sparse(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                           const double* ratings, int ratings_per_sample, const int32_t* islands, int64_t n_samples, int64_t n_bus,
                           int64_t n_pv, int64_t n_pq, double tol, int max_iter, float* severity, int32_t* worst_line,
                           int32_t* overloads, double* base_flow, int32_t* status, float* post_flow, int32_t* flags, void* ws,
                           size_t ws_bytes, const void* plan_header, const void* plan_dev, int threads, int block_route, int groups,
                           void* stream) {
    const char* who = "pfn_contingency_sparse";
    const int32_t* h = static_cast<const int32_t*>(plan_header);
    PfProblem p;
    size_t lds1;
    PFN_TRY(cs_check_call(who, CsCall{edge_index, n_lines, rx, bus_type, spec, n_samples, n_bus, n_pv, n_pq, tol, max_iter, base_flow, status, flags, ws,
                                      plan_header, plan_dev, threads, block_route, groups}, &p, &lds1));
    if (n_samples == 0 || n_lines == 0) return PFN_OK;
    const int n = h[PFP_H_N], m = h[PFP_H_M], nnz = h[PFP_H_NNZ], e = (int)n_lines;
    PFN_CHECK_ARG(islands && severity && worst_line && overloads && base_flow, "%s: null pointer", who);
    PFN_CHECK_ARG((reinterpret_cast<uintptr_t>(ratings) & 7) == 0 &&
                      ((reinterpret_cast<uintptr_t>(islands) | reinterpret_cast<uintptr_t>(severity) | reinterpret_cast<uintptr_t>(worst_line) |
                        reinterpret_cast<uintptr_t>(overloads) | reinterpret_cast<uintptr_t>(post_flow)) & 3) == 0,
                  "%s: ratings must be 8-byte aligned, fp32 and int32 arrays 4-byte", who);
    const bool lds = block_route == 1 || (block_route == 0 && cs_block_fits_lds(m));
    const size_t stride = cs_sample_bytes(n, m, nnz, e), slabs = (size_t)n_samples * stride;
    const int64_t G = cs_groups(n_samples, e, groups);
    PFN_TRY(pf_check_workspace(who, ws, ws_bytes, slabs + (lds ? 0 : (size_t)G * cs_block_bytes(m))));
    const CsArgs a{p, static_cast<const int32_t*>(plan_dev), ratings, islands, severity, worst_line, overloads, base_flow, post_flow,
                   lds ? nullptr : reinterpret_cast<float*>(static_cast<unsigned char*>(ws) + slabs), stride, m, nnz, (int)n_pv,
                   ratings_per_sample != 0, pf_f_in_lds(m)};
    hipStream_t s = static_cast<hipStream_t>(stream);
    PFN_TRY(cs_launch_base(a, h, threads, n_samples, lds1, s));
    {
        const double ss = (double)n_samples, ee = (double)e, nz = (double)nnz;
        const double tl = (double)cs_tiles(e);
        ProfScope ps("contingency_sparse_outages", ss * (tl * (nz * 6.0 + ee * 20.0) + ee * (12.0 + (post_flow ? 4.0 * ee : 0.0))),
                     ss * tl * 64.0 * (2.0 * nz + 8.0 * ee), s);
        PFN_TRY((launch_either<contingency_sparse_outages_kernel<true>, contingency_sparse_outages_kernel<false>>(
            lds, (int)G, 64, cs_block_bytes(m), 0, s, static_cast<const unsigned char*>(plan_dev), static_cast<const unsigned char*>(ws), a.blocks, status,
            islands, severity, worst_line, overloads, post_flow, stride, n, e, m, nnz, (int)n_samples)));
    }
    return PFN_OK;
}

}  // extern "C"
