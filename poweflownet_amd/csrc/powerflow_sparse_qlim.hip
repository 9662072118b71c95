// AC power flow with generator Q-limits and per-sample bus types on the sparse route (gfx950): pfn_powerflow_solve_sparse_qlim, ONE
// launch, one workgroup per sample, the rounds inside the kernel, no host read.  It joins powerflow_sparse.hip's Newton pass -- the
// plan's line-end walk, the fp32 left-looking factor under a static order, the fp64 right-hand side (powerflow_sparse_core.hpp) --
// with powerflow_qlim.hip's round loop, for grids beyond the dense cap (6470 buses: m_max = 12938).
//
// The plan is the grid's plan for the type row in which EVERY non-slack bus is PQ (utils/powerflow.py qlim_plan: the unchanged host
// builder), so it holds a theta and a Vm unknown at every non-slack bus and m = m_max = 2 (n - 1).  A sample's live types only say
// which Vm unknowns are DEAD: the Vm of a bus that is PV now.  A dead unknown is an identity row and column -- diagonal 1, every
// other entry of its row and column a structural zero, right-hand side 0 --, so its pivot is exactly 1, its L and U parts stay
// zero, its solution is 0 and it contributes nothing to any other column: the factor is the factor of the live matrix under the
// induced order (a factorisation under a static order without pivoting stays valid on any superset of the pattern).
// Nothing is renumbered between rounds: switching a PV bus to PQ flips its live type, and the next assembly fills the row and
// column in.  The update skips dead unknowns, so a PV bus's Vm stays its set point bit for bit.
//
// Storage.  The live type ty [n] stands as BYTES in LDS behind the work vector w (and the right-hand side, where that is in LDS):
// every line end reads ty[j].  The effective Q specification qs [n] (fp64: the given Q, or the limit a switched bus was fixed at) is
// read once per bus and pass and stands in the workspace behind the sample's slab.  pf_sample_bytes is unchanged; the sizer here
// adds qs.
//
// Rounds, statuses and the table are powerflow_qlim.hip's exactly, by the same text (powerflow_qlim.hpp: pfq_switch tests the live PV
// buses against their limits, pfq_write_back writes the table and the final types); max_iter bounds the solves of each inner loop,
// max_rounds the re-solves (-7 after them); status >= 0 is the total of solves.  With a line mask (the cover route's,
// powerflow_cover.hip) every sample has its own line list as well.
//
// Every loop bound comes from the plan or is uniform over the workgroup, and every exit is taken by all threads after a barrier.
// powerflow_common.hpp's device functions (the start state reads ty) and powerflow_sparse_core.hpp are called as they stand; the
// round's limit test and the write-back, which read ty and qs, are powerflow_qlim.hpp's, shared with powerflow_qlim.hip.  A sample's
// bits are a function of (sample, plan) alone.
#include "powerflow_qlim.hpp"
#include "powerflow_sparse_core.hpp"

namespace pfn {

// LDS: powerflow_sparse.hip's w (and F), then ty [n] bytes;  workspace: its sample, then qs [n] doubles
__host__ __device__ inline size_t pfsq_lds_bytes(int n, int m) { return pf_lds_bytes(m) + (((size_t)n + 15) & ~(size_t)15); }
__host__ __device__ inline size_t pfsq_sample_bytes(int n, int m, int nnz) { return pf_sample_bytes(n, m, nnz) + (((size_t)8 * n + 15) & ~(size_t)15); }

struct PfsqArgs {
    PfProblem p;                                    // (p.bus_type: [n] or [S, n]; p.ws: per sample pfsq_sample_bytes, ws_stride apart)
    const int32_t* plan;
    const double* q_limits;                         // [n, 2] or [S, n, 2] = (lo, hi), or null: no limits
    int32_t* bus_type_out;                          // [S, n]
    int32_t* rounds;                                // [S]
    size_t ws_stride;
    double q_tol;
    int m, nnz, f_in_lds, max_rounds, types_per_sample, limits_per_sample;
};

// Four waves per SIMD, the sparse Newton kernel's residency: left alone the kernel takes 134-135 VGPRs and holds three workgroups of
// 256 threads on a compute unit where that one holds four, which at 1024 samples of (1100, 1530) is a second pass over the device
// (DESIGN 7r).  The cap costs one 8-byte spill at the kernel's start and one reload per round, outside every Newton loop.
template <int THREADS, bool MASKED>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void powerflow_sparse_qlim_kernel(const PfsqArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pfsq_smem[];
    __shared__ double s_red[THREADS / 64];
    const int t = threadIdx.x;
    constexpr int nt = THREADS;
    const int s = blockIdx.x;
    const PfProblem& p = a.p;
    const int n = p.n, m = a.m, nnz = a.nnz;
    const PfPlanView v = pf_plan_view(reinterpret_cast<const unsigned char*>(a.plan));
    const int32_t* ua = v.ua;
    const int32_t* uv = v.uv;
    const PfcMatrix A{v.A.colptr, v.A.diag, v.A.row, m};
    const int slack = a.plan[PFP_H_SLACK];

    unsigned char* base = static_cast<unsigned char*>(p.ws) + (size_t)s * a.ws_stride;
    double* vm = reinterpret_cast<double*>(base);
    double* th = vm + n;
    double* sp = th + n;
    double* sq = sp + n;
    double* Fg = sq + n;
    float* slab = reinterpret_cast<float*>(Fg + m);
    double* qs = reinterpret_cast<double*>(base + pf_sample_bytes(n, m, nnz));
    float* w = reinterpret_cast<float*>(pfsq_smem);
    double* F = a.f_in_lds ? reinterpret_cast<double*>(pfsq_smem + pf_w_bytes(m)) : Fg;
    uint8_t* ty = pfsq_smem + pf_lds_bytes(m);
    const PfSample sm = pf_sample(p, s);
    const double* rx = sm.rx;
    const double* spec = sm.spec;
    const uint8_t* mask = MASKED ? pf_line_mask(p, s) : nullptr;
    const int32_t* ty_in = p.bus_type + (a.types_per_sample ? (int64_t)s * n : 0);
    const double* ql = a.q_limits ? a.q_limits + (a.limits_per_sample ? (int64_t)s * 2 * n : 0) : nullptr;
    double res = __builtin_nan("");

    // ---- the sample's own type row and its Q specification; from here on the workgroup reads and re-types the copy only
    const int gone = pf_unplaced(p, s);
    int ns = 0;
    for (int i = t; i < n; i += nt) {
        const int y = ty_in[i];
        ty[i] = (uint8_t)((unsigned)y > 2u ? 3 : y);
        ns += y == 0;
        qs[i] = spec[4 * i + 3];
    }
    const int one = __syncthreads_count(ns == 1), many = __syncthreads_or(ns > 1);
    // ---- the device arrays against the plan (pf_check_plan on the sample's row: a type outside 0 / 1 / 2 is PF_BAD_TYPES there): the
    // plan has theta and Vm at every bus but its slack, the sample's slack is the plan's, the line list is the plan's
    PfProblem own = p;
    own.bus_type = ty_in;
    int code = pf_check_plan(own, v, nt, gone, [&](int i, int y, int& stale) {
        stale |= (i != slack) != (ua[i] >= 0) || (i != slack) != (uv[i] >= 0) || (y == 0) != (i == slack);
        return false;
    });
    if (!gone && code != PF_BAD_TYPES && (one != 1 || many)) {      // not exactly one slack: the types' fault before the plan's
        code = PF_BAD_TYPES;
        if (t == 0) p.flags[0] = p.flags[0] | 1;    // (every writer stores the same bit over the same word)
    }

    int it = 0, rounds = 0;                          // solves over all rounds; re-solves begun
    if (code == 0 && pf_start_state(p, sm, ty, slack, false, nt, vm, th)) code = PF_NON_FINITE;
    while (code == 0) {
        for (int inner = 0;; ++inner, ++it) {
            for (int k = t; k < nnz; k += nt) slab[k] = 0.f;
            __syncthreads();
            // ---- (1) line sums, mismatch and Jacobian entries of bus i, its line ends in stored order; a row or a column that is
            // the Vm of a bus not live-PQ is skipped
            for (int i = t; i < n; i += nt) {
                const int ra = ua[i], rv = uv[i];
                const bool li = ty[i] == 2;
                const double vi = vm[i], ti = th[i];
                double sP = 0.0, sQ = 0.0, dPt = 0.0, dPv = 0.0, dQt = 0.0, dQv = 0.0;
                const int q1 = v.adjptr[i + 1];
                for (int q = v.adjptr[i]; q < q1; ++q) {
                    const int2 lj = v.adj[q];
                    const int4 pos = v.adjpos[q];
                    const int k = lj.x >> 1, j = lj.y;
                    if (MASKED && mask && !mask[k]) continue;   // a line this sample lacks: a structural zero, its rx is never read
                    const bool lv = ty[j] == 2;
                    const double r = rx[2 * k], x = rx[2 * k + 1];
                    const PfEndJac J = pf_ac_end_jac(pf_ac_end(r, x, vi, ti, vm[j], th[j], sP, sQ), vi);
                    dPt += J.pti;
                    dPv += J.pvi;
                    dQt += J.qti;
                    dQv += J.qvi;
                    if (pos.x >= 0) slab[pos.x] += (float)(-J.pti);
                    if (pos.y >= 0 && lv) slab[pos.y] += (float)J.pvj;
                    if (pos.z >= 0 && li) slab[pos.z] += (float)(-J.qti);
                    if (pos.w >= 0 && li && lv) slab[pos.w] += (float)J.qvj;
                }
                sp[i] = sP;
                sq[i] = sQ;
                const int4 bp = v.buspos[i];
                if (ra >= 0) {
                    F[ra] = spec[4 * i + 2] - sP;
                    slab[bp.x] += (float)dPt;
                    if (li) slab[bp.y] += (float)dPv;
                }
                if (rv >= 0) {
                    if (li) {
                        F[rv] = qs[i] - sQ;
                        slab[bp.z] += (float)dQt;
                        slab[bp.w] += (float)dQv;
                    } else {                        // a dead unknown: the identity row and column
                        F[rv] = 0.0;
                        slab[bp.w] = 1.0f;
                    }
                }
            }
            __syncthreads();
            // ---- (2) max |F| in fp64; a non-finite entry counts as +inf
            double mx = 0.0;
            for (int k = t; k < m; k += nt) mx = fmax(mx, pf_abs_clamped(F[k]));
            res = pf_block_max(mx, s_red, THREADS / 64);
            const int stop = pf_stop(res, p.tol, inner, p.max_iter);
            if (stop < 0) { code = stop; break; }
            if (stop) break;
            // ---- (3) left-looking factorisation in plan order, (4) L y = F, then U dx = y (powerflow_sparse_core.hpp)
            if (!pfc_factor<THREADS>(A, slab, w)) { code = PF_SINGULAR; break; }
            pfc_substitute<THREADS>(A, slab, F);
            // ---- (5) x += dx at the live unknowns
            for (int i = t; i < n; i += nt) {
                const int ia = ua[i], iv = uv[i];
                if (ia >= 0) th[i] += pfc_solution(A, slab, F, ia);
                if (iv >= 0 && ty[i] == 2) vm[i] += pfc_solution(A, slab, F, iv);
            }
            __syncthreads();
        }
        if (code) break;
        // ---- the round's limits (powerflow_qlim.hpp): no violator, done
        if (!pfq_switch(ty, qs, sq, ql, a.q_tol, n, nt)) break;
        if (rounds >= a.max_rounds) { code = PF_QLIM_ROUNDS; break; }
        ++rounds;
    }

    pfq_write_back(p, sm, s, nt, code, it, res, rounds, ty_in, ty, vm, th, sp, sq, qs, a.bus_type_out, a.rounds);
}

static int pfsq_check_header(const int32_t* h, const char* who) {
    PFN_TRY(pf_check_plan_header(who, h));
    PFN_CHECK_ARG(h[PFP_H_MODE] == 0 && h[PFP_H_M] == 2 * (h[PFP_H_N] - 1),
                  "%s: the plan has %d unknowns of %d buses in mode %d; Q-limits take the AC plan of the grid with every non-slack bus PQ, %d unknowns",
                  who, (int)h[PFP_H_M], (int)h[PFP_H_N], (int)h[PFP_H_MODE], 2 * ((int)h[PFP_H_N] - 1));
    return PFN_OK;
}

}  // namespace pfn

using namespace pfn;

extern "C" {

size_t pfn_powerflow_sparse_qlim_workspace_bytes(int64_t n_samples, const void* plan_header) {
    const int32_t* h = static_cast<const int32_t*>(plan_header);
    if (n_samples <= 0 || pfsq_check_header(h, "pfn_powerflow_sparse_qlim_workspace_bytes") != PFN_OK) return 0;
    return (size_t)n_samples * pfsq_sample_bytes(h[PFP_H_N], h[PFP_H_M], h[PFP_H_NNZ]);
}

int pfn_powerflow_solve_sparse_qlim(const int64_t* edge_index, int64_t n_lines, const double* rx, const uint8_t* line_mask,
                                    const int32_t* unplaced, const int32_t* bus_type, int types_per_sample, const double* spec,
                                    const double* init, const double* q_limits, int limits_per_sample, int64_t n_samples, int64_t n_bus,
                                    double tol, double q_tol, int max_iter, int max_rounds, const void* plan_header, const void* plan_dev,
                                    int threads, double* table, int32_t* status, double* residual, int32_t* flags, int32_t* bus_type_out,
                                    int32_t* rounds, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "pfn_powerflow_solve_sparse_qlim";
    const int32_t* h = static_cast<const int32_t*>(plan_header);
    PFN_TRY(pfsq_check_header(h, who));
    PFN_CHECK_ARG(h[PFP_H_N] == n_bus && h[PFP_H_E] == n_lines, "%s: the plan is for %d buses, %d lines; the call has %lld, %lld", who,
                  (int)h[PFP_H_N], (int)h[PFP_H_E], (long long)n_bus, (long long)n_lines);
    const int n = h[PFP_H_N], m = h[PFP_H_M], nnz = h[PFP_H_NNZ];
    PFN_TRY(pf_check_sparse_launch(who, threads, unplaced, n_samples, h, m));
    PFN_TRY(pfq_check_call(who, n_samples, bus_type, q_limits, limits_per_sample, q_tol, max_rounds, bus_type_out, rounds));
    const size_t stride = pfsq_sample_bytes(n, m, nnz), need = (size_t)n_samples * stride;
    const PfsqArgs a{{edge_index, rx, bus_type, spec, init, table, status, residual, flags, ws, tol, n, h[PFP_H_E], max_iter, line_mask, unplaced},
                     static_cast<const int32_t*>(plan_dev), q_limits, bus_type_out, rounds, stride, q_tol, m, nnz, pf_f_in_lds(m), max_rounds,
                     types_per_sample != 0, limits_per_sample != 0};
    PFN_TRY(pf_check_call(who, a.p, n_samples, &plan_dev, "the workspace and the plan 16-byte"));
    if (n_samples == 0) return PFN_OK;
    const size_t lds = pfsq_lds_bytes(n, m);
    PFN_CHECK_ARG(lds <= (size_t)(kLdsCuBytes - kLdsReserve), "%s: a work vector of %d unknowns and %d type bytes need %zu bytes of LDS, %d are there",
                  who, m, n, lds, kLdsCuBytes - kLdsReserve);
    PFN_TRY(pf_check_workspace(who, ws, ws_bytes, need));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double madds = (double)(((int64_t)h[PFP_H_MADDS_HI] << 32) | (uint32_t)h[PFP_H_MADDS_LO]);
    // (the figures of eight solves, a sample that switches in two rounds: an estimate, as the dense entry's)
    ProfScope ps("powerflow_sparse_qlim",
                 (double)n_samples * ((double)n_lines * 16.0 + (double)n * 76.0 + (init ? (double)n * 16.0 : 0.0) + (q_limits ? (double)n * 16.0 : 0.0)) +
                     (double)h[PFP_H_BYTES],
                 (double)n_samples * 8.0 * 2.0 * (madds + 2.0 * (double)h[PFP_H_NNZ_L]), s);
    if (line_mask)
        return pf_launch_sparse<1>(powerflow_sparse_qlim_kernel<64, true>, powerflow_sparse_qlim_kernel<256, true>, threads, h[PFP_H_MAX_COL], n_samples, lds, s, a);
    return pf_launch_sparse(powerflow_sparse_qlim_kernel<64, false>, powerflow_sparse_qlim_kernel<256, false>, threads, h[PFP_H_MAX_COL], n_samples, lds, s, a);
}

}  // extern "C"
