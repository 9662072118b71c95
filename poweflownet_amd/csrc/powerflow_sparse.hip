// The sparse route of the batched power-flow solver (gfx950): pfn_powerflow_solve_sparse, ONE launch, one workgroup per sample, for
// grids beyond the dense cap of powerflow.hip (6470 buses: 10782 unknowns).  The same Newton loop -- fp64 state, mismatch and
// convergence test, an fp32 factor that "only has to point downhill", the right-hand side kept in fp64 -- on a factor that is sparse:
// the elimination order, the filled pattern and the place of every Jacobian entry come from the host plan (powerflow_plan.cpp,
// powerflow_plan.hpp), one per grid, shared by the samples.  No pivoting: the order is static; a pivot that is tiny or NaN fails the
// sample (-2) exactly as a zero pivot column does on the dense route.
//
// One pass:  (1) bus i's owner walks the plan's list of its line ends (O(degree): the dense kernel's scan of the whole line list would
// be 58 M loads at 6470), one fp64 sincos per end, and ADDS the end's Jacobian entries at their planned slab positions -- the slab is
// zeroed first, a (row, column) entry belongs to the row's bus alone, parallel lines add in stored order, the diagonal block is summed
// in fp64 registers and added last;  (2) max |F|, the dense route's stopping rule;  (3) left-looking factorisation by columns: column j
// is scattered into a dense fp32 work vector w [m] in LDS, then for every k of its U part, ascending, U_kj = w[k] is final and the
// lanes subtract L(:, k) U_kj at w[row] -- the pattern is closed under elimination, so every such row is a row of column j -- then the
// pivot test, and the column goes back to the slab with its L part times 1 / pivot;  (4) forward and backward substitution by columns
// on the fp64 right-hand side (in LDS while w and it take at most 80 KiB, else in the workspace);
// (5) x += dx.
//
// Every loop bound comes from the plan, so every barrier is reached by the whole workgroup; what fails a sample (a pivot, a
// non-finite mismatch) is a value all threads read after a barrier, and they leave the loop together.  No float atomics; only the max
// crosses threads.  The metadata of up to 64 columns (where their L parts begin and end) is loaded by the lanes at once and handed
// round with wave shuffles, and a thread's first element of the next L column is requested before the current step's barrier (an
// LDS-only barrier, device_prims.hpp): a k-step then waits for an LDS round trip and a barrier, not for three dependent loads.
// Steps (3) and (4) are powerflow_sparse_core.hpp's, shared with the fast-decoupled kernel (powerflow_sparse_fd.hip); the line-end
// terms of step (1), step (2), the start state, the plan's view and its check against the device arrays, the table write-back and
// the sizes of a sample are powerflow_common.hpp's, shared with every route.
#include "powerflow_common.hpp"
#include "powerflow_sparse_core.hpp"

namespace pfn {

struct PfsArgs {
    PfProblem p;                                    // (p.ws: per sample pf_sample_bytes(n, m, nnz), ws_stride apart)
    const int32_t* plan;
    size_t ws_stride;
    int m, nnz, mode, f_in_lds;
};

// MASKED: the cover route's instantiation, which asks the sample's line mask about every line end.  The one-topology launch takes
// the other one, whose assembly loop is the loop it always was (the test cost the Newton walk 1-1.6 % when it was made at run time;
// DESIGN 7p).
template <int THREADS, bool MASKED>
__global__ __launch_bounds__(THREADS) void powerflow_sparse_kernel(const PfsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pfs_smem[];
    __shared__ double s_red[THREADS / 64];
    const int t = threadIdx.x;
    constexpr int nt = THREADS;
    const int s = blockIdx.x;
    const PfProblem& p = a.p;
    const int n = p.n, m = a.m, nnz = a.nnz;
    const bool dc = a.mode == 1;
    const PfPlanView v = pf_plan_view(reinterpret_cast<const unsigned char*>(a.plan));
    const int32_t* ua = v.ua;
    const int32_t* uv = v.uv;
    const PfcMatrix A{v.A.colptr, v.A.diag, v.A.row, m};

    double* vm = reinterpret_cast<double*>(static_cast<unsigned char*>(p.ws) + (size_t)s * a.ws_stride);
    double* th = vm + n;
    double* sp = th + n;
    double* sq = sp + n;
    double* Fg = sq + n;
    float* slab = reinterpret_cast<float*>(Fg + m);
    float* w = reinterpret_cast<float*>(pfs_smem);
    double* F = a.f_in_lds ? reinterpret_cast<double*>(pfs_smem + pf_w_bytes(m)) : Fg;
    const PfSample sm = pf_sample(p, s);
    const double* rx = sm.rx;
    const double* spec = sm.spec;
    const uint8_t* mask = MASKED ? pf_line_mask(p, s) : nullptr;
    double res = __builtin_nan("");

    // ---- the device arrays against the plan, then the start state; code is uniform over the workgroup wherever it is tested.  A
    // sample with a line the cover list has no place for is stale before anything is looked at
    int code = pf_check_plan(p, v, nt, pf_unplaced(p, s), [&](int i, int ty, int&) { return (ty != 0) != (ua[i] >= 0) || (ty == 2 && !dc) != (uv[i] >= 0); });
    if (code == 0 && pf_start_state(p, sm, p.bus_type, a.plan[PFP_H_SLACK], dc, nt, vm, th)) code = PF_NON_FINITE;
    int it = 0;
    if (code == 0) {
        for (;; ++it) {
            for (int k = t; k < nnz; k += nt) slab[k] = 0.f;
            __syncthreads();
            // ---- (1) line sums, mismatch and Jacobian entries of bus i, its line ends in stored order
            for (int i = t; i < n; i += nt) {
                const int ra = ua[i], rv = uv[i];
                const double vi = vm[i], ti = th[i];
                double sP = 0.0, sQ = 0.0, dPt = 0.0, dPv = 0.0, dQt = 0.0, dQv = 0.0;
                const int q1 = v.adjptr[i + 1];
                for (int q = v.adjptr[i]; q < q1; ++q) {
                    const int2 lj = v.adj[q];
                    const int4 pos = v.adjpos[q];
                    const int k = lj.x >> 1, j = lj.y;
                    if (MASKED && mask && !mask[k]) continue;   // a line this sample lacks: a structural zero, its rx is never read
                    const double r = rx[2 * k], x = rx[2 * k + 1];
                    if (dc) {
                        const double b = pf_dc_end(x, ti, th[j], sP);
                        dPt += b;
                        if (pos.x >= 0) slab[pos.x] += (float)(-b);
                        continue;
                    }
                    const PfEndJac J = pf_ac_end_jac(pf_ac_end(r, x, vi, ti, vm[j], th[j], sP, sQ), vi);
                    dPt += J.pti;
                    dPv += J.pvi;
                    dQt += J.qti;
                    dQv += J.qvi;
                    if (pos.x >= 0) slab[pos.x] += (float)(-J.pti);
                    if (pos.y >= 0) slab[pos.y] += (float)J.pvj;
                    if (pos.z >= 0) slab[pos.z] += (float)(-J.qti);
                    if (pos.w >= 0) slab[pos.w] += (float)J.qvj;
                }
                sp[i] = sP;
                sq[i] = sQ;
                const int4 bp = v.buspos[i];
                if (ra >= 0) {
                    F[ra] = spec[4 * i + 2] - sP;
                    slab[bp.x] += (float)dPt;
                    if (rv >= 0) slab[bp.y] += (float)dPv;
                }
                if (rv >= 0) {
                    F[rv] = spec[4 * i + 3] - sQ;
                    slab[bp.z] += (float)dQt;
                    slab[bp.w] += (float)dQv;
                }
            }
            __syncthreads();
            // ---- (2) max |F| in fp64; a non-finite entry counts as +inf
            double mx = 0.0;
            for (int k = t; k < m; k += nt) mx = fmax(mx, pf_abs_clamped(F[k]));
            res = pf_block_max(mx, s_red, THREADS / 64);
            const int stop = pf_stop(res, p.tol, it, p.max_iter);
            if (stop < 0) { code = stop; break; }
            if (stop) break;
            // ---- (3) left-looking factorisation in plan order (powerflow_sparse_core.hpp)
            if (!pfc_factor<THREADS>(A, slab, w)) { code = PF_SINGULAR; break; }
            // ---- (4) L y = F, then U dx = y, by columns: after its step F[j] is final (the backward one leaves U_jj dx_j)
            pfc_substitute<THREADS>(A, slab, F);
            // ---- (5) x += dx
            for (int i = t; i < n; i += nt) {
                const int ia = ua[i], iv = uv[i];
                if (ia >= 0) th[i] += pfc_solution(A, slab, F, ia);
                if (iv >= 0) vm[i] += pfc_solution(A, slab, F, iv);
            }
            __syncthreads();
        }
    }

    pf_write_back(p, sm, s, dc, nt, code, it, res, vm, th, sp, sq);
}

static int pfs_check_header(const int32_t* h, const char* who) {
    PFN_TRY(pf_check_plan_header(who, h));
    PFN_CHECK_ARG(h[PFP_H_MODE] == 0 || h[PFP_H_MODE] == 1, "%s: the plan header is inconsistent", who);
    return PFN_OK;
}

}  // namespace pfn

using namespace pfn;

extern "C" {

size_t pfn_powerflow_sparse_workspace_bytes(int64_t n_samples, const void* plan_header) {
    const int32_t* h = static_cast<const int32_t*>(plan_header);
    if (n_samples <= 0 || pfs_check_header(h, "pfn_powerflow_sparse_workspace_bytes") != PFN_OK) return 0;
    return (size_t)n_samples * pf_sample_bytes(h[PFP_H_N], h[PFP_H_M], h[PFP_H_NNZ]);
}

int pfn_powerflow_solve_sparse_masked(const int64_t* edge_index, int64_t n_lines, const double* rx, const uint8_t* line_mask,
                                      const int32_t* unplaced, const int32_t* bus_type, const double* spec, const double* init,
                                      int64_t n_samples, int64_t n_bus, int mode, double tol, int max_iter, const void* plan_header,
                                      const void* plan_dev, int threads, double* table, int32_t* status, double* residual,
                                      int32_t* flags, void* ws, size_t ws_bytes, void* stream) {
    const char* who = line_mask || unplaced ? "pfn_powerflow_solve_sparse_masked" : "pfn_powerflow_solve_sparse";
    const int32_t* h = static_cast<const int32_t*>(plan_header);
    PFN_TRY(pfs_check_header(h, who));
    PFN_CHECK_ARG(mode == 0 || mode == 1, "%s: mode must be 0 (AC) or 1 (DC); the fast-decoupled modes 2 and 3 are pfn_powerflow_solve_sparse_fd's", who);
    PFN_CHECK_ARG(h[PFP_H_N] == n_bus && h[PFP_H_E] == n_lines && h[PFP_H_MODE] == mode,
                  "%s: the plan is for %d buses, %d lines, mode %d; the call has %lld, %lld, mode %d", who, (int)h[PFP_H_N],
                  (int)h[PFP_H_E], (int)h[PFP_H_MODE], (long long)n_bus, (long long)n_lines, mode);
    const int n = h[PFP_H_N], m = h[PFP_H_M], nnz = h[PFP_H_NNZ];
    PFN_TRY(pf_check_sparse_launch(who, threads, unplaced, n_samples, h, m));
    const size_t stride = pf_sample_bytes(n, m, nnz), need = (size_t)n_samples * stride;
    const PfsArgs a{{edge_index, rx, bus_type, spec, init, table, status, residual, flags, ws, tol, n, h[PFP_H_E], max_iter, line_mask, unplaced},
                    static_cast<const int32_t*>(plan_dev), stride, m, nnz, mode, pf_f_in_lds(m)};
    PFN_TRY(pf_check_call(who, a.p, n_samples, &plan_dev, "the workspace and the plan 16-byte"));
    if (n_samples == 0) return PFN_OK;
    const size_t lds = pf_lds_bytes(m);
    PFN_CHECK_ARG(lds <= (size_t)(kLdsCuBytes - kLdsReserve), "%s: a work vector of %d unknowns needs %zu bytes of LDS, %d are there", who,
                  m, lds, kLdsCuBytes - kLdsReserve);
    PFN_TRY(pf_check_workspace(who, ws, ws_bytes, need));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double madds = (double)(((int64_t)h[PFP_H_MADDS_HI] << 32) | (uint32_t)h[PFP_H_MADDS_LO]);
    ProfScope ps(mode ? "powerflow_sparse_dc" : "powerflow_sparse_ac",
                 (double)n_samples * ((double)n_lines * 16.0 + (double)n * 64.0 + (init ? (double)n * 16.0 : 0.0)) + (double)h[PFP_H_BYTES],
                 (double)n_samples * 5.0 * 2.0 * (madds + 2.0 * (double)h[PFP_H_NNZ_L]), s);
    if (line_mask) return pf_launch_sparse<1>(powerflow_sparse_kernel<64, true>, powerflow_sparse_kernel<256, true>, threads, h[PFP_H_MAX_COL], n_samples, lds, s, a);
    return pf_launch_sparse(powerflow_sparse_kernel<64, false>, powerflow_sparse_kernel<256, false>, threads, h[PFP_H_MAX_COL], n_samples, lds, s, a);
}

int pfn_powerflow_solve_sparse(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                               const double* init, int64_t n_samples, int64_t n_bus, int mode, double tol, int max_iter,
                               const void* plan_header, const void* plan_dev, int threads, double* table, int32_t* status,
                               double* residual, int32_t* flags, void* ws, size_t ws_bytes, void* stream) {
    return pfn_powerflow_solve_sparse_masked(edge_index, n_lines, rx, nullptr, nullptr, bus_type, spec, init, n_samples, n_bus, mode, tol,
                                             max_iter, plan_header, plan_dev, threads, table, status, residual, flags, ws, ws_bytes, stream);
}

}  // extern "C"
