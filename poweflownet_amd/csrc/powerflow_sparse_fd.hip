// The fast-decoupled modes on the sparse route (gfx950): pfn_powerflow_solve_sparse_fd, ONE launch, one workgroup per sample.  The
// semantics are the dense fast-decoupled route's (powerflow.hip, tests/powerflow_fd_ref.py): B' over the angle buses and B'' over the
// PQ buses are constant -- XB: B' from 1 / x, B'' from x / (r^2 + x^2); BX the other way round --, half-iterations alternate
// theta -= B'^-1 (dP / Vm) and Vm -= B''^-1 (dQ / Vm), the P half first, the fp64 mismatch is re-formed and tested after each, and
// the count is of half-iterations.  Where the dense route inverts the two matrices, this one keeps their sparse fp32 factors: the
// fast-decoupled plan (powerflow_plan.hpp) holds one symbolic factorisation per matrix, each is assembled and factored ONCE per
// sample (powerflow_sparse_core.hpp: the Newton kernel's left-looking column factorisation), and a half-iteration is one mismatch
// walk over the bus's line ends (one fp64 sincos per end, line sums in stored order) and one pair of fp64 substitutions.
//
// Every loop bound comes from the plan, so every barrier is reached by the whole workgroup; what fails a sample (a pivot, a
// non-finite mismatch) is a value all threads read behind a barrier, and they leave together.  One owner per target per step, no
// float atomics, only the max crosses threads: a sample's bits depend neither on its batch nor on the workgroup size.
//
// The mismatch walk's line-end term, the start state, the stopping rule, the view of a sub-plan and its check against the device
// arrays, the table write-back and the sizes of a sample are powerflow_common.hpp's, shared with every route.  The host side of the
// call -- its checks and the launch -- is pfd_solve, exported through powerflow_sparse_fd.hpp: the AC N-1 screen of the sparse route
// (contingency_ac_sparse.hip) makes it for its base launch.
#include "powerflow_common.hpp"
#include "powerflow_sparse_core.hpp"
#include "powerflow_sparse_fd.hpp"

namespace pfn {

struct PfdArgs {
    PfProblem p;                                    // (p.ws: per sample pf_sample_bytes(n, max(m_p, m_q), nnz) -- P's slab first --, ws_stride apart)
    const int32_t* plan;
    size_t ws_stride;
    int m_p, m_q, nnz, bx, f_in_lds;
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void powerflow_sparse_fd_kernel(const PfdArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pfd_smem[];
    __shared__ double s_red[THREADS / 64];
    const int t = threadIdx.x;
    constexpr int nt = THREADS;
    const int s = blockIdx.x;
    const PfProblem& p = a.p;
    const int n = p.n, e = p.e, nnz = a.nnz;
    const int mmax = max(a.m_p, a.m_q);
    const unsigned char* pb = reinterpret_cast<const unsigned char*>(a.plan);
    const int32_t* H = a.plan;
    const PfPlanView hp = pf_plan_view(pb + H[PFD_H_OFF_P]), hq = pf_plan_view(pb + H[PFD_H_OFF_Q]);

    double* vm = reinterpret_cast<double*>(static_cast<unsigned char*>(p.ws) + (size_t)s * a.ws_stride);
    double* th = vm + n;
    double* sp = th + n;
    double* sq = sp + n;
    double* Fg = sq + n;
    float* slab_p = reinterpret_cast<float*>(Fg + mmax);
    float* slab_q = slab_p + hp.nnz;
    float* w = reinterpret_cast<float*>(pfd_smem);
    double* F = a.f_in_lds ? reinterpret_cast<double*>(pfd_smem + pf_w_bytes(mmax)) : Fg;
    const PfSample sm = pf_sample(p, s);
    const double* rx = sm.rx;
    const double* spec = sm.spec;
    const uint8_t* mask = pf_line_mask(p, s);
    double res = __builtin_nan("");

    // ---- the device arrays against the plan, both halves: the bus types decide who has an unknown in B' and in B'' (a PV bus the
    // plan took for PQ is noticed here), the line list the line ends.  A plan whose sizes disagree with the outer header (it cannot
    // come from the builder) is refused before anything is indexed with them, and so is a sample with a line the cover list has no
    // place for.  code is uniform over the workgroup wherever it is tested.
    int code = pf_check_plan(p, hp, nt, hp.A.m != a.m_p || hq.A.m != a.m_q || hp.nnz + hq.nnz != nnz || pf_unplaced(p, s), [&](int i, int ty, int& stale) {
        stale |= hp.adjptr[i] != hq.adjptr[i] || hp.adjptr[i + 1] != hq.adjptr[i + 1];
        return (ty != 0) != (hp.ua[i] >= 0) || (ty == 2) != (hq.ua[i] >= 0);
    });
    if (code == 0) {
        // (the two halves were built from one line list: their line ends agree where that list is the device's; checked all the same)
        int differ = 0;
        for (int q = t; q < 2 * e; q += nt) {
            const int2 x = hp.adj[q], y = hq.adj[q];
            differ |= x.x != y.x || x.y != y.y;
        }
        if (__syncthreads_or(differ)) code = PF_STALE_PLAN;
    }
    if (code == 0 && pf_start_state(p, sm, p.bus_type, H[PFP_H_SLACK], false, nt, vm, th)) code = PF_NON_FINITE;
    int it = 0;
    if (code == 0) {
        // ---- B' and B'': bus i's owner adds the off-diagonals of its row at their planned positions, line ends in stored order
        // (parallel lines add), and the diagonal -- summed in fp64 -- last
        for (int k = t; k < nnz; k += nt) slab_p[k] = 0.f;
        __syncthreads();
        for (int i = t; i < n; i += nt) {
            double dp = 0.0, dq = 0.0;
            const int q1 = hp.adjptr[i + 1];
            for (int q = hp.adjptr[i]; q < q1; ++q) {
                const int k = hp.adj[q].x >> 1;
                if (mask && !mask[k]) continue;                 // a line this sample lacks: a structural zero, its rx is never read
                const int pp = hp.adjpos[q].x, pq = hq.adjpos[q].x;
                const double r = rx[2 * k], x = rx[2 * k + 1];
                const double w_x = 1.0 / x, w_b = x / (r * r + x * x);
                const double wp = a.bx ? w_b : w_x, wq = a.bx ? w_x : w_b;
                dp += wp;
                dq += wq;
                if (pp >= 0) slab_p[pp] += (float)(-wp);
                if (pq >= 0) slab_q[pq] += (float)(-wq);
            }
            const int bp = hp.buspos[i].x, bq = hq.buspos[i].x;
            if (bp >= 0) slab_p[bp] += (float)dp;
            if (bq >= 0) slab_q[bq] += (float)dq;
        }
        __syncthreads();
        // ---- both factors, once
        if (!pfc_factor<THREADS>(hp.A, slab_p, w)) code = PF_SINGULAR;
        __syncthreads();
        if (code == 0 && !pfc_factor<THREADS>(hq.A, slab_q, w)) code = PF_SINGULAR;
        __syncthreads();
    }
    if (code == 0) {
        int half = 0;
        for (;; ++it) {
            // ---- line sums of bus i, its line ends in stored order; the mismatch; the right-hand side of the coming half
            double mx = 0.0;
            for (int i = t; i < n; i += nt) {
                const double vi = vm[i], ti = th[i];
                double sP = 0.0, sQ = 0.0;
                const int q1 = hp.adjptr[i + 1];
                for (int q = hp.adjptr[i]; q < q1; ++q) {
                    const int2 lj = hp.adj[q];
                    const int k = lj.x >> 1, j = lj.y;
                    if (mask && !mask[k]) continue;
                    pf_ac_end(rx[2 * k], rx[2 * k + 1], vi, ti, vm[j], th[j], sP, sQ);
                }
                sp[i] = sP;
                sq[i] = sQ;
                const int ra = hp.ua[i], rv = hq.ua[i];
                if (ra >= 0) {
                    const double f = spec[4 * i + 2] - sP;
                    mx = fmax(mx, pf_abs_clamped(f));
                    if (half == 0) F[ra] = f / vi;
                }
                if (rv >= 0) {
                    const double f = spec[4 * i + 3] - sQ;
                    mx = fmax(mx, pf_abs_clamped(f));
                    if (half == 1) F[rv] = f / vi;
                }
            }
            res = pf_block_max(mx, s_red, THREADS / 64);
            const int stop = pf_stop(res, p.tol, it, p.max_iter);
            if (stop < 0) { code = stop; break; }
            if (stop) break;
            // ---- the half-iteration: fp64 substitutions through the half's factor, then theta -= dx or Vm -= dx
            if (half == 0) {
                pfc_substitute<THREADS>(hp.A, slab_p, F);
                for (int i = t; i < n; i += nt) {
                    const int ra = hp.ua[i];
                    if (ra >= 0) th[i] -= pfc_solution(hp.A, slab_p, F, ra);
                }
            } else {
                pfc_substitute<THREADS>(hq.A, slab_q, F);
                for (int i = t; i < n; i += nt) {
                    const int rv = hq.ua[i];
                    if (rv >= 0) vm[i] -= pfc_solution(hq.A, slab_q, F, rv);
                }
            }
            half = a.m_q ? 1 - half : 0;
            __syncthreads();
        }
    }

    pf_write_back(p, sm, s, false, nt, code, it, res, vm, th, sp, sq);
}

int pfd_check_header(const int32_t* h, const char* who) {
    PFN_CHECK_ARG(h, "%s: null plan header", who);
    PFN_CHECK_ARG(h[PFP_H_MAGIC] == PFD_MAGIC && h[PFP_H_VERSION] == PFP_VERSION && h[PFP_H_MODE] == PFD_MODE,
                  "%s: not a fast-decoupled sparse power-flow plan (magic %08x, version %d)", who, (unsigned)h[PFP_H_MAGIC], (int)h[PFP_H_VERSION]);
    PFN_CHECK_ARG(h[PFP_H_N] >= 1 && h[PFP_H_E] >= 0 && h[PFP_H_M] >= 0 && h[PFD_H_M_Q] >= 0 && h[PFD_H_M_Q] <= h[PFP_H_M] &&
                      h[PFP_H_M] < h[PFP_H_N] && h[PFP_H_NNZ] >= h[PFP_H_M] + h[PFD_H_M_Q] && h[PFD_H_OFF_P] >= 4 * PFP_HEADER_WORDS &&
                      h[PFD_H_OFF_Q] > h[PFD_H_OFF_P] && h[PFD_H_OFF_Q] < h[PFP_H_BYTES] && ((h[PFD_H_OFF_P] | h[PFD_H_OFF_Q]) & 15) == 0,
                  "%s: the plan header is inconsistent", who);
    return PFN_OK;
}

// the whole call under the caller's name: the checks, then the one launch (powerflow_sparse_fd.hpp)
int pfd_solve(const char* who, const int64_t* edge_index, int64_t n_lines, const double* rx, const uint8_t* line_mask, const int32_t* unplaced,
              const int32_t* bus_type, const double* spec, const double* init, int64_t n_samples, int64_t n_bus, int mode, double tol, int max_iter,
              const void* plan_header, const void* plan_dev, int threads, double* table, int32_t* status, double* residual, int32_t* flags, void* ws,
              size_t ws_bytes, void* stream) {
    const int32_t* h = static_cast<const int32_t*>(plan_header);
    PFN_TRY(pfd_check_header(h, who));
    PFN_CHECK_ARG(mode == 2 || mode == 3, "%s: mode must be 2 (fdxb) or 3 (fdbx); modes 0 and 1 are pfn_powerflow_solve_sparse's", who);
    PFN_CHECK_ARG(h[PFP_H_N] == n_bus && h[PFP_H_E] == n_lines, "%s: the plan is for %d buses, %d lines; the call has %lld, %lld", who,
                  (int)h[PFP_H_N], (int)h[PFP_H_E], (long long)n_bus, (long long)n_lines);
    const int n = h[PFP_H_N], m_p = h[PFP_H_M], m_q = h[PFD_H_M_Q], nnz = h[PFP_H_NNZ], mmax = std::max(m_p, m_q);
    PFN_TRY(pf_check_sparse_launch(who, threads, unplaced, n_samples, h, mmax));
    const size_t stride = pf_sample_bytes(n, mmax, nnz), need = (size_t)n_samples * stride;
    const PfdArgs a{{edge_index, rx, bus_type, spec, init, table, status, residual, flags, ws, tol, n, h[PFP_H_E], max_iter, line_mask, unplaced},
                    static_cast<const int32_t*>(plan_dev), stride, m_p, m_q, nnz, mode == 3, pf_f_in_lds(mmax)};
    PFN_TRY(pf_check_call(who, a.p, n_samples, &plan_dev, "the workspace and the plan 16-byte"));
    if (n_samples == 0) return PFN_OK;
    const size_t lds = pf_lds_bytes(mmax);
    PFN_CHECK_ARG(lds <= (size_t)(kLdsCuBytes - kLdsReserve), "%s: a work vector of %d unknowns needs %zu bytes of LDS, %d are there", who, mmax, lds,
                  kLdsCuBytes - kLdsReserve);
    PFN_TRY(pf_check_workspace(who, ws, ws_bytes, need));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double madds = (double)(((int64_t)h[PFP_H_MADDS_HI] << 32) | (uint32_t)h[PFP_H_MADDS_LO]);
    // (the model: one factor of each half, and some twenty half-iterations of one pair of substitutions and one mismatch walk)
    ProfScope ps(mode == 3 ? "powerflow_sparse_fdbx" : "powerflow_sparse_fdxb",
                 (double)n_samples * ((double)n_lines * 16.0 + (double)n * 64.0 + (init ? (double)n * 16.0 : 0.0)) + (double)h[PFP_H_BYTES],
                 (double)n_samples * 2.0 * (madds + 20.0 * (double)h[PFP_H_NNZ]), s);
    return pf_launch_sparse(powerflow_sparse_fd_kernel<64>, powerflow_sparse_fd_kernel<256>, threads, h[PFP_H_MAX_COL], n_samples, lds, s, a);
}

}  // namespace pfn

using namespace pfn;

extern "C" {

size_t pfn_powerflow_sparse_fd_workspace_bytes(int64_t n_samples, const void* plan_header) {
    const int32_t* h = static_cast<const int32_t*>(plan_header);
    if (n_samples <= 0 || pfd_check_header(h, "pfn_powerflow_sparse_fd_workspace_bytes") != PFN_OK) return 0;
    return (size_t)n_samples * pf_sample_bytes(h[PFP_H_N], std::max(h[PFP_H_M], h[PFD_H_M_Q]), h[PFP_H_NNZ]);
}

int pfn_powerflow_solve_sparse_fd_masked(const int64_t* edge_index, int64_t n_lines, const double* rx, const uint8_t* line_mask,
                                         const int32_t* unplaced, const int32_t* bus_type, const double* spec, const double* init,
                                         int64_t n_samples, int64_t n_bus, int mode, double tol, int max_iter, const void* plan_header,
                                         const void* plan_dev, int threads, double* table, int32_t* status, double* residual,
                                         int32_t* flags, void* ws, size_t ws_bytes, void* stream) {
    return pfd_solve(line_mask || unplaced ? "pfn_powerflow_solve_sparse_fd_masked" : "pfn_powerflow_solve_sparse_fd", edge_index, n_lines, rx, line_mask,
                     unplaced, bus_type, spec, init, n_samples, n_bus, mode, tol, max_iter, plan_header, plan_dev, threads, table, status, residual, flags,
                     ws, ws_bytes, stream);
}

int pfn_powerflow_solve_sparse_fd(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                                  const double* init, int64_t n_samples, int64_t n_bus, int mode, double tol, int max_iter,
                                  const void* plan_header, const void* plan_dev, int threads, double* table, int32_t* status,
                                  double* residual, int32_t* flags, void* ws, size_t ws_bytes, void* stream) {
    return pfn_powerflow_solve_sparse_fd_masked(edge_index, n_lines, rx, nullptr, nullptr, bus_type, spec, init, n_samples, n_bus, mode, tol,
                                                max_iter, plan_header, plan_dev, threads, table, status, residual, flags, ws, ws_bytes, stream);
}

}  // extern "C"
