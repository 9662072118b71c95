// Batched AC / DC power flow on the device (gfx950): pfn_powerflow_solve, ONE launch, one workgroup per sample.  The solver side of
// the reference (dataset_generator.py's pp.runpp, dc_error.py's pp.rundcpp) for this project's network model: series admittance
// only, every stored line counted in both directions, P and Q demand-positive per-unit, Va in degrees -- the mismatch is exactly
// pfn_power_imbalance's dP_i, dQ_i (physics.hip), so the two check each other.
//
// Newton-Raphson in polar form from a flat start.  The state, the mismatch F and the convergence test are fp64; the matrix
// A = d(line sums)/d(unknowns) = -dF/dx is assembled analytically, stored and factorised in fp32 (LU, partial pivoting, ties to the
// lowest row) and A dx = F is solved from that factor with the right-hand side kept in fp64.  An fp32 factor costs convergence
// rate only: the residual that decides is fp64.  mode 1 (DC) runs the same loop on F(theta) = B' theta + P, B' from 1 / x: the
// loop is then iterative refinement of an fp32 factor (re-formed per pass: it is a constant) under the same fp64 tolerance.
//
// Unknowns / equations: theta of the non-slack buses in bus order (P equations), then Vm of the PQ buses in bus order (Q equations).
// A bus row is gathered by scanning the stored line list -- n * e loads against m^3 / 3 multiply-adds -- which keeps stored order:
// one owner per row, sequential sums, no float atomics, max-reductions only across threads.  A sample's result is a pure function
// of its own inputs; nothing depends on the batch around it.
//
// The matrix is row-major with an ODD leading dimension ld = m | 1: the rank-1 update walks rows (lanes on consecutive columns, the
// multiplier a broadcast), the pivot search and the back substitution walk columns (stride ld: odd, so coprime to the 32 banks a
// dword access of a 32-lane half is spread over: no conflict).  LDS route: the matrix sits behind the sample's vectors in LDS;
// global route: in a per-sample slab of the caller's workspace, same code.
//
// pfn_powerflow_solve_init adds a warm start (the state begins at the caller's Vm / Va instead of the flat start) and the two
// fast-decoupled iterations, modes 2 (XB) and 3 (BX): the same fp64 state, mismatch and convergence test, but the update comes from
// two CONSTANT matrices -- B' over the angle buses, B'' over the PQ buses, both Laplacians of the stored lines -- that are built once
// per sample in fp32, inverted in place once (Gauss-Jordan, no pivoting: they are symmetric and diagonally dominant for x > 0, and the
// elimination keeps that) and stay resident together; a half-iteration is then a mat-vec, theta -= B'^-1 (dP / Vm) or
// Vm -= B''^-1 (dQ / Vm), one owner per row, with no sequential chain and one barrier.  The FD template instantiation carries that
// code; the Newton / DC instantiation does not pay registers for it.
//
// What this kernel shares with the sparse routes -- the status codes, the start state, the line-end terms, the stopping rule, the
// table write-back, the argument checks -- is powerflow_common.hpp's; the Newton pass itself (rows, LU, update), shared with the
// Q-limit kernel, and the route decision are powerflow_dense.hpp's -- and so is the sample's whole solve (pf_solve_sample, with the
// fast-decoupled matrices' build in pf_fd_inverses): the AC contingency screen's base launch (contingency_ac.hip) runs the same text,
// so its base table is this kernel's, bit for bit.  The kernel below places the matrix and calls it.
#include <algorithm>

#include "powerflow_dense.hpp"

namespace pfn {

// (the dense cap, the workgroup sizes, pf_ld, pf_mat_floats and the Gauss-Jordan inverse: powerflow_dense.hpp, with contingency.hip)
// (the sample's vectors, pf_vec_bytes / pf_fd_extra_bytes, the argument block PfArgs and the sample's whole solve, pf_solve_sample:
// powerflow_dense.hpp, with contingency_ac.hip's base launch)

template <bool LDS, bool FD>
__global__ __launch_bounds__(PF_BIG_THREADS) void powerflow_kernel(const PfArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pf_smem[];
    const int s = blockIdx.x;
    const PfProblem& p = a.p;
    const int n = p.n, m = a.m;
    const int mp = n - 1, mq = a.n_pq;
    float* A;
    if constexpr (LDS) A = reinterpret_cast<float*>(pf_smem + pf_vec_bytes(n, m) + (FD ? pf_fd_extra_bytes(m) : 0));
    else A = static_cast<float*>(p.ws) + (size_t)s * (FD ? pf_mat_floats(mp) + pf_mat_floats(mq) : pf_mat_floats(m));
    pf_solve_sample<FD>(a, s, pf_smem, A);
}

static int pf_unknowns(int64_t n, int64_t n_pq, int mode) { return (int)((n - 1) + (mode == 1 ? 0 : n_pq)); }
static bool pf_fits_lds(int n, int m) { return pf_vec_bytes(n, m) + pf_mat_floats(m) * 4 <= (size_t)(kLdsCuBytes - kLdsReserve); }
// modes 2, 3: the vectors (with F / Vm behind them) and BOTH matrices, resident together
static size_t pf_fd_mat_floats(int n, int n_pq) { return pf_mat_floats(n - 1) + pf_mat_floats(n_pq); }
static size_t pf_fd_lds_bytes(int n, int n_pq) {
    const int m = (n - 1) + n_pq;
    return pf_vec_bytes(n, m) + pf_fd_extra_bytes(m) + pf_fd_mat_floats(n, n_pq) * 4;
}
static bool pf_fd_fits_lds(int n, int n_pq) { return pf_fd_lds_bytes(n, n_pq) <= (size_t)(kLdsCuBytes - kLdsReserve); }

}  // namespace pfn

using namespace pfn;

extern "C" {

int64_t pfn_powerflow_max_unknowns(void) { return PF_MAX_UNKNOWNS; }

size_t pfn_powerflow_workspace_bytes(int64_t n_samples, int64_t n_bus, int64_t n_lines, int64_t n_pq, int route) {
    (void)n_lines;
    if (n_samples <= 0 || n_bus <= 0 || n_pq < 0 || n_pq >= n_bus || n_bus > PF_MAX_UNKNOWNS + 1) return 0;
    const int m = pf_unknowns(n_bus, n_pq, 0);      // (mode 1: the caller passes n_pq = 0)
    if (m > PF_MAX_UNKNOWNS || route == 1 || (route != 2 && pf_fits_lds((int)n_bus, m))) return 0;
    return (size_t)n_samples * pf_mat_floats(m) * sizeof(float);
}

size_t pfn_powerflow_workspace_bytes_mode(int64_t n_samples, int64_t n_bus, int64_t n_lines, int64_t n_pq, int mode, int route) {
    if (mode == 0) return pfn_powerflow_workspace_bytes(n_samples, n_bus, n_lines, n_pq, route);
    if (mode < 0 || mode > 3 || n_samples <= 0 || n_bus <= 0 || n_pq < 0 || n_pq >= n_bus || n_bus > PF_MAX_UNKNOWNS + 1) return 0;
    if (mode == 1) return pfn_powerflow_workspace_bytes(n_samples, n_bus, n_lines, 0, route);       // its m is n_bus - 1
    if (route == 1 || (route != 2 && pf_fd_fits_lds((int)n_bus, (int)n_pq))) return 0;
    return (size_t)n_samples * pf_fd_mat_floats((int)n_bus, (int)n_pq) * sizeof(float);
}

int pfn_powerflow_solve_init(const int64_t* edge_index, int lines_per_sample, int64_t n_lines, const double* rx, const int32_t* bus_type,
                             const double* spec, const double* init, int64_t n_samples, int64_t n_bus, int64_t n_pv, int64_t n_pq, int mode,
                             double tol, int max_iter, int route, double* table, int32_t* status, double* residual, int32_t* flags,
                             void* ws, size_t ws_bytes, void* stream) {
    PFN_CHECK_ARG(n_samples >= 0 && n_bus >= 1 && n_lines >= 0 && n_samples < (1ll << 29) && n_lines < (1ll << 24) && n_bus < (1ll << 24),
                  "pfn_powerflow_solve: bad sizes (%lld samples of %lld buses and %lld lines)", (long long)n_samples, (long long)n_bus,
                  (long long)n_lines);
    PFN_CHECK_ARG(n_pv >= 0 && n_pq >= 0 && n_pv + n_pq == n_bus - 1,
                  "pfn_powerflow_solve: %lld PV and %lld PQ buses do not leave exactly one slack among %lld buses", (long long)n_pv,
                  (long long)n_pq, (long long)n_bus);
    PFN_CHECK_ARG(mode >= 0 && mode <= 3, "pfn_powerflow_solve: mode must be 0 (AC), 1 (DC), 2 (fast-decoupled XB) or 3 (fast-decoupled BX)");
    PFN_CHECK_ARG(route >= 0 && route <= 2, "pfn_powerflow_solve: route must be 0 (auto), 1 (LDS) or 2 (global)");
    const bool fd = mode >= 2;
    const int64_t m64 = (n_bus - 1) + (mode == 1 ? 0 : n_pq);      // equations; modes 2, 3 hold no matrix of that order: their larger one is n_bus - 1
    PFN_CHECK_ARG((fd ? n_bus - 1 : m64) <= PF_MAX_UNKNOWNS,
                  "pfn_powerflow_solve: %lld unknowns per sample exceed the dense solver's %d; a sparse factorisation is needed (pfn_powerflow_solve_sparse, route \"sparse\")",
                  (long long)(fd ? n_bus - 1 : m64), PF_MAX_UNKNOWNS);
    const int n = (int)n_bus, m = (int)m64;
    PfArgs a{{edge_index, rx, bus_type, spec, init, table, status, residual, flags, ws, tol, n, (int)n_lines, max_iter},
             m, (int)n_pv, (int)n_pq, mode, lines_per_sample != 0};
    PFN_TRY(pf_check_call("pfn_powerflow_solve", a.p, n_samples, nullptr, "the workspace 16-byte"));
    if (n_samples == 0) return PFN_OK;
    const size_t lds_need = fd ? pf_fd_lds_bytes(n, (int)n_pq) : pf_vec_bytes(n, m) + pf_mat_floats(m) * 4;
    const size_t mat_floats = fd ? pf_fd_mat_floats(n, (int)n_pq) : pf_mat_floats(m);
    bool lds;
    PFN_TRY(pf_dense_route("pfn_powerflow_solve", route, m, n, lds_need, n_samples, mat_floats, ws, ws_bytes, &lds));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int big = fd ? std::max(n - 1, (int)n_pq) : m;            // the rule of the one matrix, applied to the larger of the two
    const int threads = big > PF_BIG_M ? PF_BIG_THREADS : PF_SMALL_THREADS;
    const size_t bytes = pf_vec_bytes(n, m) + (fd ? pf_fd_extra_bytes(m) : 0) + (lds ? mat_floats * 4 : 0);
    const double iters = 5.0, mm = (double)m, mp = (double)(n - 1), mq = (double)n_pq;
    static const char* const names[4] = {"powerflow_ac", "powerflow_dc", "powerflow_fdxb", "powerflow_fdbx"};
    ProfScope ps(names[mode], (double)n_samples * ((double)n_lines * (16.0 + (lines_per_sample ? 16.0 : 0.0)) + (double)n * 64.0 + (init ? (double)n * 16.0 : 0.0)),
                 fd ? (double)n_samples * (2.0 * (mp * mp * mp + mq * mq * mq) + 20.0 * (mp * mp + mq * mq))
                    : (double)n_samples * iters * (2.0 / 3.0 * mm * mm * mm + 2.0 * mm * mm), s);
    static std::atomic<uint64_t> raised{0}, raised_fd{0};
    if (lds && !fd) {
        PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(powerflow_kernel<true, false>), kLdsCuBytes - kLdsReserve, raised));
        powerflow_kernel<true, false><<<(int)n_samples, threads, bytes, s>>>(a);
    } else if (lds) {
        PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(powerflow_kernel<true, true>), kLdsCuBytes - kLdsReserve, raised_fd));
        powerflow_kernel<true, true><<<(int)n_samples, threads, bytes, s>>>(a);
    } else if (!fd) {
        powerflow_kernel<false, false><<<(int)n_samples, threads, bytes, s>>>(a);
    } else {
        powerflow_kernel<false, true><<<(int)n_samples, threads, bytes, s>>>(a);
    }
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

int pfn_powerflow_solve(const int64_t* edge_index, int lines_per_sample, int64_t n_lines, const double* rx, const int32_t* bus_type,
                        const double* spec, int64_t n_samples, int64_t n_bus, int64_t n_pv, int64_t n_pq, int mode, double tol,
                        int max_iter, int route, double* table, int32_t* status, double* residual, int32_t* flags, void* ws,
                        size_t ws_bytes, void* stream) {
    PFN_CHECK_ARG(mode == 0 || mode == 1, "pfn_powerflow_solve: mode must be 0 (AC) or 1 (DC)");
    return pfn_powerflow_solve_init(edge_index, lines_per_sample, n_lines, rx, bus_type, spec, nullptr, n_samples, n_bus, n_pv, n_pq, mode,
                                    tol, max_iter, route, table, status, residual, flags, ws, ws_bytes, stream);
}

}  // extern "C"
