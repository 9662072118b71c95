// AC power flow with generator Q-limits on the device (gfx950): pfn_powerflow_solve_qlim, ONE launch, one workgroup per sample.  The
// reference's `pp.runpp(..., enforce_q_lims=True)` (dataset_generator.py's ENFORCE_Q_LIMS) for this project's network model: a PV bus
// whose reactive line sum leaves its limits becomes a PQ bus fixed at the limit and the sample is solved again, inside the kernel.
//
// The inner loop is powerflow.hip's dense Newton-Raphson, the same text (powerflow_dense.hpp: pf_dense_rows, pf_lu_solve,
// pf_dense_update): fp64 state, mismatch and stopping rule, the analytic Jacobian in fp32, row-major with an odd leading dimension,
// LU with partial pivoting (ties to the lowest row) and an fp64 right-hand side.  What differs is whose the bus types are: the
// workgroup copies ITS row of `bus_type` ([n] shared or [S, n]) into LDS, numbers its unknowns from that copy and re-types and
// renumbers it between rounds, so the PV / PQ counts are no launch constants and nothing on the host depends on them.  Storage is
// therefore sized for the worst case, every non-slack bus PQ: m_max = 2 (n - 1).  Next to the dense kernel's vectors stand the
// live type ty [n] and the effective Q specification qs [n] (the given Q, or the limit a switched bus was fixed at).
//
// Rounds.  After an inner loop converges, sq [i] of its last pass is the Q the table would write at a PV bus.  Every thread tests
// its PV buses against (lo, hi) -- demand-positive per-unit, the table's Q column; NaN or +-inf: no limit on that side --:
// sq beyond hi + q_tol fixes Q at hi, sq below lo - q_tol at lo, the bus becomes PQ (pfq_switch, powerflow_qlim.hpp).  All violators
// of a round switch together (MATPOWER's and pandapower's default rule), none switches back, the slack is never limited.  No
// violator: done.  Otherwise the unknowns are numbered again -- theta of the non-slack buses in bus order, then Vm of the live PQ
// buses in bus order -- and Newton continues from the current state.  max_iter bounds the solves of each inner loop, max_rounds
// the re-solves; status >= 0 is the total of solves.
//
// The start state is powerflow_common.hpp's, read from the LDS type row; the round's limit test and the write-back, which read that
// row and qs, are powerflow_qlim.hpp's, shared with the sparse route.  The workgroup-size rule is the dense
// kernel's, applied to m_max (the host knows no other m).  A sample's bits are a function of the sample alone.
#include "powerflow_dense.hpp"
#include "powerflow_qlim.hpp"

namespace pfn {

__host__ __device__ inline int pfq_m_max(int n) { return 2 * (n - 1); }
// the sample's vectors: double vm, th, sp, sq, qs [n], F [m_max]; int aidx, vidx, ty [n]; rounded to 16 bytes
__host__ __device__ inline size_t pfq_vec_bytes(int n) {
    return ((size_t)8 * (5 * (size_t)n + pfq_m_max(n)) + (size_t)12 * n + 15) & ~(size_t)15;
}

struct PfQlimArgs {
    PfProblem p;                                    // (p.bus_type: [n] or [S, n]; p.ws: the global route's fp32 slabs)
    const double* q_limits;                         // [n, 2] or [S, n, 2] = (lo, hi), or null: no limits
    int32_t* bus_type_out;                          // [S, n]
    int32_t* rounds;                                // [S]
    double q_tol;
    int max_rounds, lines_per_sample, types_per_sample, limits_per_sample;
};

// the unknowns of the live types, by thread 0: theta of the non-slack buses in bus order, then Vm of the PQ buses in bus order;
// returns their count
__device__ __forceinline__ int pfq_number(const int* ty, int n, int* aidx, int* vidx) {
    int na = 0, nv = 0;
    for (int i = 0; i < n; ++i) {
        const int y = ty[i];
        aidx[i] = y != 0 ? na++ : -1;
        vidx[i] = y == 2 ? (n - 1) + nv++ : -1;
    }
    return na + nv;
}

template <bool LDS>
__global__ __launch_bounds__(PF_BIG_THREADS) void powerflow_qlim_kernel(const PfQlimArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pfq_smem[];
    __shared__ double s_red[16];
    __shared__ int s_ok, s_slack, s_m;
    const int t = threadIdx.x, nt = blockDim.x, nw = nt >> 6;
    const int s = blockIdx.x;
    const PfProblem& p = a.p;
    const int n = p.n, e = p.e;
    double* vm = reinterpret_cast<double*>(pfq_smem);
    double* th = vm + n;
    double* sp = th + n;
    double* sq = sp + n;
    double* qs = sq + n;
    double* F = qs + n;
    int* aidx = reinterpret_cast<int*>(F + pfq_m_max(n));
    int* vidx = aidx + n;
    int* ty = vidx + n;
    float* A;
    if constexpr (LDS) A = reinterpret_cast<float*>(pfq_smem + pfq_vec_bytes(n));
    else A = static_cast<float*>(p.ws) + (size_t)s * pf_mat_floats(pfq_m_max(n));
    const PfSample sm = pf_sample(p, s);
    const int64_t* ei = p.edge_index + (a.lines_per_sample ? (int64_t)s * 2 * e : 0);
    const int32_t* ty_in = p.bus_type + (a.types_per_sample ? (int64_t)s * n : 0);
    const double* ql = a.q_limits ? a.q_limits + (a.limits_per_sample ? (int64_t)s * 2 * n : 0) : nullptr;
    const double* spec = sm.spec;
    const PfDense d{ei, sm.rx, spec, qs, 1, n, e, aidx, vidx, vm, th, sp, sq, F};
    int code = 0;                                   // (uniform over the workgroup wherever it is tested)
    double res = __builtin_nan("");

    // ---- the lines name buses of the grid?  (an id outside [0, n) is never followed)
    int bad = 0;
    for (int k = t; k < e; k += nt) bad |= (uint64_t)ei[k] >= (uint64_t)n || (uint64_t)ei[e + k] >= (uint64_t)n;
    // ---- the sample's own type row and its Q specification; from here on the workgroup reads and re-types the copy only
    for (int i = t; i < n; i += nt) {
        ty[i] = ty_in[i];
        qs[i] = spec[4 * i + 3];
    }
    __syncthreads();
    if (t == 0) {
        int ns = 0, odd = 0, slack = 0;
        for (int i = 0; i < n; ++i) {
            const int y = ty[i];
            if (y == 0) { ++ns; slack = i; }
            odd |= (unsigned)y > 2u;
        }
        s_slack = slack;
        s_ok = !odd && ns == 1;
        s_m = s_ok ? pfq_number(ty, n, aidx, vidx) : 0;     // (a row that is refused is not numbered: its counts bound nothing)
    }
    bad = __syncthreads_or(bad);
    if (!s_ok) {
        code = PF_BAD_TYPES;
        if (t == 0) p.flags[0] = p.flags[0] | 1;    // (every writer stores the same bit over the same word)
    } else if (bad) {
        code = PF_BAD_LINE;
    }

    int it = 0, rounds = 0;                          // solves over all rounds; re-solves begun
    if (code == 0 && pf_start_state(p, sm, ty, s_slack, false, nt, vm, th)) code = PF_NON_FINITE;
    while (code == 0) {
        const int m = s_m, ld = pf_ld(m);
        for (int inner = 0;; ++inner, ++it) {
            pf_dense_rows<false>(d, false, A, m, ld, nullptr);
            // ---- max |F| in fp64; a non-finite entry counts as +inf
            double mx = 0.0;
            for (int k = t; k < m; k += nt) mx = fmax(mx, pf_abs_clamped(F[k]));
            res = pf_block_max(mx, s_red, nw);
            const int stop = pf_stop(res, p.tol, inner, p.max_iter);
            if (stop < 0) { code = stop; break; }
            if (stop) break;
            if (!pf_lu_solve(A, ld, m, F)) { code = PF_SINGULAR; break; }
            pf_dense_update(d, A, ld);
        }
        if (code) break;
        // ---- the round's limits (powerflow_qlim.hpp): no violator, done; else the unknowns are numbered again
        if (!pfq_switch(ty, qs, sq, ql, a.q_tol, n, nt)) break;
        if (rounds >= a.max_rounds) { code = PF_QLIM_ROUNDS; break; }
        ++rounds;
        if (t == 0) s_m = pfq_number(ty, n, aidx, vidx);
        __syncthreads();
    }

    pfq_write_back(p, sm, s, nt, code, it, res, rounds, ty_in, ty, vm, th, sp, sq, qs, a.bus_type_out, a.rounds);
}

static bool pfq_fits_lds(int n) { return pfq_vec_bytes(n) + pf_mat_floats(pfq_m_max(n)) * 4 <= (size_t)(kLdsCuBytes - kLdsReserve); }

}  // namespace pfn

using namespace pfn;

extern "C" {

size_t pfn_powerflow_qlim_workspace_bytes(int64_t n_samples, int64_t n_bus, int route) {
    if (n_samples <= 0 || n_bus <= 0 || 2 * (n_bus - 1) > pfn_powerflow_max_unknowns()) return 0;
    if (route == 1 || (route != 2 && pfq_fits_lds((int)n_bus))) return 0;
    return (size_t)n_samples * pf_mat_floats(pfq_m_max((int)n_bus)) * sizeof(float);
}

int pfn_powerflow_solve_qlim(const int64_t* edge_index, int lines_per_sample, int64_t n_lines, const double* rx, const int32_t* bus_type,
                             int types_per_sample, const double* spec, const double* init, const double* q_limits, int limits_per_sample,
                             int64_t n_samples, int64_t n_bus, double tol, double q_tol, int max_iter, int max_rounds, int route,
                             double* table, int32_t* status, double* residual, int32_t* flags, int32_t* bus_type_out, int32_t* rounds,
                             void* ws, size_t ws_bytes, void* stream) {
    PFN_CHECK_ARG(n_samples >= 0 && n_bus >= 1 && n_lines >= 0 && n_samples < (1ll << 29) && n_lines < (1ll << 24) && n_bus < (1ll << 24),
                  "pfn_powerflow_solve_qlim: bad sizes (%lld samples of %lld buses and %lld lines)", (long long)n_samples, (long long)n_bus,
                  (long long)n_lines);
    PFN_CHECK_ARG(route >= 0 && route <= 2, "pfn_powerflow_solve_qlim: route must be 0 (auto), 1 (LDS) or 2 (global)");
    PFN_TRY(pfq_check_call("pfn_powerflow_solve_qlim", n_samples, bus_type, q_limits, limits_per_sample, q_tol, max_rounds, bus_type_out, rounds));
    const int64_t m_max = 2 * (n_bus - 1);
    PFN_CHECK_ARG(m_max <= pfn_powerflow_max_unknowns(),
                  "pfn_powerflow_solve_qlim: %lld unknowns per sample exceed the dense solver's %d; a sparse factorisation is needed (pfn_powerflow_solve_sparse, route \"sparse\")",
                  (long long)m_max, (int)pfn_powerflow_max_unknowns());
    const int n = (int)n_bus;
    PfQlimArgs a{{edge_index, rx, bus_type, spec, init, table, status, residual, flags, ws, tol, n, (int)n_lines, max_iter},
                 q_limits, bus_type_out, rounds, q_tol, max_rounds, lines_per_sample != 0, types_per_sample != 0, limits_per_sample != 0};
    PFN_TRY(pf_check_call("pfn_powerflow_solve_qlim", a.p, n_samples, nullptr, "the workspace 16-byte"));
    if (n_samples == 0) return PFN_OK;
    bool lds;
    const size_t mat_floats = pf_mat_floats((int)m_max);
    PFN_TRY(pf_dense_route("pfn_powerflow_solve_qlim", route, (int)m_max, n, pfq_vec_bytes(n) + mat_floats * 4, n_samples, mat_floats, ws, ws_bytes, &lds));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int threads = m_max > PF_BIG_M ? PF_BIG_THREADS : PF_SMALL_THREADS;
    const size_t bytes = pfq_vec_bytes(n) + (lds ? mat_floats * 4 : 0);
    const double iters = 8.0, mm = (double)m_max;  // (the figures of a sample that ends all-PQ after two rounds: an upper estimate)
    ProfScope ps("powerflow_qlim", (double)n_samples * ((double)n_lines * (16.0 + (lines_per_sample ? 16.0 : 0.0)) + (double)n * 72.0 +
                                                       (init ? (double)n * 16.0 : 0.0) + (q_limits ? (double)n * 16.0 : 0.0)),
                 (double)n_samples * iters * (2.0 / 3.0 * mm * mm * mm + 2.0 * mm * mm), s);
    static std::atomic<uint64_t> raised{0};
    if (lds) {
        PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(powerflow_qlim_kernel<true>), kLdsCuBytes - kLdsReserve, raised));
        powerflow_qlim_kernel<true><<<(int)n_samples, threads, bytes, s>>>(a);
    } else {
        powerflow_qlim_kernel<false><<<(int)n_samples, threads, bytes, s>>>(a);
    }
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

}  // extern "C"
