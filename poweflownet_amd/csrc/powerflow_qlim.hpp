// What the two Q-limit kernels (powerflow_qlim.hip dense, powerflow_sparse_qlim.hip sparse) do around their Newton loops, spelled
// once: the round's limit test -- the rule that decides a dataset's bus types --, the write-back of the table, the final types and
// the sample's status / residual / rounds, and the host checks of the Q-limit arguments.  `ty` is the workgroup's live copy of the
// sample's own type row in LDS (int on the dense route, bytes on the sparse one), `qs` its effective Q specification: the given Q,
// or the limit a switched bus was fixed at.  Every device function is called by ALL threads with the same arguments.
#pragma once
#include "powerflow_common.hpp"

namespace pfn {

// ---- the round's limits after a converged inner loop: a thread tests the PV buses it owns against ql = (lo, hi) [n, 2] --
// demand-positive per-unit; NaN or +-inf: no limit on that side; null: no limits --: sq beyond hi + q_tol fixes Q at hi, sq below
// lo - q_tol at lo, and the bus becomes PQ.  All violators switch together, none switches back.  True (uniform) when one switched.
template <typename Ty>
__device__ __forceinline__ bool pfq_switch(Ty* ty, double* qs, const double* sq, const double* ql, double q_tol, int n, int nt) {
    int viol = 0;
    if (ql) {
        for (int i = threadIdx.x; i < n; i += nt) {
            if (ty[i] != 1) continue;
            const double lo = ql[2 * i], hi = ql[2 * i + 1], q = sq[i];
            double fix;
            if (fabs(hi) < __builtin_inf() && q > hi + q_tol) fix = hi;
            else if (fabs(lo) < __builtin_inf() && q < lo - q_tol) fix = lo;
            else continue;
            ty[i] = 2;
            qs[i] = fix;
            viol = 1;
        }
    }
    return __syncthreads_or(viol);
}

// ---- the table, the final types and the sample's status / residual / rounds: slack P, Q and the Q of a bus still PV are the line
// sums of the last pass, a switched bus holds its solved Vm and its limit; a failed sample's rows are NaN and its types the ones
// it came with (ty_in)
template <typename Ty>
__device__ __forceinline__ void pfq_write_back(const PfProblem& p, const PfSample& sm, int s, int nt, int code, int it, double res, int rounds,
                                               const int32_t* ty_in, const Ty* ty, const double* vm, const double* th, const double* sp,
                                               const double* sq, const double* qs, int32_t* bus_type_out, int32_t* rounds_out) {
    const double nanv = __builtin_nan("");
    const int n = p.n;
    for (int i = threadIdx.x; i < n; i += nt) {
        double4 row = make_double4(nanv, nanv, nanv, nanv);
        int y = ty_in[i];
        if (code == 0) {
            y = ty[i];
            row.x = vm[i];
            row.y = y == 0 ? sm.spec[4 * i + 1] : th[i] * (1.0 / PF_RAD);
            row.z = y == 0 ? sp[i] : sm.spec[4 * i + 2];
            row.w = y == 2 ? qs[i] : sq[i];
        }
        *reinterpret_cast<double4*>(sm.out + 4 * i) = row;
        bus_type_out[(int64_t)s * n + i] = y;
    }
    if (threadIdx.x == 0) {
        p.status[s] = code ? code : it;
        p.residual[s] = res;
        rounds_out[s] = rounds;
    }
}

// ---- host side: what both Q-limit entries ask of their own arguments, before pf_check_call looks at the problem's; the pointers
// are looked at only when there are samples
static inline int pfq_check_call(const char* who, int64_t n_samples, const int32_t* bus_type, const double* q_limits, int limits_per_sample,
                                 double q_tol, int max_rounds, const int32_t* bus_type_out, const int32_t* rounds) {
    PFN_CHECK_ARG(max_rounds >= 0 && q_tol >= 0.0 && q_tol < __builtin_inf(), "%s: max_rounds must be >= 0 and q_tol finite and >= 0", who);
    if (n_samples <= 0) return PFN_OK;
    PFN_CHECK_ARG(bus_type_out && rounds, "%s: null bus_type_out or rounds", who);
    PFN_CHECK_ARG(((reinterpret_cast<uintptr_t>(bus_type_out) | reinterpret_cast<uintptr_t>(rounds)) & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(q_limits) & 7) == 0,
                  "%s: q_limits must be 8-byte aligned, bus_type_out and rounds 4-byte", who);
    PFN_CHECK_ARG(q_limits || !limits_per_sample, "%s: limits_per_sample without q_limits", who);
    PFN_CHECK_ARG(bus_type_out != bus_type, "%s: bus_type_out must not be bus_type (a failed sample reads its input row back)", who);
    return PFN_OK;
}

}  // namespace pfn
