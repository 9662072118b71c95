// AC power flow with generator Q-limits on the device (gfx950): pfn_powerflow_solve_qlim, ONE launch, one workgroup per sample.  The
// reference's `pp.runpp(..., enforce_q_lims=True)` (dataset_generator.py's ENFORCE_Q_LIMS) for this project's network model: a PV bus
// whose reactive line sum leaves its limits becomes a PQ bus fixed at the limit and the sample is solved again, inside the kernel.
//
// The inner loop is powerflow.hip's dense Newton-Raphson, statement for statement: fp64 state, mismatch and stopping rule, the
// analytic Jacobian in fp32, row-major with an odd leading dimension, LU with partial pivoting (ties to the lowest row) and an fp64
// right-hand side.  What differs is whose the bus types are: the workgroup copies ITS row of `bus_type` ([n] shared or [S, n]) into
// LDS, numbers its unknowns from that copy and re-types and renumbers it between rounds, so the PV / PQ counts are no launch
// constants and nothing on the host depends on them.  Storage is therefore sized for the worst case, every non-slack bus PQ:
// m_max = 2 (n - 1).  Next to the dense kernel's vectors stand the live type ty [n] and the effective Q specification qs [n] (the
// given Q, or the limit a switched bus was fixed at).
//
// Rounds.  After an inner loop converges, sq [i] of its last pass is the Q the table would write at a PV bus.  Every thread tests
// its PV buses against (lo, hi) -- demand-positive per-unit, the table's Q column; NaN or +-inf: no limit on that side --:
// sq > hi + q_tol fixes Q at hi, sq < lo - q_tol at lo, the bus becomes PQ.  All violators of a round switch together (MATPOWER's and
// pandapower's default rule), none switches back, the slack is never limited.  No violator: done.  Otherwise the unknowns are
// numbered again -- theta of the non-slack buses in bus order, then Vm of the live PQ buses in bus order -- and Newton continues from
// the current state.  max_iter bounds the solves of each inner loop, max_rounds the re-solves; status >= 0 is the total of solves.
//
// powerflow.hip and powerflow_common.hpp's device functions are untouched: the start state and the write-back here are variants
// that read the LDS type row and qs.  A sample's bits are a function of the sample alone.
#include "powerflow_common.hpp"

namespace pfn {

constexpr int PFQ_SMALL_THREADS = 256, PFQ_BIG_THREADS = 1024;
constexpr int PFQ_BIG_M = 90;                      // the dense kernel's rule, applied to m_max (the host knows no other m)

__host__ __device__ inline int pfq_ld(int m) { return m | 1; }
__host__ __device__ inline int pfq_m_max(int n) { return 2 * (n - 1); }
// the sample's vectors: double vm, th, sp, sq, qs [n], F [m_max]; int aidx, vidx, ty [n]; rounded to 16 bytes
__host__ __device__ inline size_t pfq_vec_bytes(int n) {
    return ((size_t)8 * (5 * (size_t)n + pfq_m_max(n)) + (size_t)12 * n + 15) & ~(size_t)15;
}
__host__ __device__ inline size_t pfq_mat_floats(int n) { return ((size_t)pfq_m_max(n) * pfq_ld(pfq_m_max(n)) + 3) & ~(size_t)3; }

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
__global__ __launch_bounds__(PFQ_BIG_THREADS) void powerflow_qlim_kernel(const PfQlimArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pfq_smem[];
    __shared__ double s_red[16];
    __shared__ float s_pval;
    __shared__ int s_piv, s_ok, s_slack, s_m;
    const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6, nw = nt >> 6;
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
    else A = static_cast<float*>(p.ws) + (size_t)s * pfq_mat_floats(n);
    const PfSample sm = pf_sample(p, s);
    const int64_t* ei = p.edge_index + (a.lines_per_sample ? (int64_t)s * 2 * e : 0);
    const int32_t* ty_in = p.bus_type + (a.types_per_sample ? (int64_t)s * n : 0);
    const double* ql = a.q_limits ? a.q_limits + (a.limits_per_sample ? (int64_t)s * 2 * n : 0) : nullptr;
    const double* rx = sm.rx;
    const double* spec = sm.spec;
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
    if (code == 0) {
        // ---- the start state: flat, or the caller's -- Va at the non-slack buses, Vm at the buses that are PQ on entry
        const double th0 = spec[4 * s_slack + 1] * PF_RAD;
        int wild = 0;
        for (int i = t; i < n; i += nt) {
            const int y = ty[i];
            double v = y == 2 ? 1.0 : spec[4 * i], ang = th0;
            if (sm.init) {
                if (y == 2) v = sm.init[2 * i];
                if (y != 0) ang = sm.init[2 * i + 1] * PF_RAD;
                wild |= !(fabs(v) < __builtin_inf()) || !(fabs(ang) < __builtin_inf());
            }
            vm[i] = v;
            th[i] = ang;
        }
        if (__syncthreads_or(wild)) code = PF_NON_FINITE;
    }
    while (code == 0) {
        const int m = s_m, ld = pfq_ld(m);
        for (int inner = 0;; ++inner, ++it) {
            for (int k = t; k < m * ld; k += nt) A[k] = 0.f;
            __syncthreads();
            // ---- line sums, mismatch and matrix rows of bus i, its lines in stored order
            for (int i = t; i < n; i += nt) {
                const int ra = aidx[i], rv = vidx[i];
                const double vi = vm[i], ti = th[i];
                double sP = 0.0, sQ = 0.0, dPt = 0.0, dPv = 0.0, dQt = 0.0, dQv = 0.0;
                for (int k = 0; k < e; ++k) {
                    const int la = (int)ei[k], lb = (int)ei[e + k];
                    if (la != i && lb != i) continue;
                    const double r = rx[2 * k], x = rx[2 * k + 1];
#pragma unroll 1
                    for (int side = 0; side < 2; ++side) {       // the stored direction, then the reverse (a self-loop: both)
                        if ((side ? lb : la) != i) continue;
                        const int j = side ? la : lb;
                        const int ca = aidx[j], cv = vidx[j];
                        const PfEnd end = pf_ac_end(r, x, vi, ti, vm[j], th[j], sP, sQ);
                        const PfEndJac J = pf_ac_end_jac(end, vi);
                        dPt += J.pti;
                        dPv += J.pvi;
                        dQt += J.qti;
                        dQv += J.qvi;
                        if (ra >= 0) {
                            if (ca >= 0) A[ra * ld + ca] += (float)(-J.pti);
                            if (cv >= 0) A[ra * ld + cv] += (float)J.pvj;
                        }
                        if (rv >= 0) {
                            if (ca >= 0) A[rv * ld + ca] += (float)(-J.qti);
                            if (cv >= 0) A[rv * ld + cv] += (float)J.qvj;
                        }
                    }
                }
                sp[i] = sP;
                sq[i] = sQ;
                if (ra >= 0) {
                    F[ra] = spec[4 * i + 2] - sP;
                    A[ra * ld + ra] += (float)dPt;
                    if (rv >= 0) A[ra * ld + rv] += (float)dPv;
                }
                if (rv >= 0) {
                    F[rv] = qs[i] - sQ;
                    A[rv * ld + ra] += (float)dQt;
                    A[rv * ld + rv] += (float)dQv;
                }
            }
            __syncthreads();
            // ---- max |F| in fp64; a non-finite entry counts as +inf
            double mx = 0.0;
            for (int k = t; k < m; k += nt) mx = fmax(mx, pf_abs_clamped(F[k]));
            res = pf_block_max(mx, s_red, nw);
            const int stop = pf_stop(res, p.tol, inner, p.max_iter);
            if (stop < 0) { code = stop; break; }
            if (stop) break;
            // ---- LU with partial pivoting, the right-hand side F eliminated along (fp64); L is not kept
            for (int k = 0; k < m; ++k) {
                if (wave == 0) {
                    float best = -1.f;
                    int bi = m;
                    for (int i = k + lane; i < m; i += 64) {
                        const float v = fabsf(A[i * ld + k]);
                        if (v > best) { best = v; bi = i; }
                    }
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) {
                        const float ob = __shfl_xor(best, off);
                        const int oi = __shfl_xor(bi, off);
                        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
                    }
                    if (lane == 0) { s_piv = bi; s_pval = best; }
                }
                __syncthreads();
                const int pr = s_piv;
                if (!(s_pval > PF_TINY_PIVOT)) { code = PF_SINGULAR; break; }
                if (pr != k) {
                    for (int j = k + t; j < m; j += nt) {
                        const float u = A[k * ld + j];
                        A[k * ld + j] = A[pr * ld + j];
                        A[pr * ld + j] = u;
                    }
                    if (t == 0) {
                        const double f = F[k];
                        F[k] = F[pr];
                        F[pr] = f;
                    }
                }
                __syncthreads();
                const float piv = A[k * ld + k];
                for (int i = k + 1 + wave; i < m; i += nw) {
                    const float l = A[i * ld + k] / piv;
                    for (int j = k + 1 + lane; j < m; j += 64) A[i * ld + j] = fmaf(-l, A[k * ld + j], A[i * ld + j]);
                    if (lane == 0) F[i] -= (double)l * F[k];
                }
                __syncthreads();
            }
            if (code) break;
            // ---- back substitution by columns: after step k, F[k] / U[k][k] is x_k
            for (int k = m - 1; k > 0; --k) {
                const double xk = F[k] / (double)A[k * ld + k];
                for (int i = t; i < k; i += nt) F[i] -= (double)A[i * ld + k] * xk;
                __syncthreads();
            }
            for (int i = t; i < n; i += nt) {
                const int ia = aidx[i], iv = vidx[i];
                if (ia >= 0) th[i] += F[ia] / (double)A[ia * ld + ia];
                if (iv >= 0) vm[i] += F[iv] / (double)A[iv * ld + iv];
            }
            __syncthreads();
        }
        if (code) break;
        // ---- the round's limits: a thread tests the PV buses it owns; all violators switch together and stay switched
        int viol = 0;
        if (ql) {
            for (int i = t; i < n; i += nt) {
                if (ty[i] != 1) continue;
                const double lo = ql[2 * i], hi = ql[2 * i + 1], q = sq[i];
                double fix;
                if (fabs(hi) < __builtin_inf() && q > hi + a.q_tol) fix = hi;
                else if (fabs(lo) < __builtin_inf() && q < lo - a.q_tol) fix = lo;
                else continue;
                ty[i] = 2;
                qs[i] = fix;
                viol = 1;
            }
        }
        if (!__syncthreads_or(viol)) break;
        if (rounds >= a.max_rounds) { code = PF_QLIM_ROUNDS; break; }
        ++rounds;
        if (t == 0) s_m = pfq_number(ty, n, aidx, vidx);
        __syncthreads();
    }

    // ---- the table, the final types and the sample's status / residual / rounds: slack P, Q and the Q of a bus still PV are the
    // line sums of the last pass, a switched bus holds its solved Vm and its limit; a failed sample's rows are NaN and its types
    // the ones it came with
    const double nanv = __builtin_nan("");
    for (int i = t; i < n; i += nt) {
        double4 row = make_double4(nanv, nanv, nanv, nanv);
        int y = ty_in[i];
        if (code == 0) {
            y = ty[i];
            row.x = vm[i];
            row.y = y == 0 ? spec[4 * i + 1] : th[i] * (1.0 / PF_RAD);
            row.z = y == 0 ? sp[i] : spec[4 * i + 2];
            row.w = y == 2 ? qs[i] : sq[i];
        }
        *reinterpret_cast<double4*>(sm.out + 4 * i) = row;
        a.bus_type_out[(int64_t)s * n + i] = y;
    }
    if (t == 0) {
        p.status[s] = code ? code : it;
        p.residual[s] = res;
        a.rounds[s] = rounds;
    }
}

static bool pfq_fits_lds(int n) { return pfq_vec_bytes(n) + pfq_mat_floats(n) * 4 <= (size_t)(kLdsCuBytes - kLdsReserve); }

}  // namespace pfn

using namespace pfn;

extern "C" {

size_t pfn_powerflow_qlim_workspace_bytes(int64_t n_samples, int64_t n_bus, int route) {
    if (n_samples <= 0 || n_bus <= 0 || 2 * (n_bus - 1) > pfn_powerflow_max_unknowns()) return 0;
    if (route == 1 || (route != 2 && pfq_fits_lds((int)n_bus))) return 0;
    return (size_t)n_samples * pfq_mat_floats((int)n_bus) * sizeof(float);
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
    PFN_CHECK_ARG(max_rounds >= 0 && q_tol >= 0.0 && q_tol < __builtin_inf(), "pfn_powerflow_solve_qlim: max_rounds must be >= 0 and q_tol finite and >= 0");
    const int64_t m_max = 2 * (n_bus - 1);
    PFN_CHECK_ARG(m_max <= pfn_powerflow_max_unknowns(),
                  "pfn_powerflow_solve_qlim: %lld unknowns per sample exceed the dense solver's %d; a sparse factorisation is needed (pfn_powerflow_solve_sparse, route \"sparse\")",
                  (long long)m_max, (int)pfn_powerflow_max_unknowns());
    const int n = (int)n_bus;
    PfQlimArgs a{{edge_index, rx, bus_type, spec, init, table, status, residual, flags, ws, tol, n, (int)n_lines, max_iter},
                 q_limits, bus_type_out, rounds, q_tol, max_rounds, lines_per_sample != 0, types_per_sample != 0, limits_per_sample != 0};
    PFN_TRY(pf_check_call("pfn_powerflow_solve_qlim", a.p, n_samples, nullptr, "the workspace 16-byte"));
    if (n_samples == 0) return PFN_OK;
    PFN_CHECK_ARG(bus_type_out && rounds, "pfn_powerflow_solve_qlim: null bus_type_out or rounds");
    PFN_CHECK_ARG(((reinterpret_cast<uintptr_t>(bus_type_out) | reinterpret_cast<uintptr_t>(rounds)) & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(q_limits) & 7) == 0,
                  "pfn_powerflow_solve_qlim: q_limits must be 8-byte aligned, bus_type_out and rounds 4-byte");
    PFN_CHECK_ARG(q_limits || !limits_per_sample, "pfn_powerflow_solve_qlim: limits_per_sample without q_limits");
    PFN_CHECK_ARG(bus_type_out != bus_type, "pfn_powerflow_solve_qlim: bus_type_out must not be bus_type (a failed sample reads its input row back)");
    const bool fits = pfq_fits_lds(n);
    PFN_CHECK_ARG(route != 1 || fits, "pfn_powerflow_solve_qlim: route 1 (LDS): %d unknowns of %d buses need %zu bytes of LDS, %d are there",
                  (int)m_max, n, pfq_vec_bytes(n) + pfq_mat_floats(n) * 4, kLdsCuBytes - kLdsReserve);
    const bool lds = route == 1 || (route == 0 && fits);
    if (!lds) {
        const size_t need = (size_t)n_samples * pfq_mat_floats(n) * sizeof(float);
        if (need && (!ws || ws_bytes < need)) {
            set_error("pfn_powerflow_solve_qlim: the global route needs a workspace of %zu bytes (got %zu)", need, ws ? ws_bytes : (size_t)0);
            return PFN_ENOSPACE;
        }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int threads = m_max > PFQ_BIG_M ? PFQ_BIG_THREADS : PFQ_SMALL_THREADS;
    const size_t bytes = pfq_vec_bytes(n) + (lds ? pfq_mat_floats(n) * 4 : 0);
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
