// What the dense kernels that keep a sample's fp32 matrix resident -- powerflow.hip's solver, powerflow_qlim.hip's Q-limit solver,
// contingency.hip's N-1 screen, contingency_ac.hip's AC screen (which runs the solver's whole sample, pf_solve_sample, as its base) -- share: the dense cap, the workgroup-size rule, the odd leading dimension with the size of a matrix
// slab, the in-place Gauss-Jordan inverse of a symmetric, diagonally dominant matrix (B' or B''), the dense Newton pass -- the rows
// of a bus from the stored line list, LU with partial pivoting under an fp64 right-hand side, x += dx -- and, host side, the choice
// between the LDS and the global route.  Spelled once: the screen's B'^-1 is the fast-decoupled modes', the Q-limit rounds' Newton
// pass is the solver's.  Every device function here is called by ALL threads of the workgroup with the same arguments.
#pragma once
#include "powerflow_common.hpp"

namespace pfn {

constexpr int PF_MAX_UNKNOWNS = 1024;              // dense cap of the global route: 4 MiB per sample, 3.6e8 multiply-adds per factor
constexpr int PF_SMALL_THREADS = 256, PF_BIG_THREADS = 1024;
constexpr int PF_BIG_M = 90;                       // 4 m^2 beyond ~32 KiB: few workgroups per CU, so each gets 16 waves

__host__ __device__ inline int pf_ld(int m) { return m | 1; }
__host__ __device__ inline size_t pf_mat_floats(int m) { return ((size_t)m * pf_ld(m) + 3) & ~(size_t)3; }

// B (mm x mm, leading dimension ld) becomes its inverse, in place: Gauss-Jordan without pivoting, two barriers per column.  Every
// thread calls it; false (uniform: all threads read the same pivot) when a pivot is tiny or NaN.
__device__ __forceinline__ bool pf_invert_in_place(float* B, int mm, int ld) {
    const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6, nw = nt >> 6;
    for (int k = 0; k < mm; ++k) {
        const float p = B[k * ld + k];              // (written last before the barrier that ended step k - 1)
        if (!(fabsf(p) > PF_TINY_PIVOT)) return false;
        const float pinv = 1.f / p;
        for (int j = t; j < mm; j += nt)
            if (j != k) B[k * ld + j] *= pinv;
        __syncthreads();
        for (int i = wave; i < mm; i += nw) {
            if (i == k) continue;
            const float f = B[i * ld + k];
            for (int j = lane; j < mm; j += 64)
                if (j != k) B[i * ld + j] = fmaf(-f, B[k * ld + j], B[i * ld + j]);
            if (lane == 0) B[i * ld + k] = -f * pinv;
        }
        if (t == 0) B[k * ld + k] = pinv;
        __syncthreads();
    }
    return true;
}

// ---- one sample as the dense Newton pass sees it: the line list, the unknown of every bus (aidx: theta, vidx: Vm, -1: none) and
// the state, the line sums and the right-hand side in LDS.  qspec [qstride * i] is the Q a PQ bus is held to: the table's column
// (spec + 3, stride 4), or the Q-limit kernel's effective Q (qs, stride 1).
struct PfDense {
    const int64_t* ei;
    const double* rx;
    const double* spec;
    const double* qspec;
    int qstride, n, e;
    const int* aidx;
    const int* vidx;
    double* vm;
    double* th;
    double* sp;
    double* sq;
    double* F;
};

// ---- line sums, mismatch and matrix rows of bus i, its lines in stored order: A (m x m, leading dimension ld) is zeroed and
// filled with d(line sums)/d(unknowns), F with the mismatch.  dc: F(theta) = B' theta + P and its constant matrix.  FD: the line
// sums and the mismatch only, and G = F / Vm, the right-hand sides of the two halves; A is not touched.
template <bool FD>
__device__ __forceinline__ void pf_dense_rows(const PfDense& d, bool dc, float* A, int m, int ld, double* G) {
    const int t = threadIdx.x, nt = blockDim.x, n = d.n, e = d.e;
    const int64_t* ei = d.ei;
    const double* rx = d.rx;
    const double* spec = d.spec;
    const int* aidx = d.aidx;
    const int* vidx = d.vidx;
    double* F = d.F;
    if constexpr (!FD) {
        for (int k = t; k < m * ld; k += nt) A[k] = 0.f;
        __syncthreads();
    }
    for (int i = t; i < n; i += nt) {
        const int ra = aidx[i], rv = vidx[i];
        const double vi = d.vm[i], ti = d.th[i];
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
                if (dc) {
                    const double b = pf_dc_end(x, ti, d.th[j], sP);
                    dPt += b;
                    if (ra >= 0 && ca >= 0) A[ra * ld + ca] += (float)(-b);
                    continue;
                }
                const PfEnd end = pf_ac_end(r, x, vi, ti, d.vm[j], d.th[j], sP, sQ);
                if constexpr (FD) continue;
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
        d.sp[i] = sP;
        d.sq[i] = sQ;
        if constexpr (FD) {
            if (ra >= 0) {
                F[ra] = spec[4 * i + 2] - sP;
                G[ra] = F[ra] / vi;
            }
            if (rv >= 0) {
                F[rv] = d.qspec[d.qstride * i] - sQ;
                G[rv] = F[rv] / vi;
            }
            continue;
        }
        if (ra >= 0) {
            F[ra] = spec[4 * i + 2] - sP;
            A[ra * ld + ra] += (float)dPt;
            if (rv >= 0) A[ra * ld + rv] += (float)dPv;
        }
        if (rv >= 0) {
            F[rv] = d.qspec[d.qstride * i] - sQ;
            A[rv * ld + ra] += (float)dQt;
            A[rv * ld + rv] += (float)dQv;
        }
    }
    __syncthreads();
}

// ---- A dx = F: LU with partial pivoting (ties to the lowest row), the right-hand side F eliminated along in fp64, L not kept; then
// back substitution by columns, which leaves U[k][k] dx_k in F[k] (pf_dense_update divides).  False, for all threads alike (they
// read the same pivot behind a barrier), when a pivot is tiny or NaN.
__device__ __forceinline__ bool pf_lu_solve(float* A, int ld, int m, double* F) {
    __shared__ float s_pval;
    __shared__ int s_piv;
    const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6, nw = nt >> 6;
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
        const int p = s_piv;
        if (!(s_pval > PF_TINY_PIVOT)) return false;
        if (p != k) {
            for (int j = k + t; j < m; j += nt) {
                const float u = A[k * ld + j];
                A[k * ld + j] = A[p * ld + j];
                A[p * ld + j] = u;
            }
            if (t == 0) {
                const double f = F[k];
                F[k] = F[p];
                F[p] = f;
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
    for (int k = m - 1; k > 0; --k) {
        const double xk = F[k] / (double)A[k * ld + k];
        for (int i = t; i < k; i += nt) F[i] -= (double)A[i * ld + k] * xk;
        __syncthreads();
    }
    return true;
}

// ---- x += dx from what pf_lu_solve left
__device__ __forceinline__ void pf_dense_update(const PfDense& d, const float* A, int ld) {
    for (int i = threadIdx.x; i < d.n; i += blockDim.x) {
        const int ia = d.aidx[i], iv = d.vidx[i];
        if (ia >= 0) d.th[i] += d.F[ia] / (double)A[ia * ld + ia];
        if (iv >= 0) d.vm[i] += d.F[iv] / (double)A[iv * ld + iv];
    }
    __syncthreads();
}

// ---- the fast-decoupled modes' two constant matrices, built and inverted in place: B' (mp x mp, ld = mp | 1) at A, B'' (mq x mq)
// behind it.  Laplacians of the stored lines (parallel lines add, a self-loop cancels), bus i's rows by bus i in stored order, the
// diagonal summed in fp64 and added last.  False (uniform) when a pivot is tiny or NaN.  The AC screen's base launch calls it too,
// for a scenario whose start is converged already: its outages need the inverses.
__device__ __forceinline__ bool pf_fd_inverses(const PfDense& d, const bool xb, float* A, const int mp, const int mq) {
    const int t = threadIdx.x, nt = blockDim.x, n = d.n, e = d.e, ldp = pf_ld(mp), ldq = pf_ld(mq);
    const int64_t* ei = d.ei;
    const double* rx = d.rx;
    const int* aidx = d.aidx;
    const int* vidx = d.vidx;
    float* Bq = A + pf_mat_floats(mp);
    for (int k = t; k < (int)(pf_mat_floats(mp) + pf_mat_floats(mq)); k += nt) A[k] = 0.f;
    __syncthreads();
    for (int i = t; i < n; i += nt) {
        const int ra = aidx[i], rv = vidx[i];
        double dp = 0.0, dq = 0.0;
        for (int k = 0; k < e; ++k) {
            const int la = (int)ei[k], lb = (int)ei[e + k];
            if (la != i && lb != i) continue;
            const double r = rx[2 * k], x = rx[2 * k + 1];
            const double w1 = 1.0 / x, w2 = x / (r * r + x * x);
            const double wp = xb ? w1 : w2, wq = xb ? w2 : w1;
#pragma unroll 1
            for (int side = 0; side < 2; ++side) {
                if ((side ? lb : la) != i) continue;
                const int j = side ? la : lb;
                const int ca = aidx[j], cv = vidx[j];
                dp += wp;
                dq += wq;
                if (ra >= 0 && ca >= 0) A[ra * ldp + ca] += (float)(-wp);
                if (rv >= 0 && cv >= 0) Bq[(rv - mp) * ldq + (cv - mp)] += (float)(-wq);
            }
        }
        if (ra >= 0) A[ra * ldp + ra] += (float)dp;
        if (rv >= 0) Bq[(rv - mp) * ldq + (rv - mp)] += (float)dq;
    }
    __syncthreads();
    return pf_invert_in_place(A, mp, ldp) && pf_invert_in_place(Bq, mq, ldq);
}

// ---- one sample's whole solve, the body of powerflow.hip's kernel: the AC screen's base launch (contingency_ac.hip) runs the SAME
// text, so its base table, status and residual are the solver's bits.
// the sample's vectors: double vm, th, sp, sq [n], F [m]; int aidx, vidx [n]; rounded to 16 bytes
__host__ __device__ inline size_t pf_vec_bytes(int n, int m) { return ((size_t)8 * (4 * (size_t)n + m) + (size_t)8 * n + 15) & ~(size_t)15; }
__host__ __device__ inline size_t pf_fd_extra_bytes(int m) { return ((size_t)8 * m + 15) & ~(size_t)15; }      // modes 2, 3: F / Vm [m]

struct PfArgs {
    PfProblem p;                                    // (p.ws: the global route's fp32 slabs)
    int m, n_pv, n_pq, mode, lines_per_sample;
};

// Sample s in the workgroup's dynamic LDS `pf_smem` (pf_vec_bytes, then pf_fd_extra_bytes where FD), its matrix -- FD: B' [mp x mp]
// with B'' [mq x mq] behind it -- at A (LDS or a slab).  Every thread calls it.  Returns the sample's code (0 or the negative
// status), uniform; on 0 the vectors hold the final state (vm, th at the start of pf_smem; aidx, vidx behind F) and, FD, A holds
// both inverses wherever at least one half-iteration ran or the start was not converged (the matrices are built on the first pass
// that does not stop).
template <bool FD>
__device__ __forceinline__ int pf_solve_sample(const PfArgs& a, const int s, unsigned char* pf_smem, float* A) {
    __shared__ double s_red[16];
    __shared__ int s_ok, s_slack;
    const int t = threadIdx.x, nt = blockDim.x, nw = nt >> 6;
    const PfProblem& p = a.p;
    const int n = p.n, e = p.e, m = a.m, ld = pf_ld(m);
    const bool dc = !FD && a.mode == 1;
    const int mp = n - 1, mq = a.n_pq, ldp = pf_ld(mp), ldq = pf_ld(mq);      // FD: B' [mp x mp], B'' [mq x mq] behind it
    double* vm = reinterpret_cast<double*>(pf_smem);
    double* th = vm + n;
    double* sp = th + n;
    double* sq = sp + n;
    double* F = sq + n;
    int* aidx = reinterpret_cast<int*>(F + m);
    int* vidx = aidx + n;
    double* G = reinterpret_cast<double*>(pf_smem + pf_vec_bytes(n, m));      // FD only: F / Vm [m]
    float* Bq = A + pf_mat_floats(mp);
    const PfSample sm = pf_sample(p, s);
    const int64_t* ei = p.edge_index + (a.lines_per_sample ? (int64_t)s * 2 * e : 0);
    const double* rx = sm.rx;
    const PfDense d{ei, rx, sm.spec, sm.spec + 3, 4, n, e, aidx, vidx, vm, th, sp, sq, F};
    int code = 0;                                   // (uniform over the workgroup wherever it is tested)
    double res = __builtin_nan("");

    // ---- the lines name buses of the grid?  (an id outside [0, n) is never followed)
    int bad = 0;
    for (int k = t; k < e; k += nt) bad |= (uint64_t)ei[k] >= (uint64_t)n || (uint64_t)ei[e + k] >= (uint64_t)n;
    // ---- unknown numbering; the host's n_pv / n_pq (they decided m, the route and the LDS size) against the device bus types
    if (t == 0) {
        int na = 0, nv = 0, ns = 0, npv = 0, npq = 0, odd = 0, slack = 0;
        for (int i = 0; i < n; ++i) {
            const int ty = p.bus_type[i];
            int ia = -1, iv = -1;
            if (ty == 0) { ++ns; slack = i; }
            else if (ty == 1) { ++npv; ia = na++; }
            else if (ty == 2) { ++npq; ia = na++; if (!dc) iv = (n - 1) + nv++; }
            else odd = 1;
            aidx[i] = ia;
            vidx[i] = iv;
        }
        s_slack = slack;
        s_ok = !odd && ns == 1 && npv == a.n_pv && npq == a.n_pq;
    }
    bad = __syncthreads_or(bad);
    if (!s_ok) {
        code = PF_BAD_TYPES;
        if (t == 0) p.flags[0] = p.flags[0] | 1;    // (every writer stores the same bit over the same word)
    } else if (bad) {
        code = PF_BAD_LINE;
    }

    int it = 0;
    if (code == 0 && pf_start_state(p, sm, p.bus_type, s_slack, dc, nt, vm, th)) code = PF_NON_FINITE;
    if (code == 0) {
        int half = 0;                               // FD: 0 the P half comes next, 1 the Q half
        for (;; ++it) {
            // ---- line sums, mismatch and matrix rows (above)
            pf_dense_rows<FD>(d, dc, A, m, ld, G);
            // ---- max |F| in fp64; a non-finite entry counts as +inf
            double mx = 0.0;
            for (int k = t; k < m; k += nt) mx = fmax(mx, pf_abs_clamped(F[k]));
            res = pf_block_max(mx, s_red, nw);
            const int stop = pf_stop(res, p.tol, it, p.max_iter);
            if (stop < 0) { code = stop; break; }
            if (stop) break;
            if constexpr (FD) {
                if (it == 0) {
                    // ---- B' and B'', once (above)
                    if (!pf_fd_inverses(d, a.mode == 2, A, mp, mq)) { code = PF_SINGULAR; break; }
                }
                // ---- one half-iteration: a mat-vec with the resident inverse, row by its owner, fp64 sum in column order
                for (int i = t; i < n; i += nt) {
                    const int r = half ? vidx[i] - mp : aidx[i];
                    if (r < 0) continue;
                    const float* row = half ? Bq + r * ldq : A + r * ldp;
                    const double* g = half ? G + mp : G;
                    const int cols = half ? mq : mp;
                    double acc = 0.0;
                    for (int c = 0; c < cols; ++c) acc += (double)row[c] * g[c];
                    if (half) vm[i] -= acc;
                    else th[i] -= acc;
                }
                __syncthreads();
                half = mq ? !half : 0;
                continue;
            }
            // ---- A dx = F by LU with partial pivoting, then x += dx (above)
            if (!pf_lu_solve(A, ld, m, F)) { code = PF_SINGULAR; break; }
            pf_dense_update(d, A, ld);
        }
    }

    pf_write_back(p, sm, s, dc, nt, code, it, res, vm, th, sp, sq);
    return code;
}

// ---- host side: the route of a dense launch.  Route 1 (LDS) is refused when the sample's `lds_need` bytes are not there, route 0
// takes LDS when they are; the global route needs a workspace of `mat_floats` per sample.  *lds is the decision.
static inline int pf_dense_route(const char* who, int route, int m, int n, size_t lds_need, int64_t n_samples, size_t mat_floats, const void* ws,
                                 size_t ws_bytes, bool* lds) {
    const bool fits = lds_need <= (size_t)(kLdsCuBytes - kLdsReserve);
    PFN_CHECK_ARG(route != 1 || fits, "%s: route 1 (LDS): %d unknowns of %d buses need %zu bytes of LDS, %d are there", who, m, n, lds_need,
                  kLdsCuBytes - kLdsReserve);
    *lds = route == 1 || (route == 0 && fits);
    const size_t need = (size_t)n_samples * mat_floats * sizeof(float);
    if (!*lds && need && (!ws || ws_bytes < need)) {
        set_error("%s: the global route needs a workspace of %zu bytes (got %zu)", who, need, ws ? ws_bytes : (size_t)0);
        return PFN_ENOSPACE;
    }
    return PFN_OK;
}

}  // namespace pfn
