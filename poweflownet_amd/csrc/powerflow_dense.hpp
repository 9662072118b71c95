// What the dense kernels that keep a sample's fp32 matrix resident -- powerflow.hip's solver, powerflow_qlim.hip's Q-limit solver,
// contingency.hip's N-1 screen -- share: the dense cap, the workgroup-size rule, the odd leading dimension with the size of a matrix
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
