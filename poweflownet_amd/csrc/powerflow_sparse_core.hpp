// The numeric core of a sparse power-flow kernel as workgroup-wide device functions over one planned matrix (powerflow_plan.hpp):
// the left-looking column factorisation in fp32 and the forward and backward substitutions on an fp64 right-hand side (the matrix
// view PfcMatrix, the pivot threshold and everything a kernel does around them are powerflow_common.hpp's).  Two kernels share them: the Newton / DC kernel (powerflow_sparse.hip), which factors and substitutes once per
// pass, and the fast-decoupled kernel (powerflow_sparse_fd.hip), which factors two matrices once and substitutes many times.
//
// Every function is called by ALL threads of the workgroup with the same arguments; every loop bound comes from the plan, so every
// barrier inside is reached by all of them.  One owner per target per step; no float atomics.
#pragma once
#include "powerflow_common.hpp"

namespace pfn {

// slab (global, this sample's) holds A at the planned positions on entry, U (with its diagonal) and the L parts times 1 / pivot on
// exit.  w: m floats of LDS.  Returns false -- for all threads alike -- at a pivot that is tiny or NaN; the slab is then half done.
// Column j is scattered into w; for every k of its U part, ascending, U_kj = w[k] is final and the lanes subtract L(:, k) U_kj at
// w[row]: the pattern is closed under elimination, so every such row is a row of column j.  The metadata of up to 64 columns is
// loaded by the lanes at once and handed round with wave shuffles, and a thread's first element of the next L column is requested
// before the current step's barrier (LDS-only): a k-step waits for an LDS round trip and a barrier, not for three dependent loads.
template <int THREADS>
__device__ __forceinline__ bool pfc_factor(const PfcMatrix A, float* slab, float* w) {
    const int t = threadIdx.x, lane = t & 63;
    constexpr int nt = THREADS;
    const int32_t* colptr = A.colptr;
    const int32_t* diag = A.diag;
    const uint16_t* row = A.row;
    for (int j = 0; j < A.m; ++j) {
        const int c0 = colptr[j], dg = diag[j], c1 = colptr[j + 1];
        for (int i = c0 + t; i < c1; i += nt) w[row[i]] = slab[i];
        __syncthreads();
        for (int p0 = c0; p0 < dg; p0 += 64) {
            const int cnt = min(64, dg - p0);
            int myk = 0, myb = 0, mye = 0;
            if (lane < cnt) {
                myk = row[p0 + lane];
                myb = diag[myk] + 1;
                mye = colptr[myk + 1];
            }
            int k = __shfl(myk, 0), lb = __shfl(myb, 0), le = __shfl(mye, 0), r0 = 0;
            float l0 = 0.f;
            if (lb + t < le) {
                r0 = row[lb + t];
                l0 = slab[lb + t];
            }
            for (int q = 0; q < cnt; ++q) {
                const int kc = k, lbc = lb, lec = le, rc = r0;
                const float lc = l0;
                if (q + 1 < cnt) {
                    k = __shfl(myk, q + 1);
                    lb = __shfl(myb, q + 1);
                    le = __shfl(mye, q + 1);
                    if (lb + t < le) {
                        r0 = row[lb + t];
                        l0 = slab[lb + t];
                    }
                }
                const float ukj = w[kc];             // final: every earlier step that could reach row k is behind a barrier
                if (lbc + t < lec) w[rc] = fmaf(-lc, ukj, w[rc]);
                for (int i = lbc + t + nt; i < lec; i += nt) {
                    const int r = row[i];
                    w[r] = fmaf(-slab[i], ukj, w[r]);
                }
                lds_barrier();                       // (w only: no thread reads another's global writes before the column's last barrier)
            }
        }
        const float piv = w[j];
        if (!(fabsf(piv) > PF_TINY_PIVOT)) return false;
        const float pinv = 1.f / piv;
        for (int i = c0 + t; i < c1; i += nt) {
            const float v = w[row[i]];
            slab[i] = i > dg ? v * pinv : v;
        }
        __syncthreads();
    }
    return true;
}

// L y = F, then U x = y, by columns, in fp64 on F [m] (LDS or global); on exit F[j] = U_jj x_j: the caller divides by the
// diagonal (pfc_solution).  Ends behind a barrier.
template <int THREADS>
__device__ __forceinline__ void pfc_substitute(const PfcMatrix A, const float* slab, double* F) {
    const int t = threadIdx.x, lane = t & 63;
    constexpr int nt = THREADS;
    const int m = A.m;
    for (int j0 = 0; j0 < m; j0 += 64) {
        const int cnt = min(64, m - j0);
        int myb = 0, mye = 0;
        if (lane < cnt) {
            myb = A.diag[j0 + lane] + 1;
            mye = A.colptr[j0 + lane + 1];
        }
        for (int q = 0; q < cnt; ++q) {
            const int lb = __shfl(myb, q), le = __shfl(mye, q);
            if (lb >= le) continue;                  // (uniform: nothing is written, the next step reads what a barrier already covers)
            const double yj = F[j0 + q];
            for (int i = lb + t; i < le; i += nt) F[A.row[i]] -= (double)slab[i] * yj;
            __syncthreads();
        }
    }
    for (int j1 = m; j1 > 0; j1 -= 64) {
        const int cnt = min(64, j1);
        int myb = 0, mye = 0;
        if (lane < cnt) {
            myb = A.colptr[j1 - 1 - lane];
            mye = A.diag[j1 - 1 - lane];
        }
        for (int q = 0; q < cnt; ++q) {
            const int ub = __shfl(myb, q), ue = __shfl(mye, q);
            if (ub >= ue) continue;
            const double xj = F[j1 - 1 - q] / (double)slab[ue];
            for (int i = ub + t; i < ue; i += nt) F[A.row[i]] -= (double)slab[i] * xj;
            __syncthreads();
        }
    }
    __syncthreads();
}

__device__ __forceinline__ double pfc_solution(const PfcMatrix A, const float* slab, const double* F, int j) {
    return F[j] / (double)slab[A.diag[j]];
}

}  // namespace pfn
