// What the dense kernels that keep a sample's fp32 matrix resident -- powerflow.hip's solver, contingency.hip's N-1 screen -- share:
// the dense cap, the workgroup-size rule, the odd leading dimension with the size of a matrix slab, and the in-place Gauss-Jordan
// inverse of a symmetric, diagonally dominant matrix (B' or B'').  Spelled once: the screen's B'^-1 is the fast-decoupled modes'.
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

}  // namespace pfn
