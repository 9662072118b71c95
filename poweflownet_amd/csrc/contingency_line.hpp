// The per-line arithmetic of the contingency screens, spelled once: for the dense N-1 kernel (contingency.hip) and the sparse route
// (contingency_sparse.hip) den_k and the post-outage flow of line l from the outage's sensitivity vector; for the N-2 pair screen
// (contingency_pairs.hip, contingency_pairs_sparse.hip) the ct_pair_* functions below.  All fp32.  What becomes of a line's flow
// afterwards -- its loading, the maximum with its ties, the overload count, the three stores -- is contingency_monitor.hpp, for every
// screen; the dense sensitivity column itself is contingency_base.hpp's ct_column.
#pragma once
#include <hip/hip_runtime.h>

namespace pfn {

// den_k and the post-outage flow of line l, every operation rounded on its own: what hipcc fuses must not depend on the
// instantiation or on whether the table row is written
__device__ __forceinline__ float ct_den(float wi, float wj, float x) {
#pragma clang fp contract(off)
    const float phi = (wi - wj) / x;
    return 1.f - phi;
}
__device__ __forceinline__ float ct_post(float wa, float wb, float x, float den, float fl, float fk) {
#pragma clang fp contract(off)
    const float phi = (wa - wb) / x;
    const float q = phi / den;
    const float d = q * fk;
    return fl + d;
}

// ---- the N-2 screen (contingency_pairs.hip): the simultaneous outage of lines a and b is a rank-2 update of the same inverse.
//     M = [[1 - phi_aa, -phi_ab], [-phi_ba, 1 - phi_bb]]      t = M^-1 (f_a, f_b)      f_l^(a,b) = f_l + phi_la t_a + phi_lb t_b
// pair p = (lines[i], lines[j]), i < j, row-major in (i, j) among c candidates (also contingency_pairs_sparse.hip): the index of pair (i, i + 1)
__host__ __device__ inline int64_t cp_first_pair(int64_t i, int64_t c) { return i * (2 * c - i - 1) / 2; }
// phi_{l,k}, the sensitivity of line l = (a -> b) to the outage of line k, from w_k
__device__ __forceinline__ float ct_pair_phi(float wa, float wb, float x) {
#pragma clang fp contract(off)
    return (wa - wb) / x;
}
// t = M^-1 (f_a, f_b) by Cramer's rule; a singular M (an islanding pair, which the line list decides and nobody reads) divides by 0
__device__ __forceinline__ void ct_pair_solve(float paa, float pab, float pba, float pbb, float fa, float fb, float* ta, float* tb) {
#pragma clang fp contract(off)
    const float da = 1.f - paa, db = 1.f - pbb;
    const float dd = da * db;
    const float oo = pab * pba;
    const float det = dd - oo;
    const float na1 = db * fa, na2 = pab * fb;
    const float nb1 = pba * fa, nb2 = da * fb;
    const float na = na1 + na2, nb = nb1 + nb2;
    *ta = na / det;
    *tb = nb / det;
}
__device__ __forceinline__ float ct_pair_post(float pla, float plb, float fl, float ta, float tb) {
#pragma clang fp contract(off)
    const float d1 = pla * ta;
    const float d2 = plb * tb;
    const float s1 = fl + d1;
    return s1 + d2;
}

}  // namespace pfn
