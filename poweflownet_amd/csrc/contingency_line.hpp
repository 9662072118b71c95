// The per-line arithmetic of the N-1 screen, spelled once for the dense kernel (contingency.hip) and the sparse route
// (contingency_sparse.hip): den_k and the post-outage flow of line l from the outage's sensitivity vector, in fp32.
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

}  // namespace pfn
