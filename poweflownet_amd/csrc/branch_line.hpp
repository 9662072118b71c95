// The per-bus and per-line arithmetic of the line-current kernels, spelled once: branch_flows.hip (the flows of finished bus tables)
// and contingency_model.hip (the loadings of the network's N-1 screen) agree bit for bit because they share this text.  All fp32.
#pragma once
#include "pfn_internal.hpp"

namespace pfn {

// the largest n_bus whose rectangular voltages the flows kernels keep in LDS (8 bytes per bus and table, two tables in pfn_branch_flows)
constexpr int BF_LDS_MAX_BUS = (kLdsCuBytes - kLdsReserve) / 16;        // 10176 buses

// (e, f) of one bus row; the angle as bus_of (physics.hip) forms it.  No contraction: the direct kernel inlines this into the
// line expressions, where vm * c - ... would otherwise fuse and differ from the value the LDS kernel stores
__device__ __forceinline__ float2 bf_phasor(const float* __restrict__ table, int64_t row, bool norm, const float* sd, const float* mu) {
#pragma clang fp contract(off)
    const float2 v = *reinterpret_cast<const float2*>(table + 4 * row);
    const float vm = norm ? denorm(v.x, sd[0], mu[0]) : v.x;
    const float va = (norm ? denorm(v.y, sd[1], mu[1]) : v.y) * (3.14159265358979323846f / 180.0f);
    float s, c;
    sincosf(va, &s, &c);
    return make_float2(vm * c, vm * s);
}

// the same for a (Vm, Va in degrees) pair that is already in registers -- a row merged from two sources (contingency_model.hip):
// bf_phasor's arithmetic on a finished, de-normalised row
__device__ __forceinline__ float2 bf_phasor_of(float vm, float va_deg) {
#pragma clang fp contract(off)
    const float va = va_deg * (3.14159265358979323846f / 180.0f);
    float s, c;
    sincosf(va, &s, &c);
    return make_float2(vm * c, vm * s);
}

// {I, P, Q, loss} of the line i -> j with series impedance r + jx; P and Q as power_imbalance_fwd_kernel writes them.  Every
// operation rounded on its own: what hipcc fuses differs between the instantiations of branch_flows_kernel, and the flows of a table
// must not depend on whether a second table came along or on which kernel served the gathers
__device__ __forceinline__ float4 bf_line(float2 vi, float2 vj, float r, float x) {
#pragma clang fp contract(off)
    const float d = r * r + x * x;
    const float g = r / d, b = -x / d;
    const float de = vi.x - vj.x, df = vi.y - vj.y;
    const float m2 = de * de + df * df;
    const float t1 = vi.x * vj.x - vi.x * vi.x + vi.y * vj.y - vi.y * vi.y, t2 = vi.y * vj.x - vi.x * vj.y;
    return make_float4(sqrtf(m2) / sqrtf(d), g * t1 + b * t2, g * t2 - b * t1, g * m2);
}

}  // namespace pfn
