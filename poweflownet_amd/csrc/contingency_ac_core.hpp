// The outage arithmetic of the AC N-1 screens, spelled once: what the dense route (contingency_ac.hip, a wave per outage, the state
// in rows of stride 1) and the sparse route (contingency_ac_sparse.hip, a lane per outage, the state in columns of stride 64) do with
// one (scenario, outage) apart from the half step itself.  Both kernels and both C entries go through these functions, so "same
// definitions, same outputs, same statuses" holds because the rules are one text:
//   a bus's mismatch is spec - (the sum of pf_ac_end over its line ends in stored order, line k skipped), fp64; |F| by
//     pf_abs_clamped (a non-finite entry counts as +inf); the half's scaled mismatch is g = F / Vm by the half's unknown;
//   a line's weight c_k in a matrix is 1 / x or x / (r^2 + x^2) -- XB: B' from the first, B'' from the second; BX the other way
//     round -- and the rank-1 denominator is 1 / c_k - a^T w;
//   the kept state is fp32 (Vm, Va in degrees), the slack's angle the specified one; the phasors are bf_phasor_of of that state;
//   the lowest voltage runs over the PQ buses: a non-finite Vm is the lowest (key -inf), a violation, and makes vm_min NaN; ties
//     go to the lowest bus -- strict < over a thread's ascending buses, (key, bus) in every merge; no PQ bus gives (NaN, -1, 0);
//   a line's current is bf_line(...).x of the two phasors, NaN at l = k; line k and a line whose rating is not > 0 are not
//     monitored; the loading is current / rating, reduced by contingency_monitor.hpp;
//   a skipped item -- its scenario failed, or it islands buses -- carries ct_skip's figures, NaN rows, NaN vm_min and mismatch and
//     -1 in vm_min_bus and v_violations.
// Left to each route on purpose: the half step (X g by rows of an inverse against two substitutions through a factor), the w . g
// sum (butterfly against serial), the outer loops (lanes own buses and lines against one lane walking all) and the base launch.
// The host half: the option, null-pointer and alignment checks the two entries share, one message text each.
#pragma once
#include "branch_line.hpp"
#include "contingency_monitor.hpp"
#include "powerflow_common.hpp"

namespace pfn {

// where an outage's results go: item o = s * e + k
struct CaOut {
    float* severity;                                // [S, e]
    int32_t* worst_line;
    int32_t* overloads;
    float* vm_min;
    int32_t* vm_min_bus;
    int32_t* v_violations;
    double* mismatch;
    float* post_current;                            // [S, e, e] or null
    float* post_state;                              // [S, e, n, 2] or null
};

// ---- bus i (not the slack) of the grid without line k: its line ends adj[q0 .. q1) in stored order, adj[q] = (line << SHIFT | .,
// other end); TH, VM by bus and G by unknown with STRIDE doubles between entries.  mode 0: G = dP / Vm at the angle unknown ra;
// mode 1: G = dQ / Vm at the PQ unknown rq (< 0: not a PQ bus); mode 2: nothing stored.  Returns mx raised to the bus's |F|.
template <int STRIDE, int SHIFT>
__device__ __forceinline__ double ca_bus_mismatch(double mx, const double* TH, const double* VM, double* G, const int2* adj, int q0, int q1,
                                                  const double* rx, const double* spec, int i, int ra, int rq, int k, int mode) {
    const double vi = VM[(size_t)i * STRIDE], ti = TH[(size_t)i * STRIDE];
    double sP = 0.0, sQ = 0.0;
    for (int q = q0; q < q1; ++q) {
        const int2 lj = adj[q];
        const int line = lj.x >> SHIFT;
        if (line == k) continue;
        pf_ac_end(rx[2 * line], rx[2 * line + 1], vi, ti, VM[(size_t)lj.y * STRIDE], TH[(size_t)lj.y * STRIDE], sP, sQ);
    }
    const double fp = spec[4 * i + 2] - sP;
    mx = fmax(mx, pf_abs_clamped(fp));
    if (mode == 0) G[(size_t)ra * STRIDE] = fp / vi;
    if (rq >= 0) {
        const double fq = spec[4 * i + 3] - sQ;
        mx = fmax(mx, pf_abs_clamped(fq));
        if (mode == 1) G[(size_t)rq * STRIDE] = fq / vi;
    }
    return mx;
}

// ---- 1 / c_k - a^T w of a half; c = ca_weights(r_k, x_k), the two weights a line can have in a matrix
__device__ __forceinline__ double2 ca_weights(double rk, double xk) { return make_double2(1.0 / xk, xk / (rk * rk + xk * xk)); }
__device__ __forceinline__ double ca_den(double2 c, bool bx, bool qhalf, double atw) { return 1.0 / (qhalf == bx ? c.x : c.y) - atw; }

// ---- the lowest voltage over the PQ buses
struct CaLow {
    float best;                                     // the lowest key so far; +inf: none (a key is a finite Vm or -inf, so "none" loses every merge)
    int arg, cnt, wild;                             // its bus, -1: none; the violations; a non-finite Vm was seen
};
__device__ __forceinline__ CaLow ca_low_none() { return CaLow{__builtin_inff(), -1, 0, 0}; }
__device__ __forceinline__ void ca_low_add(CaLow& w, int bus, float vm32, float v_lo, float v_hi) {
    const bool finite = fabsf(vm32) < __builtin_inff();
    const float key = finite ? vm32 : -__builtin_inff();
    w.wild |= !finite;
    w.cnt += !finite || vm32 < v_lo || vm32 > v_hi;
    if (key < w.best) { w.best = key; w.arg = bus; }
}
__device__ __forceinline__ void ca_low_merge(CaLow& w, const CaLow& o) {
    if (o.best < w.best || (o.best == w.best && o.arg < w.arg)) { w.best = o.best; w.arg = o.arg; }
    w.cnt += o.cnt;
    w.wild |= o.wild;
}

// ---- bus b of the final state: the fp32 (Vm, Va in degrees), its phasor, the kept row and, at a PQ bus, the voltage figures
template <int STRIDE>
__device__ __forceinline__ void ca_bus_tail(CaLow& low, const double* TH, const double* VM, float2* PH, float* srow, const double* spec, int b,
                                            bool slack, bool pq, float v_lo, float v_hi) {
    const float vm32 = (float)VM[(size_t)b * STRIDE];
    const float va32 = (float)(slack ? spec[4 * b + 1] : TH[(size_t)b * STRIDE] * (1.0 / PF_RAD));
    PH[(size_t)b * STRIDE] = bf_phasor_of(vm32, va32);
    if (srow) *reinterpret_cast<float2*>(srow + 2 * b) = make_float2(vm32, va32);
    if (pq) ca_low_add(low, b, vm32, v_lo, v_hi);
}

// ---- line l under outage k: its current (NaN at k), the kept row, its loading where it is monitored
template <int STRIDE>
__device__ __forceinline__ void ca_line_tail(CtWorst& worst, const float2* PH, const int64_t* ei, const double* rx, const double* rat, float* crow,
                                             int e, int l, int k) {
    float cur = bf_line(PH[(size_t)ei[l] * STRIDE], PH[(size_t)ei[e + l] * STRIDE], (float)rx[2 * l], (float)rx[2 * l + 1]).x;
    if (l == k) cur = __builtin_nanf("");
    if (crow) crow[l] = cur;
    const float r = rat ? (float)rat[l] : 1.f;
    if (l != k && r > 0.f) ct_worst_add(worst, l, cur / r);
}

// ---- item o's figures, by its one owner
__device__ __forceinline__ void ca_store(const CaOut& out, int64_t o, const CtWorst& worst, const CaLow& low, double mx) {
    ct_store(ct_figures(worst), out.severity[o], out.worst_line[o], out.overloads[o]);
    out.vm_min[o] = low.arg < 0 || low.wild ? __builtin_nanf("") : low.best;
    out.vm_min_bus[o] = low.arg;
    out.v_violations[o] = low.cnt;
    out.mismatch[o] = mx;
}
// ---- a skipped item, ct_skip's shape: its threads (first, first + step, ...) fill the kept rows, thread 0 stores the figures
__device__ __forceinline__ void ca_skip(bool failed, const CaOut& out, int64_t o, float* crow, float* srow, int e, int n, int first, int step) {
    if (srow)
        for (int q = first; q < 2 * n; q += step) srow[q] = __builtin_nanf("");
    ct_skip(failed, crow, e, first, step, out.severity[o], out.worst_line[o], out.overloads[o]);
    if (first == 0) {
        out.vm_min[o] = __builtin_nanf("");
        out.vm_min_bus[o] = -1;
        out.v_violations[o] = -1;
        out.mismatch[o] = __builtin_nan("");
    }
}

// ------------------------------------------------------------------------------------------------------------ host
static inline int ca_check_options(const char* who, int64_t n_bus, int64_t n_pv, int64_t n_pq, int variant, int halves, float v_lo, float v_hi,
                                   double tol, int max_iter) {
    PFN_CHECK_ARG(n_pv >= 0 && n_pq >= 0 && n_pv + n_pq == n_bus - 1, "%s: %lld PV and %lld PQ buses do not leave exactly one slack among %lld buses",
                  who, (long long)n_pv, (long long)n_pq, (long long)n_bus);
    PFN_CHECK_ARG(variant == 0 || variant == 1, "%s: variant must be 0 (XB) or 1 (BX)", who);
    PFN_CHECK_ARG(halves >= 0, "%s: halves must be >= 0; got %d", who, halves);
    PFN_CHECK_ARG(v_lo <= v_hi, "%s: v_limits must be in order (low <= high, no NaN); got (%g, %g)", who, (double)v_lo, (double)v_hi);
    PFN_CHECK_ARG(max_iter >= 0 && tol > 0.0, "%s: max_iter must be >= 0 and tol > 0", who);
    return PFN_OK;
}

// the null test and the three-tier alignment test of an entry's pointers; has_plan: the route reads a device plan (16-byte, like ws)
static inline int ca_check_pointers(const char* who, const int64_t* edge_index, const double* rx, const int32_t* bus_type, const double* spec,
                                    const double* init, const double* ratings, const int32_t* islands, const CaOut& o, const double* base_table,
                                    const int32_t* status, const double* residual, const int32_t* flags, const void* ws, bool has_plan,
                                    const void* plan_dev) {
    PFN_CHECK_ARG(edge_index && rx && bus_type && spec && islands && o.severity && o.worst_line && o.overloads && o.vm_min && o.vm_min_bus &&
                      o.v_violations && o.mismatch && base_table && status && residual && flags && (plan_dev || !has_plan),
                  "%s: null pointer", who);
    const auto at = [](const void* q) { return reinterpret_cast<uintptr_t>(q); };
    PFN_CHECK_ARG((at(base_table) & 31) == 0 && ((at(ws) | at(plan_dev)) & 15) == 0 &&
                      ((at(edge_index) | at(rx) | at(spec) | at(init) | at(ratings) | at(residual) | at(o.mismatch) | at(o.post_state)) & 7) == 0 &&
                      ((at(bus_type) | at(islands) | at(o.severity) | at(o.worst_line) | at(o.overloads) | at(o.vm_min) | at(o.vm_min_bus) |
                        at(o.v_violations) | at(status) | at(o.post_current) | at(flags)) & 3) == 0,
                  "%s: base_table must be 32-byte aligned, the workspace%s 16-byte, fp64 and int64 arrays and post_state 8-byte, fp32 and int32 arrays 4-byte",
                  who, has_plan ? " and the plan" : "");
    return PFN_OK;
}

}  // namespace pfn
