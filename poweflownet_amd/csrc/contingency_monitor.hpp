// The per-item tail of the contingency screens, spelled once: how the loadings of the monitored lines of one item -- a (scenario,
// outage) or a (scenario, pair) -- become its three figures, and what a skipped item carries.  The dense and sparse N-1 and N-2
// kernels (contingency.hip, contingency_sparse.hip, contingency_pairs.hip, contingency_pairs_sparse.hip) and the network's screen
// (contingency_model.hip) all reduce through these functions, so the rules are the same on every route because they are one text:
//   a rating that is not > 0 (zero, negative, NaN) leaves its line unmonitored -- the caller's test, one expression at the call;
//   a loading is >= 0; a non-finite one counts as +inf, so that the lowest such line is the worst, and makes the severity NaN;
//   the largest loading wins, ties go to the lowest line: strict > over a thread's ascending lines, (key, line) in every merge;
//   overloads are an integer count of loading > 1; no monitored line gives (0, -1, 0);
//   a failed scenario is (NaN, -1, -1), an islanding item (+inf, -1, -1) so that it ranks first; both with a NaN table row.
// Every cross-thread step is a max or an integer sum: no order to keep, no float atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pfn {

struct CtWorst {
    float best;                                     // the largest key so far; -1: none (a loading is >= 0)
    int arg;                                        // its line, the lowest among equals
    int cnt, wild;                                  // loadings > 1; a non-finite loading was seen
};
constexpr int CT_NO_LINE = 0x7fffffff;              // (above every line id: loses every tie, marks "nothing monitored")
__device__ __forceinline__ CtWorst ct_worst_none() { return CtWorst{-1.f, CT_NO_LINE, 0, 0}; }

// the DC screens' loading of a line
__device__ __forceinline__ float ct_loading(float post, float rating) { return fabsf(post) / rating; }

// line l, monitored, with this loading.  A thread adds its lines in ascending order: strict > keeps the lowest of equals.
__device__ __forceinline__ void ct_worst_add(CtWorst& w, int l, float load) {
    const float infv = __builtin_inff();
    const bool finite = load < infv;
    const float key = finite ? load : infv;
    w.wild |= !finite;
    w.cnt += load > 1.f;
    if (key > w.best) { w.best = key; w.arg = l; }
}

__device__ __forceinline__ void ct_worst_merge(CtWorst& w, const CtWorst& o) {
    if (o.best > w.best || (o.best == w.best && o.arg < w.arg)) { w.best = o.best; w.arg = o.arg; }
    w.cnt += o.cnt;
    w.wild |= o.wild;
}

// over the 64 lanes of a wave: every lane ends with the wave's
__device__ __forceinline__ CtWorst ct_worst_wave(CtWorst w) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        ct_worst_merge(w, CtWorst{__shfl_xor(w.best, off), __shfl_xor(w.arg, off), __shfl_xor(w.cnt, off), __shfl_xor(w.wild, off)});
    return w;
}

// the three figures of an item: a computed one's from its accumulator; a skipped one's -- its scenario failed, or else it islands
// buses -- as the rule sets them.  By value, so that a lane that owns an item selects between the two; the item's one owner stores.
struct CtFigures {
    float severity;
    int32_t worst_line, overloads;
};
__device__ __forceinline__ CtFigures ct_figures(const CtWorst& w) {
    const bool none = w.arg == CT_NO_LINE;
    return CtFigures{none ? 0.f : (w.wild ? __builtin_nanf("") : w.best), none ? -1 : w.arg, w.cnt};
}
__device__ __forceinline__ CtFigures ct_figures_skipped(bool failed) { return CtFigures{failed ? __builtin_nanf("") : __builtin_inff(), -1, -1}; }
__device__ __forceinline__ void ct_store(const CtFigures& f, float& severity, int32_t& worst_line, int32_t& overloads) {
    severity = f.severity;
    worst_line = f.worst_line;
    overloads = f.overloads;
}
// a skipped item whose owner is a wave or a workgroup: its threads (first, first + step, ...) fill the table row, where there is
// one, with NaN; thread 0 stores the figures
__device__ __forceinline__ void ct_skip(bool failed, float* row, int e, int first, int step, float& severity, int32_t& worst_line,
                                        int32_t& overloads) {
    if (row)
        for (int l = first; l < e; l += step) row[l] = __builtin_nanf("");
    if (first == 0) ct_store(ct_figures_skipped(failed), severity, worst_line, overloads);
}

}  // namespace pfn
