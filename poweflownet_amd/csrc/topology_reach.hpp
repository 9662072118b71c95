// The reach routine of the topology kernels, spelled once: topology.hip's draw and unsupplied count and contingency.hip's islands
// per removed line all ask which buses a root reaches over a line list held in LDS.
#pragma once
#include "pfn_internal.hpp"

namespace pfn {

__host__ __device__ inline size_t tp_align4(size_t v) { return (v + 3) & ~(size_t)3; }

// The lines name buses of the grid?  Checked on the 64-bit ids before any is narrowed or followed; every thread calls it.
__device__ __forceinline__ int tp_bad_lines(const int64_t* __restrict__ ei, int e, int n) {
    int bad = 0;
    for (int j = threadIdx.x; j < e; j += blockDim.x) bad |= (uint64_t)ei[j] >= (uint64_t)n || (uint64_t)ei[e + j] >= (uint64_t)n;
    return __syncthreads_or(bad);
}

// Buses NOT reachable from `root` over the lines (keep == null: all of them; else those with keep[j] != 0).  Level-synchronous
// relaxation like khop.hip's BFS without a queue: a round lets every line whose ends differ mark both reached; the writers of a
// flag all store 1, a round may see flags of its own round (it then gets further, never elsewhere: the flags only rise and the
// fixed point is the component of the root), and `changed` is combined by the barrier itself.  At most n - 1 rounds can change
// anything, so the loop is bounded by n whatever the input.  A thread reads the ids and keep flags of its OWN lines only (t,
// t + nt, ...: the ones it staged and flagged itself), so the first barrier it needs is the one behind the clearing of the flags.
// Every thread calls it; the count is uniform.
template <typename ID>
__device__ __forceinline__ int tp_unreached(const ID* __restrict__ from, const ID* __restrict__ to, const uint8_t* __restrict__ keep,
                                            int e, int n, int root, uint8_t* __restrict__ reached, int* __restrict__ s_count) {
    const int t = threadIdx.x, nt = blockDim.x;
    for (int i = t; i < n; i += nt) reached[i] = i == root;
    if (t == 0) *s_count = 0;
    __syncthreads();
    for (int round = 0; round < n; ++round) {
        int changed = 0;
        for (int j = t; j < e; j += nt) {
            if (keep && !keep[j]) continue;
            const int f = from[j], g = to[j];
            if (reached[f] != reached[g]) {
                reached[f] = 1;
                reached[g] = 1;
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
    int c = 0;
    for (int i = t; i < n; i += nt) c += !reached[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((t & 63) == 0 && c) atomicAdd(s_count, c);   // (an LDS word; integer sums have no order)
    __syncthreads();
    const int total = *s_count;
    __syncthreads();                                 // (the next call clears the word)
    return total;
}

// threads of a workgroup that walks n buses and e lines: one wave while a barrier would cost more than it hides, 1024 for 6470rte
static inline int tp_threads(int n, int e) {
    const int items = n > e ? n : e;
    return items <= 64 ? 64 : items <= 2048 ? 256 : 1024;
}

}  // namespace pfn
