// The ordered reductions of the loss and analysis kernels (gfx950), each written ONCE: tests pin their results bit for bit, so the
// order of every addition is part of the interface.  Device code only; included by the units that reduce (util_kernels.hip,
// physics.hip, bus_errors.hip, branch_flows.hip), not by pfn_internal.hpp.  The hand-off the grid-wide sums end with is
// device_prims.hpp's ("the last-arriver hand-off").
#pragma once
#include "pfn_internal.hpp"

namespace pfn {

// ---------------------------------------------------------------------------- the 256-thread tree
// red[t] += red[t + off], off = 128 ... 1, for one or several arrays of 256 entries at a time (one barrier per level for all of
// them); red[0] holds the sums when it returns.  The leading barrier publishes the entries the callers have just written.
template <typename... T>
__device__ __forceinline__ void block_tree_256(int t, T*... red) {
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) ((red[t] += red[t + off]), ...);
        __syncthreads();
    }
}

// Sum of one float per thread over the whole grid (<= 256 blocks of 256 threads) in ONE launch: every block reduces its values to
// a partial, publishes it and takes a ticket; the last arriver sums the partials in BLOCK order (not arrival order: deterministic)
// and re-arms the counter for the next call.  True in the last block only, `total` valid there.  DRAINED: the hand-off flavour.
template <bool DRAINED>
__device__ __forceinline__ bool grid_sum_ordered(float acc, float* __restrict__ partial, int* __restrict__ counter, float& total) {
    __shared__ float red[256];
    __shared__ int s_last;
    const int t = threadIdx.x;
    red[t] = acc;
    block_tree_256(t, red);
    if (t == 0) {
        if (DRAINED) {
            agent_store(partial + blockIdx.x, red[0]);
            s_last = handoff_drained_publish(counter);
        } else {
            partial[blockIdx.x] = red[0];
            s_last = handoff_fenced_publish(counter);
        }
    }
    __syncthreads();
    if (!s_last) return false;
    if (!DRAINED) handoff_fenced_consume();
    red[t] = t < (int)gridDim.x ? agent_load(partial + t) : 0.f;
    block_tree_256(t, red);
    total = red[0];
    if (t == 0) *counter = 0;
    return true;
}

// -------------------------------------------------------------------------- the masked-L2 combine
// (sum, count) of the two entry sets of Masked_L2_loss over the grid, as grid_sum_ordered (fenced flavour) on four values at once:
// the last arriver leaves the block-order totals in the workspace -- the gradient kernels read them -- and re-arms the counter.
struct MaskedL2Ws {
    float s1[256], s0[256];
    int c1[256], c0[256];
    float tot_s1, tot_s0;
    int tot_c1, tot_c0;
    int pad_[3];
    int counter;   // byte 4124
};
__device__ __forceinline__ bool masked_l2_combine(float a1, float a0, int k1, int k0, MaskedL2Ws* __restrict__ w) {
    __shared__ float rs1[256], rs0[256];
    __shared__ int rc1[256], rc0[256];
    __shared__ int s_last;
    const int t = threadIdx.x;
    rs1[t] = a1; rs0[t] = a0; rc1[t] = k1; rc0[t] = k0;
    block_tree_256(t, rs1, rs0, rc1, rc0);
    if (t == 0) {
        w->s1[blockIdx.x] = rs1[0]; w->s0[blockIdx.x] = rs0[0]; w->c1[blockIdx.x] = rc1[0]; w->c0[blockIdx.x] = rc0[0];
        s_last = handoff_fenced_publish(&w->counter);
    }
    __syncthreads();
    if (!s_last) return false;
    handoff_fenced_consume();
    const bool in = t < (int)gridDim.x;
    rs1[t] = in ? agent_load(&w->s1[t]) : 0.f;
    rs0[t] = in ? agent_load(&w->s0[t]) : 0.f;
    rc1[t] = in ? agent_load(&w->c1[t]) : 0;
    rc0[t] = in ? agent_load(&w->c0[t]) : 0;
    block_tree_256(t, rs1, rs0, rc1, rc0);
    if (t == 0) {
        w->tot_s1 = rs1[0]; w->tot_s0 = rs0[0]; w->tot_c1 = rc1[0]; w->tot_c0 = rc0[0];
        w->counter = 0;
    }
    return true;
}

// ---------------------------------------------------------------------------- the moments engine
// Six running moments {count, sum e, sum |e|, sum e^2, min e, max e} per OWNER (a bus, a line) and group, from a table walked by a
// workgroup of MO_OWNERS owner lanes x MO_SLICES slices: slice s takes the samples s, s + MO_SLICES, ... (16 lanes read 16
// consecutive 16-byte rows of ONE sample: 256 contiguous bytes), MO_UNROLL of them per trip, and keeps its moments in registers.
// They reach the running table in rounds of two accumulators per thread (moments_round).  The split depends on nothing but these
// constants, so a launch is a pure function of its inputs.
constexpr int MO_OWNERS = 16, MO_SLICES = 16, MO_THREADS = MO_OWNERS * MO_SLICES, MO_UNROLL = 4;
constexpr int MO_VALUES = 12;                      // the six moments of the two accumulators of a round
constexpr int MO_PART_LD = MO_THREADS + 1;         // (odd stride: the combine's lanes differ in the value index)

// e is a widened float, so e * e is exact in double and the fused and the unfused sum of squares are the same bits; the rounding is
// spelled out all the same, as hipcc compiled each kernel before the two shared this text: add() fuses, add_if() does not.
struct Moments6 {
    int cnt = 0;
    double sum = 0.0, sab = 0.0, ssq = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
    __device__ __forceinline__ void add(double e) {
        cnt += 1;
        sum += e;
        sab += fabs(e);
        ssq = fma(e, e, ssq);
        mn = fmin(mn, e);                          // fmin / fmax ignore a NaN operand
        mx = fmax(mx, e);
    }
    // branch-free: an entry that is not `in` adds 0 / offers +-inf, so a NaN poisons the group it belongs to only
    __device__ __forceinline__ void add_if(bool in, double e) {
#pragma clang fp contract(off)
        const double inf = __builtin_inf(), sq = e * e;
        cnt += in ? 1 : 0;
        sum += in ? e : 0.0;
        sab += in ? fabs(e) : 0.0;
        ssq += in ? sq : 0.0;
        mn = fmin(mn, in ? e : inf);
        mx = fmax(mx, in ? e : -inf);
    }
};

// One round: every thread hands two accumulators over through LDS; thread (owner cb, value cv) -- t < 16 * 12 -- then combines the
// MO_SLICES slice partials in slice order (sums add, min / max fold) and folds the result into the running value it found at
// table[owner * stride + 12 * round + cv].  `round` > 0 waits for the previous round's readers first.
__device__ __forceinline__ void moments_round(const Moments6& m0, const Moments6& m1, int round, int n_owners, int64_t stride,
                                              double* __restrict__ table) {
    __shared__ double part[MO_VALUES * MO_PART_LD];
    const int t = threadIdx.x;
    if (round) __syncthreads();
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const Moments6& m = g ? m1 : m0;
        double* q = part + (g * 6) * MO_PART_LD + t;
        q[0] = (double)m.cnt;
        q[MO_PART_LD] = m.sum;
        q[2 * MO_PART_LD] = m.sab;
        q[3 * MO_PART_LD] = m.ssq;
        q[4 * MO_PART_LD] = m.mn;
        q[5 * MO_PART_LD] = m.mx;
    }
    __syncthreads();
    const int cb = t / MO_VALUES, cv = t - cb * MO_VALUES;
    const int owner = blockIdx.x * MO_OWNERS + cb;
    if (t < MO_OWNERS * MO_VALUES && owner < n_owners) {
        const int k = cv % 6;
        const double* q = part + cv * MO_PART_LD + cb;
        double a = q[0];
#pragma unroll
        for (int s = 1; s < MO_SLICES; ++s) {
            const double v = q[s * MO_OWNERS];
            a = k < 4 ? a + v : (k == 4 ? fmin(a, v) : fmax(a, v));
        }
        double* m = table + (int64_t)owner * stride + MO_VALUES * round + cv;
        const double was = *m;
        *m = k < 4 ? was + a : (k == 4 ? fmin(was, a) : fmax(was, a));
    }
}

}  // namespace pfn
