// What the two screens of the sparse route share (contingency_sparse.hip: N-1; contingency_pairs_sparse.hip: N-2): the layout of a
// scenario's workspace slab, the outage block W [m + 1][64] with its column updates, the tile substitution -- named once,
// cs_substitute --, and the host side of the base launch, which contingency_sparse.hip owns and exports: one copy of
// contingency_sparse_base_kernel serves both entries.
#pragma once
#include "powerflow_common.hpp"
#include "powerflow_sparse_core.hpp"

namespace pfn {

constexpr int CS_GROUPS_PER_CU = 16;                // groups = 0: min(items, this many one-wave workgroups per compute unit): the sweep of DESIGN 7v

// a scenario's slab: double vm, th [n], F [m]; float factor [nnz], f32, x32, rat [e]; int pa, pb [e]; rounded to 16 bytes; behind it,
// on the pair screen, the column table float cols [c][m + 1] (candidate-major, plan order, row m the slack's zero), rounded to 16
__host__ __device__ inline size_t cs_sample_bytes(int n, int m, int nnz, int e) {
    return ((size_t)8 * (2 * (size_t)n + m) + (size_t)4 * nnz + (size_t)20 * e + 15) & ~(size_t)15;
}
__host__ __device__ inline size_t cs_cols_bytes(int c, int m) { return ((size_t)4 * c * ((size_t)m + 1) + 15) & ~(size_t)15; }
// an outage block: m + 1 rows of 64 floats
__host__ __device__ inline size_t cs_block_bytes(int m) { return (size_t)256 * ((size_t)m + 1); }
static inline bool cs_block_fits_lds(int m) { return cs_block_bytes(m) <= (size_t)(kLdsCuBytes - kLdsReserve); }
static inline int64_t cs_tiles(int64_t e) { return (e + 63) / 64; }
static inline int64_t cs_groups(int64_t n_samples, int64_t e, int groups) {
    const int64_t items = n_samples * cs_tiles(e);
    const int64_t want = groups > 0 ? (int64_t)groups : (int64_t)CS_GROUPS_PER_CU * device_cus();
    return items < want ? items : want;
}

struct CsSlab {
    double* vm;
    double* th;
    double* F;
    float* factor;
    float* f32;
    float* x32;
    float* rat;
    int32_t* pa;
    int32_t* pb;
};
__device__ __forceinline__ CsSlab cs_slab(void* ws, size_t stride, int s, int n, int m, int nnz, int e) {
    CsSlab b;
    b.vm = reinterpret_cast<double*>(static_cast<unsigned char*>(ws) + (size_t)s * stride);
    b.th = b.vm + n;
    b.F = b.th + n;
    b.factor = reinterpret_cast<float*>(b.F + m);
    b.f32 = b.factor + nnz;
    b.x32 = b.f32 + e;
    b.rat = b.x32 + e;
    b.pa = reinterpret_cast<int32_t*>(b.rat + e);
    b.pb = b.pa + e;
    return b;
}

// what the launches behind the base launch read of a scenario's slab (cs_slab's layout from the factor on), and the column table
struct CsLines {
    const float* fac;
    const float* f32;
    const float* x32;
    const float* rat;
    const int32_t* pa;
    const int32_t* pb;
};
__device__ __forceinline__ CsLines cs_lines(const unsigned char* slabs, size_t stride, int s, int n, int m, int nnz, int e) {
    CsLines b;
    b.fac = reinterpret_cast<const float*>(slabs + (size_t)s * stride + (size_t)8 * (2 * (size_t)n + m));
    b.f32 = b.fac + nnz;
    b.x32 = b.f32 + e;
    b.rat = b.x32 + e;
    b.pa = reinterpret_cast<const int32_t*>(b.rat + e);
    b.pb = b.pa + e;
    return b;
}

struct CsArgs {
    PfProblem p;                                    // (table, residual, init, line_mask, unplaced: null; ws: the scenarios' slabs)
    const int32_t* plan;
    const double* ratings;                          // [e], [S, e] or null (1.0 everywhere)
    const int32_t* islands;                         // [e]
    float* severity;                                // [S, e]
    int32_t* worst_line;                            // [S, e]
    int32_t* overloads;                             // [S, e]
    double* base_flow;                              // [S, e]
    float* post_flow;                               // [S, e, e] or null
    float* blocks;                                  // the global placement's outage blocks, one per workgroup, or null
    size_t ws_stride;
    int m, nnz, n_pv, ratings_per_sample, f_in_lds;
};

// What a substitution launch reads but never writes comes in through const __restrict__ pointers: hipcc may then take the
// wave-uniform loads (column bounds, row ids, factor values, the per-line vectors) for what they are, whatever the lanes store into W
// meanwhile.  A row id is read as half of an aligned 32-bit word (the plan's sections are 16-byte aligned).
__device__ __forceinline__ size_t cs_row(const uint32_t* __restrict__ row32, int i) {
    const uint32_t wd = row32[i >> 1];
    return (size_t)((i & 1) ? wd >> 16 : wd & 0xffffu) * 64;
}
// W[r] = fma(-v, y, W[r]) for the B entries at i of one column: the rows of a column are distinct, so the B loads go out together
template <int B>
__device__ __forceinline__ void cs_update(float* __restrict__ W, const uint32_t* __restrict__ row32, const float* __restrict__ fac, int i, float y) {
    size_t r[B];
    float f[B], w[B];
#pragma unroll
    for (int u = 0; u < B; ++u) {
        r[u] = cs_row(row32, i + u);
        f[u] = fac[i + u];
    }
#pragma unroll
    for (int u = 0; u < B; ++u) w[u] = W[r[u]];
#pragma unroll
    for (int u = 0; u < B; ++u) W[r[u]] = fmaf(-f[u], y, w[u]);
}
__device__ __forceinline__ void cs_column(float* __restrict__ W, const uint32_t* __restrict__ row32, const float* __restrict__ fac, int cb, int ce,
                                          float y) {
    int i = cb;
    for (; i + 8 <= ce; i += 8) cs_update<8>(W, row32, fac, i, y);
    if (i + 4 <= ce) {
        cs_update<4>(W, row32, fac, i, y);
        i += 4;
    }
    for (; i < ce; ++i) cs_update<1>(W, row32, fac, i, y);
}

// THE tile substitution: this lane's column of W [m + 1][64] (W points at the lane's word of row 0; row m, the slack's, is zero and
// no column of the factor reaches it) becomes B'^-1 (e_pi - e_pj) in plan order, or stays zero without `run`.
__device__ __forceinline__ void cs_substitute(float* __restrict__ W, const int32_t* __restrict__ colptr, const int32_t* __restrict__ diag,
                                              const uint32_t* __restrict__ row32, const float* __restrict__ fac, int m, bool run, int pi, int pj) {
    // ---- the right-hand side e_i - e_j in plan order; a slack end adds nothing
    for (int r = 0; r < m; ++r) W[(size_t)r * 64] = 0.f;
    if (run) {
        if (pi < m) W[(size_t)pi * 64] += 1.f;
        if (pj < m) W[(size_t)pj * 64] -= 1.f;
    }
    // ---- L y = rhs, columns ascending: the bounds of the next column are requested while this one runs
    int lb = diag[0] + 1, le = colptr[1];
    for (int j = 0; j < m; ++j) {
        const int cb = lb, ce = le;
        if (j + 1 < m) {
            lb = diag[j + 1] + 1;
            le = colptr[j + 2];
        }
        if (cb >= ce) continue;
        cs_column(W, row32, fac, cb, ce, W[(size_t)j * 64]);
    }
    // ---- U x = y, columns descending
    int ub = colptr[m - 1], ue = diag[m - 1];
    for (int j = m - 1; j >= 0; --j) {
        const int cb = ub, ce = ue;
        if (j > 0) {
            ub = colptr[j - 1];
            ue = diag[j - 1];
        }
        const float x = W[(size_t)j * 64] / fac[ce];
        W[(size_t)j * 64] = x;
        cs_column(W, row32, fac, cb, ce, x);
    }
}

// ---- the host side of the base launch (defined in contingency_sparse.hip)
struct CsCall {                                     // what both entries take for the base launch
    const int64_t* edge_index;
    int64_t n_lines;
    const double* rx;
    const int32_t* bus_type;
    const double* spec;
    int64_t n_samples, n_bus, n_pv, n_pq;
    double tol;
    int max_iter;
    double* base_flow;
    int32_t* status;
    int32_t* flags;
    void* ws;
    const void* plan_header;
    const void* plan_dev;
    int threads, block_route, groups;
};
int cs_check_header(const int32_t* h, const char* who);
// the header, sizes, counts, plan, pointers and LDS budget of a call; fills the problem (table and residual null) and the base
// launch's dynamic LDS bytes
int cs_check_call(const char* who, const CsCall& c, PfProblem* p, size_t* base_lds);
int cs_launch_base(const CsArgs& a, const int32_t* h, int threads, int64_t n_samples, size_t base_lds, hipStream_t s);

}  // namespace pfn
