// The N-2 line-pair outage screen beyond the dense cap (gfx950): pfn_contingency_pairs_sparse, three launches behind
// pfn_contingency_pair_islands.  Same model, same definitions, same pair order and statuses as pfn_contingency_pairs; where that keeps
// the dense inverse of B' this one keeps the sparse fp32 FACTOR of pfn_contingency_sparse and one column w_k = B'^-1 (e_i - e_j) per
// candidate line.
//
// BASE: contingency_sparse.hip's contingency_sparse_base_kernel, the same code (cs_launch_base): base_flow and status carry
// contingency_screen(route="sparse")'s bits; the slab keeps the factor and the per-line vectors, and gets a column table appended.
//
// COLUMNS, contingency_pairs_sparse_columns_kernel: a lane per candidate, a one-wave workgroup per tile of 64 consecutive candidates
// (in `lines` order); workgroup g of G takes the items (scenario, tile) g, g + G, ...  The block W [m + 1][64] sits in LDS or in the
// workgroup's block of the workspace by pfn_contingency_sparse's rule; cs_substitute (contingency_sparse_core.hpp) is the N-1 outage
// kernel's substitution, so column k holds the bits that kernel holds for outage lines[k].  The tile then goes into the scenario's
// column table cols [c][m + 1] fp32 -- candidate-major, plan order, row m (the slack) zero -- 64 consecutive rows of one candidate per
// store: the pair launch reads whole columns.  A candidate all of whose pairs island (a bridge among them) keeps a zero column that
// nobody reads; a failed scenario substitutes nothing; lanes past c are idle.
//
// PAIRS, contingency_pairs_sparse_kernel, the hot path: one workgroup of `waves` waves per (scenario, first candidate i).  Wave w
// takes the second candidates i + 1 + w, i + 1 + w + waves, ...: the four phi of M, t by ct_pair_solve, then the lanes stride over the
// lines -- ct_pair_phi twice, ct_pair_post, the loading |f| / rating -- and the one tail of all screens (contingency_monitor.hpp):
// max with ties to the lowest line, an integer sum, the non-finite flag; lane 0 writes the three outputs, the lanes write the table
// row coalesced.  The per-line vectors (f32, x32, rat, pa, pb: 20 bytes a line) stay in the slab and are read coalesced; only the two
// columns are placed: in LDS (w_a once per workgroup, one w_b per wave) or gathered from the column table -- one template, the same bits.
// The arithmetic is contingency_line.hpp's ct_pair_*, compiled without contraction; one owner per output: the bits of (scenario, a,
// b) are a pure function of the scenario's inputs, the plan and the two lines, whatever the batch, the candidate list, G, `threads`,
// `waves` or either placement.  No host sync, no allocation (capturable), no float atomics.
#include "contingency_line.hpp"
#include "contingency_monitor.hpp"
#include "contingency_sparse_core.hpp"

namespace pfn {

constexpr int CPS_WAVES = 4;                        // waves = 0: the sweep of DESIGN 7x

// the pair launch's columns in LDS: float wa [m + 1] | float wb [waves][m + 1]; rounded to 16 bytes
__host__ __device__ inline size_t cps_lds_bytes(int m, int waves) { return ((size_t)4 * ((size_t)m + 1) * (1 + waves) + 15) & ~(size_t)15; }
static inline bool cps_fits_lds(int m, int waves) { return cps_lds_bytes(m, waves) <= (size_t)(kLdsCuBytes - kLdsReserve); }
static inline bool cps_waves_ok(int waves) { return waves == 0 || waves == 1 || waves == 2 || waves == 4 || waves == 8 || waves == 16; }

// ------------------------------------------------------------------------------------------------------ columns
template <bool LDS>
__global__ __launch_bounds__(64) void contingency_pairs_sparse_columns_kernel(const unsigned char* __restrict__ plan, const unsigned char* __restrict__ slabs,
                                                                              float* cols0, float* __restrict__ blocks,
                                                                              const int32_t* __restrict__ status, const int32_t* __restrict__ lines,
                                                                              const int32_t* __restrict__ islands, size_t ws_stride, int n, int e, int m,
                                                                              int nnz, int c, int n_samples) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cps_smem[];
    const int lane = threadIdx.x;
    const int32_t* H = reinterpret_cast<const int32_t*>(plan);
    const int32_t* __restrict__ colptr = reinterpret_cast<const int32_t*>(plan + H[PFP_H_OFF_COLPTR]);
    const int32_t* __restrict__ diag = reinterpret_cast<const int32_t*>(plan + H[PFP_H_OFF_DIAG]);
    const uint32_t* __restrict__ row32 = reinterpret_cast<const uint32_t*>(plan + H[PFP_H_OFF_ROWIDX]);
    float* block;                                   // [m + 1][64]
    if constexpr (LDS) block = reinterpret_cast<float*>(cps_smem);
    else block = blocks + (size_t)blockIdx.x * 64 * ((size_t)m + 1);
    float* W = block + lane;                        // this lane's column is W[r * 64], r = 0 .. m
    const int tiles = (c + 63) >> 6;
    const int64_t items = (int64_t)n_samples * tiles;
    const size_t rows = (size_t)m + 1;
    W[(size_t)m * 64] = 0.f;                        // (the slack's row: no column of the factor reaches it)

    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int s = (int)(item / tiles);
        if (status[s] < 0) continue;                // a failed scenario: nothing is substituted, its table is never read
        const int k0 = (int)(item - (int64_t)s * tiles) * 64;
        const int k = k0 + lane;
        const bool live = k < c;                    // (lanes past c in the last tile are idle)
        const int kc = live ? k : c - 1;
        const int line = lines[kc];
        const bool named = (unsigned)line < (unsigned)e;   // (a candidate that is no line: its pairs carry -4 and are never computed)
        const int lc = named ? line : 0;
        // a candidate whose every pair islands -- a bridge, or a bad id anywhere -- keeps a zero right-hand side: nobody reads its column
        bool read = false;
        for (int j = 0; j < c; ++j)
            if (j != kc) read |= islands[kc < j ? cp_first_pair(kc, c) + (j - kc - 1) : cp_first_pair(j, c) + (kc - j - 1)] == 0;
        const CsLines v = cs_lines(slabs, ws_stride, s, n, m, nnz, e);
        const float* __restrict__ fac = v.fac;
        cs_substitute(W, colptr, diag, row32, fac, m, live && named && read, v.pa[lc], v.pb[lc]);
        __syncwarp();                               // (the wave's own block: written by columns, read out by rows)
        // ---- the tile into the table: 64 consecutive rows of ONE candidate per store (from LDS the 64 reads of a store share a bank:
        //      10 x 64 serialised reads per tile at the largest block that fits, against its ~10^5 dependent updates)
        float* cols = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(cols0) + (size_t)s * ws_stride);
        const int width = c - k0 < 64 ? c - k0 : 64;
        for (size_t r0 = 0; r0 < rows; r0 += 64) {
            const size_t r = r0 + lane;
            if (r < rows)
                for (int kk = 0; kk < width; ++kk) cols[(size_t)(k0 + kk) * rows + r] = block[r * 64 + kk];
        }
        __syncwarp();                               // (the next item overwrites the block)
    }
}

// -------------------------------------------------------------------------------------------------------- pairs
struct CpsArgs {
    const unsigned char* slabs;                     // the scenarios' slabs as the base launch left them
    const float* cols0;                             // scenario 0's column table; the others a stride further each
    const int32_t* status;                          // [S], the base launch's
    const int32_t* lines;                           // [c] candidates
    const int32_t* islands;                         // [P]
    float* severity;                                // [S, P]
    int32_t* worst_line;                            // [S, P]
    int32_t* overloads;                             // [S, P]
    float* post_flow;                               // [S, P, e] or null
    size_t ws_stride;
    int64_t P;
    int n, e, m, nnz, c;
};

template <bool LDS>
__global__ __launch_bounds__(1024) void contingency_pairs_sparse_kernel(const CpsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cps_smem[];
    const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6, nw = nt >> 6;
    const int e = a.e, c = a.c, m = a.m;
    const size_t rows = (size_t)m + 1;
    const int s = blockIdx.x / (c - 1), i = blockIdx.x - s * (c - 1);
    const CsLines v = cs_lines(a.slabs, a.ws_stride, s, a.n, m, a.nnz, e);
    const float* f32 = v.f32;
    const float* x32 = v.x32;
    const float* rat = v.rat;
    const int32_t* pa = v.pa;
    const int32_t* pb = v.pb;
    const float* cols = reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(a.cols0) + (size_t)s * a.ws_stride);
    const int failed = a.status[s] < 0;             // (uniform: the base launch's word)
    const int la_id = a.lines[i];
    const bool a_ok = (unsigned)la_id < (unsigned)e;   // (a candidate that is no line: its pairs carry islands -4 and are never computed)
    const float* wa = cols + (size_t)i * rows;      // w_a in plan order, zero at row m (the slack)
    if constexpr (LDS) {
        float* wl = reinterpret_cast<float*>(cps_smem);
        if (!failed && a_ok)
            for (size_t r = t; r < rows; r += nt) wl[r] = wa[r];
        __syncthreads();                            // (failed and a_ok are uniform over the workgroup)
        wa = wl;
    }

    const int64_t p0 = cp_first_pair(i, c);
    for (int j = i + 1 + wave; j < c; j += nw) {
        const int64_t p = p0 + (j - i - 1);
        const int64_t o = (int64_t)s * a.P + p;
        float* row = a.post_flow ? a.post_flow + o * e : nullptr;
        const int lb_id = a.lines[j];
        if (failed || !a_ok || (unsigned)lb_id >= (unsigned)e || a.islands[p] != 0) {   // a failed scenario, an islanding pair
            ct_skip(failed, row, e, lane, 64, a.severity[o], a.worst_line[o], a.overloads[o]);
            continue;
        }
        // ---- w_b: the wave's own vector, or the table's column where it lies
        const float* wb = cols + (size_t)j * rows;
        if constexpr (LDS) {
            float* wl = reinterpret_cast<float*>(cps_smem) + rows * (size_t)(1 + wave);
            for (size_t r = lane; r < rows; r += 64) wl[r] = wb[r];
            __syncwarp();                           // (the wave's own LDS vector: written by its lanes, gathered by its lanes)
            wb = wl;
        }
        const int aa = pa[la_id], ab = pb[la_id], ba = pa[lb_id], bb = pb[lb_id];
        const float xa = x32[la_id], xb = x32[lb_id];
        float ta, tb;
        ct_pair_solve(ct_pair_phi(wa[aa], wa[ab], xa), ct_pair_phi(wb[aa], wb[ab], xa), ct_pair_phi(wa[ba], wa[bb], xb),
                      ct_pair_phi(wb[ba], wb[bb], xb), f32[la_id], f32[lb_id], &ta, &tb);
        // ---- the lines: post-pair flow, loading; the wave's worst (contingency_monitor.hpp)
        CtWorst worst = ct_worst_none();
        for (int l = lane; l < e; l += 64) {
            const bool out = l == la_id || l == lb_id;
            const int fa = pa[l], fb = pb[l];
            const float x = x32[l];
            const float post = out ? 0.f : ct_pair_post(ct_pair_phi(wa[fa], wa[fb], x), ct_pair_phi(wb[fa], wb[fb], x), f32[l], ta, tb);
            if (row) row[l] = post;
            const float r = rat[l];
            if (!out && r > 0.f) ct_worst_add(worst, l, ct_loading(post, r));
        }
        worst = ct_worst_wave(worst);
        if (lane == 0) ct_store(ct_figures(worst), a.severity[o], a.worst_line[o], a.overloads[o]);
        if constexpr (LDS) __syncwarp();            // (the next pair overwrites the vector)
    }
}

// the sizes of a call beyond what cs_check_call asks: the candidates, the grid of the pair launch, the two new options
static bool cps_sizes_ok(int64_t S, int64_t e, int64_t c) { return c >= 0 && c <= e && (c < 2 || S * (c - 1) < (1ll << 31)); }

}  // namespace pfn

using namespace pfn;

extern "C" {

size_t pfn_contingency_pairs_sparse_workspace_bytes(int64_t n_samples, int64_t n_lines, int64_t n_candidates, const void* plan_header,
                                                    int block_route, int groups, int column_route, int waves) {
    const char* who = "pfn_contingency_pairs_sparse_workspace_bytes";
    const int32_t* h = static_cast<const int32_t*>(plan_header);
    if (n_samples <= 0 || n_samples >= (1ll << 29) || cs_check_header(h, who) != PFN_OK) return 0;
    if (n_lines < 1 || n_lines != h[PFP_H_E] || block_route < 0 || block_route > 2 || groups < 0) return 0;
    if (!cps_sizes_ok(n_samples, n_lines, n_candidates) || column_route < 0 || column_route > 2 || !cps_waves_ok(waves)) return 0;
    const int n = h[PFP_H_N], m = h[PFP_H_M], nnz = h[PFP_H_NNZ], e = (int)n_lines, c = (int)n_candidates;
    if (pf_lds_bytes(m) > (size_t)(kLdsCuBytes - kLdsReserve)) return 0;
    if (block_route == 1 && !cs_block_fits_lds(m)) return 0;
    if (column_route == 1 && !cps_fits_lds(m, waves ? waves : CPS_WAVES)) return 0;
    const bool lds = block_route == 1 || (block_route == 0 && cs_block_fits_lds(m));
    return (size_t)n_samples * (cs_sample_bytes(n, m, nnz, e) + cs_cols_bytes(c, m)) +
           (lds ? 0 : (size_t)cs_groups(n_samples, c, groups) * cs_block_bytes(m));
}

int pfn_contingency_pairs_sparse(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                                 const double* ratings, int ratings_per_sample, const int32_t* lines, int64_t n_candidates,
                                 const int32_t* islands, int64_t n_samples, int64_t n_bus, int64_t n_pv, int64_t n_pq, double tol,
                                 int max_iter, float* severity, int32_t* worst_line, int32_t* overloads, double* base_flow,
                                 int32_t* status, float* post_flow, int32_t* flags, void* ws, size_t ws_bytes, const void* plan_header,
                                 const void* plan_dev, int threads, int block_route, int groups, int column_route, int waves,
                                 void* stream) {
    const char* who = "pfn_contingency_pairs_sparse";
    const int32_t* h = static_cast<const int32_t*>(plan_header);
    PfProblem p;
    size_t lds1;
    PFN_TRY(cs_check_call(who, CsCall{edge_index, n_lines, rx, bus_type, spec, n_samples, n_bus, n_pv, n_pq, tol, max_iter, base_flow, status, flags, ws,
                                      plan_header, plan_dev, threads, block_route, groups}, &p, &lds1));
    PFN_CHECK_ARG(cps_sizes_ok(n_samples, n_lines, n_candidates), "%s: bad sizes (%lld scenarios, %lld candidates among %lld lines)", who,
                  (long long)n_samples, (long long)n_candidates, (long long)n_lines);
    PFN_CHECK_ARG(column_route >= 0 && column_route <= 2, "%s: column_route must be 0 (auto), 1 (LDS) or 2 (global)", who);
    PFN_CHECK_ARG(cps_waves_ok(waves), "%s: waves must be 0 (the default), 1, 2, 4, 8 or 16", who);
    const int n = h[PFP_H_N], m = h[PFP_H_M], nnz = h[PFP_H_NNZ], e = (int)n_lines, c = (int)n_candidates;
    const int nw = waves ? waves : CPS_WAVES;
    const bool col_fits = cps_fits_lds(m, nw);
    PFN_CHECK_ARG(column_route != 1 || col_fits, "%s: column_route 1 (LDS): %d columns of %d unknowns need %zu bytes of LDS, %d are there", who, 1 + nw, m,
                  cps_lds_bytes(m, nw), kLdsCuBytes - kLdsReserve);
    if (n_samples == 0 || n_lines == 0) return PFN_OK;
    PFN_CHECK_ARG(base_flow && (c < 2 || (lines && islands && severity && worst_line && overloads)), "%s: null pointer", who);
    PFN_CHECK_ARG((reinterpret_cast<uintptr_t>(ratings) & 7) == 0 &&
                      ((reinterpret_cast<uintptr_t>(lines) | reinterpret_cast<uintptr_t>(islands) | reinterpret_cast<uintptr_t>(severity) |
                        reinterpret_cast<uintptr_t>(worst_line) | reinterpret_cast<uintptr_t>(overloads) | reinterpret_cast<uintptr_t>(post_flow)) & 3) == 0,
                  "%s: ratings must be 8-byte aligned, fp32 and int32 arrays 4-byte", who);
    const bool blk_lds = block_route == 1 || (block_route == 0 && cs_block_fits_lds(m));
    const bool col_lds = column_route == 1 || (column_route == 0 && col_fits);
    const size_t slab = cs_sample_bytes(n, m, nnz, e), stride = slab + cs_cols_bytes(c, m), slabs = (size_t)n_samples * stride;
    const int64_t G = cs_groups(n_samples, c, groups);
    PFN_TRY(pf_check_workspace(who, ws, ws_bytes, slabs + (blk_lds ? 0 : (size_t)G * cs_block_bytes(m))));
    // (the base launch knows nothing of pairs: islands and the three outputs are the pair launch's)
    const CsArgs a{p, static_cast<const int32_t*>(plan_dev), ratings, nullptr, nullptr, nullptr, nullptr, base_flow, nullptr, nullptr, stride, m, nnz,
                   (int)n_pv, ratings_per_sample != 0, pf_f_in_lds(m)};
    hipStream_t s = static_cast<hipStream_t>(stream);
    PFN_TRY(cs_launch_base(a, h, threads, n_samples, lds1, s));
    if (c < 2) return PFN_OK;
    unsigned char* ws_b = static_cast<unsigned char*>(ws);
    float* cols0 = reinterpret_cast<float*>(ws_b + slab);
    const double ss = (double)n_samples, ee = (double)e, nz = (double)nnz, cc = (double)c, mm = (double)m, pp = 0.5 * cc * (cc - 1.0);
    {
        const double tl = (double)cs_tiles(c);
        ProfScope ps("contingency_pairs_sparse_columns", ss * (tl * nz * 6.0 + cc * (mm + 1.0) * 4.0), ss * tl * 64.0 * 2.0 * nz, s);
        const unsigned char* plan_b = static_cast<const unsigned char*>(plan_dev);
        float* blocks = blk_lds ? nullptr : reinterpret_cast<float*>(ws_b + slabs);
        PFN_TRY((launch_either<contingency_pairs_sparse_columns_kernel<true>, contingency_pairs_sparse_columns_kernel<false>>(
            blk_lds, (int)G, 64, cs_block_bytes(m), 0, s, plan_b, ws_b, cols0, blocks, status, lines, islands, stride, n, e, m, nnz, c, (int)n_samples)));
    }
    {
        const int64_t P = (int64_t)c * (c - 1) / 2;
        const CpsArgs b{ws_b, cols0, status, lines, islands, severity, worst_line, overloads, post_flow, stride, P, n, e, m, nnz, c};
        ProfScope ps("contingency_pairs_sparse", ss * pp * (8.0 * mm + 20.0 * ee + 12.0 + (post_flow ? 4.0 * ee : 0.0)), ss * pp * 12.0 * ee, s);
        PFN_TRY((launch_either<contingency_pairs_sparse_kernel<true>, contingency_pairs_sparse_kernel<false>>(col_lds, (int)(n_samples * (c - 1)), 64 * nw,
                                                                                                              cps_lds_bytes(m, nw), 0, s, b)));
    }
    return PFN_OK;
}

}  // extern "C"
