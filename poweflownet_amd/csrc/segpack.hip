// Segment packing of mixed-size graph batches (gfx950): the device side of poweflownet_amd/segpack.py.
//
// A ragged batch (graph g owns the caller's rows ptr[g] .. ptr[g + 1]) is re-laid into n_seg segments of S rows: graph g starts at
// padded row start[g], the graphs of a segment are contiguous, the segment's last S - fill[seg] rows are isolated padding.  No edge
// then crosses a multiple of S (pfn_graph_segments), so the unchanged graph-resident kernels run on the padded layout with
// seg_nodes = S; the caller only ever sees ragged tensors.  Three entry points, all row movers of 16- and 32-byte rows -- latency,
// not bandwidth: plain C++, one 16-byte access per lane, consecutive lanes on consecutive rows.
//   segpack_rows_kernel   every real row finds its graph (binary search over ptr, G + 1 ints that stay in cache) and with it its
//                         padded row: writes row_of / src_of and the x / mask rows; every padding row is zeroed by the thread that
//                         owns it -- the same launch, disjoint rows, no memset and nothing to wait for across workgroups
//   segpack_edges_kernel  edge endpoints relabelled through row_of, edge order kept (edge_attr, its gradient and the edge-id
//                         summation order stay what they were); an id outside [0, N) becomes -1, which pfn_graph_build flags
//   segpack_gather_rows_kernel / segpack_scatter_rows_kernel   dst[i] = src_pad[row_of[i]] and its adjoint, written as a gather
//                         through src_of so that every padded row -- padding as zeros -- is written exactly once, by one launch
#include <algorithm>

#include "pfn_internal.hpp"

namespace pfn {

struct SegPackArgs {
    const int* ptr;          // [G + 1]
    const int* start;        // [G]
    const int* fill;         // [n_pad / S]
    int G, n, S, n_pad;
    const float* x;          // [n][4]
    const void* mask;        // [n][4] int64 or f32
    int mask_dtype;
    float* x_pad;            // [n_pad][4]
    float* mask_pad;         // [n_pad][4]
    int* row_of;             // [n]
    int* src_of;             // [n_pad]
};

__global__ __launch_bounds__(256) void segpack_rows_kernel(SegPackArgs a) {
    const int items = a.n > a.n_pad ? a.n : a.n_pad;
    for (int64_t t64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t64 < items; t64 += (int64_t)gridDim.x * blockDim.x) {
        const int t = (int)t64;
        if (t < a.n) {
            int lo = 0, hi = a.G;                  // the last g with ptr[g] <= t (graphs without rows are stepped over)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (a.ptr[mid] <= t) lo = mid; else hi = mid;
            }
            const int r = a.start[lo] + (t - a.ptr[lo]);
            const bool ok = r >= 0 && r < a.n_pad;   // (a plan that disagrees with n_pad writes nothing out of bounds: the row's
            a.row_of[t] = ok ? r : -1;               //  edges then carry the id -1 and the adjacency build reports them)
            if (ok) {
                a.src_of[r] = t;
                st4(a.x_pad + (size_t)r * 4, ld4(a.x + (size_t)t * 4));
                st4(a.mask_pad + (size_t)r * 4, mask_row4(a.mask, a.mask_dtype, t));
            }
        }
        if (t < a.n_pad) {
            const int seg = t / a.S;
            if (t - seg * a.S >= a.fill[seg]) {
                const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
                a.src_of[t] = -1;
                st4(a.x_pad + (size_t)t * 4, z);
                st4(a.mask_pad + (size_t)t * 4, z);
            }
        }
    }
}

// two consecutive entries of the flat [2][E] list per lane (2 E is even; 16 bytes in, 16 bytes out)
__global__ __launch_bounds__(256) void segpack_edges_kernel(const longlong2* __restrict__ ei, int64_t pairs, int n,
                                                            const int* __restrict__ row_of, longlong2* __restrict__ out) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < pairs; k += (int64_t)gridDim.x * blockDim.x) {
        const longlong2 v = ei[k];
        longlong2 r;
        r.x = (v.x >= 0 && v.x < n) ? row_of[v.x] : -1;
        r.y = (v.y >= 0 && v.y < n) ? row_of[v.y] : -1;
        out[k] = r;
    }
}

// dst[i][:f] = src[map[i]][:f] for i < rows; a map entry outside [0, src_rows) gives a zero row.  One item = one row x one
// four-column chunk: a 16-byte access where the strides and pointers allow it (`vec`), element by element otherwise.
__global__ __launch_bounds__(256) void segpack_move_rows_kernel(const float* __restrict__ src, int64_t ld_src, int64_t src_rows,
                                                                const int* __restrict__ map, float* __restrict__ dst, int64_t ld_dst,
                                                                int64_t rows, int f, int vec) {
    const int ncg = (f + 3) >> 2;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < rows * ncg; it += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = it / ncg;
        const int c = (int)(it - i * ncg) * 4;
        const int64_t j = map[i];
        const bool in = j >= 0 && j < src_rows;
        if (vec && c + 4 <= f) {
            st4(dst + i * ld_dst + c, in ? ld4(src + j * ld_src + c) : make_float4(0.f, 0.f, 0.f, 0.f));
        } else {
            for (int e = c; e < f && e < c + 4; ++e) dst[i * ld_dst + e] = in ? src[j * ld_src + e] : 0.f;
        }
    }
}

static int move_rows(const char* what, const float* src, int64_t ld_src, int64_t src_rows, const int* map, float* dst, int64_t ld_dst,
                     int64_t rows, int64_t f, hipStream_t s) {
    if (rows == 0) return PFN_OK;
    const int vec = ((ld_src | ld_dst) & 3) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    const int64_t items = rows * ((f + 3) / 4);
    ProfScope ps(what, (double)rows * f * 8.0 + rows * 4.0, 0.0, s);
    segpack_move_rows_kernel<<<(int)std::min<int64_t>((items + 255) / 256, 8192), 256, 0, s>>>(src, ld_src, src_rows, map, dst, ld_dst,
                                                                                             rows, (int)f, vec);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

}  // namespace pfn

using namespace pfn;

extern "C" {

int pfn_segpack_pack(const int32_t* ptr, const int32_t* start, const int32_t* fill, int64_t n_graphs, int64_t n_nodes,
                     int64_t seg_nodes, int64_t n_pad, const float* x, const void* pred_mask, int mask_dtype, const int64_t* edge_index,
                     int64_t e_stored, float* x_pad, float* mask_pad, int64_t* edge_index_pad, int32_t* row_of, int32_t* src_of,
                     void* stream) {
    PFN_CHECK_ARG(ptr && start && fill && x && pred_mask && x_pad && mask_pad && row_of && src_of &&
                      (e_stored == 0 || (edge_index && edge_index_pad)), "pfn_segpack_pack: null pointer");
    PFN_CHECK_ARG(mask_dtype == 0 || mask_dtype == 1, "pfn_segpack_pack: mask_dtype must be 0 (int64) or 1 (float32)");
    PFN_CHECK_ARG(n_graphs >= 1 && n_graphs < (1ll << 30) && n_nodes >= 1 && n_nodes < (1ll << 31) && e_stored >= 0,
                  "pfn_segpack_pack: bad sizes (graphs %lld, nodes %lld, edges %lld)", (long long)n_graphs, (long long)n_nodes,
                  (long long)e_stored);
    PFN_CHECK_ARG(seg_nodes >= 1 && n_pad >= n_nodes && n_pad < (1ll << 31) && n_pad % seg_nodes == 0,
                  "pfn_segpack_pack: n_pad %lld must be a multiple of seg_nodes %lld and hold the %lld real rows", (long long)n_pad,
                  (long long)seg_nodes, (long long)n_nodes);
    PFN_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(pred_mask) | reinterpret_cast<uintptr_t>(x_pad) |
                    reinterpret_cast<uintptr_t>(mask_pad) | reinterpret_cast<uintptr_t>(edge_index) |
                    reinterpret_cast<uintptr_t>(edge_index_pad)) & 15) == 0,
                  "pfn_segpack_pack: x, pred_mask, edge_index and their padded copies must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    SegPackArgs a;
    a.ptr = ptr;
    a.start = start;
    a.fill = fill;
    a.G = (int)n_graphs;
    a.n = (int)n_nodes;
    a.S = (int)seg_nodes;
    a.n_pad = (int)n_pad;
    a.x = x;
    a.mask = pred_mask;
    a.mask_dtype = mask_dtype;
    a.x_pad = x_pad;
    a.mask_pad = mask_pad;
    a.row_of = row_of;
    a.src_of = src_of;
    {
        ProfScope ps("segpack_rows", (double)n_nodes * (mask_dtype == 0 ? 56.0 : 40.0) + (double)n_pad * 36.0, 0.0, s);
        segpack_rows_kernel<<<(int)std::min<int64_t>((n_pad + 255) / 256, 4096), 256, 0, s>>>(a);
        PFN_CHECK_LAUNCH();
    }
    if (e_stored > 0) {
        ProfScope ps("segpack_edges", (double)e_stored * 40.0, 0.0, s);
        segpack_edges_kernel<<<(int)std::min<int64_t>((e_stored + 255) / 256, 4096), 256, 0, s>>>(
            reinterpret_cast<const longlong2*>(edge_index), e_stored, (int)n_nodes, row_of, reinterpret_cast<longlong2*>(edge_index_pad));
        PFN_CHECK_LAUNCH();
    }
    return PFN_OK;
}

int pfn_segpack_gather_rows(const float* src_pad, int64_t ld_src, int64_t n_pad, const int32_t* row_of, float* dst, int64_t ld_dst,
                            int64_t n_nodes, int64_t f, void* stream) {
    PFN_CHECK_ARG(n_nodes == 0 || (src_pad && row_of && dst), "pfn_segpack_gather_rows: null pointer");
    PFN_CHECK_ARG(n_nodes >= 0 && n_pad >= 0 && n_pad < (1ll << 31) && f >= 1 && f < (1ll << 20) && ld_src >= f && ld_dst >= f,
                  "pfn_segpack_gather_rows: bad sizes (rows %lld of %lld, f %lld, ld %lld -> %lld)", (long long)n_nodes, (long long)n_pad,
                  (long long)f, (long long)ld_src, (long long)ld_dst);
    return move_rows("segpack_gather", src_pad, ld_src, n_pad, row_of, dst, ld_dst, n_nodes, f, static_cast<hipStream_t>(stream));
}

int pfn_segpack_scatter_rows(const float* src, int64_t ld_src, int64_t n_nodes, const int32_t* src_of, float* dst_pad, int64_t ld_dst,
                             int64_t n_pad, int64_t seg_nodes, int64_t f, void* stream) {
    PFN_CHECK_ARG(n_pad == 0 || (src && src_of && dst_pad), "pfn_segpack_scatter_rows: null pointer");
    PFN_CHECK_ARG(n_nodes >= 0 && n_nodes < (1ll << 31) && n_pad >= 0 && f >= 1 && f < (1ll << 20) && ld_src >= f && ld_dst >= f,
                  "pfn_segpack_scatter_rows: bad sizes (rows %lld into %lld, f %lld, ld %lld -> %lld)", (long long)n_nodes,
                  (long long)n_pad, (long long)f, (long long)ld_src, (long long)ld_dst);
    PFN_CHECK_ARG(seg_nodes >= 1 && n_pad % seg_nodes == 0, "pfn_segpack_scatter_rows: n_pad %lld is not a multiple of seg_nodes %lld",
                  (long long)n_pad, (long long)seg_nodes);
    return move_rows("segpack_scatter", src, ld_src, n_nodes, src_of, dst_pad, ld_dst, n_pad, f, static_cast<hipStream_t>(stream));
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------- slot buckets
// The fused collate + pack of a mixed TRAINING batch (segpack.py "slot buckets"): the batch's samples are read straight from the
// dataset's dense per-case blocks and written at the rows / edges their SLOTS own in the bucket's static layout.  The layout is a
// constant of the bucket (row_slot / edge_slot / slot_case / slot_row0 / slot_edge0 are uploaded once); per batch only the slot
// table (sample index, validity) changes.  One item = one padded row or one edge: 16- and 32-byte rows, plain C++, nothing waits
// across workgroups, every row of every output -- padding as zeros -- is written by this one launch.
namespace pfn {

struct SlotCase {
    const float* x;            // [samples][n][4]
    const float* y;            // [samples][n][4]
    const void* mask;          // [samples][n][4] int64 or f32
    const int64_t* bus_type;   // [samples][n]
    const float* edge_attr;    // [samples][e][2]
    int n, e, samples;
};

struct SlotGatherArgs {
    SlotCase c[PFN_SLOT_MAX_CASES];
    int n_cases, n_slots, n_pad, E, mask_dtype;
    const int* slot_case;      // [n_slots]
    const int* slot_row0;      // [n_slots]
    const int* slot_edge0;     // [n_slots]
    const int* row_slot;       // [n_pad]  -1: padding row
    const int* edge_slot;      // [E]
    const int* table;          // [n_slots][2]  sample, validity
    float* x;                  // [n_pad][4]
    float* y;                  // [n_pad][4]
    void* mask_out;            // [n_pad][4] in the blocks' dtype
    int64_t* bus_type;         // [n_pad]
    float* edge_attr;          // [E][2]
    int* valid;                // [n_pad]
};

__global__ __launch_bounds__(256) void segpack_gather_slots_kernel(SlotGatherArgs a) {
    const int items = a.n_pad > a.E ? a.n_pad : a.E;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t t64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t64 < items; t64 += (int64_t)gridDim.x * blockDim.x) {
        const int t = (int)t64;
        if (t < a.n_pad) {
            const int s = a.row_slot[t];
            // a slot, a case or a sample outside its range (the host rejects them first) is written as a padding row, never followed
            bool real = s >= 0 && s < a.n_slots;
            int ci = 0, smp = 0, r = 0, ok = 0;
            if (real) {
                ci = a.slot_case[s];
                smp = a.table[2 * s];
                ok = a.table[2 * s + 1];
                r = t - a.slot_row0[s];
                real = ci >= 0 && ci < a.n_cases;
            }
            // (the struct array is indexed by a run-time value: select the fields through a short loop over the cases, so the
            //  kernel arguments stay in scalar registers instead of moving to scratch)
            const float *px = nullptr, *py = nullptr;
            const void* pm = nullptr;
            const int64_t* pb = nullptr;
            int n = 0, samples = 0;
#pragma unroll
            for (int k = 0; k < PFN_SLOT_MAX_CASES; ++k)
                if (real && k == ci) { px = a.c[k].x; py = a.c[k].y; pm = a.c[k].mask; pb = a.c[k].bus_type; n = a.c[k].n; samples = a.c[k].samples; }
            real = real && smp >= 0 && smp < samples && r >= 0 && r < n;
            float4 vx = z, vy = z;
            int64_t bt = 0;
            if (real) {
                const size_t src = (size_t)smp * n + r;
                vx = ld4(px + src * 4);
                vy = ld4(py + src * 4);
                bt = pb[src];
                if (a.mask_dtype == 0) {
                    const longlong2* mp = static_cast<const longlong2*>(pm) + src * 2;
                    longlong2* mo = static_cast<longlong2*>(a.mask_out) + (size_t)t * 2;
                    mo[0] = mp[0];
                    mo[1] = mp[1];
                } else {
                    st4(static_cast<float*>(a.mask_out) + (size_t)t * 4, ld4(static_cast<const float*>(pm) + src * 4));
                }
            } else if (a.mask_dtype == 0) {
                longlong2 zz;
                zz.x = 0;
                zz.y = 0;
                longlong2* mo = static_cast<longlong2*>(a.mask_out) + (size_t)t * 2;
                mo[0] = zz;
                mo[1] = zz;
            } else {
                st4(static_cast<float*>(a.mask_out) + (size_t)t * 4, z);
            }
            st4(a.x + (size_t)t * 4, vx);
            st4(a.y + (size_t)t * 4, vy);
            a.bus_type[t] = bt;
            a.valid[t] = real && ok != 0 ? 1 : 0;
        }
        if (t < a.E) {
            const int s = a.edge_slot[t];
            bool real = s >= 0 && s < a.n_slots;
            int ci = 0, smp = 0, q = 0;
            if (real) {
                ci = a.slot_case[s];
                smp = a.table[2 * s];
                q = t - a.slot_edge0[s];
                real = ci >= 0 && ci < a.n_cases;
            }
            const float* pe = nullptr;
            int e = 0, samples = 0;
#pragma unroll
            for (int k = 0; k < PFN_SLOT_MAX_CASES; ++k)
                if (real && k == ci) { pe = a.c[k].edge_attr; e = a.c[k].e; samples = a.c[k].samples; }
            real = real && smp >= 0 && smp < samples && q >= 0 && q < e;
            float2 v = make_float2(0.f, 0.f);
            if (real) v = *reinterpret_cast<const float2*>(pe + ((size_t)smp * e + q) * 2);
            *reinterpret_cast<float2*>(a.edge_attr + (size_t)t * 2) = v;
        }
    }
}

}  // namespace pfn

extern "C" {

int pfn_segpack_gather_slots(const pfn_slot_case* cases, int32_t n_cases, int32_t mask_dtype, const int32_t* slot_case,
                             const int32_t* slot_row0, const int32_t* slot_edge0, const int32_t* row_slot, const int32_t* edge_slot,
                             const int32_t* slot_table, int64_t n_slots, int64_t n_pad, int64_t n_edges, float* x, float* y,
                             void* pred_mask, int64_t* bus_type, float* edge_attr, int32_t* valid, void* stream) {
    PFN_CHECK_ARG(cases && slot_case && slot_row0 && slot_edge0 && row_slot && slot_table && x && y && pred_mask && bus_type && valid &&
                      (n_edges == 0 || (edge_slot && edge_attr)), "pfn_segpack_gather_slots: null pointer");
    PFN_CHECK_ARG(n_cases >= 1 && n_cases <= PFN_SLOT_MAX_CASES, "pfn_segpack_gather_slots: %d cases (1 .. %d)", (int)n_cases,
                  PFN_SLOT_MAX_CASES);
    PFN_CHECK_ARG(mask_dtype == 0 || mask_dtype == 1, "pfn_segpack_gather_slots: mask_dtype must be 0 (int64) or 1 (float32)");
    PFN_CHECK_ARG(n_slots >= 1 && n_slots < (1ll << 30) && n_pad >= 1 && n_pad < (1ll << 31) && n_edges >= 0 && n_edges < (1ll << 31),
                  "pfn_segpack_gather_slots: bad sizes (slots %lld, rows %lld, edges %lld)", (long long)n_slots, (long long)n_pad,
                  (long long)n_edges);
    pfn::SlotGatherArgs a;
    uintptr_t align = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(pred_mask) |
                      reinterpret_cast<uintptr_t>(edge_attr);
    for (int k = 0; k < PFN_SLOT_MAX_CASES; ++k) {
        pfn::SlotCase& c = a.c[k];
        if (k >= n_cases) {
            c.x = c.y = c.edge_attr = nullptr;
            c.mask = nullptr;
            c.bus_type = nullptr;
            c.n = c.e = c.samples = 0;
            continue;
        }
        const pfn_slot_case& h = cases[k];
        PFN_CHECK_ARG(h.n_nodes >= 1 && h.n_nodes < (1ll << 31) && h.n_edges >= 0 && h.n_edges < (1ll << 31) && h.n_samples >= 0 &&
                          h.n_samples < (1ll << 31),
                      "pfn_segpack_gather_slots: case %d: bad sizes (nodes %lld, edges %lld, samples %lld)", k, (long long)h.n_nodes,
                      (long long)h.n_edges, (long long)h.n_samples);
        PFN_CHECK_ARG(h.n_samples == 0 || (h.x && h.y && h.pred_mask && h.bus_type && (h.n_edges == 0 || h.edge_attr)),
                      "pfn_segpack_gather_slots: case %d: null pointer", k);
        c.x = h.x;
        c.y = h.y;
        c.mask = h.pred_mask;
        c.bus_type = h.bus_type;
        c.edge_attr = h.edge_attr;
        c.n = (int)h.n_nodes;
        c.e = (int)h.n_edges;
        c.samples = (int)h.n_samples;
        align |= reinterpret_cast<uintptr_t>(h.x) | reinterpret_cast<uintptr_t>(h.y) | reinterpret_cast<uintptr_t>(h.pred_mask) |
                 reinterpret_cast<uintptr_t>(h.edge_attr);
    }
    PFN_CHECK_ARG((align & 15) == 0, "pfn_segpack_gather_slots: x, y, pred_mask, edge_attr of the blocks and of the batch must be 16-byte aligned");
    a.n_cases = n_cases;
    a.n_slots = (int)n_slots;
    a.n_pad = (int)n_pad;
    a.E = (int)n_edges;
    a.mask_dtype = mask_dtype;
    a.slot_case = slot_case;
    a.slot_row0 = slot_row0;
    a.slot_edge0 = slot_edge0;
    a.row_slot = row_slot;
    a.edge_slot = edge_slot;
    a.table = slot_table;
    a.x = x;
    a.y = y;
    a.mask_out = pred_mask;
    a.bus_type = bus_type;
    a.edge_attr = edge_attr;
    a.valid = valid;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t items = std::max(n_pad, n_edges);
    pfn::ProfScope ps("segpack_gather_slots", (double)n_pad * (mask_dtype == 0 ? 2.0 * 80.0 : 2.0 * 64.0) + (double)n_edges * 20.0, 0.0, s);
    pfn::segpack_gather_slots_kernel<<<(int)std::min<int64_t>((items + 255) / 256, 4096), 256, 0, s>>>(a);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

}  // extern "C"
