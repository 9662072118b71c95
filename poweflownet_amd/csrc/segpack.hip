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
                float4 m;
                if (a.mask_dtype == 0) {
                    const longlong2* mp = static_cast<const longlong2*>(a.mask) + (size_t)t * 2;
                    const longlong2 m0 = mp[0], m1 = mp[1];
                    m = make_float4((float)m0.x, (float)m0.y, (float)m1.x, (float)m1.y);
                } else {
                    m = ld4(static_cast<const float*>(a.mask) + (size_t)t * 4);
                }
                st4(a.mask_pad + (size_t)r * 4, m);
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
