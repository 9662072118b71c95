// Per-sample topology perturbation on the device (gfx950): pfn_topology_perturb draws, for every sample, the line list that the
// reference's perturb_topology (utils/data_utils.py:12-59) draws on the host -- remove r random lines, start over while a bus is
// left unsupplied, add a lines between random bus pairs as copies of random existing lines -- in ONE launch, one workgroup per
// sample, like the solver it feeds (powerflow.hip).  pfn_topology_unsupplied is the reference's `unsupplied_buses` count for given
// line lists, from the same reach routine.
//
// THE DRAWING RULE is part of the interface (include/pfn_hip.h states it; tests/topology_ref.py is its numpy transcription, held
// bit for bit): Philox4x32-10 words keyed by the seed and counted by {item, attempt, sample, stream}, so a sample's draw is a pure
// function of (seed, sample number) -- not of the batch it is drawn in, the block size or the order threads run in.  No floating
// point anywhere.
//
// One sample's state lives in LDS; global memory holds inputs and outputs only, there is no atomic on it and no workgroup knows of
// another.  Layout of the dynamic region (ID = uint16_t while n_bus <= 65536, else uint32_t):
//     uint32 key[e] | uint32 removed[r] | ID from[e] | ID to[e] | uint8 keep[e] | uint8 reached[n]
// 6470rte (6470, 9005): 36,020 + 4 r + 36,020 + 9,005 + 6,470 bytes, 87.5 KB of the 159 KB a workgroup may take.
//   * key / from / to / keep are read by lane at consecutive indices: consecutive dwords (keys), two lanes per dword (16-bit ids),
//     four lanes per dword (flags) -- no bank is asked for two different dwords by one 32-lane half;
//   * reached[] is gathered by bus id: whatever conflicts the grid's numbering gives.  Lanes that name the same dword are served by
//     one broadcast, and a byte per bus puts four buses in a dword.
// Threads per workgroup: 64 up to 64 lines and buses (one wave: a barrier costs nothing to wait for), 256 up to 2048, 1024 beyond
// (6470rte: 9 lines per thread and round).  The kernel is a chain of short phases between barriers, so a sample wants one item per
// thread where it can have it, and many samples per compute unit hide each other's barriers: at 256 threads and 1.8 KB (case118) the
// 32-wave limit of a compute unit admits 8 samples at once, at 64 threads and 200 bytes (case14) 32.
#include "topology_reach.hpp"

namespace pfn {

constexpr int TP_MAX_ATTEMPTS = 1024;
enum { TP_NO_DRAW = -1, TP_BAD_LINE = -4 };        // (-4: powerflow_common.hpp's PF_BAD_LINE)

struct TpArgs {
    const int64_t* edge_index;   // [2, e] base list (perturb) / [2, e] or [S, 2, e] (unsupplied)
    int64_t* edge_index_out;     // [S, 2, e - r + a]
    int32_t* source;             // [S, e - r + a]
    int32_t* status;             // [S] (perturb) / count [S] (unsupplied)
    uint32_t k0, k1;             // Philox key: seed[31:0], seed[63:32]
    uint32_t first_sample;
    int n, e, r, a, root, max_attempts, lines_per_sample;
};

// dynamic LDS of one sample; `draw`: the keys, the removed list and the keep flags of pfn_topology_perturb on top of the reach state
__host__ __device__ inline size_t tp_lds_bytes(int n, int e, int r, bool draw) {
    const size_t id = n <= 65536 ? 2 : 4;
    return (draw ? (size_t)4 * e + (size_t)4 * r : 0) + tp_align4(2 * id * (size_t)e) + (draw ? tp_align4((size_t)e) : 0) + tp_align4((size_t)n);
}
// (tp_align4, tp_threads, tp_bad_lines and the reach routine tp_unreached: topology_reach.hpp, with contingency.hip)

// min over the workgroup of one 64-bit word per thread (exact, order-free).  `red`: two rows of 16 words, used in turn, so that one
// barrier per call is enough: a row is rewritten two calls later, behind the barrier of the call in between.  Every thread calls it.
__device__ __forceinline__ uint64_t tp_block_min(uint64_t v, uint64_t (*red)[16], int turn) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    const int nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) red[turn & 1][threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t m = red[turn & 1][0];
    for (int w = 1; w < nw; ++w) m = red[turn & 1][w] < m ? red[turn & 1][w] : m;
    return m;
}

template <typename ID>
__global__ __launch_bounds__(1024) void topology_perturb_kernel(const TpArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tp_smem[];
    __shared__ uint64_t s_red[2][16];
    __shared__ int s_count;
    const int t = threadIdx.x, nt = blockDim.x;
    const int s = blockIdx.x;
    const int n = a.n, e = a.e, r = a.r, kept = e - a.r, eo = kept + a.a;
    uint32_t* key = reinterpret_cast<uint32_t*>(tp_smem);
    uint32_t* removed = key + e;
    ID* from = reinterpret_cast<ID*>(removed + r);
    ID* to = from + e;
    uint8_t* keep = tp_smem + (size_t)4 * e + (size_t)4 * r + tp_align4(2 * sizeof(ID) * (size_t)e);
    uint8_t* reached = keep + tp_align4((size_t)e);
    const uint32_t sample = a.first_sample + (uint32_t)s;
    int64_t* out = a.edge_index_out + (int64_t)s * 2 * eo;
    int32_t* src = a.source + (int64_t)s * eo;

    int code = tp_bad_lines(a.edge_index, e, n) ? TP_BAD_LINE : TP_NO_DRAW;
    if (code != TP_BAD_LINE) {
        for (int j = t; j < e; j += nt) {
            from[j] = (ID)a.edge_index[j];
            to[j] = (ID)a.edge_index[e + j];
        }
        int turn = 0;
        // (every condition of this loop is uniform over the workgroup: `code` comes from barrier-combined values only)
        for (int attempt = 0; attempt < a.max_attempts && code == TP_NO_DRAW; ++attempt) {
            // a thread owns the lines t, t + nt, ...: it alone reads and writes their keys and keep flags until the barrier in front
            // of the reach pass (the staging loop above has the same ownership: no barrier is needed in between)
            for (int j = t; j < e; j += nt) {
                uint32_t c[4] = {(uint32_t)j, (uint32_t)attempt, sample, 0u};
                philox4x32_10(c, a.k0, a.k1);
                key[j] = c[0];
                keep[j] = 1;
            }
            // the r smallest (key, line): r times the minimum of what is left
            for (int k = 0; k < r; ++k) {
                uint64_t v = ~0ull;
                for (int j = t; j < e; j += nt) {
                    const uint64_t w = ((uint64_t)key[j] << 32) | (uint32_t)j;
                    v = keep[j] && w < v ? w : v;
                }
                const int j = (int)(uint32_t)tp_block_min(v, s_red, turn++);
                if (j % nt == t) {
                    keep[j] = 0;
                    removed[k] = (uint32_t)j;
                }
            }
            if (tp_unreached<ID>(from, to, keep, e, n, a.root, reached, &s_count) == 0) code = attempt + 1;
        }
    }

    if (code >= 1) {
        // stable compaction: a kept line moves up by the number of removed lines in front of it
        for (int j = t; j < e; j += nt) {
            if (!keep[j]) continue;
            int p = j;
            for (int k = 0; k < r; ++k) p -= removed[k] < (uint32_t)j;
            out[p] = from[j];
            out[eo + p] = to[j];
            src[p] = j;
        }
        for (int k = t; k < a.a; k += nt) {
            uint32_t c[4] = {(uint32_t)k, 0u, sample, 1u};
            philox4x32_10(c, a.k0, a.k1);
            const uint32_t f = c[0] % (uint32_t)n;
            const uint32_t g = (f + 1u + c[1] % (uint32_t)(n - 1)) % (uint32_t)n;     // (a > 0 only with n >= 2: the host refuses it)
            out[kept + k] = f;
            out[eo + kept + k] = g;
            src[kept + k] = (int32_t)(c[2] % (uint32_t)e);
        }
    } else {
        for (int p = t; p < eo; p += nt) {
            out[p] = -1;
            out[eo + p] = -1;
            src[p] = -1;
        }
    }
    if (t == 0) a.status[s] = code;
}

template <typename ID>
__global__ __launch_bounds__(1024) void topology_unsupplied_kernel(const TpArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tp_smem[];
    __shared__ int s_count;
    const int t = threadIdx.x, nt = blockDim.x;
    const int s = blockIdx.x;
    const int n = a.n, e = a.e;
    ID* from = reinterpret_cast<ID*>(tp_smem);
    ID* to = from + e;
    uint8_t* reached = tp_smem + tp_align4(2 * sizeof(ID) * (size_t)e);
    const int64_t* ei = a.edge_index + (a.lines_per_sample ? (int64_t)s * 2 * e : 0);
    int count = TP_BAD_LINE;
    if (!tp_bad_lines(ei, e, n)) {
        for (int j = t; j < e; j += nt) {
            from[j] = (ID)ei[j];
            to[j] = (ID)ei[e + j];
        }
        count = tp_unreached<ID>(from, to, nullptr, e, n, a.root, reached, &s_count);
    }
    if (t == 0) a.status[s] = count;
}

template <typename K>
static int tp_launch(K kernel, const TpArgs& a, int64_t n_samples, size_t bytes, std::atomic<uint64_t>& raised, hipStream_t s) {
    PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), kLdsCuBytes - kLdsReserve, raised));
    kernel<<<(int)n_samples, tp_threads(a.n, a.e), bytes, s>>>(a);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

}  // namespace pfn

using namespace pfn;

extern "C" {

int pfn_topology_perturb(const int64_t* edge_index, int64_t n_lines, int64_t n_bus, int64_t n_samples, int64_t first_sample,
                         int64_t n_remove, int64_t n_add, uint64_t seed, int64_t root, int max_attempts, int64_t* edge_index_out,
                         int32_t* source, int32_t* status, void* stream) {
    PFN_CHECK_ARG(n_samples >= 0 && n_bus >= 1 && n_lines >= 0 && n_samples < (1ll << 29) && n_lines < (1ll << 24) && n_bus < (1ll << 24),
                  "pfn_topology_perturb: bad sizes (%lld samples of %lld buses and %lld lines)", (long long)n_samples, (long long)n_bus,
                  (long long)n_lines);
    PFN_CHECK_ARG(n_remove >= 0 && n_add >= 0 && n_remove <= n_lines && n_add < (1ll << 24),
                  "pfn_topology_perturb: cannot remove %lld and add %lld lines of %lld", (long long)n_remove, (long long)n_add,
                  (long long)n_lines);
    PFN_CHECK_ARG(n_lines - n_remove >= n_bus - 1, "pfn_topology_perturb: %lld lines less %lld cannot connect %lld buses",
                  (long long)n_lines, (long long)n_remove, (long long)n_bus);
    PFN_CHECK_ARG(n_add == 0 || n_bus >= 2, "pfn_topology_perturb: a line cannot be added to a grid of %lld bus", (long long)n_bus);
    PFN_CHECK_ARG(root >= 0 && root < n_bus, "pfn_topology_perturb: root %lld is outside [0, %lld)", (long long)root, (long long)n_bus);
    PFN_CHECK_ARG(max_attempts >= 1 && max_attempts <= TP_MAX_ATTEMPTS, "pfn_topology_perturb: max_attempts %d is outside [1, %d]",
                  max_attempts, TP_MAX_ATTEMPTS);
    PFN_CHECK_ARG(first_sample >= 0 && first_sample + n_samples <= (1ll << 32),
                  "pfn_topology_perturb: sample numbers %lld + [0, %lld) do not fit the 32-bit counter word", (long long)first_sample,
                  (long long)n_samples);
    const int n = (int)n_bus, e = (int)n_lines, r = (int)n_remove;
    const size_t bytes = tp_lds_bytes(n, e, r, true);
    PFN_CHECK_ARG(bytes <= (size_t)(kLdsCuBytes - kLdsReserve),
                  "pfn_topology_perturb: %d buses and %d lines less %d need %zu bytes of LDS, %d are there", n, e, r, bytes,
                  kLdsCuBytes - kLdsReserve);
    if (n_samples == 0) return PFN_OK;
    PFN_CHECK_ARG(edge_index || n_lines == 0, "pfn_topology_perturb: null edge_index");
    PFN_CHECK_ARG((edge_index_out && source) || n_lines - n_remove + n_add == 0, "pfn_topology_perturb: null output");
    PFN_CHECK_ARG(status, "pfn_topology_perturb: null status");
    PFN_CHECK_ARG(((reinterpret_cast<uintptr_t>(edge_index) | reinterpret_cast<uintptr_t>(edge_index_out)) & 7) == 0 &&
                      ((reinterpret_cast<uintptr_t>(source) | reinterpret_cast<uintptr_t>(status)) & 3) == 0,
                  "pfn_topology_perturb: int64 arrays must be 8-byte aligned, int32 arrays 4-byte");
    TpArgs a;
    a.edge_index = edge_index;
    a.edge_index_out = edge_index_out;
    a.source = source;
    a.status = status;
    a.k0 = (uint32_t)seed;
    a.k1 = (uint32_t)(seed >> 32);
    a.first_sample = (uint32_t)first_sample;
    a.n = n;
    a.e = e;
    a.r = r;
    a.a = (int)n_add;
    a.root = (int)root;
    a.max_attempts = max_attempts;
    a.lines_per_sample = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double eo = (double)(n_lines - n_remove + n_add);
    ProfScope ps("topology_perturb", (double)n_samples * (16.0 * (double)n_lines + 20.0 * eo + 4.0), 0.0, s);
    static std::atomic<uint64_t> raised16{0}, raised32{0};
    if (n <= 65536) return tp_launch(topology_perturb_kernel<uint16_t>, a, n_samples, bytes, raised16, s);
    return tp_launch(topology_perturb_kernel<uint32_t>, a, n_samples, bytes, raised32, s);
}

int pfn_topology_unsupplied(const int64_t* edge_index, int lines_per_sample, int64_t n_lines, int64_t n_samples, int64_t n_bus,
                            int64_t root, int32_t* count, void* stream) {
    PFN_CHECK_ARG(n_samples >= 0 && n_bus >= 1 && n_lines >= 0 && n_samples < (1ll << 29) && n_lines < (1ll << 24) && n_bus < (1ll << 24),
                  "pfn_topology_unsupplied: bad sizes (%lld samples of %lld buses and %lld lines)", (long long)n_samples,
                  (long long)n_bus, (long long)n_lines);
    PFN_CHECK_ARG(root >= 0 && root < n_bus, "pfn_topology_unsupplied: root %lld is outside [0, %lld)", (long long)root, (long long)n_bus);
    const int n = (int)n_bus, e = (int)n_lines;
    const size_t bytes = tp_lds_bytes(n, e, 0, false);
    PFN_CHECK_ARG(bytes <= (size_t)(kLdsCuBytes - kLdsReserve), "pfn_topology_unsupplied: %d buses and %d lines need %zu bytes of LDS, %d are there",
                  n, e, bytes, kLdsCuBytes - kLdsReserve);
    if (n_samples == 0) return PFN_OK;
    PFN_CHECK_ARG(edge_index || n_lines == 0, "pfn_topology_unsupplied: null edge_index");
    PFN_CHECK_ARG(count, "pfn_topology_unsupplied: null count");
    PFN_CHECK_ARG((reinterpret_cast<uintptr_t>(edge_index) & 7) == 0 && (reinterpret_cast<uintptr_t>(count) & 3) == 0,
                  "pfn_topology_unsupplied: edge_index must be 8-byte aligned, count 4-byte");
    TpArgs a = {};
    a.edge_index = edge_index;
    a.status = count;
    a.n = n;
    a.e = e;
    a.root = (int)root;
    a.lines_per_sample = lines_per_sample != 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope ps("topology_unsupplied", (double)(lines_per_sample ? n_samples : 1) * 16.0 * (double)n_lines + 4.0 * (double)n_samples, 0.0, s);
    static std::atomic<uint64_t> raised16{0}, raised32{0};
    if (n <= 65536) return tp_launch(topology_unsupplied_kernel<uint16_t>, a, n_samples, bytes, raised16, s);
    return tp_launch(topology_unsupplied_kernel<uint32_t>, a, n_samples, bytes, raised32, s);
}

}  // extern "C"
