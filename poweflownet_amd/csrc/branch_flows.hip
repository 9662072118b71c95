// Per-line branch flows and currents on the device (gfx950): do the predicted bus voltages give the right line currents and line
// flows?  pfn_branch_flows turns one or two finished bus tables [S, n, 4] (Vm, Va in degrees, P, Q) and the line list(s) of the
// split into four quantities per (sample, stored line i -> j) -- current magnitude, the P and Q message of the stored direction in
// PowerImbalance.message's convention (physics.hip), and the series loss -- into their error pred - truth, and into running moments
// per (line, quantity).  It is the table the reference's error_per_feature.py:186-223 left commented out as a Python double loop.
// Two launches: a flows kernel (a workgroup takes whole samples, the sample's bus phasors in LDS) and a moments kernel over the
// finished error table.  Pure functions of their inputs: one owner per (line, quantity), a fixed combine order, no float atomics.
#include <algorithm>

#include "branch_line.hpp"
#include "pfn_internal.hpp"
#include "reduce.hpp"

namespace pfn {

// ------------------------------------------------------------------------------------------------------ flows
// A workgroup takes the samples blockIdx.x, blockIdx.x + gridDim.x, ...  Per sample it first turns every bus row into its
// rectangular voltage (e, f) = Vm (cos, sin)(Va pi / 180) -- one sincosf per bus and table, not one per line end -- and keeps them
// in LDS, 8 bytes per bus and table; then thread k walks the lines k, k + blockDim.x, ... with both gathers served from LDS and
// writes 16-byte rows.  Where 16 n_bus bytes do not fit the LDS of a compute unit (BF_LDS_MAX_BUS) the direct kernel forms the
// phasors per line end from global memory.  Nothing here depends on the work split: every output element is a function of its
// own inputs.
// (BF_LDS_MAX_BUS: branch_line.hpp)
constexpr int BF_SMALL_THREADS = 256, BF_BIG_THREADS = 1024;
constexpr int BF_BIG_LDS = 32 * 1024;              // a sample's phasors beyond this: few workgroups per CU, so each gets 16 waves

struct BfArgs {
    const float* pred;
    const float* truth;
    const int64_t* edge_index;
    const float* edge_attr;
    float* flows_pred;
    float* flows_true;
    float* err;
    int32_t* flags;
    int n_samples, n_bus, n_lines;
    int pred_norm, truth_norm, lines_per_sample, attr_per_sample;
    float std[2], mean[2], estd[2], emean[2];      // (Vm, Va) and (r, x)
};

// (the rectangular voltage of a bus row and the four quantities of a line, bf_phasor and bf_line: branch_line.hpp, shared with the
//  network's N-1 screen, contingency_model.hip)

template <bool TWO, bool LDS>
__global__ __launch_bounds__(BF_BIG_THREADS) void branch_flows_kernel(const BfArgs a) {
    extern __shared__ __attribute__((aligned(16))) float2 bf_lds[];        // LDS: [n_bus][TWO ? 2 : 1] (e, f)
    constexpr int NT = TWO ? 2 : 1;
    const int t = threadIdx.x, nt = blockDim.x;
    const float nanv = __builtin_nanf("");
    const uint64_t nb = (uint64_t)a.n_bus;
    bool bad_seen = false;
    for (int s = blockIdx.x; s < a.n_samples; s += gridDim.x) {           // (uniform over the workgroup: the barriers are safe)
        const int64_t row0 = (int64_t)s * a.n_bus;
        if (LDS) {
            for (int b = t; b < a.n_bus; b += nt) {
                bf_lds[b * NT] = bf_phasor(a.pred, row0 + b, a.pred_norm != 0, a.std, a.mean);
                if (TWO) bf_lds[b * NT + 1] = bf_phasor(a.truth, row0 + b, a.truth_norm != 0, a.std, a.mean);
            }
            __syncthreads();
        }
        const int64_t* ei = a.edge_index + (a.lines_per_sample ? (int64_t)s * 2 * a.n_lines : 0);
        const float* ea = a.edge_attr + (a.attr_per_sample ? (int64_t)s * 2 * a.n_lines : 0);
        for (int k = t; k < a.n_lines; k += nt) {
            const int64_t i = ei[k], j = ei[a.n_lines + k];
            const float2 rx = *reinterpret_cast<const float2*>(ea + 2 * k);
            const float r = fmaf(rx.x, a.estd[0], a.emean[0]), x = fmaf(rx.y, a.estd[1], a.emean[1]);      // `admittance`, physics.hip
            float4 fp = make_float4(nanv, nanv, nanv, nanv), ft = fp;
            if ((uint64_t)i < nb && (uint64_t)j < nb) {                    // an id outside [0, n_bus) is never followed
                if (LDS) {
                    fp = bf_line(bf_lds[(int)i * NT], bf_lds[(int)j * NT], r, x);
                    if (TWO) ft = bf_line(bf_lds[(int)i * NT + 1], bf_lds[(int)j * NT + 1], r, x);
                } else {
                    fp = bf_line(bf_phasor(a.pred, row0 + i, a.pred_norm != 0, a.std, a.mean),
                                 bf_phasor(a.pred, row0 + j, a.pred_norm != 0, a.std, a.mean), r, x);
                    if (TWO)
                        ft = bf_line(bf_phasor(a.truth, row0 + i, a.truth_norm != 0, a.std, a.mean),
                                     bf_phasor(a.truth, row0 + j, a.truth_norm != 0, a.std, a.mean), r, x);
                }
            } else {
                bad_seen = true;
            }
            const int64_t o = 4 * ((int64_t)s * a.n_lines + k);
            if (a.flows_pred) st4(a.flows_pred + o, fp);
            if (TWO) {
                if (a.flows_true) st4(a.flows_true + o, ft);
                if (a.err) st4(a.err + o, make_float4(fp.x - ft.x, fp.y - ft.y, fp.z - ft.z, fp.w - ft.w));
            }
        }
        if (LDS) __syncthreads();                                          // the next sample overwrites the phasors
    }
    if (bad_seen) a.flags[0] = a.flags[0] | 1;       // (every writer stores the same bit over the same word)
}

// ---------------------------------------------------------------------------------------------------- moments
// The moments engine of reduce.hpp over the finished error table, with a line as the owner: slice s walks the samples s,
// s + MO_SLICES, ..., keeps the 24 moments of its line -- one accumulator per quantity -- in registers and hands them over two
// quantities per round.  A (sample, line) whose line names a bus outside [0, n_bus) is left out (its table row is NaN by
// construction, which must not reach the sums): the ids are read again here, never followed.
__global__ __launch_bounds__(MO_THREADS) void branch_moments_kernel(const float* __restrict__ err, const int64_t* __restrict__ edge_index,
                                                                   int lines_per_sample, int n_samples, int n_lines, int n_bus,
                                                                   double* __restrict__ moments) {
    const int t = threadIdx.x, ll = t & (MO_OWNERS - 1), sl = t / MO_OWNERS;
    const int line = blockIdx.x * MO_OWNERS + ll;
    const bool live = line < n_lines;
    const uint64_t nb = (uint64_t)n_bus;
    Moments6 mo[4];
    const bool shared_ok = live && !lines_per_sample && (uint64_t)edge_index[line] < nb && (uint64_t)edge_index[n_lines + line] < nb;
    for (int s0 = sl; s0 < n_samples; s0 += MO_UNROLL * MO_SLICES) {
        float4 v[MO_UNROLL];
        bool on[MO_UNROLL];
#pragma unroll
        for (int u = 0; u < MO_UNROLL; ++u) {       // every load of the trip is requested before the first row is consumed
            const int s = s0 + u * MO_SLICES;
            on[u] = live && s < n_samples;
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (on[u]) {
                if (lines_per_sample) {
                    const int64_t* ei = edge_index + (int64_t)s * 2 * n_lines;
                    on[u] = (uint64_t)ei[line] < nb && (uint64_t)ei[n_lines + line] < nb;
                } else {
                    on[u] = shared_ok;
                }
                if (on[u]) v[u] = ld4(err + 4 * ((int64_t)s * n_lines + line));
            }
        }
#pragma unroll
        for (int u = 0; u < MO_UNROLL; ++u) {
            if (!on[u]) continue;
            const float ev[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int f = 0; f < 4; ++f) mo[f].add((double)ev[f]);
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) moments_round(mo[2 * h], mo[2 * h + 1], h, n_lines, 24, moments);      // two quantities per round
}

static bool bf_use_lds(int64_t n_bus) {
    static const bool off = diag_env("PFN_BRANCH_NO_LDS") != nullptr;      // A/B switch: the direct kernel for every size
    return !off && n_bus <= BF_LDS_MAX_BUS;
}

template <bool TWO>
static int bf_launch(const BfArgs& a, hipStream_t s) {
    const bool lds = bf_use_lds(a.n_bus);
    const size_t bytes = lds ? (size_t)a.n_bus * (TWO ? 16 : 8) : 0;
    const int threads = bytes > (size_t)BF_BIG_LDS ? BF_BIG_THREADS : BF_SMALL_THREADS;
    const int grid = std::max(1, std::min(a.n_samples, 8 * device_cus()));
    if (lds) {
        static std::atomic<uint64_t> raised{0};
        PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(branch_flows_kernel<TWO, true>), kLdsCuBytes - kLdsReserve, raised));
        branch_flows_kernel<TWO, true><<<grid, threads, bytes, s>>>(a);
    } else {
        branch_flows_kernel<TWO, false><<<grid, threads, 0, s>>>(a);
    }
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

}  // namespace pfn

using namespace pfn;

extern "C" {

int64_t pfn_branch_flows_lds_max_bus(void) { return BF_LDS_MAX_BUS; }

size_t pfn_branch_flows_workspace_bytes(int64_t n_samples, int64_t n_lines, int moments_without_err_table) {
    if (!moments_without_err_table || n_samples <= 0 || n_lines <= 0) return 0;
    return (size_t)n_samples * (size_t)n_lines * 4 * sizeof(float);
}

int pfn_branch_flows(const float* pred, int pred_normalised, const float* truth, int truth_normalised, int64_t n_samples, int64_t n_bus,
                     const float* std4, const float* mean4, const int64_t* edge_index, int lines_per_sample, int64_t n_lines,
                     const float* edge_attr, int attr_per_sample, const float* edge_std2, const float* edge_mean2, float* flows_pred,
                     float* flows_true, float* err_table, double* moments, int32_t* flags, void* ws, size_t ws_bytes, void* stream) {
    PFN_CHECK_ARG(n_samples >= 0 && n_bus >= 0 && n_lines >= 0 && n_bus < (1ll << 29) && n_samples < (1ll << 29) && n_lines < (1ll << 29) &&
                      n_samples * n_bus < (1ll << 29) && n_samples * n_lines < (1ll << 29),
                  "pfn_branch_flows: bad sizes (%lld samples of %lld buses and %lld lines)", (long long)n_samples, (long long)n_bus,
                  (long long)n_lines);
    PFN_CHECK_ARG(pred || n_samples == 0, "pfn_branch_flows: null prediction table");
    PFN_CHECK_ARG(truth || !(moments || err_table || flows_true) || n_samples == 0,
                  "pfn_branch_flows: moments, err_table and flows_true need a truth table (null truth: the flows of one table only)");
    PFN_CHECK_ARG(flags, "pfn_branch_flows: null flags");
    const bool any = n_samples > 0 && n_lines > 0;
    PFN_CHECK_ARG(!any || (edge_index && edge_attr), "pfn_branch_flows: null edge_index or edge_attr");
    PFN_CHECK_ARG(((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(truth) | reinterpret_cast<uintptr_t>(flows_pred) |
                    reinterpret_cast<uintptr_t>(flows_true) | reinterpret_cast<uintptr_t>(err_table) | reinterpret_cast<uintptr_t>(ws)) & 15) == 0,
                  "pfn_branch_flows: the bus tables, the line tables and the workspace must be 16-byte aligned");
    PFN_CHECK_ARG(((reinterpret_cast<uintptr_t>(moments) | reinterpret_cast<uintptr_t>(edge_index) | reinterpret_cast<uintptr_t>(edge_attr)) & 7) == 0 &&
                      (reinterpret_cast<uintptr_t>(flags) & 3) == 0,
                  "pfn_branch_flows: moments, edge_index and edge_attr must be 8-byte aligned, flags 4-byte aligned");
    if (!any) return PFN_OK;
    float* err = err_table;
    if (moments && !err) {
        const size_t need = pfn_branch_flows_workspace_bytes(n_samples, n_lines, 1);
        if (!ws || ws_bytes < need) {
            set_error("pfn_branch_flows: moments without err_table need a workspace of %zu bytes (got %zu)", need, ws ? ws_bytes : (size_t)0);
            return PFN_ENOSPACE;
        }
        err = static_cast<float*>(ws);
    }
    BfArgs a;
    a.pred = pred;
    a.truth = truth;
    a.edge_index = edge_index;
    a.edge_attr = edge_attr;
    a.flows_pred = flows_pred;
    a.flows_true = flows_true;
    a.err = err;
    a.flags = flags;
    a.n_samples = (int)n_samples;
    a.n_bus = (int)n_bus;
    a.n_lines = (int)n_lines;
    a.pred_norm = pred_normalised != 0;
    a.truth_norm = truth_normalised != 0;
    a.lines_per_sample = lines_per_sample != 0;
    a.attr_per_sample = attr_per_sample != 0;
    for (int f = 0; f < 2; ++f) {
        a.std[f] = std4 ? std4[f] : 1.f;
        a.mean[f] = mean4 ? mean4[f] : 0.f;
        a.estd[f] = edge_std2 ? edge_std2[f] : 1.f;
        a.emean[f] = edge_mean2 ? edge_mean2[f] : 0.f;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double lines = (double)n_samples * (double)n_lines, buses = (double)n_samples * (double)n_bus;
    {
        const int tables = truth ? 2 : 1;
        ProfScope ps("branch_flows", buses * 8.0 * tables + lines * ((lines_per_sample ? 16.0 : 0.0) + (attr_per_sample ? 8.0 : 0.0) +
                                                                      16.0 * ((flows_pred ? 1 : 0) + (flows_true ? 1 : 0) + (err ? 1 : 0))),
                     (buses * 24.0 + lines * 40.0) * tables, s);
        PFN_TRY(truth ? bf_launch<true>(a, s) : bf_launch<false>(a, s));
    }
    if (moments) {
        ProfScope ps("branch_moments", lines * (16.0 + (lines_per_sample ? 16.0 : 0.0)) + (double)n_lines * 384.0, lines * 32.0, s);
        branch_moments_kernel<<<(int)((n_lines + MO_OWNERS - 1) / MO_OWNERS), MO_THREADS, 0, s>>>(err, edge_index, a.lines_per_sample, a.n_samples,
                                                                                          a.n_lines, a.n_bus, moments);
        PFN_CHECK_LAUNCH();
    }
    return PFN_OK;
}

}  // extern "C"
