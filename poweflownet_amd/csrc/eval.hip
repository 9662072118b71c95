// Evaluation metrics of one batch in one launch, with the epoch's running sums kept on the device (gfx950): pfn_eval_metrics
// turns the rows (out, y, x, pred_mask) of a batch into every term test.py reports -- MaskedL2V2 / MaskedL1 (normalised and
// de-normalised), the two means of Masked_L2_loss, the plain MSE -- and pfn_eval_accumulate adds one loss scalar to a running
// double.  Both are pure functions of their inputs (no float atomics, a fixed reduction tree), so a hipGraph replay of an
// evaluation epoch gives the bits of the eager loop.
#include <algorithm>

#include "pfn_internal.hpp"

namespace pfn {

// per-block partial sums, slot-major: slot s of block b at part[s * 256 + b]
//   0-3 cnt[f] | 4-7 sum m*d^2 | 8-11 sum m*|d| | 12-15 sum m*(d*std)^2 | 16-19 sum m*|d*std| | 20 selected sum | 21 regulariser sum
//   | 22 sum d^2 | 23 unused | 24, 25 the two selection counts (int32 bit patterns)
constexpr int kEvalFloatSlots = 24, kEvalSlots = 26;
struct EvalWs {
    float part[kEvalSlots * 256];
    int counter;   // byte 26624
    int pad_[3];
};
struct EvalStd {
    float s[4];
};

// Products and sums that must round ONE operation at a time (bit for bit torch's separate kernels / the host's double arithmetic):
// contraction into an fma is switched off for these bodies -- hipcc contracts a plain a * b + c, also when it is written with
// the _rn intrinsics.
__device__ __forceinline__ float eval_mix(float o, float x, float m) {
#pragma clang fp contract(off)
    const float a = o * m;
    const float k = 1.f - m;
    const float b = x * k;
    return a + b;
}
__device__ __forceinline__ double eval_acc_add(double acc, double v, double w) {
#pragma clang fp contract(off)
    const double p = v * w;
    return acc + p;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// terms of one family from its four column sums: per-feature means, their overall and their balanced mean
// (custom_loss_functions._per_feature_terms)
__device__ __forceinline__ void eval_family(const float* S, const float* cntc, float cnt_all, float* t) {
    float pf[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) pf[f] = S[f] / cntc[f];
    t[0] = (((pf[0] * cntc[0] + pf[1] * cntc[1]) + pf[2] * cntc[2]) + pf[3] * cntc[3]) / cnt_all;
    t[1] = (((pf[0] + pf[1]) + pf[2]) + pf[3]) * 0.25f;
#pragma unroll
    for (int f = 0; f < 4; ++f) t[2 + f] = pf[f];
}

// One thread per row (grid-stride past 256 x 256 rows), 16-byte loads, 25 accumulators; wave butterflies, a fixed LDS combine of the
// four waves, then the drained hand-off (device_prims.hpp): partials stored write-through and drained before the ticket, the last
// arriver reads them with agent-scope loads, sums them in an order that depends on the grid only, writes the terms, updates the
// epoch accumulators and re-arms the ticket.
__global__ __launch_bounds__(256) void eval_metrics_kernel(const float* __restrict__ o, const float* __restrict__ y,
                                                           const float* __restrict__ x, const void* __restrict__ mask,
                                                           int mask_dtype, int64_t n, EvalStd sd, double weight,
                                                           int first_unweighted, EvalWs* __restrict__ w,
                                                           float* __restrict__ terms, double* __restrict__ acc,
                                                           float* __restrict__ mixed) {
    __shared__ float red[4][kEvalSlots];
    __shared__ float tot[kEvalSlots + 2];
    __shared__ int s_last;
    float cnt[4] = {0.f, 0.f, 0.f, 0.f}, l2[4] = {0.f, 0.f, 0.f, 0.f}, l1[4] = {0.f, 0.f, 0.f, 0.f};
    float l2d[4] = {0.f, 0.f, 0.f, 0.f}, l1d[4] = {0.f, 0.f, 0.f, 0.f};
    float s1 = 0.f, s0 = 0.f, sq = 0.f;
    int c1 = 0, c0 = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const float4 vo = ld4(o + 4 * r), vy = ld4(y + 4 * r), vm = mask_row4(mask, mask_dtype, r);
        const float ov[4] = {vo.x, vo.y, vo.z, vo.w}, yv[4] = {vy.x, vy.y, vy.z, vy.w}, mv[4] = {vm.x, vm.y, vm.z, vm.w};
        float mix[4] = {0.f, 0.f, 0.f, 0.f};
        if (mixed) {
            // out * mask + x * (1 - mask), every product and the sum rounded on their own (torch's three kernels)
            const float4 vx = ld4(x + 4 * r);
            const float xv[4] = {vx.x, vx.y, vx.z, vx.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) mix[e] = eval_mix(ov[e], xv[e], mv[e]);
            st4(mixed + 4 * r, make_float4(mix[0], mix[1], mix[2], mix[3]));
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = ov[e] - yv[e], m = mv[e];
            const float dd = d * sd.s[e];                           // the de-normalised error: the mean cancels
            cnt[e] += m;
            // the mask MULTIPLIES (error * mask.float()): a NaN under a zero mask entry poisons its column, as in the reference
            l2[e] = fmaf(m, d * d, l2[e]);
            l1[e] = fmaf(m, fabsf(d), l1[e]);
            l2d[e] = fmaf(m, dd * dd, l2d[e]);
            l1d[e] = fmaf(m, fabsf(dd), l1d[e]);
            if (m != 0.f) { s1 = fmaf(d, d, s1); ++c1; }           // mask.type(bool)
            if (1.f - m != 0.f) { s0 = fmaf(d, d, s0); ++c0; }     // (1 - mask).type(bool)
            sq = fmaf(d, d, sq);
        }
    }
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const float4 g0 = wave_sum4(make_float4(cnt[0], cnt[1], cnt[2], cnt[3]));
    const float4 g1 = wave_sum4(make_float4(l2[0], l2[1], l2[2], l2[3]));
    const float4 g2 = wave_sum4(make_float4(l1[0], l1[1], l1[2], l1[3]));
    const float4 g3 = wave_sum4(make_float4(l2d[0], l2d[1], l2d[2], l2d[3]));
    const float4 g4 = wave_sum4(make_float4(l1d[0], l1d[1], l1d[2], l1d[3]));
    const float4 g5 = wave_sum4(make_float4(s1, s0, sq, 0.f));
    c1 = wave_sum_int(c1);
    c0 = wave_sum_int(c0);
    if (lane == 0) {
        float* q = red[wv];
        q[0] = g0.x; q[1] = g0.y; q[2] = g0.z; q[3] = g0.w;
        q[4] = g1.x; q[5] = g1.y; q[6] = g1.z; q[7] = g1.w;
        q[8] = g2.x; q[9] = g2.y; q[10] = g2.z; q[11] = g2.w;
        q[12] = g3.x; q[13] = g3.y; q[14] = g3.z; q[15] = g3.w;
        q[16] = g4.x; q[17] = g4.y; q[18] = g4.z; q[19] = g4.w;
        q[20] = g5.x; q[21] = g5.y; q[22] = g5.z; q[23] = 0.f;
        q[24] = __int_as_float(c1); q[25] = __int_as_float(c0);
    }
    __syncthreads();
    if (wv == 0) {
        // the drained hand-off (device_prims.hpp).  Its contract holds: all 26 stores are lanes of wave 0, whose lane 0 drains and
        // takes the ticket.
        if (t < kEvalSlots) {
            float v;
            if (t < kEvalFloatSlots) v = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
            else v = __int_as_float(((__float_as_int(red[0][t]) + __float_as_int(red[1][t])) + __float_as_int(red[2][t])) +
                                    __float_as_int(red[3][t]));
            agent_store(w->part + t * 256 + blockIdx.x, v);
        }
        if (t == 0) s_last = handoff_drained_publish(&w->counter);
    }
    __syncthreads();
    if (!s_last) return;
    // the last arriver: wave wv sums slot groups wv and wv + 4 -- per lane the blocks lane, lane + 64, lane + 128, lane + 192 in
    // that order, then the butterfly: an order fixed by the grid, not by arrival
    const int nb = (int)gridDim.x;
    for (int g = wv; g < 7; g += 4) {
        if (g < 6) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int b = lane + 64 * j;
                if (b < nb) {
                    const float* p = w->part + (4 * g) * 256 + b;
                    a.x += agent_load(p);
                    a.y += agent_load(p + 256);
                    a.z += agent_load(p + 512);
                    a.w += agent_load(p + 768);
                }
            }
            a = wave_sum4(a);
            if (lane == 0) { tot[4 * g] = a.x; tot[4 * g + 1] = a.y; tot[4 * g + 2] = a.z; tot[4 * g + 3] = a.w; }
        } else {
            int k1 = 0, k0 = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int b = lane + 64 * j;
                if (b < nb) {
                    k1 += __float_as_int(agent_load(w->part + 24 * 256 + b));
                    k0 += __float_as_int(agent_load(w->part + 25 * 256 + b));
                }
            }
            k1 = wave_sum_int(k1);
            k0 = wave_sum_int(k0);
            if (lane == 0) { tot[24] = __int_as_float(k1); tot[25] = __int_as_float(k0); }
        }
    }
    __syncthreads();
    __shared__ float s_terms[PFN_EVAL_N_TERMS];
    if (t == 0) {
        float cntc[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            s_terms[PFN_EVAL_CNT_VM + f] = tot[f];
            cntc[f] = fmaxf(tot[f], 1e-6f);                          // .clamp(min=1e-6)
        }
        const float cnt_all = fmaxf(((tot[0] + tot[1]) + tot[2]) + tot[3], 1e-6f);
        eval_family(tot + 4, cntc, cnt_all, s_terms + PFN_EVAL_L2_TOTAL);
        eval_family(tot + 12, cntc, cnt_all, s_terms + PFN_EVAL_L2D_TOTAL);
        eval_family(tot + 8, cntc, cnt_all, s_terms + PFN_EVAL_L1_TOTAL);
        eval_family(tot + 16, cntc, cnt_all, s_terms + PFN_EVAL_L1D_TOTAL);
        s_terms[PFN_EVAL_ML2_SELECTED] = tot[20] / (float)__float_as_int(tot[24]);     // 0/0 = NaN: torch's mean of an empty selection
        s_terms[PFN_EVAL_ML2_REGULARIZER] = tot[21] / (float)__float_as_int(tot[25]);
        s_terms[PFN_EVAL_MSE] = tot[22] / (4.f * (float)n);                        // (an empty batch: NaN, torch's mean of nothing)
        w->counter = 0;
    }
    __syncthreads();
    if (t < PFN_EVAL_N_TERMS) {
        const float v = s_terms[t];
        terms[t] = v;
        if (acc) {
            // acc[k] += w * (double)term[k]: product and sum rounded separately -- the host loop `acc += float(term) * w`
            const long long batches = reinterpret_cast<const long long*>(acc)[PFN_EVAL_ACC_BATCHES];
            const double wt = (first_unweighted && batches == 0) ? 1.0 : weight;
            acc[t] = eval_acc_add(acc[t], (double)v, wt);
        }
    }
    if (acc) {
        __syncthreads();                                             // every term has read the batch counter
        if (t == 0) reinterpret_cast<long long*>(acc)[PFN_EVAL_ACC_BATCHES] += 1;
    }
}

// acc[0] += (double)loss[0] * w; ++batches (acc[1], an int64).  A float widened to double times len(data) is what the host loop's
// `loss.item() * len(data)` computes, so an epoch value accumulated here keeps its bits.
__global__ void eval_accumulate_kernel(const float* __restrict__ loss, double weight, int first_unweighted, double* __restrict__ acc) {
    long long* batches = reinterpret_cast<long long*>(acc) + 1;
    const long long b = *batches;
    const double wt = (first_unweighted && b == 0) ? 1.0 : weight;
    acc[0] = eval_acc_add(acc[0], (double)loss[0], wt);
    *batches = b + 1;
}

}  // namespace pfn

using namespace pfn;

extern "C" {

int pfn_eval_metrics(const float* out, const float* y, const float* x, const void* mask, int mask_dtype, int64_t n_rows,
                     const float* std4, double weight, int first_unweighted, float* terms, double* epoch_acc, float* mixed_out,
                     void* ws, size_t ws_bytes, void* stream) {
    PFN_CHECK_ARG(terms && ws && (n_rows == 0 || (out && y && mask)), "pfn_eval_metrics: null pointer");
    PFN_CHECK_ARG(mask_dtype == 0 || mask_dtype == 1, "pfn_eval_metrics: mask_dtype must be 0 (int64) or 1 (float32)");
    PFN_CHECK_ARG(n_rows >= 0 && n_rows < (1ll << 29), "pfn_eval_metrics: bad row count %lld", (long long)n_rows);
    PFN_CHECK_ARG(!mixed_out || x || n_rows == 0, "pfn_eval_metrics: mixed_out needs x");
    PFN_CHECK_ARG(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(x) |
                    reinterpret_cast<uintptr_t>(mask) | reinterpret_cast<uintptr_t>(mixed_out)) & 15) == 0,
                  "pfn_eval_metrics: out, y, x, mask and mixed_out must be 16-byte aligned");
    PFN_CHECK_ARG((reinterpret_cast<uintptr_t>(epoch_acc) & 7) == 0, "pfn_eval_metrics: epoch_acc must be 8-byte aligned");
    if (ws_bytes < sizeof(EvalWs)) {
        set_error("pfn_eval_metrics: workspace too small (need %zu bytes)", sizeof(EvalWs));
        return PFN_ENOSPACE;
    }
    EvalStd sd;
    for (int f = 0; f < 4; ++f) sd.s[f] = std4 ? std4[f] : 1.f;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // an empty batch still launches ONE block: it writes the terms of nothing (0 for the clamped means, NaN for the selected ones)
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((n_rows + 255) / 256, 256));
    ProfScope ps("eval_metrics", (double)n_rows * (32.0 + (mask_dtype == 0 ? 32.0 : 16.0) + (mixed_out ? 32.0 : 0.0)),
                 (double)n_rows * 80.0, s);
    eval_metrics_kernel<<<nb, 256, 0, s>>>(out, y, x, mask, mask_dtype, n_rows, sd, weight, first_unweighted,
                                           static_cast<EvalWs*>(ws), terms, epoch_acc, (mixed_out && n_rows > 0) ? mixed_out : nullptr);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

int pfn_eval_accumulate(const float* loss, double weight, int first_unweighted, double* acc, void* stream) {
    PFN_CHECK_ARG(loss && acc, "pfn_eval_accumulate: null pointer");
    PFN_CHECK_ARG((reinterpret_cast<uintptr_t>(acc) & 7) == 0, "pfn_eval_accumulate: acc must be 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope ps("eval_accumulate", 28.0, 2.0, s);
    eval_accumulate_kernel<<<1, 1, 0, s>>>(loss, weight, first_unweighted, acc);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

}  // extern "C"
