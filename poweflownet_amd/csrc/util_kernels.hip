// The small kernels around a training step and their C ABI (gfx950): MSELoss, Masked_L2_loss, AdamW, the dropout-mask replay and
// the ReLU gate export.  None of them takes part in choosing a step's kernels (model.hip); each is launched as written here.
#include <algorithm>

#include "pfn_internal.hpp"
#include "reduce.hpp"

namespace pfn {

// ---- Masked_L2_loss (utils/custom_loss_functions.py:10-46): two masked means of (out - y)^2.  Kernel 1 reduces
// (sum, count) of both sets with an ordered last-arriver combine (reduce.hpp masked_l2_combine: MaskedL2Ws) and writes the loss and
// the totals; kernel 2 turns the totals into the two gradient scales.
__global__ __launch_bounds__(256) void masked_l2_reduce_kernel(const float* __restrict__ o, const float* __restrict__ y,
                                                               const void* __restrict__ mask, int mask_dtype, int64_t n,
                                                               int regularize, float regcoeff, MaskedL2Ws* __restrict__ w,
                                                               float* __restrict__ loss) {
    float a1 = 0.f, a0 = 0.f;
    int k1 = 0, k0 = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float d = o[i] - y[i], m = mask_elem(mask, mask_dtype, i);
        if (m != 0.f) { a1 = fmaf(d, d, a1); ++k1; }                 // mask.type(bool)
        if (1.f - m != 0.f) { a0 = fmaf(d, d, a0); ++k0; }           // (1 - mask).type(bool)
    }
    if (!masked_l2_combine(a1, a0, k1, k0, w)) return;
    if (threadIdx.x == 0) {
        float l = w->tot_s1 / (float)w->tot_c1;                      // 0/0 = NaN: torch's mean of an empty selection
        if (regularize) l += regcoeff * (w->tot_s0 / (float)w->tot_c0);
        loss[0] = l;
    }
}
__global__ __launch_bounds__(256) void masked_l2_grad_kernel(const float* __restrict__ o, const float* __restrict__ y,
                                                             const void* __restrict__ mask, int mask_dtype, int64_t n,
                                                             int regularize, float regcoeff, const MaskedL2Ws* __restrict__ w,
                                                             float* __restrict__ grad) {
    const float g1 = 2.f / (float)w->tot_c1, g0 = regularize ? 2.f * regcoeff / (float)w->tot_c0 : 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float d = o[i] - y[i], m = mask_elem(mask, mask_dtype, i);
        float g = 0.f;
        if (m != 0.f) g += g1 * d;
        if (regularize && 1.f - m != 0.f) g += g0 * d;
        grad[i] = g;
    }
}

// One launch: every block reduces its slice to a partial and takes a ticket; the last arriver sums the partials in
// block order (not arrival order: deterministic) and re-arms the counter for the next call.
__global__ __launch_bounds__(256) void mse_kernel(const float* __restrict__ o, const float* __restrict__ y, int64_t n,
                                                  float inv_n, float* __restrict__ grad, float* __restrict__ partial,
                                                  int* __restrict__ counter, float* __restrict__ loss) {
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float d = o[i] - y[i];
        acc = fmaf(d, d, acc);
        if (grad) grad[i] = 2.f * d * inv_n;
    }
    // (the drained hand-off, device_prims.hpp: no __threadfence on either side of the ticket; the kernel had two)
    float total = 0.f;
    if (grid_sum_ordered<true>(acc, partial, counter, total) && threadIdx.x == 0) loss[0] = total * inv_n;
}

// one block per CU at most: every block ends with one atomic on the arrival counter (64 blocks of 1024 threads were tried for
// that reason: 8.9 against 8.4 us)
static int adamw_blocks(int64_t count) { return (int)std::max<int64_t>(1, std::min<int64_t>((count + 255) / 256, 256)); }

// hp (optional): device {lr, beta1, beta2, eps, weight_decay} read instead of the by-value arguments, so that a captured
// launch follows a learning-rate schedule without being captured again
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, int64_t n, float lr,
                                                    float b1, float b2, float eps, float wd, int64_t* step,
                                                    const float* __restrict__ hp, const float* __restrict__ guard) {
    // guard (optional): a device scalar -- normally the step's loss; not finite = the batch was flagged bad on the device
    // (pfn_graph_poison_if_bad): every block sees the same value and leaves, nothing is updated, the step is not counted
    if (guard) {
        const float gv = *guard;
        if (!(fabsf(gv) <= 3.402823466e+38f)) {
            if (blockIdx.x == 0 && threadIdx.x == 0) step[2] += 1;   // skipped updates: visible to the host loop (train_epoch warns)
            return;
        }
    }
    // 16 bytes per lane and array when the four flat buffers allow it (they are whole allocations: 256-byte aligned); the
    // update is a chain of dependent loads per element otherwise (10 us for 355 k parameters, 2x its memory time).  A thread's
    // FIRST four-element group is requested before the hyper-parameters are even read: their load -> powf chain and this load
    // were two serial round trips.
    const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                       reinterpret_cast<uintptr_t>(v)) & 15) == 0;
    const int64_t n4 = vec ? n >> 2 : 0;
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    float4 p4 = make_float4(0.f, 0.f, 0.f, 0.f), m4 = p4, v4 = p4, g4 = p4;
    if (i0 < n4) {
        p4 = reinterpret_cast<float4*>(p)[i0];
        m4 = reinterpret_cast<float4*>(m)[i0];
        v4 = reinterpret_cast<float4*>(v)[i0];
        g4 = reinterpret_cast<const float4*>(g)[i0];
    }
    if (hp) {
        lr = hp[0]; b1 = hp[1]; b2 = hp[2]; eps = hp[3]; wd = hp[4];
    }
    // step[0] = completed steps, step[1] = arrival counter: the last block to ARRIVE bumps the step and re-arms the counter, so the
    // whole update is ONE launch and stays hipGraph-replayable.  The ticket is taken as soon as every wave of the block has READ
    // step[0] (the barrier below waits for that scalar load only, not for the element loads in flight) -- the bump has to come after
    // all blocks' reads, not after their updates; taken behind the update, the launch ended with stores drained -> atomic round
    // trip -> store, ~1 us of nothing.
    const int64_t step_now = step[0];
    const float t = (float)(step_now + 1);
    asm volatile("s_barrier" ::"s"((int)step_now) : "memory");   // (the operand: this wave's read of step[0] has returned)
    if (threadIdx.x == 0) {
        const unsigned long long prev = atomicAdd(reinterpret_cast<unsigned long long*>(step + 1), 1ull);
        if (prev == (unsigned long long)gridDim.x - 1) {
            step[1] = 0;
            step[0] = step_now + 1;
        }
    }
    const float bc1 = 1.f - powf(b1, t), bc2 = 1.f - powf(b2, t);
    const float step_size = lr / bc1, inv_sqrt_bc2 = 1.f / sqrtf(bc2);
    auto upd = [&](float& pi, float gi, float& mi, float& vi) {
        pi *= (1.f - lr * wd);                           // decoupled weight decay
        mi = b1 * mi + (1.f - b1) * gi;
        vi = b2 * vi + (1.f - b2) * gi * gi;
        const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
        pi -= step_size * (mi / denom);
    };
    for (int64_t i = i0; i < n4; i += stride) {
        if (i != i0) {
            p4 = reinterpret_cast<float4*>(p)[i];
            m4 = reinterpret_cast<float4*>(m)[i];
            v4 = reinterpret_cast<float4*>(v)[i];
            g4 = reinterpret_cast<const float4*>(g)[i];
        }
        upd(p4.x, g4.x, m4.x, v4.x);
        upd(p4.y, g4.y, m4.y, v4.y);
        upd(p4.z, g4.z, m4.z, v4.z);
        upd(p4.w, g4.w, m4.w, v4.w);
        st4_wt(p + 4 * i, p4);      // (write-through: the next step's first kernel does not wait for 4 MB of dirty lines)
        st4_wt(m + 4 * i, m4);
        st4_wt(v + 4 * i, v4);
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float pi = p[i], mi = m[i], vi = v[i];
        upd(pi, g[i], mi, vi);
        p[i] = pi;
        m[i] = mi;
        v[i] = vi;
    }
}

// The keep mask (1 = kept, 0 = dropped) the dropout epilogue of layer `stream` applies for the CURRENT {seed, offset} of
// rng -- the same dropout_uniform4 call, element for element -- so a test can replay a train-mode pass on the CPU oracle.
__global__ __launch_bounds__(256) void dropout_mask_kernel(const uint64_t* __restrict__ rng, uint32_t stream, int64_t rows,
                                                           int ncols, float p, float* __restrict__ out) {
    const int ncg = (ncols + 3) >> 2;
    const DropKey dk = drop_key(rng[0], rng[1], stream);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * ncg; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / ncg;
        const int cg = (int)(i - row * ncg);
        float u[4];
        dropout_uniform4(dk, (uint32_t)row, (uint32_t)cg, u);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * cg + e < ncols) out[row * ncols + 4 * cg + e] = u[e] >= p ? 1.f : 0.f;
    }
}

// ---- ReLU gate export (verification aid, pfn_mpn_export_gates): the decisions of the three kinds of ReLU a forward pass
// took, as bytes, so that a float64 run of the oracle can be held to the SAME piecewise-linear branch and the gradients compared
// at north_star's tolerance (a pre-activation within the fp32 forward error of zero otherwise flips its gate in one of the two
// runs and moves a weight gradient by 1e-5..2e-4 of its largest entry).
// Edge stage of an EdgeAggregation layer: out[eid][k] = (P[dst][k] + Q[src][k] + sum_f a_e[f] We[k][f] > 0) with EXACTLY the
// expression the walks evaluate (edge.hip edge_sum_chunk / edge_bwd_*_body, ea_seg.hip: add, then one fmaf per attribute, in
// attribute order) on the P | Q the forward saved -- which is also what the saved mask bytes hold where the forward saved them.
__global__ __launch_bounds__(256) void export_edge_gates_kernel(int n, int e_stored, const int* __restrict__ rowptr,
                                                                const int* __restrict__ nbr, const int* __restrict__ eid,
                                                                const float* __restrict__ P, const float* __restrict__ Q,
                                                                const float* __restrict__ ea, const float* __restrict__ w1,
                                                                int ld, int h, int fi, int fe, uint8_t* __restrict__ out) {
    const int ldw = 2 * fi + fe;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < (int64_t)n * h; it += (int64_t)gridDim.x * blockDim.x) {
        const int row = (int)(it / h), k = (int)(it - (int64_t)row * h);
        const float p = P[(size_t)row * ld + k];
        for (int q = rowptr[row]; q < rowptr[row + 1]; ++q) {
            const int id = eid[q], idm = id >= e_stored ? id - e_stored : id;
            float v = p + Q[(size_t)nbr[q] * ld + k];
            for (int f = 0; f < fe; ++f) v = fmaf(ea[(size_t)idm * fe + f], w1[(size_t)k * ldw + 2 * fi + f], v);
            out[(size_t)id * h + k] = relu_on(v) ? 1 : 0;
        }
    }
}
// Layer outputs (and mask_embd's hidden layer): out[row][k] = y[row][k] > 0, the test the backward pass applies (GemmArgs::gate).
__global__ __launch_bounds__(256) void export_row_gates_kernel(int64_t n, int h, int ld, const float* __restrict__ y,
                                                               uint8_t* __restrict__ out, int cm) {
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < n * h; it += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = it / h, col = it - row * h;
        const float v = cm ? y[((col >> 2) * n + row) * 4 + (col & 3)] : y[row * ld + col];   // (chunk-major: Act::out_cm)
        out[it] = relu_on(v) ? 1 : 0;
    }
}

int launch_export_edge_gates(const GraphView& g, const float* P, const float* Q, const float* ea, const float* w1, int ld, int h, int fi,
                             int fe, uint8_t* out, hipStream_t s) {
    const int blocks = (int)std::min<int64_t>(((int64_t)g.n * h + 255) / 256, 16384);
    export_edge_gates_kernel<<<blocks, 256, 0, s>>>(g.n, g.e_stored, g.rowptr_in, g.in_src, g.in_eid, P, Q, ea, w1, ld, h, fi, fe, out);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}
int launch_export_row_gates(int64_t n, int h, int ld, const float* y, int cm, uint8_t* out, hipStream_t s) {
    const int blocks = (int)std::min<int64_t>((n * h + 255) / 256, 16384);
    export_row_gates_kernel<<<blocks, 256, 0, s>>>(n, h, ld, y, out, cm);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

}  // namespace pfn

using namespace pfn;

extern "C" {

int pfn_mse_loss(const float* out, const float* y, int64_t count, float* loss, float* grad, void* ws, size_t ws_bytes,
                 void* stream) {
    PFN_CHECK_ARG(out && y && loss && ws, "pfn_mse_loss: null pointer");
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((count + 1023) / 1024, 256));
    if (ws_bytes < 257 * sizeof(float)) {
        set_error("pfn_mse_loss: workspace too small (need %zu bytes)", 257 * sizeof(float));
        return PFN_ENOSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float inv_n = count > 0 ? 1.0f / (float)count : 0.f;
    mse_kernel<<<nb, 256, 0, s>>>(out, y, count, inv_n, grad, static_cast<float*>(ws),
                                  reinterpret_cast<int*>(static_cast<float*>(ws) + 256), loss);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

int pfn_masked_l2_loss(const float* out, const float* y, const void* mask, int mask_dtype, int64_t count, int regularize,
                       float regcoeff, float* loss, float* grad, void* ws, size_t ws_bytes, void* stream) {
    PFN_CHECK_ARG(out && y && mask && loss && ws, "pfn_masked_l2_loss: null pointer");
    PFN_CHECK_ARG(mask_dtype == 0 || mask_dtype == 1, "pfn_masked_l2_loss: mask_dtype must be 0 (int64) or 1 (float32)");
    if (ws_bytes < sizeof(MaskedL2Ws)) {
        set_error("pfn_masked_l2_loss: workspace too small (need %zu bytes)", sizeof(MaskedL2Ws));
        return PFN_ENOSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    MaskedL2Ws* w = static_cast<MaskedL2Ws*>(ws);
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((count + 1023) / 1024, 256));
    masked_l2_reduce_kernel<<<nb, 256, 0, s>>>(out, y, mask, mask_dtype, count, regularize, regcoeff, w, loss);
    PFN_CHECK_LAUNCH();
    if (grad && count > 0) {
        masked_l2_grad_kernel<<<(int)std::min<int64_t>((count + 255) / 256, 1024), 256, 0, s>>>(out, y, mask, mask_dtype, count,
                                                                                              regularize, regcoeff, w, grad);
        PFN_CHECK_LAUNCH();
    }
    return PFN_OK;
}

int pfn_dropout_mask(const uint64_t* rng_state, int32_t layer, int64_t rows, int64_t ncols, float p, float* keep,
                     void* stream) {
    PFN_CHECK_ARG(rng_state && (rows == 0 || keep), "pfn_dropout_mask: null pointer");
    PFN_CHECK_ARG(layer >= 0 && rows >= 0 && rows < (1ll << 32) && ncols > 0 && ncols < (1ll << 30), "pfn_dropout_mask: bad sizes");
    if (rows == 0) return PFN_OK;
    const int64_t items = rows * ((ncols + 3) / 4);
    dropout_mask_kernel<<<(int)std::min<int64_t>((items + 255) / 256, 4096), 256, 0, static_cast<hipStream_t>(stream)>>>(
        rng_state, (uint32_t)layer, rows, (int)ncols, p, keep);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

int pfn_adamw_step(float* p, const float* g, float* m, float* v, int64_t count, float lr, float b1, float b2,
                   float eps, float wd, int64_t* step, void* stream) {
    PFN_CHECK_ARG(p && g && m && v && step, "pfn_adamw_step: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    adamw_kernel<<<adamw_blocks(count), 256, 0, s>>>(p, g, m, v, count, lr, b1, b2, eps, wd, step, nullptr, nullptr);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

int pfn_adamw_step_dev(float* p, const float* g, float* m, float* v, int64_t count, const float* hyper, int64_t* step,
                       void* stream) {
    PFN_CHECK_ARG(p && g && m && v && step && hyper, "pfn_adamw_step_dev: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    adamw_kernel<<<adamw_blocks(count), 256, 0, s>>>(p, g, m, v, count, 0.f, 0.f, 0.f, 0.f, 0.f, step, hyper, nullptr);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

int pfn_adamw_step_guarded(float* p, const float* g, float* m, float* v, int64_t count, const float* hyper, int64_t* step,
                           const float* guard, void* stream) {
    PFN_CHECK_ARG(p && g && m && v && step && hyper && guard, "pfn_adamw_step_guarded: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    adamw_kernel<<<adamw_blocks(count), 256, 0, s>>>(p, g, m, v, count, 0.f, 0.f, 0.f, 0.f, 0.f, step, hyper, guard);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

}  // extern "C"

// ---- MSELoss / Masked_L2_loss over the VALID rows of a slot batch (segpack.py "slot buckets": filler graphs and padding rows carry
// validity 0).  The denominators depend on the batch, so they are counted on the device: kernel 1 reduces (sum, count) of the valid
// rows -- one row of four entries per thread, block partials combined by the last arriver IN BLOCK ORDER, as above -- and writes the
// loss and the totals; kernel 2 writes the gradient rows: the expressions of mse_kernel / masked_l2_grad_kernel on a valid row
// (bit-identical to those kernels run on the compacted valid rows), exact zeros on every other row.  MASKED = false: every entry
// of a valid row belongs to set 1 (MSELoss).
namespace pfn {

template <bool MASKED>
__global__ __launch_bounds__(256) void loss_rows_reduce_kernel(const float* __restrict__ o, const float* __restrict__ y,
                                                               const void* __restrict__ mask, int mask_dtype,
                                                               const int* __restrict__ valid, int64_t n_rows, int regularize,
                                                               float regcoeff, MaskedL2Ws* __restrict__ w, float* __restrict__ loss) {
    float a1 = 0.f, a0 = 0.f;
    int k1 = 0, k0 = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * blockDim.x) {
        if (valid[r] == 0) continue;
        const float4 vo = ld4(o + r * 4), vy = ld4(y + r * 4);
        const float d[4] = {vo.x - vy.x, vo.y - vy.y, vo.z - vy.z, vo.w - vy.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float m = MASKED ? mask_elem(mask, mask_dtype, r * 4 + e) : 1.f;
            if (m != 0.f) { a1 = fmaf(d[e], d[e], a1); ++k1; }
            if (MASKED && 1.f - m != 0.f) { a0 = fmaf(d[e], d[e], a0); ++k0; }
        }
    }
    if (!masked_l2_combine(a1, a0, k1, k0, w)) return;
    if (threadIdx.x == 0) {
        float l = 0.f;                                                   // no valid row at all: the loss of nothing is 0 here
        if (w->tot_c1 + w->tot_c0 > 0) {
            if (MASKED) {
                l = w->tot_s1 / (float)w->tot_c1;                        // (an empty set of a non-empty batch: NaN, as above)
                if (regularize) l += regcoeff * (w->tot_s0 / (float)w->tot_c0);
            } else {
                l = w->tot_s1 * __fdiv_rn(1.0f, (float)w->tot_c1);       // mse_kernel: sum * inv_n, inv_n = 1 / count rounded once
            }
        }
        loss[0] = l;
    }
}

template <bool MASKED>
__global__ __launch_bounds__(256) void loss_rows_grad_kernel(const float* __restrict__ o, const float* __restrict__ y,
                                                             const void* __restrict__ mask, int mask_dtype,
                                                             const int* __restrict__ valid, int64_t n_rows, int regularize,
                                                             float regcoeff, const MaskedL2Ws* __restrict__ w, float* __restrict__ grad) {
    const float g1 = 2.f / (float)w->tot_c1, g0 = regularize ? 2.f * regcoeff / (float)w->tot_c0 : 0.f;      // masked_l2_grad_kernel's
    const float inv_n = w->tot_c1 > 0 ? __fdiv_rn(1.0f, (float)w->tot_c1) : 0.f;                              // pfn_mse_loss's
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * blockDim.x) {
        float gr[4] = {0.f, 0.f, 0.f, 0.f};
        if (valid[r] != 0) {
            const float4 vo = ld4(o + r * 4), vy = ld4(y + r * 4);
            const float dd[4] = {vo.x - vy.x, vo.y - vy.y, vo.z - vy.z, vo.w - vy.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = dd[e];
                if (MASKED) {
                    const float m = mask_elem(mask, mask_dtype, r * 4 + e);
                    float g = 0.f;
                    if (m != 0.f) g += g1 * d;
                    if (regularize && 1.f - m != 0.f) g += g0 * d;
                    gr[e] = g;
                } else {
                    gr[e] = 2.f * d * inv_n;
                }
            }
        }
        st4(grad + r * 4, make_float4(gr[0], gr[1], gr[2], gr[3]));
    }
}

template <bool MASKED>
static int launch_loss_rows(const char* what, const float* out, const float* y, const void* mask, int mask_dtype, const int32_t* valid,
                            int64_t n_rows, int regularize, float regcoeff, float* loss, float* grad, void* ws, size_t ws_bytes,
                            hipStream_t s) {
    if (ws_bytes < sizeof(MaskedL2Ws)) {
        set_error("%s: workspace too small (need %zu bytes)", what, sizeof(MaskedL2Ws));
        return PFN_ENOSPACE;
    }
    MaskedL2Ws* w = static_cast<MaskedL2Ws*>(ws);
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((n_rows + 255) / 256, 256));
    ProfScope ps(what, (double)n_rows * (MASKED ? 84.0 : 52.0), (double)n_rows * 12.0, s);
    loss_rows_reduce_kernel<MASKED><<<nb, 256, 0, s>>>(out, y, mask, mask_dtype, valid, n_rows, regularize, regcoeff, w, loss);
    PFN_CHECK_LAUNCH();
    if (grad && n_rows > 0) {
        loss_rows_grad_kernel<MASKED><<<(int)std::min<int64_t>((n_rows + 255) / 256, 1024), 256, 0, s>>>(out, y, mask, mask_dtype, valid,
                                                                                                        n_rows, regularize, regcoeff, w, grad);
        PFN_CHECK_LAUNCH();
    }
    return PFN_OK;
}

}  // namespace pfn

extern "C" {

int pfn_mse_loss_rows(const float* out, const float* y, const int32_t* valid, int64_t n_rows, float* loss, float* grad, void* ws,
                      size_t ws_bytes, void* stream) {
    PFN_CHECK_ARG(loss && ws && (n_rows == 0 || (out && y && valid)), "pfn_mse_loss_rows: null pointer");
    PFN_CHECK_ARG(n_rows >= 0 && n_rows < (1ll << 29), "pfn_mse_loss_rows: bad row count %lld", (long long)n_rows);
    PFN_CHECK_ARG(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(grad)) & 15) == 0,
                  "pfn_mse_loss_rows: out, y and grad must be 16-byte aligned");
    return pfn::launch_loss_rows<false>("mse_loss_rows", out, y, nullptr, 1, valid, n_rows, 0, 0.f, loss, grad, ws, ws_bytes,
                                        static_cast<hipStream_t>(stream));
}

int pfn_masked_l2_loss_rows(const float* out, const float* y, const void* mask, int mask_dtype, const int32_t* valid, int64_t n_rows,
                            int regularize, float regcoeff, float* loss, float* grad, void* ws, size_t ws_bytes, void* stream) {
    PFN_CHECK_ARG(loss && ws && (n_rows == 0 || (out && y && mask && valid)), "pfn_masked_l2_loss_rows: null pointer");
    PFN_CHECK_ARG(mask_dtype == 0 || mask_dtype == 1, "pfn_masked_l2_loss_rows: mask_dtype must be 0 (int64) or 1 (float32)");
    PFN_CHECK_ARG(n_rows >= 0 && n_rows < (1ll << 29), "pfn_masked_l2_loss_rows: bad row count %lld", (long long)n_rows);
    PFN_CHECK_ARG(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(grad)) & 15) == 0,
                  "pfn_masked_l2_loss_rows: out, y and grad must be 16-byte aligned");
    return pfn::launch_loss_rows<true>("masked_l2_loss_rows", out, y, mask, mask_dtype, valid, n_rows, regularize, regcoeff, loss, grad,
                                       ws, ws_bytes, static_cast<hipStream_t>(stream));
}

}  // extern "C"
