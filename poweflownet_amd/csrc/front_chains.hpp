// The arithmetic of the network's 4-wide front, each rule spelled ONCE:
//     me_h = relu(Wa mask + ba)      x0 = x + (Wb me_h + bb)      P = b1 + W1i x0      Q = W1j x0
//     g0   = dP W1i + dQ W1j         dh = [me_h > 0] (g0 Wb)
// Several kernels compute these -- front.hip's bodies, ea_seg.hip's front_seg_fwd_kernel, edge.hip's FLY walks -- and the loss
// tails, the gate export, the saved ReLU gates and hipGraph replay rest on all of them producing the SAME BITS.  A kernel keeps its
// own thread mapping, staging and summation tree; the per-element operand order lives here.  Every function is one fma per term,
// terms in ascending feature order, so whoever calls it with the same operands gets the same bits (fma's product commutes: which
// factor a call site names first does not matter).
#pragma once
#include "device_prims.hpp"

namespace pfn {

// ------------------------------------------------------------------------------------ pred_mask rows
// pred_mask.float() (networks/MPN.py:533) as the caller holds it -- dtype 0: int64, 1: float32.  One element / one row of four.
__device__ __forceinline__ float mask_elem(const void* m, int dtype, int64_t i) {
    return dtype == 0 ? (float)static_cast<const int64_t*>(m)[i] : static_cast<const float*>(m)[i];
}
__device__ __forceinline__ float4 mask_row4(const void* m, int dtype, int64_t r) {
    if (dtype == 0) {
        const int64_t* p = static_cast<const int64_t*>(m) + 4 * r;
        return make_float4((float)p[0], (float)p[1], (float)p[2], (float)p[3]);
    }
    return ld4(static_cast<const float*>(m) + 4 * r);
}

// --------------------------------------------------------------------- a thread's slice of the weights
// Hidden unit u of a thread whose chunk may reach past H (or whose lane is idle): the loads are UNCONDITIONAL, from the clamped
// unit uc = unit_clamp(u, h), and zeroed by a select afterwards -- `ok ? load : 0` compiles to an exec-masked branch with an
// immediate wait per load (72 serialized round trips to L2 in the forward front, 40 us).  Zero past H: the pad units then come out
// as, and contribute, exact zeros.  row4: w[0..3] of a row-major weight row (Wa[u], W1[u] + 0 / + 4; element loads, a W1 row is
// not 16-byte aligned); col4: w[f * h + uc], f = 0..3 (Wb's column u).  (Load and select alternate, in a loop: with the four loads
// written out ahead of the four selects hipcc no longer paired the block body's fmas -- 16 v_pk_fma_f32 became 32 scalar ones.)
__device__ __forceinline__ int unit_clamp(int u, int h) { return min(u, h - 1); }
__device__ __forceinline__ float unit_val(const float* b, int uc, bool ok) {
    const float v = b[uc];
    return ok ? v : 0.f;
}
__device__ __forceinline__ float4 unit_row4(const float* w, bool ok) {
    float v[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const float x = w[f];
        v[f] = ok ? x : 0.f;
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ float4 unit_col4(const float* w, int h, int uc, bool ok) {
    float v[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const float x = w[(size_t)f * h + uc];
        v[f] = ok ? x : 0.f;
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}

// ------------------------------------------------------------------------------------------ the chains
// acc + w . x over the four features, f ascending, one fma per term: THE chain of the front
__device__ __forceinline__ float chain4(float4 w, float4 x, float acc) {
    acc = fmaf(w.x, x.x, acc);
    acc = fmaf(w.y, x.y, acc);
    acc = fmaf(w.z, x.z, acc);
    return fmaf(w.w, x.w, acc);
}
// four units at once from TRANSPOSED weights (wf = feature f's weights of the four units): chain4 per component, the factors of
// each product swapped -- fma(a, b, c) is fma(b, a, c)
__device__ __forceinline__ float4 chain4_t(float4 x, float4 w0, float4 w1, float4 w2, float4 w3, float4 acc) {
    acc = fma4(x.x, w0, acc);
    acc = fma4(x.y, w1, acc);
    acc = fma4(x.z, w2, acc);
    return fma4(x.w, w3, acc);
}
// mask_embd's hidden unit: relu(ba + Wa[u] . m)
__device__ __forceinline__ float me_unit(float4 wa, float ba, float4 m) { return relu1(chain4(wa, m, ba)); }
// ... and its step into the row's Wb me_h (wb = Wb[0..3][u]); a chunk of four units is a chain of these from zero
__device__ __forceinline__ float4 wb_step(float4 acc, float4 wb, float v) { return fma4(v, wb, acc); }
// the residual, in this association: s = the row's summed Wb me_h
__device__ __forceinline__ float4 x0_row(float4 x, float4 s, float4 bb) {
    return make_float4(x.x + (s.x + bb.x), x.y + (s.y + bb.y), x.z + (s.z + bb.z), x.w + (s.w + bb.w));
}
// the first EdgeAggregation layer's unit u: p = b1 + W1[u][0:4] . x0, q = W1[u][4:8] . x0
__device__ __forceinline__ void pq_unit(float4 w1i, float4 w1j, float b1, float4 x0, float& p, float& q) {
    p = chain4(w1i, x0, b1);
    q = chain4(w1j, x0, 0.f);
}
// backward: unit u's step into the chunk's share of g0 -- dP's four terms, then dQ's
__device__ __forceinline__ float4 g0_step(float4 acc, float p, float q, float4 w1i, float4 w1j) { return fma4(q, w1j, fma4(p, w1i, acc)); }
// ... and one element of dh: (g0 . Wb[0..3][u]) where the hidden unit y was on
__device__ __forceinline__ float dh_unit(float4 g, float4 wb, float y) { return gate1(y, chain4(g, wb, 0.f)); }

// ------------------------------------------------------------------------------------------ the row sum
// Sum of a row's nchunk float4 partials in a FIXED order, in two levels (a single thread walking all 33 was a chain of 33
// dependent LDS reads, ~1 us per row group): lanes c < 8 each add the partials c, c + 8, c + 16, ... in that order, then lane 0
// adds the eight sub-sums in lane order.  Called by every thread of the block (two barriers inside); result in part[r * nchunk].
// LDS_ONLY: the two barriers are lds_barrier() (device_prims.hpp: for a kernel that keeps global loads in flight across them).
template <bool LDS_ONLY = false>
__device__ __forceinline__ void row_sum(float4* part, int r, int c, int nchunk, bool on) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (on && c < 8) {
        for (int k = c; k < nchunk; k += 8) {
            const float4 p = part[r * nchunk + k];
            s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
        }
    }
    if (LDS_ONLY) lds_barrier(); else __syncthreads();
    if (on && c < 8) part[r * nchunk + c] = s;
    if (LDS_ONLY) lds_barrier(); else __syncthreads();
    if (on && c == 0) {
        float4 t = part[r * nchunk];
        const int m = nchunk < 8 ? nchunk : 8;
        for (int k = 1; k < m; ++k) {
            const float4 p = part[r * nchunk + k];
            t.x += p.x; t.y += p.y; t.z += p.z; t.w += p.w;
        }
        part[r * nchunk] = t;
    }
}

}  // namespace pfn
