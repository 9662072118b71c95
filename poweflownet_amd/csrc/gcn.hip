// PyG GCNConv(in, out) with its defaults on the CSR adjacency of pfn_graph_build mode 0 (gfx950): the layer of the reference's GCN
// baseline (networks/GCN.py:8-19).
//
//   out = A_gcn X W^T + b,   A_gcn = D~^-1/2 (A' + I) D~^-1/2
//
// A' = the stored list without its self edges (add_remaining_self_loops), parallel lines kept once each, every node one unit self
// loop, d_i = 1 + #{stored e: dst(e) = i, src(e) != i}.  launch_hop (edge.hip) walks the same CSR but weighs with the graph
// workspace's deg^-1/2 (multiplicity of the UNDIRECTED model adjacency, 0 on isolated nodes) and has no self term; the walk here has
// its own d~^-1/2 -- kept in the LAYER's workspace: the graph workspace is shared by every layer over the batch and is never written
// by a layer call -- skips self edges and adds the self term.  Work item = (node row, float4 column), rows summed by one lane in
// edge-id order like hop_kernel: no float atomics, the same call gives the same bits.
//
// The aggregation acts on rows, the Linear on columns, so they commute: the layer aggregates on whichever side is NARROWER
// (padded widths): cin <= cout: (A_gcn X) W^T with bias and ReLU in the GEMM's epilogue; else A_gcn (X W^T) with bias / ReLU in
// the walk's epilogue.  The backward mirrors it with the by-source CSR (A_gcn^T).
#include <string.h>

#include <algorithm>

#include "pfn_internal.hpp"

namespace pfn {

// ------------------------------------------------------------------------------------------ d~^-1/2
__global__ __launch_bounds__(256) void gcn_dis_kernel(int n, const int* __restrict__ rowptr_in, const int* __restrict__ in_src,
                                                      float* __restrict__ dis) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const int beg = rowptr_in[row], end = rowptr_in[row + 1];
    int d = 1;                                    // the unit self loop: d >= 1, so dis is never 0 or inf
    for (int p = beg; p < end; ++p) d += in_src[p] != row ? 1 : 0;
    dis[row] = 1.0f / sqrtf((float)d);
}

// ------------------------------------------------------------------------------------------ the walk
// bytes of four gate decisions <-> one dword (byte i = column 4c + i; 1 = on)
__device__ __forceinline__ unsigned gate_dword(float4 v) {
    return (relu_on(v.x) ? 1u : 0u) | (relu_on(v.y) ? 0x100u : 0u) | (relu_on(v.z) ? 0x10000u : 0u) | (relu_on(v.w) ? 0x1000000u : 0u);
}
__device__ __forceinline__ float4 gate_apply(unsigned m, float4 g) {   // g where the byte is set, else 0 (a select: NaN stays NaN)
    return make_float4((m & 0xffu) ? g.x : 0.f, (m & 0xff00u) ? g.y : 0.f, (m & 0xff0000u) ? g.z : 0.f, (m & 0xff000000u) ? g.w : 0.f);
}

struct GcnWalkArgs {
    const int* rowptr;          // by destination (forward) or by source (backward: A_gcn^T)
    const int* nbr;
    const float* dis;
    const float* v;             // [n][ld] rows that are gathered
    float* y;                   // [n][ld]
    const float* bias;          // forward epilogue, or null
    unsigned* gate_out;         // forward epilogue with ReLU: the decisions, [n][ld] bytes
    const unsigned* gate_in;    // backward: v rows are taken through these decisions on the way in, or null
    float* gated_self;          // backward, optional: [n][ld] the row's own gated v (what the bias gradient sums)
    int n, ld, ncols, relu;
};

// y[i] = dis_i * ( sum_{p in row i, nbr(p) != i} dis_nbr * v[nbr] + dis_i * v[i] )  (+ bias, ReLU)
template <bool GATE_IN>
__global__ __launch_bounds__(256) void gcn_aggregate_kernel(GcnWalkArgs a) {
    const int nchunk = a.ld >> 2;
    const long item = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int row = (int)(item / nchunk);
    if (row >= a.n) return;
    const int chunk = (int)(item - (long)row * nchunk), col = chunk * 4;
    const int beg = a.rowptr[row], end = a.rowptr[row + 1];
    const float di = a.dis[row];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    // four slots per trip, four gathers in flight (see hop_kernel): a slot past the row's end re-reads the last edge; it and a
    // self edge are dropped by a SELECT, never by a zero weight, so a NaN row reaches exactly its neighbours
    for (int p = beg; p < end; p += 4) {
        const int last = end - 1;
        const int s0 = a.nbr[p], s1 = a.nbr[min(p + 1, last)], s2 = a.nbr[min(p + 2, last)], s3 = a.nbr[min(p + 3, last)];
        float4 v0 = ld4(a.v + (size_t)s0 * a.ld + col), v1 = ld4(a.v + (size_t)s1 * a.ld + col);
        float4 v2 = ld4(a.v + (size_t)s2 * a.ld + col), v3 = ld4(a.v + (size_t)s3 * a.ld + col);
        if (GATE_IN) {
            v0 = gate_apply(a.gate_in[(size_t)s0 * nchunk + chunk], v0);
            v1 = gate_apply(a.gate_in[(size_t)s1 * nchunk + chunk], v1);
            v2 = gate_apply(a.gate_in[(size_t)s2 * nchunk + chunk], v2);
            v3 = gate_apply(a.gate_in[(size_t)s3 * nchunk + chunk], v3);
        }
        const float w0 = a.dis[s0], w1 = a.dis[s1], w2 = a.dis[s2], w3 = a.dis[s3];
        const bool k0 = s0 != row, k1 = p + 1 < end && s1 != row, k2 = p + 2 < end && s2 != row, k3 = p + 3 < end && s3 != row;
        acc = sel4(k0, fma4(w0, v0, acc), acc);
        acc = sel4(k1, fma4(w1, v1, acc), acc);
        acc = sel4(k2, fma4(w2, v2, acc), acc);
        acc = sel4(k3, fma4(w3, v3, acc), acc);
    }
    const size_t o = (size_t)row * a.ld + col;
    float4 self = ld4(a.v + o);
    if (GATE_IN) {
        self = gate_apply(a.gate_in[(size_t)row * nchunk + chunk], self);
        if (a.gated_self) st4(a.gated_self + o, self);
    }
    acc = mul4(di, fma4(di, self, acc));
    if (a.bias) {
        acc.x += col + 0 < a.ncols ? a.bias[col + 0] : 0.f;
        acc.y += col + 1 < a.ncols ? a.bias[col + 1] : 0.f;
        acc.z += col + 2 < a.ncols ? a.bias[col + 2] : 0.f;
        acc.w += col + 3 < a.ncols ? a.bias[col + 3] : 0.f;
    }
    if (a.relu) {
        a.gate_out[(size_t)row * nchunk + chunk] = gate_dword(acc);
        acc = make_float4(relu1(acc.x), relu1(acc.y), relu1(acc.z), relu1(acc.w));
    }
    st4(a.y + o, acc);
}

// the rows of a ReLU output -> gate bytes (mode 0: the GEMM's epilogue took the decisions; a unit is on iff its output is > 0 or
// NaN), or rows taken through saved gate bytes (mode 1: the gated grad_out the GEMM-side backward multiplies)
__global__ __launch_bounds__(256) void gcn_gate_rows_kernel(long nitem, const float* __restrict__ src, unsigned* __restrict__ gate_out,
                                                            const unsigned* __restrict__ gate_in, float* __restrict__ dst) {
    const long item = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= nitem) return;
    const float4 v = ld4(src + item * 4);
    if (gate_out) gate_out[item] = gate_dword(v);
    if (dst) st4(dst + item * 4, gate_apply(gate_in[item], v));
}

static int launch_gcn_walk(const GraphView& g, GcnWalkArgs a, int transpose, hipStream_t s) {
    if (g.n == 0) return PFN_OK;
    a.rowptr = transpose ? g.rowptr_out : g.rowptr_in;
    a.nbr = transpose ? g.out_dst : g.in_src;
    a.n = g.n;
    const long items = (long)g.n * (a.ld / 4);
    const int blocks = (int)((items + 255) / 256);
    ProfScope ps("gcn_aggregate", 0.0, 0.0, s);
    if (a.gate_in)
        gcn_aggregate_kernel<true><<<blocks, 256, 0, s>>>(a);
    else
        gcn_aggregate_kernel<false><<<blocks, 256, 0, s>>>(a);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}
static int launch_gcn_gate_rows(int64_t n, int ld, const float* src, unsigned* gate_out, const unsigned* gate_in, float* dst,
                                hipStream_t s) {
    const long items = (long)n * (ld / 4);
    if (items == 0) return PFN_OK;
    gcn_gate_rows_kernel<<<(int)((items + 255) / 256), 256, 0, s>>>(items, src, gate_out, gate_in, dst);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

// ------------------------------------------------------------------------------------------ the layer
// The gate bytes come FIRST in the workspace (include/pfn_hip.h says so: the caller may read them).
struct GcnWs {
    unsigned* gates;     // [n][ldo] bytes
    float* dis;          // [n]
    float* wt;           // packed image of W^T: (N x cin) -> (N x cout)
    float* wd;           // packed image of W:   (N x cout) -> (N x cin)
    float* t1;           // forward, kept: A_gcn X [n][ldx] (aggregate first) or X W^T [n][ldo]
    float* t2;           // backward: the gated grad_out [n][ldo]
    float* t3;           // backward: g W [n][ldx] (aggregate first) or A_gcn^T g [n][ldo]
    float* dummy;        // [cout] the product that carries the bias sum where no other pair has the gated grad_out as its A
    ReduceWs red;
    size_t bytes;
};
static bool gcn_aggregate_first(int cin, int cout) { return ld_of(cin) <= ld_of(cout); }
static GcnWs gcn_ws(void* ws, int64_t n, int cin, int cout) {
    Carver cv(ws);
    GcnWs w;
    const int ldx = ld_of(cin), ldo = ld_of(cout);
    const bool af = gcn_aggregate_first(cin, cout);
    w.gates = cv.take<unsigned>((size_t)n * (ldo / 4));
    w.dis = cv.take<float>((size_t)n);
    w.wt = cv.take<float>(packed_floats(cin, ldo));
    w.wd = cv.take<float>(packed_floats(cout, ldx));
    w.t1 = cv.take<float>((size_t)n * (af ? ldx : ldo));
    w.t2 = cv.take<float>((size_t)n * ldo);
    w.t3 = cv.take<float>((size_t)n * (af ? ldx : ldo));
    w.dummy = cv.take<float>((size_t)cout);
    w.red.floats = reduce_ws_floats(n, std::max(cin, cout), std::max(cin, cout), 2);
    w.red.partial = cv.take<float>(w.red.floats);
    w.bytes = cv.off;
    return w;
}

static int gcn_check(const char* who, const void* gws, int64_t n, int64_t e, int cin, int cout, int relu, const void* ws,
                     size_t ws_bytes, size_t need) {
    PFN_CHECK_ARG(gws && ws, "%s: null pointer", who);
    PFN_CHECK_ARG(n >= 0 && e >= 0 && n < (1LL << 31) && e < (1LL << 30), "%s: n_nodes / e_stored out of range", who);
    PFN_CHECK_ARG(cin >= 1 && cout >= 1, "%s: in_channels and out_channels must be >= 1", who);
    PFN_CHECK_ARG(relu == 0 || relu == 1, "%s: relu must be 0 or 1", who);
    if (ws_bytes < need) {
        set_error("%s: workspace too small (%zu bytes, need %zu)", who, ws_bytes, need);
        return PFN_ENOSPACE;
    }
    return PFN_OK;
}

static GemmArgs gcn_gemm(int M, const float* A, int lda, int K, const float* Bp, float* C, int ncols, int ldc) {
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.M = M; a.ncols = ncols; a.ldc = ldc; a.ngroup = 1; a.nterm = 1; a.gate_scale = 1.f; a.bias_group = -1;
    a.C[0] = C;
    a.term[0].A = A; a.term[0].Bp = Bp; a.term[0].lda = lda; a.term[0].K = K; a.term[0].group = 0; a.term[0].cm_rows = 0;
    return a;
}

}  // namespace pfn

using namespace pfn;

extern "C" {

size_t pfn_gcn_conv_workspace_bytes(int64_t n, int64_t e, int cin, int cout) {
    (void)e;
    if (n < 0 || cin < 1 || cout < 1) return 0;
    return gcn_ws(nullptr, n, cin, cout).bytes;
}

int pfn_gcn_conv_forward(const void* gws, int64_t n, int64_t e, int cin, int cout, const float* x, int64_t ldx, const float* weight,
                         const float* bias, int relu, float* out, int64_t ldo, void* ws, size_t ws_bytes, void* stream) {
    PFN_CHECK_ARG(cin >= 1 && cout >= 1 && n >= 0, "pfn_gcn_conv_forward: bad sizes");
    GcnWs w = gcn_ws(ws, n, cin, cout);
    PFN_TRY(gcn_check("pfn_gcn_conv_forward", gws, n, e, cin, cout, relu, ws, ws_bytes, w.bytes));
    PFN_CHECK_ARG(weight && (n == 0 || (x && out)), "pfn_gcn_conv_forward: null pointer");
    PFN_CHECK_ARG(ldx == ld_of(cin) && ldo == ld_of(cout), "pfn_gcn_conv_forward: row strides must be pfn_padded_ld(F)");
    GraphView g = graph_view(const_cast<void*>(gws), n, e);
    hipStream_t s = static_cast<hipStream_t>(stream);
    PackJob jobs[2] = {{weight, w.wt, cin, 0, 0, 1, cin, cout, (int)ldo}, {weight, w.wd, cin, 0, 0, 0, cout, cin, (int)ldx}};
    PFN_TRY(launch_pack(jobs, 2, nullptr, s));
    if (n == 0) return PFN_OK;
    gcn_dis_kernel<<<(int)((n + 255) / 256), 256, 0, s>>>((int)n, g.rowptr_in, g.in_src, w.dis);
    PFN_CHECK_LAUNCH();
    GcnWalkArgs wa{};
    wa.dis = w.dis;
    if (gcn_aggregate_first(cin, cout)) {
        wa.v = x; wa.y = w.t1; wa.ld = (int)ldx; wa.ncols = cin;
        PFN_TRY(launch_gcn_walk(g, wa, 0, s));
        GemmArgs ga = gcn_gemm((int)n, w.t1, (int)ldx, cin, w.wt, out, cout, (int)ldo);
        ga.bias = bias;
        ga.act = relu ? ACT_RELU : ACT_NONE;
        PFN_TRY(launch_gemm_nt(ga, s));
        if (relu) PFN_TRY(launch_gcn_gate_rows(n, (int)ldo, out, w.gates, nullptr, nullptr, s));
        return PFN_OK;
    }
    PFN_TRY(launch_gemm_nt(gcn_gemm((int)n, x, (int)ldx, cin, w.wt, w.t1, cout, (int)ldo), s));
    wa.v = w.t1; wa.y = out; wa.ld = (int)ldo; wa.ncols = cout; wa.bias = bias; wa.relu = relu; wa.gate_out = w.gates;
    return launch_gcn_walk(g, wa, 0, s);
}

int pfn_gcn_conv_backward(const void* gws, int64_t n, int64_t e, int cin, int cout, const float* x, int64_t ldx, const float* weight,
                          const float* gout, int64_t ldgo, int relu, float* gx, int64_t ldgx, float* gw, float* gb, void* ws,
                          size_t ws_bytes, void* stream) {
    PFN_CHECK_ARG(cin >= 1 && cout >= 1 && n >= 0, "pfn_gcn_conv_backward: bad sizes");
    GcnWs w = gcn_ws(ws, n, cin, cout);
    PFN_TRY(gcn_check("pfn_gcn_conv_backward", gws, n, e, cin, cout, relu, ws, ws_bytes, w.bytes));
    PFN_CHECK_ARG(weight && gw && (n == 0 || (x && gout)), "pfn_gcn_conv_backward: null pointer");
    PFN_CHECK_ARG(ldx == ld_of(cin) && ldgo == ld_of(cout) && (!gx || ldgx == ld_of(cin)),
                  "pfn_gcn_conv_backward: row strides must be pfn_padded_ld(F)");
    GraphView g = graph_view(const_cast<void*>(gws), n, e);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int ldo = (int)ldgo;
    // (dis and the packed images were left in `ws` by the forward call)
    TnPair pairs[2];
    int npairs = 1;
    memset(pairs, 0, sizeof(pairs));
    GcnWalkArgs wa{};
    wa.dis = w.dis;
    if (gcn_aggregate_first(cin, cout)) {
        const float* gg = gout;
        if (relu) {
            PFN_TRY(launch_gcn_gate_rows(n, ldo, gout, nullptr, w.gates, w.t2, s));
            gg = w.t2;
        }
        if (gx && n > 0) {
            PFN_TRY(launch_gemm_nt(gcn_gemm((int)n, gg, ldo, cout, w.wd, w.t3, cin, (int)ldx), s));
            wa.v = w.t3; wa.y = gx; wa.ld = (int)ldx; wa.ncols = cin;
            PFN_TRY(launch_gcn_walk(g, wa, 1, s));
        }
        pairs[0].A = gg; pairs[0].lda = ldo; pairs[0].na = cout;
        pairs[0].B = w.t1; pairs[0].ldb = (int)ldx; pairs[0].nb = cin;
        pairs[0].G = gw; pairs[0].ldg = cin; pairs[0].bias_out = gb;
    } else {
        wa.v = gout; wa.y = w.t3; wa.ld = ldo; wa.ncols = cout;
        if (relu) {
            wa.gate_in = w.gates;
            wa.gated_self = gb ? w.t2 : nullptr;
        }
        PFN_TRY(launch_gcn_walk(g, wa, 1, s));
        if (gx && n > 0) PFN_TRY(launch_gemm_nt(gcn_gemm((int)n, w.t3, ldo, cout, w.wd, gx, cin, (int)ldx), s));
        pairs[0].A = w.t3; pairs[0].lda = ldo; pairs[0].na = cout;
        pairs[0].B = x; pairs[0].ldb = (int)ldx; pairs[0].nb = cin;
        pairs[0].G = gw; pairs[0].ldg = cin;
        if (gb) {
            // grad_bias = the column sums of the gated grad_out, which no product of this route has as its A operand: it rides on a
            // (cout x 1) product of its own whose result is dropped
            pairs[1].A = relu ? w.t2 : gout; pairs[1].lda = ldo; pairs[1].na = cout;
            pairs[1].B = x; pairs[1].ldb = (int)ldx; pairs[1].nb = 1;
            pairs[1].G = w.dummy; pairs[1].ldg = 1; pairs[1].bias_out = gb;
            npairs = 2;
        }
    }
    return launch_weight_grads(pairs, npairs, n, w.red, s);
}

}  // extern "C"
