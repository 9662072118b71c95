// Layer and whole-model drivers + the C ABI of libpfn_hip.so (gfx950).
//
// Mirrors, call for call, the dataflow of the reference's MaskEmbdMultiMPN.forward
// (networks/MPN.py:525-559), EdgeAggregation.forward/message (:23-56) and PyG TAGConv.forward
// (call sites :477-484,:545), plus their autograd, as sequences of the HIP kernels in graph.hip /
// edge.hip / gemm.hip.  Nothing here synchronises or allocates: every buffer is carved out of the
// caller's workspace, so a whole training step can be captured into one hipGraph.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "pfn_internal.hpp"

namespace pfn {

static GemmArgs gemm_defaults(int M, int ncols, int ldc) {
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.M = M;
    a.ncols = ncols;
    a.ldc = ldc;
    a.ngroup = 1;
    a.gate_scale = 1.f;
    a.bias_group = -1;
    return a;
}
static GemmTerm term(const float* A, int lda, int K, const float* Bp, int group) {
    GemmTerm t;
    t.A = A; t.Bp = Bp; t.lda = lda; t.K = K; t.group = group; t.cm_rows = 0;
    return t;
}
static TnPair tn_pair(const float* A, int lda, int na, const float* B, int ldb, int nb, float* G, int ldg, int gk0,
                      float* bias_out, const float* bias_rowscale) {
    TnPair p;
    p.A = A; p.B = B; p.G = G; p.bias_out = bias_out; p.bias_rowscale = bias_rowscale;
    p.lda = lda; p.ldb = ldb; p.na = na; p.nb = nb; p.ldg = ldg; p.gn0 = 0; p.gk0 = gk0; p.b_cm_rows = 0; p.a_cm_rows = 0;
    return p;
}

// Collects the weight re-layout jobs of a forward pass (gemm_nt.hip: pack) and hands out the packed addresses.
// With base == nullptr it only measures.
struct Packer {
    float* base;
    size_t off = 0;
    std::vector<PackJob> jobs;
    explicit Packer(float* b) : base(b) {}
    // B[k][n] = trans ? W[(wn0+n)*ldw + wk0+k] : W[(wk0+k)*ldw + wn0+n],  k < K, n < ncols, for an output of ld_out columns
    const float* add(const float* W, int ldw, int trans, int wk0, int wn0, int K, int ncols, int ld_out) {
        float* dst = base ? base + off : nullptr;
        off += packed_floats(K, ld_out);
        PackJob j;
        j.src = W; j.dst = dst; j.ldw = ldw; j.wk0 = wk0; j.wn0 = wn0; j.trans = trans; j.K = K; j.ncols = ncols;
        j.ld_out = ld_out;
        jobs.push_back(j);
        return dst ? dst : reinterpret_cast<const float*>(0x10);   // non-null sentinel while measuring
    }
    int flush(hipStream_t s, uint64_t* rng_advance = nullptr, const void* mask = nullptr, int mask_dtype = 0,
              float* maskf = nullptr, int64_t mask_count = 0, const SlotEa* slot_ea = nullptr, int* stamp = nullptr,
              int stamp_value = 0) {
        return launch_pack(jobs.data(), (int)jobs.size(), rng_advance, s, mask, mask_dtype, maskf, mask_count, slot_ea, stamp, stamp_value);
    }
};

struct Act {
    int act = ACT_NONE;
    float p = 0.f;
    const uint64_t* rng = nullptr;
    uint32_t stream = 0;
    int out_cm = 0;             // > 0: the layer output is written CHUNK-major with that many rows per plane (its only reader chain
                                // is a TAGConv on big_graph_hops_kernel: Route::big_cm)
};
struct Gate {
    const float* y = nullptr;   // post-activation output of the producing layer
    int ld = 0;
    float scale = 1.f;
    int cm = 0;                 // > 0: y is chunk-major (see Act::out_cm)
};

// ------------------------------------------------------------------------------------ deferred weight gradients
// Weight gradients only feed the optimizer, so no layer's backward waits for them: every layer appends its (dY, X) pairs to
// a list and ONE launch at the end of the backward pass computes all of them (gemm.hip) -- the chip is filled by the whole
// network's dW work at once instead of by 8 small launches competing with the input-gradient chain.  (Round 1 ran them
// per layer on a second stream: measured 1-2 % over no overlap at all, and the sharing slowed the HBM-bound hops 2x.)
// The price is memory: every layer's incoming gradient and dP / dQ stay alive until the end (sized for 288 GB).
struct Deferred {
    std::vector<TnPair> pairs;
    std::vector<DweJob> dwe;     // the dWe partial reductions of the EdgeAggregation layers, one launch for all
};
typedef Deferred PairList;

// ---------------------------------------------------------------------------------- EdgeAggregation
struct EaSaved { float *P, *Q, *S; };
struct EaScratch { float *dS, *dP, *dQ, *dWe; ReduceWs red; float* gea_tmp = nullptr; };
struct EaPack { const float *w1i_t, *w1j_t, *w2_t, *w2_d, *w1i_d, *w1j_d; };

static EaPack ea_pack(Packer& pk, int fi, int fe, int h, int fo, const float* w1, const float* w2) {
    const int ldw1 = 2 * fi + fe, ld = ld_of(h);
    EaPack p;
    p.w1i_t = pk.add(w1, ldw1, 1, 0, 0, fi, h, ld);           // x (N x Fi) -> P
    p.w1j_t = pk.add(w1, ldw1, 1, fi, 0, fi, h, ld);          // x -> Q
    p.w2_t = pk.add(w2, h, 1, 0, 0, h, fo, ld_of(fo));        // S (N x H) -> out
    p.w2_d = pk.add(w2, h, 0, 0, 0, fo, h, ld);               // gout (N x Fo) -> dS
    p.w1i_d = pk.add(w1, ldw1, 0, 0, 0, h, fi, ld_of(fi));    // dP (N x H) -> dx
    p.w1j_d = pk.add(w1, ldw1, 0, 0, fi, h, fi, ld_of(fi));   // dQ -> dx
    return p;
}

static bool back_fused_ok() {
    static const bool off = diag_env("PFN_NO_FUSED_BACK") != nullptr;   // A/B switch: the last layer's fused kernels
    return !off;
}

// What a whole model decides for one EdgeAggregation layer (model_forward, from its Route); a single layer runs on the defaults.
struct EaFwdOpts {
    int seg = 0;                         // nodes per graph (pfn_graph_segments), 0: unknown
    bool back_fused = back_fused_ok();   // (a model passes Route::back_fused: the same switch)
    bool pq_ready = false;               // layer 0: P | Q already written by the fused front
    bool pq_fly = false;                 // layer 0: P | Q not written, the walk forms them from x0 (Route::l0_fly)
    bool walk_done = false;              // layer 0 behind front_seg_fwd_kernel -- P, Q AND S are already written (ea_seg.hip)
    const float* ea_in = nullptr;        // slot-ordered edge attributes: the layer runs graph-resident in LDS (Route::ea_seg_fwd)
    unsigned* relu_mask = nullptr;       // the generic walk saves its ReLU masks here (Route::saves_mask)
    unsigned* seg_gates = nullptr;       // the graph-resident walk saves its ReLU gates here and writes no P | Q (Route::seg_gates)
    float* hop_xk = nullptr;             // the TAGConv behind this layer takes its hop_K hops from here (seg_lin_hops.hip: the S W2^T
    int hop_K = 0;                       // Linear and the hops in one launch, Route::slh_fwd)
};

static int ea_forward(const GraphView& g, int fi, int fe, int h, int fo, const float* x, int ldx, const float* ea,
                      const float* w1, const float* b1, const float* w2, const float* b2, const EaPack& pw, float* out, int ldo,
                      const Act& act, const EaSaved& sv, hipStream_t s, const EaFwdOpts& o) {
    const int ld = ld_of(h), seg = o.seg;
    // batches of small graphs: the P | Q GEMM and the edge walk in one launch, graph-resident in LDS (ea_seg.hip)
    const bool seg_walk = !o.pq_ready && o.ea_in;
    if (seg_walk) {
        EaSegFwdArgs e{x, pw.w1i_t, pw.w1j_t, b1, w1, o.ea_in, sv.P, sv.Q, sv.S, ldx, fi, ld, h, fi};
        e.gates = o.seg_gates;
        PFN_TRY(launch_ea_seg_fwd(g, e, seg, s));
    } else if (!o.pq_ready) {   // P = x W1[:, :Fi]^T + b1 ; Q = x W1[:, Fi:2Fi]^T   (layer 0: already written by the fused front)
        GemmArgs a = gemm_defaults(g.n, h, ld);
        a.ngroup = 2;
        a.C[0] = sv.P;
        a.C[1] = sv.Q;
        a.nterm = 2;
        a.term[0] = term(x, ldx, fi, pw.w1i_t, 0);
        a.term[1] = term(x, ldx, fi, pw.w1j_t, 1);
        a.bias = b1;
        a.bias_group = 0;
        PFN_TRY(launch_gemm_nt(a, s));
    }
    // the network's last layer (Fo <= 4, no activation): the second Linear rides in the edge walk's launch (edge_fwd_out_kernel)
    const bool out_in_walk = !seg_walk && !o.walk_done && w2 && act.act == ACT_NONE && edge_fwd_out_ok(fe, h, fo, ldo) && o.back_fused;
    if (!seg_walk && !o.walk_done) {
        EdgeFwdArgs e{sv.P, sv.Q, ea, w1, sv.S, ld, h, fi, fe};
        e.mask = o.relu_mask;   // (a backward pass will follow: it reads the masks instead of recomputing the pre-activations)
        e.seg = seg;
        if (o.pq_fly) {
            e.P = e.Q = nullptr;
            e.x0 = x;
            e.b1 = b1;
        }
        if (out_in_walk) {
            e.out = out;
            e.w2 = w2;
            e.b2 = b2;
            e.fo = fo;
        }
        PFN_TRY(launch_edge_fwd(g, e, s));
    }
    if (!out_in_walk && w2 && act.act == ACT_NONE && lin_out4_ok(h, fo, ldo, g.n)) {
        // the last layer at small batches: one row per wave.  out == nullptr: deferred -- pfn_mpn_backward_mse forms the rows in its
        // first launch (Route::mse_tail)
        if (out) PFN_TRY(launch_lin_out4(g.n, h, fo, sv.S, w2, b2, g.deg, out, s));
    } else if (!out_in_walk && o.hop_xk) {   // out = act(S W2^T + deg * b2) and the next TAGConv's K hops over it, one launch
        SegLinHopsArgs f;
        memset(&f, 0, sizeof(f));
        f.A0 = sv.S; f.B0 = pw.w2_t; f.rowscale = g.deg; f.rowbias = b2; f.rng = act.rng; f.rng_stream = act.stream;
        f.y = out; f.xk = o.hop_xk; f.stride = (size_t)g.n * ldo; f.gate_scale = 1.f; f.p_drop = act.p; f.act = act.act;
        f.lda = ld; f.K = h; f.ld = ldo; f.ncols = fo; f.nhops = o.hop_K; f.adjt = 0;
        PFN_TRY(launch_seg_lin_hops(g, f, seg, s));
    } else if (!out_in_walk) {   // out = S W2^T + deg * b2   (the second Linear commutes with the segment sum)
        GemmArgs a = gemm_defaults(g.n, fo, ldo);
        a.C[0] = out;
        a.nterm = 1;
        a.term[0] = term(sv.S, ld, h, pw.w2_t, 0);
        a.rowscale = g.deg;
        a.rowbias = b2;
        a.act = act.act;
        a.p_drop = act.p;
        a.rng = act.rng;
        a.rng_stream = act.stream;
        a.c_cm_rows = act.out_cm;
        PFN_TRY(launch_gemm_nt(a, s));
    } else if (act.out_cm) {
        set_error("EdgeAggregation: a chunk-major output needs the S W2^T GEMM (internal)");
        return PFN_EINVAL;
    }
    return PFN_OK;
}

struct EaBwdOpts {
    int seg = 0;
    bool back_fused = back_fused_ok();       // (a model passes Route::back_fused: the same switch)
    const float* ea_in = nullptr;            // both set: the layer runs graph-resident in LDS (Route::ea_seg_bwd, no edge-attribute
    const float* ea_out = nullptr;           // gradient asked for)
    const unsigned* relu_mask = nullptr;     // written by this layer's generic forward walk (Route::saves_mask): read instead of P | Q
    const unsigned* seg_gates = nullptr;     // written by this layer's graph-resident forward walk (Route::seg_gates), read by the
                                             // graph-resident backward instead of P | Q
    int gx_cm = 0;                           // > 0: gx is written chunk-major (Route::big_cm)
    float* hop_out = nullptr;                // gx is the output gradient of a TAGConv whose backward hops it hop_K times over A_hat^T
    int hop_K = 0;                           // first: the dx Linear and those hops in one launch (seg_lin_hops.hip, Route::slh_bwd)
    const MseTail* mse = nullptr;            // `gout` is not written yet -- the graph-resident launch forms out, the loss and gout itself
};

static int ea_backward(const GraphView& g, int fi, int fe, int h, int fo, const float* x, int ldx, const float* ea,
                       const float* w1, const float* w2, const EaPack& pw, const float* gout, int ldgo, const Gate& gate, float* gx,
                       int ldgx, float* gw1, float* gb1, float* gw2, float* gb2, float* gea, const EaSaved& sv,
                       const EaScratch& sc, hipStream_t s, PairList* defer, const EaBwdOpts& o) {
    const int ld = ld_of(h), ldw1 = 2 * fi + fe, seg = o.seg;
    // batches of small graphs: the dS GEMM and both backward walks in one launch, graph-resident in LDS (ea_seg.hip)
    const bool seg_walk = o.ea_in && o.ea_out && (fo > 4 || ldgo == 4);
    if (seg_walk) {
        const bool last = fo <= 4 && ldgo == 4;
        EaSegBwdArgs e{gout, last ? nullptr : pw.w2_d, w2, sv.P, sv.Q, o.ea_in, o.ea_out, w1, sc.dP, sc.dQ, sc.dWe, ldgo, fo, ld, h, fi};
        if (o.mse) e.mse = *o.mse;
        e.gates = o.seg_gates;
        PFN_TRY(launch_ea_seg_bwd(g, e, seg, s));
    } else if (o.mse) {
        set_error("EdgeAggregation backward: the MSELoss tail without the graph-resident launch (internal)");
        return PFN_EINVAL;
    }
    // the network's last layer (Fo <= 4): the walks form dS rows from the 16-byte gout rows themselves (edge.hip ds_row), so
    // the K = 4 GEMM that would write N x H (and the walks' re-read of it) goes away
    const bool ds_in_walk = !seg_walk && w2 && fo <= 4 && ldgo == 4 && !gea && o.back_fused;
    if (!seg_walk && !ds_in_walk) {   // dS = gout W2
        GemmArgs a = gemm_defaults(g.n, h, ld);
        a.C[0] = sc.dS;
        a.nterm = 1;
        a.term[0] = term(gout, ldgo, fo, pw.w2_d, 0);
        PFN_TRY(launch_gemm_nt(a, s));
    }
    EdgeBwdArgs e{sv.P, sv.Q, sc.dS, ea, w1, sc.dP, sc.dQ, sc.dWe, gea, ld, h, fi, fe};
    e.mask = o.relu_mask;
    e.gea_tmp = sc.gea_tmp;
    if (ds_in_walk) {
        e.gout = gout;
        e.w2 = w2;
        e.fo = fo;
    }
    if (!seg_walk) PFN_TRY(launch_edge_bwd(g, e, nullptr, s));
    if (gea) PFN_TRY(launch_edge_attr_grad(g, e, s));
    if (gx && o.hop_out) {
        SegLinHopsArgs f;
        memset(&f, 0, sizeof(f));
        f.A0 = sc.dP; f.A1 = sc.dQ; f.B0 = pw.w1i_d; f.B1 = pw.w1j_d; f.gate = gate.y; f.ldg = gate.ld; f.gate_scale = gate.scale;
        f.y = gx; f.xk = o.hop_out; f.stride = (size_t)g.n * ldgx; f.act = ACT_NONE;
        f.lda = ld; f.K = h; f.ld = ldgx; f.ncols = fi; f.nhops = o.hop_K; f.adjt = 1;
        PFN_TRY(launch_seg_lin_hops(g, f, seg, s));
    } else if (gx) {   // dx = dP W1[:, :Fi] + dQ W1[:, Fi:2Fi], gated by the producing layer's activation
        GemmArgs a = gemm_defaults(g.n, fi, ldgx);
        a.C[0] = gx;
        a.nterm = 2;
        a.term[0] = term(sc.dP, ld, h, pw.w1i_d, 0);
        a.term[1] = term(sc.dQ, ld, h, pw.w1j_d, 0);
        a.gate = gate.y;
        a.ldg = gate.ld;
        a.gate_scale = gate.scale;
        a.aux_cm_rows = gate.cm;
        a.c_cm_rows = o.gx_cm;   // (the gradient handed to a TAGConv on the big-graph hop kernel: chunk-major, like its input)
        PFN_TRY(launch_gemm_nt(a, s));
    }
    // weight gradients: dWe partials -> W1[:, 2Fi:], and three (dY, X) pairs
    const int dwe_blocks = g.n > 0 ? (seg_walk ? ea_seg_blocks(seg, g.n, ld) : edge_bwd_dst_blocks(g, ld)) : 0;
    if (defer) defer->dwe.push_back(DweJob{sc.dWe, gw1, dwe_blocks, ldw1, 2 * fi, 0});
    else PFN_TRY(launch_dwe_reduce(sc.dWe, dwe_blocks, fe, ld, h, gw1, ldw1, 2 * fi, s));
    const TnPair pairs[3] = {
        tn_pair(gout, ldgo, fo, sv.S, ld, h, gw2, h, 0, gb2, g.deg),      // dW2 ; db2 = sum_i deg_i gout_i
        tn_pair(sc.dP, ld, h, x, ldx, fi, gw1, ldw1, 0, gb1, nullptr),    // dW1[:, :Fi] ; db1 = sum_i dP_i
        tn_pair(sc.dQ, ld, h, x, ldx, fi, gw1, ldw1, fi, nullptr, nullptr),
    };
    if (defer) {
        defer->pairs.insert(defer->pairs.end(), pairs, pairs + 3);
        return PFN_OK;
    }
    return launch_weight_grads(pairs, 3, g.n, sc.red, s);
}

// ------------------------------------------------------------------------------------------ TAGConv
struct TagPack { const float* wt[8]; const float* wd[8]; };
static TagPack tag_pack(Packer& pk, int cin, int cout, int K, const float* const* w) {
    TagPack p;
    for (int k = 0; k <= K; ++k) {
        p.wt[k] = pk.add(w[k], cin, 1, 0, 0, cin, cout, ld_of(cout));   // x^(k) (N x cin) -> out
        p.wd[k] = pk.add(w[k], cin, 0, 0, 0, cout, cin, ld_of(cin));    // gout (N x cout) -> G_k
    }
    return p;
}

// Which kernel runs a TAGConv's K hops: the two-tile / row kernels (whole graphs in LDS), big_graph_hops_kernel (CHUNK-major in and
// out) or K generic launches.  Asked once per model step (make_route) or, for a single layer, by its entry point.
enum HopKind { HOPS_NONE = 0, HOPS_FUSED, HOPS_BIG, HOPS_GENERIC };
static HopKind hop_kind(int seg, int ld, int n, int64_t e_stored, int K) {
    if (K > 0 && fused_hops_fit(seg, ld, n)) return HOPS_FUSED;
    if (K > 0 && big_hops_fit(seg, n, e_stored)) return HOPS_BIG;
    return K > 0 ? HOPS_GENERIC : HOPS_NONE;
}
// dst + (k - 1) * stride = A^k src, k = 1..K, A = A_hat (adjt = 0) or A_hat^T (adjt = 1); src (n x ld) is chunk-major when cm_in > 0.
// Returns the rows per plane of the chunk-major hop outputs in cm_out (0: row-major).
static int run_hops(const GraphView& g, HopKind kind, const float* src, float* dst, size_t stride, int ld, int K, int adjt, int seg,
                    int cm_in, int& cm_out, hipStream_t s) {
    cm_out = 0;
    if (kind == HOPS_FUSED || kind == HOPS_BIG) {
        FusedHopsArgs fh{src, dst, nullptr, nullptr, nullptr, 1.f, stride, ld, K, 0, seg, adjt ? 1 : -1};
        if (kind == HOPS_FUSED) return launch_fused_hops(g, fh, s);
        fh.x0_cm = cm_in;
        cm_out = g.n;
        return launch_big_graph_hops(g, fh, s);   // (writes the hop outputs chunk-major)
    }
    for (int k = 1; k <= K; ++k) {
        HopArgs hp{src, nullptr, dst + (size_t)(k - 1) * stride, nullptr, 1.f, ld, 1, adjt};
        PFN_TRY(launch_hop(g, hp, s));
        src = hp.y;
    }
    return PFN_OK;
}

struct TagOpts {
    int seg = 0;
    HopKind hops = HOPS_NONE;    // hop_kind() of this layer and batch (Route::hops)
    int x_cm = 0;                // > 0: x is chunk-major with that many rows per plane (the producing layer wrote it so: Route::big_cm)
    int gout_cm = 0;             // backward: the same for gout
    bool hops_done = false;      // the neighbouring EdgeAggregation's launch already ran the hops (seg_lin_hops.hip, Route::slh_*)
};

static int tag_forward(const GraphView& g, int cin, int cout, int K, const float* x, int ldx, const TagPack& pw,
                       const float* bias, float* out, int ldo, const Act& act, float* xk, hipStream_t s, const TagOpts& o) {
    // xk: K buffers of n * ldx floats holding A_hat^k x, k = 1..K
    const size_t stride = (size_t)g.n * ldx;
    int xk_cm = 0;   // > 0: the hop outputs are chunk-major with that many rows per plane (big-graph hops)
    if (o.x_cm && o.hops != HOPS_BIG) {
        set_error("TAGConv: chunk-major input without the big-graph hop kernel (internal)");
        return PFN_EINVAL;
    }
    if (!o.hops_done) PFN_TRY(run_hops(g, o.hops, x, xk, stride, ldx, K, 0, o.seg, o.x_cm, xk_cm, s));
    GemmArgs a = gemm_defaults(g.n, cout, ldo);
    a.C[0] = out;
    a.nterm = K + 1;
    for (int k = 0; k <= K; ++k) {
        a.term[k] = term(k == 0 ? x : xk + (size_t)(k - 1) * stride, ldx, cin, pw.wt[k], 0);
        a.term[k].cm_rows = k > 0 ? xk_cm : o.x_cm;
    }
    a.bias = bias;
    a.act = act.act;
    a.p_drop = act.p;
    a.rng = act.rng;
    a.rng_stream = act.stream;
    return launch_gemm_nt(a, s);
}

struct TagScratch { float* G; float *z0, *z1; ReduceWs red; };

static int tag_backward(const GraphView& g, int cin, int cout, int K, const float* x, int ldx, const TagPack& pw,
                        const float* gout, int ldgo, const Gate& gate, float* gx, int ldgx, float* const* gw,
                        float* gbias, const float* xk, const TagScratch& sc, hipStream_t s, PairList* defer, const TagOpts& o) {
    // o.hops_done: the layer behind (whose dx Linear produced gout) already hopped it into sc.G
    const size_t stride = (size_t)g.n * ldx;
    const int seg = o.seg, x_cm = o.x_cm, gout_cm = o.gout_cm;
    float* hk = sc.G;
    const HopKind hops = o.hops;   // the forward's hops over x and this pass's over gout: the choice looks at the graphs, not at ld
    if (gout_cm && !(gx && ldgo <= ldx && hops == HOPS_BIG)) {
        set_error("TAGConv backward: chunk-major output gradient without the big-graph hop kernel (internal)");
        return PFN_EINVAL;
    }
    if (gx) {
        if (ldgx != ldx) {
            set_error("TAGConv backward: grad_x stride %d != x stride %d", ldgx, ldx);
            return PFN_EINVAL;
        }
        if (K > 0 && ldgo <= ldx) {
            // dx = sum_k (A^T)^k (gout W_k) = sum_k ((A^T)^k gout) W_k: hop the incoming gradient first (K hops over the
            // transposed adjacency, LDS-resident when the graphs fit), then ONE multi-term GEMM with the gate in its epilogue --
            // one output instead of K + 1 (measured 607 vs 754 us for the GEMM at 414 k nodes) and no Horner pass.
            const size_t gstride = (size_t)g.n * ldgo;
            int hk_cm = 0;
            if (!o.hops_done) PFN_TRY(run_hops(g, hops, gout, hk, gstride, ldgo, K, 1, seg, gout_cm, hk_cm, s));
            GemmArgs a = gemm_defaults(g.n, cin, ldx);
            a.C[0] = gx;
            a.nterm = K + 1;
            for (int k = 0; k <= K; ++k) {
                a.term[k] = term(k == 0 ? gout : hk + (size_t)(k - 1) * gstride, ldgo, cout, pw.wd[k], 0);
                a.term[k].cm_rows = k > 0 ? hk_cm : gout_cm;
            }
            a.gate = gate.y;
            a.ldg = gate.ld;
            a.gate_scale = gate.scale;
            a.aux_cm_rows = gate.cm;
            PFN_TRY(launch_gemm_nt(a, s));
        } else {
            if (gate.cm || x_cm || gout_cm || o.hops_done) {
                set_error("TAGConv backward: chunk-major tensors on the Horner path (internal)");
                return PFN_EINVAL;
            }
            // G_k = gout W_k ; dx = G_0 + A^T (G_1 + A^T (G_2 + ...))   (Horner over the transposed adjacency)
            GemmArgs a = gemm_defaults(g.n, cin, ldx);
            a.ngroup = K + 1;
            a.nterm = K + 1;
            for (int k = 0; k <= K; ++k) {
                a.C[k] = (K == 0) ? gx : sc.G + (size_t)k * stride;
                a.term[k] = term(gout, ldgo, cout, pw.wd[k], k);
            }
            if (K == 0) {
                a.gate = gate.y;
                a.ldg = gate.ld;
                a.gate_scale = gate.scale;
            }
            PFN_TRY(launch_gemm_nt(a, s));
            if (hops == HOPS_FUSED) {   // (the two-tile kernel in its Horner form, else K generic launches)
                FusedHopsArgs fh{nullptr, nullptr, sc.G, gx, gate.y, gate.scale, stride, ldx, K, 1, seg};
                PFN_TRY(launch_fused_hops(g, fh, s));
            } else {
                const float* z = sc.G + (size_t)K * stride;
                for (int k = K - 1; k >= 0; --k) {
                    float* dst = (k == 0) ? gx : ((k & 1) ? sc.z1 : sc.z0);
                    HopArgs hp{z, sc.G + (size_t)k * stride, dst, k == 0 ? gate.y : nullptr, k == 0 ? gate.scale : 1.f, ldx, 1, 1};
                    PFN_TRY(launch_hop(g, hp, s));
                    z = dst;
                }
            }
        }
    }
    // weight gradients need only gout and the saved hops
    std::vector<TnPair> local;
    std::vector<TnPair>& pairs = defer ? defer->pairs : local;
    const int xk_cm = hops == HOPS_BIG ? g.n : 0;   // (what tag_forward's run_hops returned)
    for (int k = 0; k <= K; ++k) {
        pairs.push_back(tn_pair(gout, ldgo, cout, k == 0 ? x : xk + (size_t)(k - 1) * stride, ldx, cin, gw[k], cin, 0,
                                k == 0 ? gbias : nullptr, nullptr));
        pairs.back().b_cm_rows = k > 0 ? xk_cm : x_cm;
        pairs.back().a_cm_rows = gout_cm;
    }
    if (defer) return PFN_OK;
    return launch_weight_grads(local.data(), (int)local.size(), g.n, sc.red, s);
}

// -------------------------------------------------------------------------------------- whole model
struct Layout {
    // dims
    int n, e, f0, fe, fo, h, L, K, ld, ld0, ldo, nlayers;
    int* stamp;                  // guard word: WS_STAMP_TRAIN after a forward that saved what the backward pass reads
    int* mask_counts;            // [1024 row blocks][2]: front_seg_fwd_kernel's mask census (FrontFwdArgs::mask_counts; training only)
    // forward-saved
    float *maskf, *me_h, *x0, *packed;
    float *ea_in, *ea_out;       // edge attributes in CSR slot order (Fe = 2; SlotEa), filled once per forward
    std::vector<unsigned*> relu_mask;   // per EA layer: the edge stage's ReLU masks (EdgeFwdArgs::mask; need_backward)
    size_t packed_floats;
    std::vector<float*> y;       // per layer output (post-activation); last = nullptr (caller's out)
    std::vector<EaSaved> ea;     // per EA layer
    std::vector<float*> xk;      // per TAG layer: K * n * ld
    // backward: per-layer buffers that stay alive until the deferred weight-gradient launch ...
    std::vector<float*> gin;     // gradient w.r.t. the INPUT of layer i (= the incoming gradient of layer i - 1)
    std::vector<float*> dP, dQ, dWe;   // per EA layer
    // ... and scratch shared by all layers
    float* dh;
    EaScratch eas;               // dS, reduction workspace (dP / dQ / dWe are taken from the per-layer buffers)
    TagScratch tags;
    size_t bytes;
};
static bool is_ea(int i) { return (i & 1) == 0; }
static int param_offset(int i, int K) { return (i + 1) / 2 * 4 + i / 2 * (K + 2); }   // layer i's first tensor: E T E T ... E
// The forward pass stamps its workspace (a rider of its first launch): TRAIN when it saved what a backward pass reads
// (need_backward), INFER otherwise.  pfn_mpn_backward hands the word to its weight-gradient launch, which writes every
// parameter gradient as NaN unless it reads TRAIN -- a caller that ran the forward with need_backward = 0 on a training-sized
// workspace (nothing on the host can tell) gets NaN gradients instead of plausible garbage.  Device-side, no host sync.
enum { WS_STAMP_INFER = 0x1f0e4e00, WS_STAMP_TRAIN = 0x7a11e7a1 };

// packed-weight plan of the whole network (identical walk in forward, which fills it, and backward, which reads it)
struct ModelPack {
    std::vector<EaPack> ea;
    std::vector<TagPack> tag;
    const float *wa_t, *wb_t, *wb_d;
};
static void plan_pack(Packer& pk, int f0, int fe, int fo, int h, int L, int K, const float* const* params,
                      ModelPack& mp) {
    const int nlayers = 2 * L - 1;
    mp.ea.assign(nlayers, EaPack{});
    mp.tag.assign(nlayers, TagPack{});
    int pi = 0;
    for (int i = 0; i < nlayers; ++i) {
        if (is_ea(i)) {
            const int fi = i == 0 ? f0 : h, fo_ = (i + 1 == nlayers) ? fo : h;
            mp.ea[i] = ea_pack(pk, fi, fe, h, fo_, params ? params[pi] : nullptr, params ? params[pi + 2] : nullptr);
            pi += 4;
        } else {
            const float* none[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            mp.tag[i] = tag_pack(pk, h, h, K, params ? params + pi : none);
            pi += K + 2;
        }
    }
    const float* wa = params ? params[pi] : nullptr;
    const float* wb = params ? params[pi + 2] : nullptr;
    mp.wa_t = pk.add(wa, f0, 1, 0, 0, f0, h, ld_of(h));      // maskf (N x F0) -> me_h
    mp.wb_t = pk.add(wb, h, 1, 0, 0, h, f0, ld_of(f0));      // me_h (N x H) -> x0
    mp.wb_d = pk.add(wb, h, 0, 0, 0, f0, h, ld_of(h));       // g (N x F0) -> dh
}

static int make_layout(const pfn_mpn_config& c, int64_t n, int64_t e, void* ws, Layout& lo) {
    PFN_CHECK_ARG(c.n_gnn_layers >= 2, "n_gnn_layers must be >= 2 (L == 1 is shape-broken in the reference)");
    PFN_CHECK_ARG(c.K >= 0 && c.K <= 7, "K must be in [0, 7]");
    PFN_CHECK_ARG(c.nfeature_dim > 0 && c.efeature_dim > 0 && c.efeature_dim <= 6 && c.output_dim > 0 && c.hidden_dim > 0,
                  "bad feature dimensions");
    PFN_CHECK_ARG(c.dropout_rate >= 0.f && c.dropout_rate < 1.f, "dropout_rate must be in [0, 1)");
    lo.n = (int)n; lo.e = (int)e;
    lo.f0 = c.nfeature_dim; lo.fe = c.efeature_dim; lo.fo = c.output_dim; lo.h = c.hidden_dim;
    lo.L = c.n_gnn_layers; lo.K = c.K;
    lo.ld = ld_of(lo.h); lo.ld0 = ld_of(lo.f0); lo.ldo = ld_of(lo.fo);
    lo.nlayers = 2 * lo.L - 1;   // E T E T ... E
    Carver cv(ws);
    const size_t nld = (size_t)n * lo.ld;
    {
        Packer measure(nullptr);
        ModelPack mp;
        plan_pack(measure, lo.f0, lo.fe, lo.fo, lo.h, lo.L, lo.K, nullptr, mp);
        lo.packed_floats = measure.off;
    }
    lo.stamp = cv.take<int>(4);
    lo.mask_counts = cv.take<int>(2048);
    lo.packed = cv.take<float>(lo.packed_floats);
    lo.maskf = cv.take<float>((size_t)n * lo.ld0);
    lo.ea_in = cv.take<float>((size_t)4 * e + 4);
    lo.ea_out = cv.take<float>((size_t)4 * e + 4);
    lo.me_h = cv.take<float>(nld);
    lo.x0 = cv.take<float>((size_t)n * lo.ld0);
    lo.y.assign(lo.nlayers, nullptr);
    lo.ea.assign(lo.nlayers, EaSaved{nullptr, nullptr, nullptr});
    lo.xk.assign(lo.nlayers, nullptr);
    for (int i = 0; i < lo.nlayers; ++i) {
        if (i + 1 < lo.nlayers) lo.y[i] = cv.take<float>(nld);
        if (is_ea(i)) {
            lo.ea[i].P = cv.take<float>(nld);
            lo.ea[i].Q = cv.take<float>(nld);
            lo.ea[i].S = cv.take<float>(nld);
        } else {
            lo.xk[i] = cv.take<float>(nld * std::max(1, lo.K));
        }
    }
    lo.gin.assign(lo.nlayers, nullptr);
    lo.dP.assign(lo.nlayers, nullptr);
    lo.dQ.assign(lo.nlayers, nullptr);
    lo.dWe.assign(lo.nlayers, nullptr);
    lo.relu_mask.assign(lo.nlayers, nullptr);
    lo.dh = nullptr;
    lo.eas = EaScratch{nullptr, nullptr, nullptr, nullptr, ReduceWs{nullptr, 0}};
    lo.tags = TagScratch{nullptr, nullptr, nullptr, ReduceWs{nullptr, 0}};
    if (!c.need_backward) {   // inference: none of the backward pass's buffers exist (they were ~2/3 of the footprint)
        lo.bytes = cv.off;
        return PFN_OK;
    }
    for (int i = 0; i < lo.nlayers; ++i) {
        lo.gin[i] = cv.take<float>(i == 0 ? (size_t)n * lo.ld0 : nld);
        if (is_ea(i)) {
            lo.dP[i] = cv.take<float>(nld);
            lo.dQ[i] = cv.take<float>(nld);
            lo.dWe[i] = cv.take<float>((size_t)1025 * lo.fe * lo.ld);
            lo.relu_mask[i] = cv.take<unsigned>(mask_dwords((size_t)n, (size_t)e, lo.ld));
        }
    }
    lo.dh = cv.take<float>(nld);
    lo.eas.dS = cv.take<float>(nld);
    lo.eas.dP = lo.eas.dQ = lo.eas.dWe = nullptr;
    lo.eas.gea_tmp = cv.take<float>((size_t)2 * e * lo.fe);   // (edge-attribute gradients: one slot per edge copy, edge.hip)
    lo.tags.G = cv.take<float>(nld * (lo.K + 1));
    lo.tags.z0 = cv.take<float>(nld);
    lo.tags.z1 = cv.take<float>(nld);
    const int maxf = std::max(std::max(lo.h, lo.f0), lo.fo);
    const size_t red = reduce_ws_floats(n, maxf, maxf, 8);
    lo.eas.red.partial = cv.take<float>(red);
    lo.eas.red.floats = red;
    lo.tags.red = lo.eas.red;
    lo.bytes = cv.off;
    return PFN_OK;
}

// ------------------------------------------------------------------------------------------- route
// Every dispatch decision of a whole-model step, taken ONCE per entry point (open_model) from the model, the batch and the segment
// hint; forward, backward, the loss tails and the gate export read it, so they cannot disagree on what was saved and in which
// layout.  What a call-time argument decides on top (an edge-attribute gradient was asked for) is said in model_backward.
struct Route {
    bool back_fused;      // the last layer's fused kernels (back_fused_ok)
    bool fused_front;     // mask_embd + residual + layer 0's P | Q in one launch (front.hip)
    bool ea_seg_fwd, ea_seg_bwd;   // the EdgeAggregation layers / their backward run graph-resident in LDS (ea_seg.hip); the forward
                                   // fills the slot-ordered edge attributes both read
    bool mask[2];         // does the forward edge walk of layer 0 / of every later layer save its ReLU masks (saves_mask)
    bool l0_fly;          // layer 0's P | Q are not written: its walk forms them from x0 (edge.hip FLY)
    bool meh_recompute;   // mask_embd's hidden layer is not stored: the backward front recomputes it (front_bwd_wg_kernel)
    bool seg_front;       // the front AND layer 0's edge stage in one graph-resident launch (ea_seg.hip front_seg_fwd_kernel)
    bool seg_gates;       // the graph-resident forward walks save their ReLU gates (Layout::relu_mask, the generic walks' layout) and
                          // write no P | Q; the graph-resident backward reads the gates (ea_seg.hip "SAVED GATES")
    bool mse_tail, masked_tail;   // pfn_mpn_backward_mse / pfn_mpn_backward_masked_l2 are available
    HopKind hops;         // the hop kernel of every TAGConv, forward and backward
    int big_cm;           // > 0: a TAGConv's input, its hop buffers and the gradient handed down to it are CHUNK-major, n rows per plane
    bool slh_fwd, slh_bwd;   // seg_lin_hops.hip: an EdgeAggregation's second Linear also runs the hops of the TAGConv behind it (not the
                             // last layer's); its dx Linear the backward hops of the TAGConv in front (layers 2, 4, ...)
    bool saves_mask(int i) const { return mask[i != 0]; }
};

static int make_route(const pfn_mpn_config& c, const Layout& lo, int seg, int64_t e_stored, Route& r) {
    // A/B switches: the front writes P | Q, the walk gathers them; me_h stored, its (dY, X) pairs in gemm_tn; lin_out4 + mse_kernel
    static const bool no_fly = diag_env("PFN_NO_L0_FLY") != nullptr, store_meh = diag_env("PFN_FRONT_STORE_MEH") != nullptr,
                      no_tail = diag_env("PFN_NO_MSE_TAIL") != nullptr, no_gates = diag_env("PFN_NO_SEG_GATES") != nullptr;
    const bool train = c.need_backward != 0, out4 = lin_out4_ok(lo.h, lo.fo, lo.ldo, lo.n);
    r.back_fused = back_fused_ok();
    r.fused_front = front_fused_ok(lo.f0, lo.h);
    r.ea_seg_fwd = ea_seg_fit(seg, lo.n, lo.fe, lo.ld, false);
    r.ea_seg_bwd = ea_seg_fit(seg, lo.n, lo.fe, lo.ld, true);
    // ... and the LAST layer's dS product, whose k extent is output_dim, must be one piece (roundup8(fo) <= 8 * SG_NCH = 136): a wider
    // output takes the generic backward behind the graph-resident forward, the pairing of a batch beyond the backward's 1,024 blocks
    if (!ea_seg_bwd_out_ok(lo.fo)) r.ea_seg_bwd = false;
    // ReLU masks are saved BY THE GENERIC WALK when a backward pass was announced, Fe = 2, the layer's forward walk is the generic one
    // and so are the backward walks (the graph-resident walks save and read theirs under seg_gates, below -- or recompute from P | Q)
    for (int i = 0; i < 2; ++i) {
        const bool generic_fwd = !r.ea_seg_fwd || (r.fused_front && i == 0);
        r.mask[i] = train && lo.fe == 2 && generic_fwd && !r.ea_seg_bwd;
    }
    // Layer 0 on the fly, beyond the latency regime, when nothing later reads P | Q from memory: inference, or a training pass whose
    // backward walks read the saved masks.  (An edge-attribute gradient and the gate export write the rows then: launch_front_pq.)
    r.l0_fly = !no_fly && r.fused_front && lo.nlayers > 1 && lo.fe == 2 && lo.f0 == 4 && !front_latency_regime(lo.h, lo.n) &&
               (!train || r.mask[0]);
    // ... in training me_h is not stored either: neither me_h nor dh touches memory and two N x H pairs leave the weight-gradient
    // launch (the partial sums live in the unused me_h buffer; the gate export writes me_h first)
    r.meh_recompute = !store_meh && train && r.l0_fly && front_bwd_wg_scratch_floats(lo.n, lo.h) <= (size_t)lo.n * lo.ld;
    r.seg_front = r.fused_front && r.ea_seg_fwd && !r.l0_fly && lo.nlayers > 1 &&
                  front_seg_fit(seg, lo.n, lo.h, lo.fe) && !(train && lo.fe == 2 && !r.ea_seg_bwd);
    // Saved gates: a training step whose EVERY EdgeAggregation runs graph-resident forward and backward (layer 0 behind
    // front_seg_fwd_kernel, or -- no fused front -- through ea_seg_fwd_kernel like the others) keeps P | Q in LDS.  What is decided
    // after the forward and reads P | Q from memory (an edge-attribute gradient, the gate export) writes them first: rewrite_pq.
    r.seg_gates = !no_gates && train && lo.fe == 2 && r.ea_seg_fwd && r.ea_seg_bwd && (r.seg_front || !r.fused_front);
    // The loss tails: the last layer's backward is the graph-resident launch in its last-layer form, the out rows lin_out4_wave_kernel's
    r.mse_tail = !no_tail && train && lo.n > 0 && lo.nlayers > 1 && lo.fe == 2 && lo.fo == 4 && lo.ldo == 4 &&
                 out4 && r.back_fused && r.ea_seg_fwd && r.ea_seg_bwd && lo.ld / 4 <= 34;
    r.masked_tail = r.mse_tail && r.seg_front;   // (the front launch that leaves the mask census behind)
    r.hops = hop_kind(seg, lo.ld, lo.n, e_stored, lo.K);
    r.big_cm = tag_input_cm(seg, lo.ld, lo.n, e_stored, lo.K) ? lo.n : 0;
    r.slh_fwd = !r.big_cm && seg_lin_hops_fit(seg, lo.n, lo.ld, lo.h, lo.h, lo.K, 1);
    r.slh_bwd = !r.big_cm && seg_lin_hops_fit(seg, lo.n, lo.ld, lo.h, lo.h, lo.K, 2);
    // What the passes take for granted of each other (implied by the above; tests/test_host.py sweeps the restatement): the backward
    // reads the forward's slot-ordered attributes; front_seg_fwd_kernel writes no ReLU masks, so never where layer 0's backward would
    // read them; the fly / recompute chain; the tails' launches; the hop kernel behind the seg_lin_hops launches and the layouts
    const bool sound = (!r.ea_seg_bwd || r.ea_seg_fwd) && (!r.seg_front || !r.mask[0]) &&
                       (!r.l0_fly || (r.fused_front && !r.seg_front)) && (!r.meh_recompute || r.l0_fly) &&
                       (!r.mse_tail || (r.ea_seg_fwd && r.ea_seg_bwd && out4)) &&
                       (!(r.slh_fwd || r.slh_bwd) || (r.hops == HOPS_FUSED && !r.big_cm)) && (!r.big_cm || r.hops == HOPS_BIG) &&
                       // saved gates: no layer's walk is a generic one (none saves masks into the same buffer, none needs P | Q)
                       (!r.seg_gates || (train && r.ea_seg_fwd && r.ea_seg_bwd && !r.mask[0] && !r.mask[1] && !r.l0_fly &&
                                         (r.seg_front || !r.fused_front)));
    if (!sound) {
        set_error("model route: the dispatch decisions contradict each other (internal)");
        return PFN_EINVAL;
    }
    return PFN_OK;
}

// A model entry point's view of its arguments (open_model); seg: nodes per graph, 0 where seg_nodes is no positive divisor of n
struct ModelCall { Layout lo; GraphView g; Route r; int seg; };

static int model_forward(const pfn_mpn_config& c, const ModelCall& m, const float* const* params, const float* x,
                         const void* pred_mask, int mask_dtype, const float* edge_attr, float* out, uint64_t* rng, hipStream_t s) {
    const GraphView& g = m.g;
    const Layout& lo = m.lo;
    const Route& r = m.r;
    const bool drop = c.training && c.dropout_rate > 0.f;
    PFN_CHECK_ARG(!drop || rng != nullptr, "training with dropout needs rng_state");
    const int nparams = pfn_mpn_num_params(&c);
    const float* const* me = params + (nparams - 4);   // Wa, ba, Wb, bb
    // every weight -> its packed LDS images (both orientations; backward reuses them)
    Packer pk(lo.packed);
    ModelPack mp;
    plan_pack(pk, lo.f0, lo.fe, lo.fo, lo.h, lo.L, lo.K, params, mp);
    // batches of small graphs (ea_seg.hip): the edge attributes go to CSR slot order once, riding in the pack launch
    SlotEa se;
    if (r.ea_seg_fwd) {
        se.rowptr_in = g.rowptr_in; se.in_eid = g.in_eid; se.out_eid = g.out_eid; se.ea = edge_attr;
        se.ea_in = lo.ea_in; se.ea_out = lo.ea_out; se.n = g.n; se.e_stored = g.e_stored;
    }
    // mask_embd(mask) + x   (networks/MPN.py:533,:537)
    const int ws_stamp = c.need_backward ? WS_STAMP_TRAIN : WS_STAMP_INFER;
    const SlotEa* slot_ea = r.ea_seg_fwd ? &se : nullptr;
    if (r.fused_front) {
        // ONE launch: the weight re-layout (which also advances the dropout stream for this forward) next to the front --
        // pred_mask.float(), mask_embd, the residual add and the first EdgeAggregation's P | Q (front.hip)
        FrontFwdArgs f;
        f.n = lo.n; f.h = lo.h; f.ldw1 = 2 * lo.f0 + lo.fe; f.mask_dtype = mask_dtype;
        f.x = x; f.mask = pred_mask;
        f.wa = me[0]; f.ba = me[1]; f.wb = me[2]; f.bb = me[3]; f.w1 = params[0]; f.b1 = params[1];
        f.maskf = lo.maskf; f.me_h = (c.need_backward && !r.meh_recompute) ? lo.me_h : nullptr; f.x0 = lo.x0;
        f.P = r.l0_fly ? nullptr : lo.ea[0].P;
        f.Q = r.l0_fly ? nullptr : lo.ea[0].Q;
        f.mask_counts = (r.seg_front && c.need_backward) ? lo.mask_counts : nullptr;   // (read by pfn_mpn_backward_masked_l2)
        f.gates = (r.seg_front && r.seg_gates) ? lo.relu_mask[0] : nullptr;
        if (r.seg_front)
            PFN_TRY(launch_front_seg_fwd(g, f, pk.jobs.data(), (int)pk.jobs.size(), drop ? rng : nullptr, &se, lo.stamp, ws_stamp, edge_attr,
                                         lo.ea[0].S, m.seg, s));
        else
            PFN_TRY(launch_front_fwd_pack(f, pk.jobs.data(), (int)pk.jobs.size(), drop ? rng : nullptr, s, slot_ea, lo.stamp, ws_stamp));
    } else {
        // ... the pack launch also advances the dropout stream for this forward and converts pred_mask to float32
        PFN_TRY(pk.flush(s, drop ? rng : nullptr, pred_mask, mask_dtype, lo.maskf, (int64_t)lo.n * lo.ld0, slot_ea, lo.stamp, ws_stamp));
        {
            GemmArgs a = gemm_defaults(lo.n, lo.h, lo.ld);
            a.C[0] = lo.me_h;
            a.nterm = 1;
            a.term[0] = term(lo.maskf, lo.ld0, lo.f0, mp.wa_t, 0);
            a.bias = me[1];
            a.act = ACT_RELU;
            PFN_TRY(launch_gemm_nt(a, s));
        }
        {
            GemmArgs a = gemm_defaults(lo.n, lo.f0, lo.ld0);
            a.C[0] = lo.x0;
            a.nterm = 1;
            a.term[0] = term(lo.me_h, lo.ld, lo.h, mp.wb_t, 0);
            a.bias = me[3];
            a.resid = x;
            a.ldr = lo.ld0;
            PFN_TRY(launch_gemm_nt(a, s));
        }
    }
    const float* cur = lo.x0;
    int ldc = lo.ld0, fcur = lo.f0, pi = 0;
    for (int i = 0; i < lo.nlayers; ++i) {
        const bool last = i + 1 == lo.nlayers;
        Act act;
        if (!last) act = Act{drop ? ACT_DROPOUT_RELU : ACT_RELU, c.dropout_rate, rng, (uint32_t)i, 0};   // dropout then ReLU (:546-547)
        float* y = last ? out : lo.y[i];
        const int ldy = last ? lo.ldo : lo.ld;
        if (is_ea(i)) {
            const int fo = last ? lo.fo : lo.h;
            if (!last) act.out_cm = r.big_cm;   // (feeds a TAGConv on the big-graph hop kernel)
            EaFwdOpts o;
            o.seg = m.seg; o.back_fused = r.back_fused; o.hop_K = lo.K;
            o.pq_ready = r.fused_front && i == 0; o.pq_fly = r.l0_fly && i == 0; o.walk_done = r.seg_front && i == 0;
            o.ea_in = r.ea_seg_fwd ? lo.ea_in : nullptr;
            o.relu_mask = r.saves_mask(i) ? lo.relu_mask[i] : nullptr;
            o.seg_gates = r.seg_gates ? lo.relu_mask[i] : nullptr;
            o.hop_xk = (r.slh_fwd && !last) ? lo.xk[i + 1] : nullptr;
            PFN_TRY(ea_forward(g, fcur, lo.fe, lo.h, fo, cur, ldc, edge_attr, params[pi], params[pi + 1], params[pi + 2],
                               params[pi + 3], mp.ea[i], y, ldy, act, lo.ea[i], s, o));
            pi += 4;
            fcur = fo;
        } else {
            TagOpts o;
            o.seg = m.seg; o.hops = r.hops; o.x_cm = r.big_cm;
            o.hops_done = r.slh_fwd;   // (by the EdgeAggregation in front, never the last layer)
            PFN_TRY(tag_forward(g, lo.h, lo.h, lo.K, cur, ldc, mp.tag[i], params[pi + lo.K + 1], y, ldy, act, lo.xk[i], s, o));
            pi += lo.K + 2;
        }
        cur = y;
        ldc = ldy;
    }
    return PFN_OK;
}

// P | Q of EdgeAggregation layer i written after the fact, for a reader that is decided after a forward pass that kept them in LDS
// (Route::seg_gates) or formed them on the fly (Route::l0_fly): layer 0 from x0 with the front's chains (launch_front_pq), a later
// layer as ea_forward's two-term gemm_nt -- the bits the forward's own tiles held (ea_seg.hip: gemm_nt's images and k order).
static int rewrite_pq(const ModelCall& m, const ModelPack& mp, const float* const* params, int i, hipStream_t s) {
    const Layout& lo = m.lo;
    const int pi = param_offset(i, lo.K);
    if (i == 0 && m.r.fused_front)
        return launch_front_pq(lo.n, lo.h, 2 * lo.f0 + lo.fe, lo.x0, params[0], params[1], lo.ea[0].P, lo.ea[0].Q, s);
    const int fi = i == 0 ? lo.f0 : lo.h;
    GemmArgs a = gemm_defaults(lo.n, lo.h, lo.ld);
    a.ngroup = 2;
    a.C[0] = lo.ea[i].P;
    a.C[1] = lo.ea[i].Q;
    a.nterm = 2;
    a.term[0] = term(i == 0 ? lo.x0 : lo.y[i - 1], i == 0 ? lo.ld0 : lo.ld, fi, mp.ea[i].w1i_t, 0);
    a.term[1] = term(i == 0 ? lo.x0 : lo.y[i - 1], i == 0 ? lo.ld0 : lo.ld, fi, mp.ea[i].w1j_t, 1);
    a.bias = params[pi + 1];
    a.bias_group = 0;
    return launch_gemm_nt(a, s);
}

static int model_backward(const pfn_mpn_config& c, const ModelCall& m, const float* const* params, float* const* grads,
                          const float* edge_attr, const float* gout, float* gx, float* gea, hipStream_t s,
                          const MseTail* mse = nullptr) {
    const GraphView& g = m.g;
    const Layout& lo = m.lo;
    const Route& r = m.r;
    // an edge-attribute gradient recomputes the pre-activations from P | Q in the generic walks: no graph-resident backward, the
    // saved masks unused, and layer 0's P | Q written first where the forward left them out
    const bool seg_bwd = r.ea_seg_bwd && !gea;
    const bool drop = c.training && c.dropout_rate > 0.f;
    const float gscale = drop ? 1.f / (1.f - c.dropout_rate) : 1.f;
    const int nparams = pfn_mpn_num_params(&c);
    Packer pk(lo.packed);                      // same walk as forward: addresses only, the images are already filled
    ModelPack mp;
    plan_pack(pk, lo.f0, lo.fe, lo.fo, lo.h, lo.L, lo.K, params, mp);
    if (gea) PFN_CHECK_HIP(hipMemsetAsync(gea, 0, (size_t)lo.e * lo.fe * sizeof(float), s));
    PairList pairs;                            // every weight-gradient pair of the network, launched once at the end
    const float* gcur = gout;
    int ldg = lo.ldo;
    for (int i = lo.nlayers - 1; i >= 0; --i) {
        const bool last = i + 1 == lo.nlayers;
        const float* inp = i == 0 ? lo.x0 : lo.y[i - 1];
        const int ldi = i == 0 ? lo.ld0 : lo.ld;
        Gate gate = i > 0 ? Gate{inp, ldi, gscale, 0} : Gate{};
        float* gnext = lo.gin[i];
        const int p0 = param_offset(i, lo.K);
        if (is_ea(i)) {
            const int fi = i == 0 ? lo.f0 : lo.h, fo = last ? lo.fo : lo.h;
            EaScratch sc = lo.eas;
            sc.dP = lo.dP[i]; sc.dQ = lo.dQ[i]; sc.dWe = lo.dWe[i];
            if (gea && (r.seg_gates || (i == 0 && r.l0_fly))) PFN_TRY(rewrite_pq(m, mp, params, i, s));
            EaBwdOpts o;
            o.seg = m.seg; o.back_fused = r.back_fused; o.hop_K = lo.K; o.mse = last ? mse : nullptr;
            o.ea_in = seg_bwd ? lo.ea_in : nullptr; o.ea_out = seg_bwd ? lo.ea_out : nullptr;
            o.relu_mask = (!gea && r.saves_mask(i)) ? lo.relu_mask[i] : nullptr;
            o.seg_gates = (seg_bwd && r.seg_gates) ? lo.relu_mask[i] : nullptr;
            // the gradient handed DOWN to a TAGConv (layers 2, 4, ...: their input is a TAGConv's output) is chunk-major where that
            // TAGConv's input is: its backward hops, its GEMM and the weight-gradient pairs read it through the flags
            o.gx_cm = i >= 2 ? r.big_cm : 0;
            o.hop_out = (r.slh_bwd && i >= 2) ? lo.tags.G : nullptr;
            // (layer 0 with the fused front: its input gradient is formed together with mask_embd's, below)
            PFN_TRY(ea_backward(g, fi, lo.fe, lo.h, fo, inp, ldi, edge_attr, params[p0], params[p0 + 2], mp.ea[i], gcur, ldg, gate,
                                (r.fused_front && i == 0) ? nullptr : gnext, ldi, grads[p0], grads[p0 + 1], grads[p0 + 2],
                                grads[p0 + 3], gea, lo.ea[i], sc, s, &pairs, o));
        } else {
            gate.cm = r.big_cm;     // a TAGConv's input is the EdgeAggregation output before it (model_forward)
            TagOpts o;
            o.seg = m.seg; o.hops = r.hops; o.x_cm = o.gout_cm = r.big_cm;
            o.hops_done = r.slh_bwd;   // (by the EdgeAggregation behind: layer i + 1 >= 2)
            PFN_TRY(tag_backward(g, lo.h, lo.h, lo.K, inp, ldi, mp.tag[i], gcur, ldg, gate, gnext, ldi, grads + p0,
                                 grads[p0 + lo.K + 1], lo.xk[i], lo.tags, s, &pairs, o));
        }
        gcur = gnext;
        ldg = ldi;
    }
    // mask_embd backward: x0 = me_h Wb^T + bb + x ; me_h = relu(maskf Wa^T + ba)
    float* const* gme = grads + (nparams - 4);
    if (r.meh_recompute) {      // ... and mask_embd's weight gradients too, me_h recomputed (front_bwd_wg_kernel; partials in the me_h buffer)
        PFN_TRY(launch_front_bwd_wg(lo.n, lo.h, 2 * lo.f0 + lo.fe, lo.dP[0], lo.dQ[0], lo.maskf, params[0], params[nparams - 4],
                                    params[nparams - 3], params[nparams - 2], lo.gin[0], lo.me_h, gme[0], gme[1], gme[2], gme[3], s, lo.stamp,
                                    WS_STAMP_TRAIN));
    } else if (r.fused_front) {   // g0 = dP0 W1i + dQ0 W1j and dh = (g0 Wb) [me_h > 0] in one launch (front.hip)
        PFN_TRY(launch_front_bwd(lo.n, lo.h, 2 * lo.f0 + lo.fe, lo.dP[0], lo.dQ[0], lo.me_h, params[0], params[nparams - 2],
                                 lo.gin[0], lo.dh, s));
    } else {
        GemmArgs a = gemm_defaults(lo.n, lo.h, lo.ld);
        a.C[0] = lo.dh;
        a.nterm = 1;
        a.term[0] = term(gcur, lo.ld0, lo.f0, mp.wb_d, 0);
        a.gate = lo.me_h;
        a.ldg = lo.ld;
        PFN_TRY(launch_gemm_nt(a, s));
    }
    if (!r.meh_recompute) {
        pairs.pairs.push_back(tn_pair(gcur, lo.ld0, lo.f0, lo.me_h, lo.ld, lo.h, gme[2], lo.h, 0, gme[3], nullptr));     // dWb, dbb
        pairs.pairs.push_back(tn_pair(lo.dh, lo.ld, lo.h, lo.maskf, lo.ld0, lo.f0, gme[0], lo.f0, 0, gme[1], nullptr));  // dWa, dba
    }
    // the dWe partial reductions ride in the weight-gradient launch (independent work, one launch floor less)
    if ((int)pairs.dwe.size() <= DWE_MAX_JOBS && lo.n > 0 && !pairs.pairs.empty()) {
        DweRide ride;
        ride.njobs = (int)pairs.dwe.size();
        for (int j = 0; j < ride.njobs; ++j) ride.jobs.job[j] = pairs.dwe[j];
        ride.fe = lo.fe; ride.ld = lo.ld; ride.h = lo.h;
        PFN_TRY(launch_weight_grads(pairs.pairs.data(), (int)pairs.pairs.size(), lo.n, lo.eas.red, s, &ride, lo.stamp, WS_STAMP_TRAIN));
    } else {
        PFN_TRY(launch_dwe_reduce_multi(pairs.dwe.data(), (int)pairs.dwe.size(), lo.fe, lo.ld, lo.h, s, lo.stamp, WS_STAMP_TRAIN));
        PFN_TRY(launch_weight_grads(pairs.pairs.data(), (int)pairs.pairs.size(), lo.n, lo.eas.red, s, nullptr, lo.stamp, WS_STAMP_TRAIN));
    }
    if (gx) PFN_CHECK_HIP(hipMemcpyAsync(gx, gcur, (size_t)lo.n * lo.ld0 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return PFN_OK;
}

}  // namespace pfn

using namespace pfn;

// =============================================================================================== C ABI
extern "C" {

int pfn_mpn_num_params(const pfn_mpn_config* c) {
    if (!c || c->n_gnn_layers < 2) return -1;
    return c->n_gnn_layers * 4 + (c->n_gnn_layers - 1) * (c->K + 2) + 4;
}

size_t pfn_mpn_workspace_bytes(const pfn_mpn_config* c, int64_t n, int64_t e) {
    if (!c) return 0;
    Layout lo;
    if (make_layout(*c, n, e, nullptr, lo) != PFN_OK) return 0;
    return lo.bytes;
}

static int check_common(const pfn_mpn_config* c, const void* gws, int64_t n, int64_t e, const void* ws) {
    PFN_CHECK_ARG(c != nullptr, "null config");
    PFN_CHECK_ARG(gws != nullptr, "null graph workspace");
    PFN_CHECK_ARG(ws != nullptr, "null model workspace");
    PFN_CHECK_ARG(n >= 0 && e >= 0 && n < (1ll << 30) && e < (1ll << 29), "bad graph size");
    return PFN_OK;
}

static int check_ws(const char* who, size_t have, size_t need) {
    if (have >= need) return PFN_OK;
    set_error("%s: workspace %zu < %zu bytes", who, have, need);
    return PFN_ENOSPACE;
}

// What every model entry point does between its own argument checks and its first launch: the layout, the workspace size (`who`
// names the entry point in the message), the graph view and the route.  Each entry point then says what it accepts as seg_nodes.
static int open_model(const pfn_mpn_config* c, const void* gws, int64_t n, int64_t e, void* ws, size_t ws_bytes, int64_t seg_nodes,
                      const char* who, ModelCall& m) {
    PFN_TRY(make_layout(*c, n, e, ws, m.lo));
    PFN_TRY(check_ws(who, ws_bytes, m.lo.bytes));
    m.g = graph_view(const_cast<void*>(gws), n, e);
    m.seg = (seg_nodes > 0 && n % seg_nodes == 0) ? (int)seg_nodes : 0;
    return make_route(*c, m.lo, m.seg, e, m.r);
}

int pfn_mpn_forward(const pfn_mpn_config* c, const void* gws, int64_t n, int64_t e, const float* const* params,
                    const float* x, const void* pred_mask, int mask_dtype, const float* edge_attr, float* out, void* ws,
                    size_t ws_bytes, uint64_t* rng, int64_t seg_nodes, void* stream) {
    PFN_TRY(check_common(c, gws, n, e, ws));
    PFN_CHECK_ARG(params && (n == 0 || (x && pred_mask)) && (e == 0 || edge_attr), "pfn_mpn_forward: null tensor");
    ModelCall m;
    PFN_TRY(open_model(c, gws, n, e, ws, ws_bytes, seg_nodes, "pfn_mpn_forward", m));
    // out == NULL: the output rows are left to pfn_mpn_backward_mse -- only where that entry point is available
    PFN_CHECK_ARG(n == 0 || out || m.r.mse_tail, "pfn_mpn_forward: out may be NULL only where pfn_mpn_mse_tail_ok says so");
    PFN_CHECK_ARG(c->nfeature_dim % 4 == 0, "nfeature_dim must be a multiple of 4 (the reference asserts 4, networks/MPN.py:528)");
    PFN_CHECK_ARG(seg_nodes >= 0 && (seg_nodes == 0 || n % seg_nodes == 0), "seg_nodes must be 0 or divide n_nodes");
    return model_forward(*c, m, params, x, pred_mask, mask_dtype, edge_attr, out, rng, static_cast<hipStream_t>(stream));
}

int pfn_mpn_mse_tail_ok(const pfn_mpn_config* c, int64_t n, int64_t e, int64_t seg_nodes) {
    if (!c || n <= 0 || e < 0 || n >= (1ll << 30) || e >= (1ll << 29) || seg_nodes <= 0 || n % seg_nodes != 0) return 0;
    Layout lo;
    Route r;
    if (make_layout(*c, n, e, nullptr, lo) != PFN_OK || make_route(*c, lo, (int)seg_nodes, e, r) != PFN_OK) return 0;
    return r.masked_tail ? 1 : 0;   // (one answer for both losses)
}

static int backward_with_loss_tail(const pfn_mpn_config* c, const void* gws, int64_t n, int64_t e, const float* const* params,
                                   float* const* grads, const float* x, const float* edge_attr, const float* y, float* out, float* loss,
                                   float* grad_out, float* gx, void* ws, size_t ws_bytes, void* loss_ws, size_t loss_ws_bytes,
                                   int64_t seg_nodes, void* stream, bool masked, int regularize, float regcoeff) {
    PFN_TRY(check_common(c, gws, n, e, ws));
    PFN_CHECK_ARG(params && grads && x && y && out && loss && grad_out && loss_ws, "pfn_mpn_backward_mse / _masked_l2: null tensor");
    PFN_CHECK_ARG(c->need_backward != 0, "pfn_mpn_backward_mse / _masked_l2: the forward ran with need_backward = 0");
    PFN_CHECK_ARG(loss_ws_bytes >= (masked ? 8196u : 4100u), "pfn_mpn_backward_mse: loss workspace must hold 4100 bytes (_masked_l2: 8196)");
    ModelCall m;
    PFN_TRY(open_model(c, gws, n, e, ws, ws_bytes, seg_nodes, "pfn_mpn_backward_mse", m));
    const Layout& lo = m.lo;
    PFN_CHECK_ARG(seg_nodes > 0 && n % seg_nodes == 0, "seg_nodes must divide n_nodes");
    if (!(masked ? m.r.masked_tail : m.r.mse_tail)) {
        set_error("pfn_mpn_backward_mse / _masked_l2: not available for this model / batch (ask pfn_mpn_mse_tail_ok)");
        return PFN_EINVAL;
    }
    const int nparams = pfn_mpn_num_params(c);
    MseTail t;
    t.S = lo.ea[lo.nlayers - 1].S;
    t.b2 = params[nparams - 4 - 1];   // the last EdgeAggregation's b2 (its four tensors end in front of mask_embd's)
    t.deg = m.g.deg;
    t.y = y; t.out = out; t.gout = grad_out;
    t.partial = static_cast<float*>(loss_ws);
    t.counter = reinterpret_cast<int*>(static_cast<char*>(loss_ws) + (masked ? 8192 : 4096));
    t.loss = loss;
    t.inv_n = 1.f / (float)(n * 4);
    if (masked) {
        t.maskf = lo.maskf;
        t.counts = lo.mask_counts;
        t.count_blocks = ea_seg_blocks(m.seg, lo.n, lo.ld);
        t.regularize = regularize ? 1 : 0;
        t.regcoeff = regcoeff;
    }
    return model_backward(*c, m, params, grads, edge_attr, grad_out, gx, nullptr, static_cast<hipStream_t>(stream), &t);
}

int pfn_mpn_backward_mse(const pfn_mpn_config* c, const void* gws, int64_t n, int64_t e, const float* const* params,
                         float* const* grads, const float* x, const float* edge_attr, const float* y, float* out, float* loss,
                         float* grad_out, float* gx, void* ws, size_t ws_bytes, void* loss_ws, size_t loss_ws_bytes,
                         int64_t seg_nodes, void* stream) {
    return backward_with_loss_tail(c, gws, n, e, params, grads, x, edge_attr, y, out, loss, grad_out, gx, ws, ws_bytes, loss_ws,
                                   loss_ws_bytes, seg_nodes, stream, false, 0, 0.f);
}

int pfn_mpn_backward_masked_l2(const pfn_mpn_config* c, const void* gws, int64_t n, int64_t e, const float* const* params,
                               float* const* grads, const float* x, const float* edge_attr, const float* y, int regularize,
                               float regcoeff, float* out, float* loss, float* grad_out, float* gx, void* ws, size_t ws_bytes,
                               void* loss_ws, size_t loss_ws_bytes, int64_t seg_nodes, void* stream) {
    return backward_with_loss_tail(c, gws, n, e, params, grads, x, edge_attr, y, out, loss, grad_out, gx, ws, ws_bytes, loss_ws,
                                   loss_ws_bytes, seg_nodes, stream, true, regularize, regcoeff);
}

int pfn_mpn_backward(const pfn_mpn_config* c, const void* gws, int64_t n, int64_t e, const float* const* params,
                     float* const* grads, const float* x, const void* pred_mask, int mask_dtype, const float* edge_attr,
                     const float* gout, float* gx, float* gea, void* ws, size_t ws_bytes, int64_t seg_nodes, void* stream) {
    (void)pred_mask; (void)mask_dtype;
    PFN_TRY(check_common(c, gws, n, e, ws));
    PFN_CHECK_ARG(params && grads && (n == 0 || (x && gout)), "pfn_mpn_backward: null tensor");
    PFN_CHECK_ARG(c->need_backward != 0, "pfn_mpn_backward: the forward ran with need_backward = 0 (inference: what only the backward reads was not saved)");
    ModelCall m;
    PFN_TRY(open_model(c, gws, n, e, ws, ws_bytes, seg_nodes, "pfn_mpn_backward", m));
    PFN_CHECK_ARG(seg_nodes >= 0 && (seg_nodes == 0 || n % seg_nodes == 0), "seg_nodes must be 0 or divide n_nodes");
    return model_backward(*c, m, params, grads, edge_attr, gout, gx, gea, static_cast<hipStream_t>(stream));
}

int pfn_mpn_export_gates(const pfn_mpn_config* c, const void* gws, int64_t n, int64_t e, const float* const* params,
                         const float* edge_attr, void* ws, size_t ws_bytes, int64_t seg_nodes, int32_t kind, int32_t layer,
                         uint8_t* out, void* stream) {
    PFN_TRY(check_common(c, gws, n, e, ws));
    PFN_CHECK_ARG(params && out, "pfn_mpn_export_gates: null pointer");
    PFN_CHECK_ARG(c->need_backward != 0, "pfn_mpn_export_gates: the forward ran with need_backward = 0 (mask_embd's hidden layer was not saved)");
    ModelCall m;
    PFN_TRY(open_model(c, gws, n, e, ws, ws_bytes, seg_nodes, "pfn_mpn_export_gates", m));
    const Layout& lo = m.lo;
    if (n == 0) return PFN_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (kind == 0) {
        PFN_CHECK_ARG(layer >= 0 && layer < lo.nlayers && is_ea(layer), "pfn_mpn_export_gates: kind 0 needs an EdgeAggregation layer index");
        PFN_CHECK_ARG(e == 0 || edge_attr, "pfn_mpn_export_gates: null edge_attr");
        const int pi = param_offset(layer, lo.K), fi = layer == 0 ? lo.f0 : lo.h;
        if (m.r.seg_gates || (layer == 0 && m.r.l0_fly)) {   // (the forward left them unwritten)
            Packer pk(lo.packed);                              // (addresses only: the forward filled the images)
            ModelPack mp;
            plan_pack(pk, lo.f0, lo.fe, lo.fo, lo.h, lo.L, lo.K, params, mp);
            PFN_TRY(rewrite_pq(m, mp, params, layer, s));
        }
        return launch_export_edge_gates(m.g, lo.ea[layer].P, lo.ea[layer].Q, edge_attr, params[pi], lo.ld, lo.h, fi, lo.fe, out, s);
    } else if (kind == 1) {
        PFN_CHECK_ARG(layer >= 0 && layer + 1 < lo.nlayers, "pfn_mpn_export_gates: kind 1 needs a hidden layer index");
        return launch_export_row_gates(n, lo.h, lo.ld, lo.y[layer], is_ea(layer) && m.r.big_cm, out, s);
    } else if (kind == 2) {
        if (m.r.meh_recompute) {   // (the forward did not store it)
            const int np = pfn_mpn_num_params(c);
            PFN_TRY(launch_front_meh(lo.n, lo.h, lo.maskf, 1, params[np - 4], params[np - 3], lo.me_h, s));
        }
        return launch_export_row_gates(n, lo.h, lo.ld, lo.me_h, 0, out, s);
    }
    set_error("pfn_mpn_export_gates: kind must be 0 (edge stage), 1 (layer output) or 2 (mask_embd hidden)");
    return PFN_EINVAL;
}

// ------------------------------------------------------------------------------------- single layers
struct EaLayerWs { EaSaved sv; EaScratch sc; float* packed; size_t bytes; };
static EaLayerWs ea_layer_ws(void* ws, int64_t n, int fi, int fe, int h, int fo) {
    Carver cv(ws);
    EaLayerWs w;
    const int ld = ld_of(h);
    const size_t nld = (size_t)n * ld;
    {
        Packer measure(nullptr);
        ea_pack(measure, fi, fe, h, fo, nullptr, nullptr);
        w.packed = cv.take<float>(measure.off);
    }
    w.sv.P = cv.take<float>(nld);
    w.sv.Q = cv.take<float>(nld);
    w.sv.S = cv.take<float>(nld);
    w.sc.dS = cv.take<float>(nld);
    w.sc.dP = cv.take<float>(nld);
    w.sc.dQ = cv.take<float>(nld);
    w.sc.dWe = cv.take<float>((size_t)1025 * fe * ld);
    const int maxf = std::max(std::max(h, fi), fo);
    w.sc.red.floats = reduce_ws_floats(n, maxf, maxf, 3);
    w.sc.red.partial = cv.take<float>(w.sc.red.floats);
    w.bytes = cv.off;
    return w;
}

size_t pfn_edge_aggr_workspace_bytes(int64_t n, int64_t e, int fi, int fe, int h, int fo) {
    (void)e;
    return ea_layer_ws(nullptr, n, fi, fe, h, fo).bytes;
}

int pfn_edge_aggr_forward(const void* gws, int64_t n, int64_t e, int fi, int fe, int h, int fo, const float* x,
                          int64_t ldx, const float* ea, const float* w1, const float* b1, const float* w2,
                          const float* b2, float* out, int64_t ldo, void* ws, size_t ws_bytes, void* stream) {
    PFN_CHECK_ARG(gws && ws && w1 && b1 && w2 && b2, "pfn_edge_aggr_forward: null pointer");
    PFN_CHECK_ARG(ldx == ld_of(fi) && ldo == ld_of(fo), "pfn_edge_aggr_forward: row strides must be pfn_padded_ld(F)");
    PFN_CHECK_ARG(fe >= 1 && fe <= 6, "efeature_dim must be in [1, 6]");
    EaLayerWs w = ea_layer_ws(ws, n, fi, fe, h, fo);
    PFN_TRY(check_ws("pfn_edge_aggr_forward", ws_bytes, w.bytes));
    GraphView g = graph_view(const_cast<void*>(gws), n, e);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Packer pk(w.packed);
    const EaPack pw = ea_pack(pk, fi, fe, h, fo, w1, w2);
    PFN_TRY(pk.flush(s));
    return ea_forward(g, fi, fe, h, fo, x, (int)ldx, ea, w1, b1, w2, b2, pw, out, (int)ldo, Act{}, w.sv, s, {});
}

int pfn_edge_aggr_backward(const void* gws, int64_t n, int64_t e, int fi, int fe, int h, int fo, const float* x,
                           int64_t ldx, const float* ea, const float* w1, const float* b1, const float* w2,
                           const float* b2, const float* gout, int64_t ldgo, float* gx, int64_t ldgx, float* gea,
                           float* gw1, float* gb1, float* gw2, float* gb2, void* ws, size_t ws_bytes, void* stream) {
    (void)b1; (void)b2;
    PFN_CHECK_ARG(gws && ws && w1 && w2 && gout && gw1 && gb1 && gw2 && gb2, "pfn_edge_aggr_backward: null pointer");
    PFN_CHECK_ARG(ldx == ld_of(fi) && ldgo == ld_of(fo) && (!gx || ldgx == ld_of(fi)),
                  "pfn_edge_aggr_backward: row strides must be pfn_padded_ld(F)");
    PFN_CHECK_ARG(fe >= 1 && fe <= 6, "efeature_dim must be in [1, 6]");
    EaLayerWs w = ea_layer_ws(ws, n, fi, fe, h, fo);
    PFN_TRY(check_ws("pfn_edge_aggr_backward", ws_bytes, w.bytes));
    hipStream_t s = static_cast<hipStream_t>(stream);
    GraphView g = graph_view(const_cast<void*>(gws), n, e);
    if (gea) PFN_CHECK_HIP(hipMemsetAsync(gea, 0, (size_t)e * fe * sizeof(float), s));
    Packer pk(w.packed);                       // images were filled by the forward call on the same workspace
    const EaPack pw = ea_pack(pk, fi, fe, h, fo, w1, w2);
    return ea_backward(g, fi, fe, h, fo, x, (int)ldx, ea, w1, w2, pw, gout, (int)ldgo, Gate{}, gx, (int)ldgx, gw1, gb1, gw2,
                       gb2, gea, w.sv, w.sc, s, nullptr, {});
}

struct TagLayerWs { float* xk; TagScratch sc; float* packed; size_t bytes; };
static TagLayerWs tag_layer_ws(void* ws, int64_t n, int cin, int cout, int K) {
    Carver cv(ws);
    TagLayerWs w;
    const size_t nld = (size_t)n * ld_of(cin);
    {
        Packer measure(nullptr);
        const float* none[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        tag_pack(measure, cin, cout, K, none);
        w.packed = cv.take<float>(measure.off);
    }
    w.xk = cv.take<float>(nld * std::max(1, K));
    w.sc.G = cv.take<float>(nld * (K + 1));
    w.sc.z0 = cv.take<float>(nld);
    w.sc.z1 = cv.take<float>(nld);
    const int maxf = std::max(cin, cout);
    w.sc.red.floats = reduce_ws_floats(n, maxf, maxf, K + 1);
    w.sc.red.partial = cv.take<float>(w.sc.red.floats);
    w.bytes = cv.off;
    return w;
}

size_t pfn_tag_conv_workspace_bytes(int64_t n, int64_t e, int cin, int cout, int K) {
    (void)e;
    return tag_layer_ws(nullptr, n, cin, cout, K).bytes;
}

int pfn_tag_conv_forward(const void* gws, int64_t n, int64_t e, int cin, int cout, int K, const float* x, int64_t ldx,
                         const float* const* weights, const float* bias, float* out, int64_t ldo, void* ws,
                         size_t ws_bytes, int64_t seg_nodes, void* stream) {
    PFN_CHECK_ARG(gws && ws && weights, "pfn_tag_conv_forward: null pointer");
    PFN_CHECK_ARG(ldx == ld_of(cin) && ldo == ld_of(cout), "pfn_tag_conv_forward: row strides must be pfn_padded_ld(F)");
    PFN_CHECK_ARG(K >= 0 && K <= 7, "K must be in [0, 7]");
    TagLayerWs w = tag_layer_ws(ws, n, cin, cout, K);
    PFN_TRY(check_ws("pfn_tag_conv_forward", ws_bytes, w.bytes));
    GraphView g = graph_view(const_cast<void*>(gws), n, e);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Packer pk(w.packed);
    const TagPack pw = tag_pack(pk, cin, cout, K, weights);
    PFN_TRY(pk.flush(s));
    PFN_CHECK_ARG(seg_nodes >= 0 && (seg_nodes == 0 || n % seg_nodes == 0), "seg_nodes must be 0 or divide n_nodes");
    return tag_forward(g, cin, cout, K, x, (int)ldx, pw, bias, out, (int)ldo, Act{}, w.xk, s,
                       TagOpts{(int)seg_nodes, hop_kind((int)seg_nodes, (int)ldx, g.n, g.e_stored, K)});
}

int pfn_tag_conv_backward(const void* gws, int64_t n, int64_t e, int cin, int cout, int K, const float* x, int64_t ldx,
                          const float* const* weights, const float* gout, int64_t ldgo, float* gx, int64_t ldgx,
                          float* const* gweights, float* gbias, void* ws, size_t ws_bytes, int64_t seg_nodes, void* stream) {
    PFN_CHECK_ARG(gws && ws && weights && gout && gweights, "pfn_tag_conv_backward: null pointer");
    PFN_CHECK_ARG(ldx == ld_of(cin) && ldgo == ld_of(cout), "pfn_tag_conv_backward: row strides must be pfn_padded_ld(F)");
    PFN_CHECK_ARG(K >= 0 && K <= 7, "K must be in [0, 7]");
    TagLayerWs w = tag_layer_ws(ws, n, cin, cout, K);
    PFN_TRY(check_ws("pfn_tag_conv_backward", ws_bytes, w.bytes));
    GraphView g = graph_view(const_cast<void*>(gws), n, e);
    Packer pk(w.packed);                       // images were filled by the forward call on the same workspace
    const TagPack pw = tag_pack(pk, cin, cout, K, weights);
    PFN_CHECK_ARG(seg_nodes >= 0 && (seg_nodes == 0 || n % seg_nodes == 0), "seg_nodes must be 0 or divide n_nodes");
    return tag_backward(g, cin, cout, K, x, (int)ldx, pw, gout, (int)ldgo, Gate{}, gx, (int)ldgx, gweights, gbias, w.xk,
                        w.sc, static_cast<hipStream_t>(stream), nullptr,
                        TagOpts{(int)seg_nodes, hop_kind((int)seg_nodes, (int)ldx, g.n, g.e_stored, K)});
}

// ----------------------------------------------------------------------------------------- utilities
int pfn_scatter_add(const void* gws, int64_t n, int64_t e, const float* x, float* out, int64_t f, void* stream) {
    PFN_CHECK_ARG(gws && (n == 0 || (x && out)), "pfn_scatter_add: null pointer");
    GraphView g = graph_view(const_cast<void*>(gws), n, e);
    HopArgs hp{x, nullptr, out, nullptr, 1.f, ld_of((int)f), 0, 0};
    return launch_hop(g, hp, static_cast<hipStream_t>(stream));
}

int pfn_pad_rows(const float* src, int64_t ld_src, float* dst, int64_t ld_dst, int64_t rows, int64_t f, void* stream) {
    PFN_CHECK_ARG(rows == 0 || (src && dst), "pfn_pad_rows: null pointer");
    PFN_CHECK_ARG(f <= ld_src && ld_dst >= 0, "pfn_pad_rows: bad strides");
    return launch_pad_rows(src, ld_src, dst, ld_dst, rows, std::min(f, ld_dst), static_cast<hipStream_t>(stream));
}

}  // extern "C"
