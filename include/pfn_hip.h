/*
 * pfn_hip.h -- C ABI of libpfn_hip.so: the MI355X (gfx950) implementation of PowerFlowNet's
 * message-passing hot path (MaskEmbdMultiMPN forward + backward).
 *
 * The reference has no FFI of its own: its boundary is the Python class surface of
 * networks/MPN.py.  Each entry point below names the reference interface it
 * replaces (file:line into /root/reference).  The host-side mirror of that class surface
 * (poweflownet_amd/networks/MPN.py) binds these symbols with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (except `params`/`grads` tables, which are
 *     HOST arrays of device pointers, and out-parameters documented as host);
 *   - all floating point is fp32; node/edge ids arrive as int64 (the PyG layout) and are narrowed to
 *     int32 inside pfn_graph_build;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*); no entry point synchronises,
 *     allocates or frees device memory except where stated, so every call is hipGraph-capturable;
 *   - activations handed between layers use a padded row stride ld = pfn_padded_ld(F) = roundup(F, 4)
 *     floats whose pad columns are kept zero;
 *   - return value: 0 on success, a negative PFN_E* code otherwise; pfn_last_error() gives the text.
 */
#ifndef PFN_HIP_H
#define PFN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFN_ABI_VERSION 8

enum {
    PFN_OK = 0,
    PFN_EINVAL = -1,      /* bad argument (null pointer, misaligned ld, unsupported dimension) */
    PFN_ENOSPACE = -2,    /* a caller-provided workspace is too small */
    PFN_EHIP = -3,        /* a HIP runtime call failed */
    PFN_EINDEX = -4       /* edge_index holds a node id outside [0, n_nodes) */
};

/* Model hyper-parameters: the constructor arguments of MaskEmbdMultiMPN (networks/MPN.py:462-470). */
typedef struct pfn_mpn_config {
    int32_t nfeature_dim;   /* node input width (4, asserted networks/MPN.py:528) */
    int32_t efeature_dim;   /* edge feature width (2) */
    int32_t output_dim;     /* node output width (4) */
    int32_t hidden_dim;     /* H */
    int32_t n_gnn_layers;   /* L >= 2 (L == 1 is shape-broken in the reference, networks/MPN.py:475-477) */
    int32_t K;              /* TAGConv hops */
    float dropout_rate;     /* p of nn.Dropout (networks/MPN.py:496) */
    int32_t training;       /* 1: dropout active (model.train()), 0: model.eval() */
    int32_t need_backward;  /* 1: pfn_mpn_backward will be called on this forward's workspace (autograd records the call): the
                             * forward edge walks also save their ReLU masks, which the backward walks then read instead of
                             * recomputing the edge pre-activations.  0: inference: nothing extra is written and tensors only
                             * the backward reads (mask_embd's hidden layer) are not stored; pfn_mpn_backward then returns
                             * PFN_EINVAL.  pfn_mpn_backward must be given the value the forward call had: the forward stamps
                             * its workspace on the device, and a backward pass on a workspace whose LAST forward ran with
                             * need_backward = 0 (the host cannot tell) writes every parameter gradient as NaN.          */
} pfn_mpn_config;

/* The library keeps NO process-global mutable state: no stream, event, cache or "first caller" device binding of its own
 * (per-device facts such as the CU count are looked up per call; kernel attributes are raised once per device, lock-free).
 * Every call works on the caller's stream and the caller's workspaces only, so two models on two devices or two host
 * threads may run concurrently as long as they do not share a workspace.                                              */
int pfn_abi_version(void);
const char* pfn_last_error(void);            /* thread-local, valid until the next failing call */
int64_t pfn_padded_ld(int64_t features);     /* roundup(features, 4) */

/* ------------------------------------------------------------------------------------------ graph
 * Replaces MaskEmbdMultiMPN.is_directed + undirect_graph (networks/MPN.py:498-523) and the per-call
 * PyG bookkeeping underneath propagate()/gcn_norm (degree scatter, index_select lifting):
 * one pass turns the stored edge list into destination-sorted and source-sorted CSR adjacency
 * (rows ordered by edge id, so segment sums run in the reference's edge order), in-degree and
 * D^-1/2.  `mode`: -1 = apply the reference's first-edge heuristic on device (no host sync),
 * 0 = use the list as given, 1 = always append the reversed copies.                              */
size_t pfn_graph_workspace_bytes(int64_t n_nodes, int64_t e_stored);
int pfn_graph_build(const int64_t* edge_index /* [2, e_stored] */, int64_t e_stored, int64_t n_nodes,
                    int mode, void* graph_ws, size_t graph_ws_bytes, void* stream);
/* Synchronising debug/validation read-back (host out-params): directed flag, effective edge count,
 * error flag (non-zero when an id was out of range -> PFN_EINDEX).                               */
int pfn_graph_info(const void* graph_ws, int64_t n_nodes, int64_t e_stored, int32_t* directed,
                   int64_t* e_effective, void* stream);
/* Synchronising check (once per topology): *ok = 1 iff n_nodes % seg_nodes == 0 and no effective edge crosses a multiple
 * of seg_nodes, i.e. the batch is a disjoint union of index-contiguous graphs of seg_nodes nodes (what PyG's Batch of one
 * reference case is).  A caller that got ok may pass seg_nodes to the model / TAGConv entry points, which then keep the K
 * propagation hops of a TAGConv resident in LDS per graph instead of running K gather kernels over HBM/L2.            */
int pfn_graph_segments(void* graph_ws, int64_t n_nodes, int64_t e_stored, int64_t seg_nodes, int32_t* ok, void* stream);
/* The same check WITHOUT the read-back, for callers that cannot synchronise (a topology that changes per batch inside a captured
 * hipGraph -- the reference's `perturbed` datasets, dataset_generator.py:250-253, utils/data_utils.py:12-59): the verdict stays in
 * the workspace.  The caller passes seg_nodes to the model on trust and ends its forward pass with pfn_graph_poison_if_bad, which
 * overwrites `out` (count floats) with NaN when the workspace records a node id outside [0, n_nodes) or an edge that crosses a
 * segment boundary -- so a bad batch surfaces as a NaN loss instead of a silently wrong one (pfn_graph_info still reports the
 * id error, with a sync, whenever the caller can afford one).  Both calls are hipGraph-capturable.  seg_nodes = 0 (ABI 8): no
 * segment promise is made -- the verdict a previous check left in this workspace is cleared, nothing is checked.               */
int pfn_graph_segments_async(void* graph_ws, int64_t n_nodes, int64_t e_stored, int64_t seg_nodes, void* stream);
int pfn_graph_poison_if_bad(const void* graph_ws, int64_t n_nodes, int64_t e_stored, float* out, int64_t count, void* stream);
/* The adjacency of a collated batch of ONE grid case, one workgroup per graph (graph_seg.hip; additive within ABI 8).  The
 * caller promises n_nodes = B * seg_nodes, e_stored = B * seg_edges, graph g's stored edges at entries [g * seg_edges,
 * (g + 1) * seg_edges) and both endpoints of each inside [g * seg_nodes, (g + 1) * seg_nodes).  For every input that keeps the
 * promise the workspace holds, array by array and bit for bit, what pfn_graph_build followed by
 * pfn_graph_segments_async(seg_nodes) leaves (cur_in, cur_out, scan_sums and flags[3] are scratch) -- from at most two launches,
 * no memset, no global atomic, no host sync; hipGraph-capturable.  The promise is checked on the way: an id outside [0, n_nodes)
 * (collated form) or [0, seg_nodes) (block form), or a sample index outside [0, n_samples), raises the id flag; an endpoint in
 * another graph's range raises the segment flag -- pfn_graph_poison_if_bad then turns the output into NaN.  Such an edge is never
 * obeyed (it stands as a self-loop on its graph's last node), and nothing is written outside graph g's slices of the workspace.
 *   sample_idx == NULL: `edge_index` is the collated [2, e_stored] list (global ids); edge_index_out is not used.
 *   sample_idx != NULL: `edge_index` is a dataset block [n_samples][2][seg_edges] of LOCAL ids; graph g reads sample
 *                       sample_idx[g] (device int64 [B]), and the collated list is written to edge_index_out [2, e_stored].
 * pfn_graph_build_segments_fits (host only): 1 iff 1 <= seg_nodes <= 128 and the workgroup's LDS -- 4 * (6 seg_edges +
 * 5 seg_nodes + 3) bytes: two local id lists, two histograms, three row-pointer arrays, two lists of 2 seg_edges edge keys --
 * is at most 64 KiB; pfn_graph_build_segments returns PFN_EINVAL where it answers 0 (such batches keep pfn_graph_build).
 * pfn_graph_layout (host only): writes (byte offset, element count) of every array of the workspace of (n_nodes, e_stored) into
 * `out` (`cap` int64s), in the order flags, scan_sums, rowptr_in, rowptr_out, in_src, in_eid, out_dst, out_eid, rp4, out_mbase,
 * out_ml4k, slot_of_eid, cur_in, cur_out, deg, dinv, and returns the number of arrays (16).  Elements are 4 bytes wide except
 * out_ml4k's (8: two ints).  For tests that compare two workspaces array by array.                                       */
int pfn_graph_build_segments(const int64_t* edge_index, int64_t e_stored, int64_t n_nodes, int64_t seg_nodes, int64_t seg_edges,
                             int mode, const int64_t* sample_idx, int64_t n_samples, int64_t* edge_index_out, void* graph_ws,
                             size_t graph_ws_bytes, void* stream);
int pfn_graph_build_segments_fits(int64_t seg_nodes, int64_t seg_edges);
int pfn_graph_layout(int64_t n_nodes, int64_t e_stored, int64_t* out, int64_t cap);
/* Copies the effective (post-undirect) edge list back out as int64 [2, 2*e_stored] (tests). */
int pfn_graph_export_edges(const void* graph_ws, int64_t n_nodes, int64_t e_stored,
                           int64_t* edge_index_out, void* stream);

/* -------------------------------------------------------------------------------------- whole model
 * Parameter table order (host array of device pointers), mirroring the module tree of
 * networks/MPN.py:462-496:
 *   for each layer i of `layers`:  EdgeAggregation -> W1 (H, 2*Fi+Fe), b1 (H), W2 (Fo, H), b2 (Fo)
 *                                  TAGConv         -> W_0 .. W_K (H, H) each, bias (H)
 *   then mask_embd: Wa (H, F0), ba (H), Wb (F0, H), bb (F0).
 * All in the nn.Linear (out, in) row-major layout of the state_dict.  pfn_mpn_num_params gives the
 * table length; `grads` uses the same order.                                                      */
int pfn_mpn_num_params(const pfn_mpn_config* cfg);
size_t pfn_mpn_workspace_bytes(const pfn_mpn_config* cfg, int64_t n_nodes, int64_t e_stored);

/* MaskEmbdMultiMPN.forward (networks/MPN.py:525-559), including EdgeAggregation.forward/message
 * (:23-56) and TAGConv.forward.  x [N, F0] f32, pred_mask [N, F0] (mask_dtype 0: int64, the dataset
 * layout of datasets/PowerFlowData.py:193; 1: float32), edge_attr [e_stored, Fe] f32, out [N, output_dim] f32.  `ws` receives the activations backward needs.  `rng_state`: device
 * uint64[2] {seed, offset}; when training && dropout_rate > 0 the offset is advanced by one at the start of the call
 * and then read by the dropout epilogues.  `out` may be NULL where pfn_mpn_mse_tail_ok answers 1 and
 * pfn_mpn_backward_mse follows (which then writes the rows).  Non-finite entries of x or edge_attr
 * propagate as in the reference (a ReLU unit is off iff its pre-activation compares <= 0: NaN is on);
 * the rows they do not reach are unaffected, bit for bit.                                          */
int pfn_mpn_forward(const pfn_mpn_config* cfg, const void* graph_ws, int64_t n_nodes, int64_t e_stored,
                    const float* const* params, const float* x, const void* pred_mask,
                    int mask_dtype, const float* edge_attr, float* out, void* ws, size_t ws_bytes,
                    uint64_t* rng_state, int64_t seg_nodes /* 0, or a value pfn_graph_segments accepted */, void* stream);

/* Autograd of the above (what loss.backward() runs, utils/training.py:74): grad_out [N, output_dim];
 * writes every entry of `grads` (overwrites, does not accumulate); grad_x [N, F0] and
 * grad_edge_attr [e_stored, Fe] are optional (NULL to skip).  `ws` is the buffer forward filled.   */
int pfn_mpn_backward(const pfn_mpn_config* cfg, const void* graph_ws, int64_t n_nodes, int64_t e_stored,
                     const float* const* params, float* const* grads, const float* x,
                     const void* pred_mask, int mask_dtype, const float* edge_attr, const float* grad_out,
                     float* grad_x, float* grad_edge_attr, void* ws, size_t ws_bytes, int64_t seg_nodes, void* stream);

/* `loss = torch.nn.MSELoss()(out, y); loss.backward()` (train.py:103; the else-branch of train_epoch, utils/training.py:70-74)
 * together with the autograd pass above, for batches of small graphs: the first backward launch -- the graph-resident
 * EdgeAggregation backward of the LAST layer -- forms the output rows `out = S W2^T + deg b2` (networks/MPN.py:559 hands them to
 * the loss), the loss and `grad_out = 2 (out - y) / (4 N)` itself, so the output Linear's launch and the loss launch leave the
 * step (three launches -> one).  Call pfn_mpn_forward on the same workspace first; its `out` may then be NULL (the rows are only
 * written here).  Results: `out` bit-identical to pfn_mpn_forward's, `grad_out` and every entry of `grads` bit-identical to
 * pfn_mpn_forward -> pfn_mse_loss -> pfn_mpn_backward; loss[0] = mean((out - y)^2) summed per row block, the blocks in block
 * order (deterministic; not pfn_mse_loss's partition, so equal to its value up to the rounding of a different summation order).
 * y, out, grad_out: [N, 4] f32, no padding (output_dim must be 4).  `loss_ws`: >= 4100 bytes -- 1024 float partials + one int32
 * arrival counter at byte 4096 that must be ZERO before the first call and is left zero by every call.  grad_x optional.
 * Available where pfn_mpn_mse_tail_ok returns 1 (seg_nodes from pfn_graph_segments, Fe = 2, output_dim 4, the batch in the
 * graph-resident regime); PFN_EINVAL elsewhere -- the caller then runs the three calls above.                              */
int pfn_mpn_mse_tail_ok(const pfn_mpn_config* cfg, int64_t n_nodes, int64_t e_stored, int64_t seg_nodes);
/* The same with `Masked_L2_loss(regularize, regcoeff)(out, y, pred_mask)` (utils/custom_loss_functions.py:10-46, the default
 * --train_loss_fn, dispatch utils/training.py:61-62) as the loss, `pred_mask` being THE mask the forward call was given (its
 * first launch kept the float mask rows and the per-block counts of the two index sets in `ws`): loss and grad as
 * pfn_masked_l2_loss defines them -- grad_out bit-identical to it, loss[0] to the rounding of another summation order.
 * `loss_ws`: >= 8196 bytes (2048 float partials + the int32 arrival counter at byte 8192, zero between calls).         */
int pfn_mpn_backward_masked_l2(const pfn_mpn_config* cfg, const void* graph_ws, int64_t n_nodes, int64_t e_stored,
                               const float* const* params, float* const* grads, const float* x, const float* edge_attr,
                               const float* y, int regularize, float regcoeff, float* out, float* loss, float* grad_out,
                               float* grad_x, void* ws, size_t ws_bytes, void* loss_ws, size_t loss_ws_bytes,
                               int64_t seg_nodes, void* stream);
int pfn_mpn_backward_mse(const pfn_mpn_config* cfg, const void* graph_ws, int64_t n_nodes, int64_t e_stored,
                         const float* const* params, float* const* grads, const float* x, const float* edge_attr,
                         const float* y, float* out, float* loss, float* grad_out, float* grad_x, void* ws, size_t ws_bytes,
                         void* loss_ws, size_t loss_ws_bytes, int64_t seg_nodes, void* stream);

/* Verification aid for the autograd above (what loss.backward() differentiates, utils/training.py:74; the ReLUs are
 * networks/MPN.py:19 (edge MLP), :547 (layer outputs) and :493 (mask_embd)): the ReLU gate decisions of the forward pass that
 * filled `ws`, as bytes (1 = the unit passed), so that a float64 run of the CPU oracle can be held to the same piecewise-linear
 * branch and every gradient compared at 1e-5.  Call after pfn_mpn_forward (need_backward = 1), before `ws` is reused.
 *   kind 0: edge stage of EdgeAggregation layer `layer` (index into `layers`): out [E_effective][H] in edge-id order
 *           (originals first, reversed copies second -- the order undirect_graph produces, networks/MPN.py:506-523);
 *           out must hold 2 * e_stored * H bytes;
 *   kind 1: output of hidden layer `layer` after dropout -> ReLU (:546-547): out [N][H];
 *   kind 2: mask_embd's hidden layer (:493): out [N][H].                                                              */
int pfn_mpn_export_gates(const pfn_mpn_config* cfg, const void* graph_ws, int64_t n_nodes, int64_t e_stored,
                         const float* const* params, const float* edge_attr, void* ws, size_t ws_bytes,
                         int64_t seg_nodes /* the value the forward call had: it decides the layout of saved tensors */,
                         int32_t kind, int32_t layer, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------------------- single layers
 * EdgeAggregation(nfeature_dim, efeature_dim, hidden_dim, output_dim).forward (networks/MPN.py:30-56):
 *   out[i] = sum_{e -> i} ( W2 relu(W1 [x_i ; x_src(e) ; a_e] + b1) + b2 ).
 * x [N, ldx] (ldx = pfn_padded_ld(Fi), pad zero), out [N, ldo].  `ws` (pfn_edge_aggr_workspace_bytes)
 * keeps P|Q and S for backward.  The graph must have been built from the list the layer is given
 * (mode 0 when the caller already undirected it).                                                  */
size_t pfn_edge_aggr_workspace_bytes(int64_t n_nodes, int64_t e_stored, int fi, int fe, int h, int fo);
int pfn_edge_aggr_forward(const void* graph_ws, int64_t n_nodes, int64_t e_stored, int fi, int fe, int h,
                          int fo, const float* x, int64_t ldx, const float* edge_attr, const float* w1,
                          const float* b1, const float* w2, const float* b2, float* out, int64_t ldo,
                          void* ws, size_t ws_bytes, void* stream);
int pfn_edge_aggr_backward(const void* graph_ws, int64_t n_nodes, int64_t e_stored, int fi, int fe, int h,
                           int fo, const float* x, int64_t ldx, const float* edge_attr, const float* w1,
                           const float* b1, const float* w2, const float* b2, const float* grad_out,
                           int64_t ldgo, float* grad_x, int64_t ldgx, float* grad_edge_attr, float* grad_w1,
                           float* grad_b1, float* grad_w2, float* grad_b2, void* ws, size_t ws_bytes,
                           void* stream);

/* TAGConv(in, out, K).forward (PyG; call sites networks/MPN.py:477-484,:545):
 *   out = sum_k (A_hat^k x) W_k^T + b,  A_hat = D^-1/2 A D^-1/2, no self loops.
 * weights: host array of K+1 device pointers (lins.k.weight, (out, in) each).                     */
size_t pfn_tag_conv_workspace_bytes(int64_t n_nodes, int64_t e_stored, int cin, int cout, int K);
int pfn_tag_conv_forward(const void* graph_ws, int64_t n_nodes, int64_t e_stored, int cin, int cout, int K,
                         const float* x, int64_t ldx, const float* const* weights, const float* bias,
                         float* out, int64_t ldo, void* ws, size_t ws_bytes, int64_t seg_nodes, void* stream);
int pfn_tag_conv_backward(const void* graph_ws, int64_t n_nodes, int64_t e_stored, int cin, int cout, int K,
                          const float* x, int64_t ldx, const float* const* weights, const float* grad_out,
                          int64_t ldgo, float* grad_x, int64_t ldgx, float* const* grad_weights,
                          float* grad_bias, void* ws, size_t ws_bytes, int64_t seg_nodes, void* stream);

/* GCNConv(in, out).forward (PyG, defaults add_self_loops / normalize / bias, flow source -> target; the layer of the reference's
 * GCN baseline, networks/GCN.py:8-19), over the adjacency pfn_graph_build made with MODE 0: the list is used as stored and is not
 * undirected (the reference's GCN.forward hands data.edge_index to the layer as it is).
 *   - a stored edge whose two ends are equal is dropped (add_remaining_self_loops), then every node gets ONE unit self loop;
 *     parallel lines count once each;
 *   - d_i = 1 + #{stored e : dst(e) = i, src(e) != i},  dis_i = d_i^-1/2  (never 0 or inf);
 *   - H = X W^T,  out_i = dis_i * ( sum_{e: dst = i, src != i} dis_src * H_src  +  dis_i * H_i ) + b.
 * weight (cout, cin) row-major, bias [cout] or NULL.  x [N, ldx], out [N, ldo], ld = pfn_padded_ld(F), pad columns zero.
 * relu = 1 fuses the caller's ReLU: a unit is off iff its pre-activation compares <= 0 (a NaN stays on and stays NaN).  The
 * decisions are kept in `ws` for the backward call -- as the FIRST n_nodes * pfn_padded_ld(cout) bytes of it, one byte per
 * (row, padded column), 1 = on (valid after a relu = 1 forward; callers may read them) -- together with dis, the packed weight
 * images and the forward's intermediate: the backward call takes the SAME ws, sizes, weight and relu.  Rows are summed in edge-id
 * order by one lane, without float atomics: the same call gives the same bits.  The layer multiplies on the narrower side:
 * pfn_padded_ld(cin) <= pfn_padded_ld(cout): (A X) W^T, else A (X W^T).  `graph_ws` is only read.  No host sync, no allocation.
 * Backward = exact autograd of the above; grad_x [N, ldgx = ldx] (or NULL: not formed), grad_weight (cout, cin) and grad_bias
 * [cout] (or NULL) are OVERWRITTEN, not accumulated.  Argument errors: PFN_EINVAL with pfn_last_error.                       */
size_t pfn_gcn_conv_workspace_bytes(int64_t n_nodes, int64_t e_stored, int cin, int cout);
int pfn_gcn_conv_forward(const void* graph_ws, int64_t n_nodes, int64_t e_stored, int cin, int cout, const float* x,
                         int64_t ldx, const float* weight, const float* bias, int relu, float* out, int64_t ldo,
                         void* ws, size_t ws_bytes, void* stream);
int pfn_gcn_conv_backward(const void* graph_ws, int64_t n_nodes, int64_t e_stored, int cin, int cout, const float* x,
                          int64_t ldx, const float* weight, const float* grad_out, int64_t ldgo, int relu,
                          float* grad_x, int64_t ldgx, float* grad_weight, float* grad_bias, void* ws,
                          size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------- utilities
 * The segmented scatter-add in isolation (PyG SumAggregation / scatter_add_ under propagate):
 * out[i] = sum_{e -> i} x[src(e)], F columns, ld = pfn_padded_ld(F).  Used for the roofline run.  */
int pfn_scatter_add(const void* graph_ws, int64_t n_nodes, int64_t e_stored, const float* x, float* out,
                    int64_t features, void* stream);
/* Row (un)padding between the caller's dense [N, F] tensors and the internal [N, ld] layout.      */
int pfn_pad_rows(const float* src, int64_t ld_src, float* dst, int64_t ld_dst, int64_t n_rows,
                 int64_t features, void* stream);
/* MSELoss(out, y) forward+backward in one pass (train.py:103; utils/training.py:72-74):
 * loss[0] = mean((out-y)^2), grad[i] = 2 (out[i]-y[i]) / count (grad may be NULL).  `ws`: >= 1028 bytes,
 * 256 float partials + one int32 arrival counter at byte 1024 that must be ZERO before the first call and is
 * left zero by every call (one launch: the last block to arrive sums the partials in block order).           */
int pfn_mse_loss(const float* out, const float* y, int64_t count, float* loss, float* grad, void* ws,
                 size_t ws_bytes, void* stream);
/* Masked_L2_loss(output, target, mask) forward+backward (utils/custom_loss_functions.py:10-46; the reference's default
 * --train_loss_fn, utils/argument_parser.py:36; dispatch utils/training.py:61-62), d = out - y:
 *   loss[0] = mean over {mask != 0} of d^2  +  (regularize ? regcoeff * mean over {(1 - mask) != 0} of d^2 : 0)
 *   grad[i] = 2 d_i ( [mask_i != 0] / n1 + regcoeff [mask_i != 1] / n0 )          (grad may be NULL)
 * An empty set gives NaN, as torch's mean of nothing does.  mask: `count` entries, mask_dtype 0 = int64, 1 = float32.
 * `ws`: >= 4128 bytes; its last int32 (byte 4124) is an arrival counter that must be ZERO before the first call and is
 * left zero by every call.                                                                                          */
int pfn_masked_l2_loss(const float* out, const float* y, const void* mask, int mask_dtype, int64_t count,
                       int regularize, float regcoeff, float* loss, float* grad, void* ws, size_t ws_bytes,
                       void* stream);
/* PowerImbalance(x, edge_index, edge_attr) forward+backward (utils/custom_loss_functions.py:99-286; --train_loss_fn
 * power_imbalance, train.py:95-97; dispatch utils/training.py:63-67).  `graph_ws`: the adjacency pfn_graph_build made from
 * the SAME stored-once edge_index with mode -1 (the class undirects by the model's rule, :136-157).  x [N, 4] =
 * normalised (Vm, Va deg, P, Q), edge_attr [e_stored, 2] = normalised (r, x), stats = 12 host floats
 * {xymean[4], xystd[4], edgemean[2], edgestd[2]} (de-normalisation x * std + mean, :127-132).
 *   loss[0] = mean_i (dP_i^2 + dQ_i^2),  grad_x [N, 4] = d loss / d x (NULL to skip).
 * dpq: scratch [N, 2] floats.  `ws`: >= 1280 bytes whose int32 at byte 1024 is an arrival counter that must be ZERO before
 * the first call and is left zero by every call.                                                                       */
int pfn_power_imbalance(const void* graph_ws, int64_t n_nodes, int64_t e_stored, const float* x, const float* edge_attr,
                        const float* stats, float* loss, float* grad_x, float* dpq, void* ws, size_t ws_bytes, void* stream);
/* Dropout bookkeeping (nn.Dropout, networks/MPN.py:496,546-547).  The train-mode epilogues draw their mask from
 * Philox4x32-10 with key {seed[31:0], seed[63:32] ^ offset[63:32]} and counter {row, column / 4, layer index i of
 * `layers`, offset[31:0]}; an element is KEPT (and scaled by 1/(1-p)) iff its uniform >= p.  This debug/verification entry
 * writes the keep mask (1.0 / 0.0, [rows, ncols] unpadded) layer `layer` uses for the CURRENT {seed, offset} of
 * `rng_state` (after a training forward: the mask that forward applied), so a train-mode pass can be replayed elsewhere. */
int pfn_dropout_mask(const uint64_t* rng_state, int32_t layer, int64_t rows, int64_t ncols, float p, float* keep,
                     void* stream);
/* AdamW on one flat buffer (train.py:123; torch defaults betas (0.9,0.999), eps 1e-8, wd 0.01).
 * `step` is a device int64[2] {completed steps, arrival scratch (zero)}; the call increments step[0] itself,
 * so one launch per update and the whole step stays hipGraph-replayable.                           */
int pfn_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t count,
                   float lr, float beta1, float beta2, float eps, float weight_decay, int64_t* step,
                   void* stream);
/* The same update with the five scalars {lr, beta1, beta2, eps, weight_decay} read from DEVICE memory (`hyper`, float[5]):
 * a launch captured into a hipGraph then follows a learning-rate schedule (train.py:129,145: OneCycleLR) by a 20-byte copy
 * into `hyper` between replays instead of a new capture.                                                              */
int pfn_adamw_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t count,
                       const float* hyper, int64_t* step, void* stream);
/* ... and skipped ON THE DEVICE (nothing updated, the step not counted) when the device scalar `guard` -- normally the step's
 * loss -- is not finite: for a captured training step whose batch could not be validated on the host (a topology per batch: a
 * bad batch arrives as a NaN loss, pfn_graph_poison_if_bad; the reference's train loop, utils/training.py:55-77, would have
 * raised in the forward pass instead of stepping).  `step` is a device int64[3] here: {completed steps, arrival scratch,
 * SKIPPED updates} -- the caller's loop reads step[2] to tell a poisoned / diverged batch from a healthy one (ABI 6).
 * New layer, no reference counterpart.                                                                                   */
int pfn_adamw_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t count,
                           const float* hyper, int64_t* step, const float* guard, void* stream);

/* ------------------------------------------------------------------------------- k-hop locality analysis
 * The device side of utils/explanation.py (counterpart of the reference's explain_epoch, utils/explanation.py:34-114, which
 * reruns the model on the edge list cut down to the m-hop ball around a center bus, PyG k_hop_subgraph(directed=False) over
 * _make_bidirectional(edge_index)).  Additive within ABI 8.  `graph_ws` is an adjacency pfn_graph_build made in mode 1 (always
 * undirect) from ONE graph's stored edge list (n_nodes, e_stored): no entry point assumes that list to be symmetric.
 *
 * Hop distances from each of `n_centers` centers (node ids in [0, n_nodes)): dist[c][v] (uint16, [n_centers][n_nodes], row-major)
 * = BFS hop count, 0xFFFF for a node that is unreachable or farther than `max_hops` (<= 65534); ecc[c] = the largest finite
 * distance, or -1 when some node was not reached.  dist may be NULL (eccentricities only: the all-pairs diameter without an n x n
 * table) while a distance row fits in LDS (n_nodes <= 76800); larger graphs need the buffer.                                   */
int pfn_khop_distances(const void* graph_ws, int64_t n_nodes, int64_t e_stored, const int32_t* centers, int64_t n_centers,
                       int32_t max_hops, uint16_t* dist, int32_t* ecc, void* stream);
/* Ball sizes of every (center, radius r = 0..max_radius) at once, cumulative over r ([n_centers][max_radius + 1] int32):
 * node_count = |{v : dist <= r}|, edge_count = |{edges (u, v) of the bidirectional list : max(dist u, dist v) <= r}|.          */
int pfn_khop_histograms(const void* graph_ws, int64_t n_nodes, int64_t e_stored, const uint16_t* dist, int64_t n_centers,
                        int32_t max_radius, int32_t* node_count, int32_t* edge_count, void* stream);
/* Packs `n_inst` balls as one batch of small graphs.  Instance i = (distance row inst_row[i] of `dist`, whose center is
 * centers[inst_row[i]]; radius inst_radius[i] >= 0; batch position inst_sample[i]); node_off / edge_off [n_inst + 1] are the
 * exclusive offsets of the instances' sizes (node_count / edge_count above), edge_off[n_inst] = total_edges.  Per instance:
 *   node_ids[node_off[i] ...]     the ball's nodes in ascending id order, as batch ids inst_sample * n_nodes + v;
 *   edge_index_out [2][total_edges] the induced edges in the order of the bidirectional list (stored edges in stored order, then
 *                                 their reverses), relabelled to packed rows node_off[i] + local id;
 *   edge_ids                      each edge's id in that list (< e_stored: stored edge k, >= e_stored: reverse of k - e_stored);
 *   center_pos[i]                 the packed row of the center.
 * `edge_index` is the stored list graph_ws was built from.  *err (device int, cleared by the caller) is set when an instance's
 * size disagrees with its offsets (nothing is written past them) or the build recorded an id out of range.  n_nodes <= 38400
 * (the old -> new id map lives in LDS).                                                                                     */
int pfn_khop_pack(const void* graph_ws, int64_t n_nodes, int64_t e_stored, const int64_t* edge_index, const int32_t* centers,
                  const uint16_t* dist, const int32_t* inst_row, const int32_t* inst_radius, const int32_t* inst_sample,
                  const int64_t* node_off, const int64_t* edge_off, int64_t n_inst, int64_t total_edges, int64_t* node_ids,
                  int64_t* edge_index_out, int64_t* edge_ids, int64_t* center_pos, int32_t* err, void* stream);

/* ------------------------------------------------------------------------- mixed-size batches in equal segments
 * A batch whose graphs differ in size, re-laid on the device into n_pad / seg_nodes segments of seg_nodes rows (the plan comes from
 * the host: poweflownet_amd/segpack.py, first-fit-decreasing into bins of max(size) rows): graph g -- the caller's rows
 * ptr[g] .. ptr[g + 1] -- starts at padded row start[g]; the graphs of a segment are contiguous; the last seg_nodes - fill[seg] rows
 * of a segment are padding.  No edge then crosses a multiple of seg_nodes, which is all pfn_graph_segments asks, so the model entry
 * points run on the padded tensors with that seg_nodes; an isolated padding row receives and sends no message and adds exact
 * zeros to every weight gradient.  Per-batch host -> device traffic is ptr, start and fill: O(graphs), not O(nodes).
 *
 * pfn_segpack_pack (two launches, nothing waits across workgroups): ptr [n_graphs + 1], start [n_graphs], fill [n_pad / seg_nodes]
 * int32; x [N, 4] f32; pred_mask [N, 4] (mask_dtype 0: int64, 1: float32); edge_index [2, e_stored] int64 ->
 *   x_pad, mask_pad [n_pad, 4] f32     the rows moved, mask as float, padding rows all zero
 *   edge_index_pad [2, e_stored]       the same edges in the same order, endpoints relabelled (edge_attr and the edge ids stay what
 *                                      they were); an id outside [0, N) becomes -1, which pfn_graph_build then reports
 *   row_of [N], src_of [n_pad] int32   the padded row of every real row, and the real row of every padded row (-1: padding)
 * x, pred_mask, edge_index and their padded copies must be 16-byte aligned.                                                     */
int pfn_segpack_pack(const int32_t* ptr, const int32_t* start, const int32_t* fill, int64_t n_graphs, int64_t n_nodes,
                     int64_t seg_nodes, int64_t n_pad, const float* x, const void* pred_mask, int mask_dtype, const int64_t* edge_index,
                     int64_t e_stored, float* x_pad, float* mask_pad, int64_t* edge_index_pad, int32_t* row_of, int32_t* src_of,
                     void* stream);
/* dst[i, :f] = src_pad[row_of[i], :f] for the n_nodes real rows (separate leading dimensions): un-pads outputs, input gradients
 * and exported gates.                                                                                                           */
int pfn_segpack_gather_rows(const float* src_pad, int64_t ld_src, int64_t n_pad, const int32_t* row_of, float* dst, int64_t ld_dst,
                            int64_t n_nodes, int64_t f, void* stream);
/* Its adjoint, dst_pad[row_of[i], :f] = src[i, :f], evaluated as a gather through src_of: ONE launch writes every row of dst_pad,
 * the padding rows as zeros (no memset beside it).                                                                              */
int pfn_segpack_scatter_rows(const float* src, int64_t ld_src, int64_t n_nodes, const int32_t* src_of, float* dst_pad, int64_t ld_dst,
                             int64_t n_pad, int64_t seg_nodes, int64_t f, void* stream);

/* ------------------------------------------------------------------- mixed training batches in slot buckets
 * A training batch of a split with several grid cases, described by how many samples of each case it holds, each count rounded
 * up to a granule (poweflownet_amd/segpack.py: bucket_of, slot_layout, slot_table).  A bucket has a fixed list of slots -- case
 * after case -- and with it a static shape, topology (edge_index is a constant of the bucket and is not touched here) and segment
 * layout; spare slots hold "fillers": real samples with validity 0.
 *
 * pfn_segpack_gather_slots (ONE launch, nothing waits across workgroups, no host sync: capturable) is the fused collate + pack:
 * for every slot s it copies sample slot_table[s][0] of case slot_case[s] from that case's dense block -- x, y [samples, n, 4]
 * f32, pred_mask [samples, n, 4] (mask_dtype 0: int64, 1: float32; written in the same dtype), bus_type [samples, n] int64,
 * edge_attr [samples, e, 2] f32 -- to the padded rows slot_row0[s] .. + n and the edges slot_edge0[s] .. + e of the batch, and
 * writes valid[row] = slot_table[s][1] != 0 for the slot's rows.  row_slot [n_pad] names the slot of every padded row (-1: a
 * padding row -- written as zeros in every row tensor, valid 0), edge_slot [n_edges] the slot of every edge; both, like
 * slot_case / slot_row0 / slot_edge0 [n_slots], are constants of the bucket.  slot_table: [n_slots, 2] int32, the only per-batch
 * input.  A slot, case or sample index outside its range writes zero rows with valid 0 instead of being followed (the host
 * planner rejects them first).  All float / mask pointers 16-byte aligned; at most PFN_SLOT_MAX_CASES cases.                  */
#define PFN_SLOT_MAX_CASES 8
typedef struct pfn_slot_case {
    const float* x;
    const float* y;
    const void* pred_mask;
    const int64_t* bus_type;
    const float* edge_attr;
    int64_t n_nodes, n_edges, n_samples;
} pfn_slot_case;
int pfn_segpack_gather_slots(const pfn_slot_case* cases, int32_t n_cases, int32_t mask_dtype, const int32_t* slot_case,
                             const int32_t* slot_row0, const int32_t* slot_edge0, const int32_t* row_slot, const int32_t* edge_slot,
                             const int32_t* slot_table, int64_t n_slots, int64_t n_pad, int64_t n_edges, float* x, float* y,
                             void* pred_mask, int64_t* bus_type, float* edge_attr, int32_t* valid, void* stream);
/* pfn_mse_loss / pfn_masked_l2_loss over the rows with valid[row] != 0 only (out, y, mask: [n_rows, 4]; valid: [n_rows] int32).
 * The denominators are counted on the device over the valid rows (4 x the valid rows; the two mask counts).  grad (optional):
 * exactly 0 on an invalid row; on a valid row the existing kernels' expression, so bit-identical to pfn_mse_loss /
 * pfn_masked_l2_loss run on the compacted valid rows.  loss[0]: block partials summed in block order (deterministic), equal to
 * the compacted call's value up to the rounding of another summation order.  No valid row at all: loss[0] = 0 and grad = 0
 * (a valid row but an empty mask set gives NaN, as pfn_masked_l2_loss does).  Two launches, no host sync.
 * `ws`: >= 4128 bytes; its last int32 (byte 4124) is an arrival counter, zero before the first call and after every call.     */
int pfn_mse_loss_rows(const float* out, const float* y, const int32_t* valid, int64_t n_rows, float* loss, float* grad, void* ws,
                      size_t ws_bytes, void* stream);
int pfn_masked_l2_loss_rows(const float* out, const float* y, const void* mask, int mask_dtype, const int32_t* valid, int64_t n_rows,
                            int regularize, float regcoeff, float* loss, float* grad, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------- evaluation metrics
 * Every metric test.py reports (reference test.py:113-130; utils/custom_loss_functions.py:10-97), from one pass over a batch's
 * output rows, with the epoch's running sums kept on the device.  Additive within ABI 8.  New layer: the reference runs the
 * model once per metric and syncs the host on every term of every batch (utils/evaluation.py:106-165).
 *
 * The batch terms, one fp32 each, in this order.  With m = mask as float, d = out - y, cnt[f] = sum_rows m[:, f]:
 *   CNT_*            cnt[f]
 *   L2_* / L1_*      MaskedL2V2 / MaskedL1 on the rows as given: column means pf[f] = sum m * err / max(cnt[f], 1e-6) with err = d^2
 *                    or |d| (the four named features), TOTAL = sum_f pf[f] * max(cnt[f], 1e-6) / max(sum_f cnt[f], 1e-6),
 *                    BALANCED = mean_f pf[f]
 *   L2D_* / L1D_*    the same on de-normalised rows: err from d * std[f] -- the mean cancels, and forming out * std + mean and
 *                    y * std + mean first loses up to 7.6e-5 relative in fp32 where (out - y) * std stays within 3.3e-7
 *   ML2_SELECTED     Masked_L2_loss's mean of d^2 over mask != 0;  ML2_REGULARIZER  its mean over 1 - mask != 0
 *                    (an empty selection: 0/0 = NaN, as pfn_masked_l2_loss)
 *   MSE              mean of d^2 over all 4 n entries (an empty batch: NaN)
 * The mask MULTIPLIES (error * mask.float()): a NaN under a zero mask entry poisons its column, as in the reference.        */
enum pfn_eval_term {
    PFN_EVAL_CNT_VM = 0, PFN_EVAL_CNT_VA, PFN_EVAL_CNT_P, PFN_EVAL_CNT_Q,
    PFN_EVAL_L2_TOTAL, PFN_EVAL_L2_BALANCED, PFN_EVAL_L2_VM, PFN_EVAL_L2_VA, PFN_EVAL_L2_P, PFN_EVAL_L2_Q,
    PFN_EVAL_L2D_TOTAL, PFN_EVAL_L2D_BALANCED, PFN_EVAL_L2D_VM, PFN_EVAL_L2D_VA, PFN_EVAL_L2D_P, PFN_EVAL_L2D_Q,
    PFN_EVAL_L1_TOTAL, PFN_EVAL_L1_BALANCED, PFN_EVAL_L1_VM, PFN_EVAL_L1_VA, PFN_EVAL_L1_P, PFN_EVAL_L1_Q,
    PFN_EVAL_L1D_TOTAL, PFN_EVAL_L1D_BALANCED, PFN_EVAL_L1D_VM, PFN_EVAL_L1D_VA, PFN_EVAL_L1D_P, PFN_EVAL_L1D_Q,
    PFN_EVAL_ML2_SELECTED, PFN_EVAL_ML2_REGULARIZER, PFN_EVAL_MSE,
    PFN_EVAL_N_TERMS
};
/* index of the int64 batch counter behind the PFN_EVAL_N_TERMS doubles of an epoch accumulator (32 x 8 bytes in all) */
#define PFN_EVAL_ACC_BATCHES PFN_EVAL_N_TERMS
/* One launch per batch, no host sync, capturable.  out, y [n_rows, 4] f32; x [n_rows, 4] f32 or NULL; mask [n_rows, 4]
 * (mask_dtype 0: int64, 1: float32) -- all 16-byte aligned.  std4: four HOST floats baked into the launch (NULL: 1).
 *   terms [PFN_EVAL_N_TERMS] f32    the batch terms
 *   epoch_acc (optional)            double[PFN_EVAL_N_TERMS] + the int64 batch counter: acc[k] += w * (double)terms[k], product
 *                                   and sum rounded separately; w = 1 on the FIRST batch (counter 0) when first_unweighted is
 *                                   set (the quirk of evaluate_epoch_v2, reference :158-163), else `weight`; counter += 1.
 *                                   Cleared by the caller between epochs, outside a captured graph.
 *   mixed_out (optional, needs x)   [n_rows, 4] f32 = out * mask + x * (1 - mask), bit for bit the torch expression
 * Block partials are combined by the last arriver in an order fixed by the grid: a launch is a pure function of its inputs.
 * n_rows == 0 writes the terms of an empty batch (0 for the clamped means, NaN for the selected means and the MSE).
 * `ws`: >= 26640 bytes; its int32 at byte 26624 is an arrival counter, zero before the first call and after every call.    */
int pfn_eval_metrics(const float* out, const float* y, const float* x, const void* mask, int mask_dtype, int64_t n_rows,
                     const float* std4, double weight, int first_unweighted, float* terms, double* epoch_acc, float* mixed_out,
                     void* ws, size_t ws_bytes, void* stream);
/* acc[0] += (double)loss[0] * w (w as above, from the int64 batch counter acc[1]); acc[1] += 1.  One thread: lets the per-batch
 * body of an evaluation loop with ANY loss be captured with its running sum on the device; the double is exactly what the host
 * loop's `loss.item() * len(data)` adds.                                                                                   */
int pfn_eval_accumulate(const float* loss, double weight, int first_unweighted, double* acc, void* stream);

/* ------------------------------------------------------------------------------- per-bus error analysis
 * WHERE the error of an evaluation split is (reference error_per_feature.py:120-172, :247-324, :362-405): the de-normalised error
 * and prediction of every bus of every sample, running moments per (bus, feature, mask group), and a histogram per (bus, feature).
 * Additive within ABI 8.  New layer: the reference runs one forward and one `.cpu()` per sample and n x 4 np.histogram calls.
 *
 * pfn_bus_errors_accumulate: one launch per batch, no host sync, capturable.  out, y, mask [n_graphs * n_bus, 4] are a uniform
 * batch of ONE case, graph g owning rows [g n_bus, (g + 1) n_bus); mask_dtype 0: int64, 1: float32; all 16-byte aligned.
 * std4 / mean4: four HOST floats each, baked into the launch (NULL: 1 / 0).
 *   error        e = (out - y) * std[f] in fp32, difference and product rounded separately (the expression of pfn_eval_metrics'
 *                de-normalised terms)
 *   prediction   out * std[f] + mean[f], product and sum rounded separately: torch's `denormalize`, bit for bit
 *   err_table, pred_table (each optional; [table_rows, n_bus, 4] f32): graph g writes its n_bus rows to row sample_idx[g]
 *                (device int64 [n_graphs]; may be NULL when both tables are).  A sample_idx[g] outside [0, table_rows) sets bit 0
 *                of flags[0] (a plain vector store) and the graph is skipped entirely, tables and moments: nothing is ever
 *                written outside a table.
 *   moments      double[n_bus][4][2][6], accumulated INTO (cleared by the caller between epochs, outside a captured graph, with
 *                min = +inf and max = -inf): group 0 = entries with mask != 0 (predicted), group 1 = mask == 0 (given); the
 *                six values are {count, sum e, sum |e|, sum e^2, min e, max e}, every e widened to double first.  min / max
 *                ignore NaN (fmin / fmax); the sums propagate it.
 * One owner per (bus, feature), a fixed work split and combine order, no float atomics: a launch is a pure function of its
 * inputs and of the moments it found.
 *
 * pfn_bus_errors_histogram: one launch over a finished table [n_samples, n_bus, 4] f32.  hist [n_bus, 4, nbins] and outside
 * [n_bus, 4, 3] (below the first edge, above the last, NaN) are OVERWRITTEN.  The binned value is v = table[s, b, f] * scale[b, f]
 * (one fp32 product; scale [n_bus, 4] f32 or NULL: v = table); the rule is np.histogram(v, bins=edges[f]) with an explicit edge
 * array (edges: DEVICE double [4, nbins + 1], increasing), compared in float64: bin i holds edges[i] <= v < edges[i + 1], the last
 * bin also v == edges[nbins]; nothing counted in `outside` enters a bin.  A workgroup owns a tile of consecutive buses with its
 * counters and the edges in LDS (integer LDS atomics, no global atomics).  nbins in 1..2048, n_samples < 2^31 (uint32 counts):
 * anything else is PFN_EINVAL.                                                                                              */
int pfn_bus_errors_accumulate(const float* out, const float* y, const void* mask, int mask_dtype, int64_t n_graphs, int64_t n_bus,
                              const float* std4, const float* mean4, const int64_t* sample_idx, int64_t table_rows, float* err_table,
                              float* pred_table, double* moments, int32_t* flags, void* stream);
int pfn_bus_errors_histogram(const float* table, int64_t n_samples, int64_t n_bus, const float* scale, const double* edges, int nbins,
                             uint32_t* hist, uint32_t* outside, void* stream);

/* ------------------------------------------------------------------------------------- per-line branch flows
 * pfn_branch_flows (csrc/branch_flows.hip): the line currents and line flows that one or two finished bus tables imply, their error
 * and its running moments per (line, quantity), in two launches and without a host sync (capturable).  The table the reference's
 * error_per_feature.py:186-223 left commented out.
 *   pred, truth  [n_samples, n_bus, 4] f32 rows (Vm, Va in degrees, P, Q); only Vm and Va are read.  A table whose `*_normalised`
 *                flag is set is de-normalised first as v * std4[f] + mean4[f], product and sum rounded separately (the prediction
 *                expression of pfn_bus_errors_accumulate; four HOST floats each, NULL: 1 / 0).  truth may be NULL: the flows of one
 *                table only -- flows_true, err_table and moments must then be NULL too.
 *   edge_index   DEVICE int64 local bus ids: [2, n_lines] for all samples (lines_per_sample == 0) or [n_samples, 2, n_lines].
 *   edge_attr    f32 (r, x): [n_lines, 2] (attr_per_sample == 0) or [n_samples, n_lines, 2]; de-normalised with one fmaf per value,
 *                fmaf(v, edge_std2[f], edge_mean2[f]) (two HOST floats each, NULL: 1 / 0), as pfn_power_imbalance does.
 * Per (sample, stored line i = edge_index[0] -> j = edge_index[1]) four fp32 quantities, PowerImbalance.message's convention with
 * no unit conversion:  e = Vm cos(Va pi/180), f = Vm sin(Va pi/180), d = r^2 + x^2, g = r/d, b = -x/d, de = e_i - e_j, df = f_i - f_j
 *   0  I     sqrt(de^2 + df^2) / sqrt(d)                                        the current magnitude
 *   1  P     g (e_i e_j - e_i^2 + f_i f_j - f_i^2) + b (f_i e_j - e_i f_j)      the message of the stored direction
 *   2  Q     g (f_i e_j - e_i f_j) + b (-e_i e_j + e_i^2 - f_i f_j + f_i^2)
 *   3  loss  g (de^2 + df^2) = r I^2, >= 0 whenever r >= 0
 * (the reverse direction's message is -P - r I^2, -Q - x I^2).  r = x = 0: g and b are 0/0, so P, Q and loss are NaN as in
 * pfn_power_imbalance; I is |dV| / 0.
 *   flows_pred, flows_true, err_table   each optional, [n_samples, n_lines, 4] f32; err_table = flows_pred - flows_true, ONE fp32
 *                subtraction of the two written values.
 *   moments      optional double[n_lines][4][6] = {count, sum, sum |e|, sum e^2, min, max} of the error, accumulated INTO (cleared
 *                by the caller, min = +inf and max = -inf); min / max ignore NaN, the sums propagate it.  Without err_table the
 *                error table goes to `ws` (pfn_branch_flows_workspace_bytes(n_samples, n_lines, 1) bytes; PFN_ENOSPACE otherwise).
 *   flags        bit 0 of flags[0] is set (a plain vector store) when a line names a bus outside [0, n_bus): that (sample, line)'s
 *                values are NaN, it is left out of the moments, and the id is never followed.
 * Buses up to pfn_branch_flows_lds_max_bus() keep a sample's rectangular voltages in LDS (one sincos per bus and table); beyond,
 * they are formed per line end from global memory.  One owner per (line, quantity), a fixed work split and combine order, no
 * float atomics: a call is a pure function of its inputs and of the moments it found.                                        */
int64_t pfn_branch_flows_lds_max_bus(void);
size_t pfn_branch_flows_workspace_bytes(int64_t n_samples, int64_t n_lines, int moments_without_err_table);
int pfn_branch_flows(const float* pred, int pred_normalised, const float* truth, int truth_normalised, int64_t n_samples, int64_t n_bus,
                     const float* std4, const float* mean4, const int64_t* edge_index, int lines_per_sample, int64_t n_lines,
                     const float* edge_attr, int attr_per_sample, const float* edge_std2, const float* edge_mean2, float* flows_pred,
                     float* flows_true, float* err_table, double* moments, int32_t* flags, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------- power-flow solver
 * The classical-solver side of the reference -- pandapower's Newton-Raphson behind dataset_generator.py:142 and its DC power flow
 * behind dc_error.py:120 -- for this project's network model, batched: ONE launch, one workgroup per sample, no host sync, no
 * allocation (capturable).  The mismatch is exactly pfn_power_imbalance's dP_i, dQ_i: series admittance only (g = r / (r^2 + x^2),
 * b = -x / (r^2 + x^2)), every stored line counted in both directions (parallel lines add), P and Q demand-positive per-unit, Va in
 * degrees; no shunt, charging, tap or unit conversion.  Bus types: 0 slack (gives Vm, Va), 1 PV (Vm, P), 2 PQ (P, Q); exactly one
 * slack.  Unknowns: Va at the non-slack buses, Vm at the PQ buses, m = (n_bus - 1) + n_pq.
 * THE ONE EXCEPTION to "all floating point is fp32": the inputs and the table are fp64 (raw dataset files are).
 *   edge_index   DEVICE int64 local bus ids: [2, n_lines] for all samples (lines_per_sample == 0) or [n_samples, 2, n_lines].
 *   rx           f64 [n_samples, n_lines, 2] = (r, x) per sample.
 *   bus_type     int32 [n_bus], shared by the samples.  n_pv, n_pq: its counts, HOST ints -- they decide m, the route and the LDS
 *                size.  The kernel counts the device array itself: where it disagrees (or holds a type outside 0..2, or not exactly
 *                one slack) nothing is solved, every status is -5 and bit 0 of flags[0] is set (a plain vector store).
 *   spec         f64 [n_samples, n_bus, 4] = (Vm, Va, P, Q): only the entries the bus type gives are read.
 *   mode 0 (AC)  Newton-Raphson in polar form from a flat start (Vm = 1 at PQ buses, Va = the slack's).  State, mismatch and the
 *                convergence test are fp64; the Jacobian is assembled analytically and factorised in fp32 (LU, partial pivoting, ties
 *                to the lowest row), the update is solved from that factor with an fp64 right-hand side.  Stops when
 *                max(|dP|, |dQ|) over the equations < tol, or after max_iter Jacobian solves.
 *   mode 1 (DC)  the same loop on the linear mismatch F(theta) = B' theta + P over the non-slack buses, B' the Laplacian of 1 / x:
 *                iterative refinement of an fp32 factor under the same fp64 tol.  m = n_bus - 1.
 *   table        f64 [n_samples, n_bus, 4], 32-byte aligned.  AC: (Vm, Va, P, Q) with the slack's P, Q and the PV buses' Q the
 *                aggregated line sums, everything else as given or solved.  DC: Vm as given at slack and PV buses and 1 at PQ
 *                buses, Va = theta, P as given with the slack's the aggregated line sum (lossless: minus the sum of the others),
 *                Q NaN.  A failed sample's rows are NaN; it touches nothing of another sample.
 *   status       int32 [n_samples]: >= 0 the number of Jacobian solves used; -1 not converged in max_iter; -2 singular (a pivot of
 *                magnitude <= 1e-30 or NaN, e.g. a bus without a line); -3 non-finite mismatch; -4 a line names a bus outside
 *                [0, n_bus) (never followed); -5 bus_type disagrees with n_pv / n_pq (see above).
 *   residual     f64 [n_samples]: the last max |F| (NaN where none was formed).
 *   route        0 auto, 1 LDS, 2 global.  LDS: the fp32 matrix (m rows of m | 1 floats) sits behind the sample's vectors in the
 *                160 KiB of a compute unit -- up to m = 195 at 118 buses; route 1 beyond that is PFN_EINVAL.  Global: the matrix
 *                lives in a per-sample slab of `ws`, same code, up to pfn_powerflow_max_unknowns() unknowns; beyond that PFN_EINVAL:
 *                a sparse factorisation is needed.  pfn_powerflow_workspace_bytes(n_samples, n_bus, n_lines, n_pq, route) is what the
 *                route needs in mode 0 (for mode 1 pass n_pq = 0: its m is n_bus - 1) -- 0 exactly when it is the LDS route, which is
 *                how a caller learns what route 0 takes; too little is PFN_ENOSPACE.
 * pfn_powerflow_solve_init: everything above, plus a warm start and the fast-decoupled modes; pfn_powerflow_solve is this call with
 * init = NULL and accepts modes 0 and 1 only, its results unchanged bit for bit.
 *   init         DEVICE f64 [n_samples, n_bus, 2] = (Vm, Va in degrees), 8-byte aligned, or NULL for the flat start.  Read: Va at the
 *                non-slack buses and Vm at the PQ buses (mode 1: Va only -- its Vm is no unknown); the slack's Vm / Va and a PV bus's
 *                Vm always come from `spec`, whatever `init` holds there.  A non-finite entry that is read gives that sample status
 *                -3, NaN rows and a NaN residual, and touches no other sample.  A start whose max |F| < tol returns status 0 (nothing
 *                is solved) with the table finished from it.
 *   mode 2 (fdxb), mode 3 (fdbx)  the fast-decoupled iterations.  State, mismatch and convergence test are mode 0's fp64 code.  B'
 *                (order n_bus - 1, the angle buses) and B'' (order n_pq, the PQ buses) are Laplacians over the stored lines, parallel
 *                lines adding: XB takes B' from 1 / x and B'' from -b = x / (r^2 + x^2), BX swaps the two.  Both are built ONCE per
 *                sample in fp32, inverted in place once (Gauss-Jordan without pivoting: symmetric and diagonally dominant for x > 0)
 *                and stay resident together; a half-iteration is a mat-vec with the explicit inverse, fp64 sums:
 *                theta -= B'^-1 (dP / Vm) over the angle buses, then Vm -= B''^-1 (dQ / Vm) over the PQ buses, alternating, the P
 *                half first (the sign is that of the demand-positive mismatch).  The mismatch is re-formed and tested after every
 *                half-iteration; max_iter and a status >= 0 count HALF-iterations.  n_pq == 0: only the P half runs.  Statuses -1
 *                ... -5 as above; -2: a pivot of either matrix.  n_bus - 1 <= pfn_powerflow_max_unknowns().
 *   route        modes 2, 3: LDS when the vectors (40 n + 16 m bytes, m = n_bus - 1 + n_pq: F / Vm sits behind F) plus BOTH
 *                matrices, each with its odd leading dimension, fit the same 160 KiB - 1 KiB; otherwise per-sample slabs of `ws`
 *                holding the two.  256 or 1024 threads by the rule of modes 0 / 1 applied to the larger of the two orders.
 *                pfn_powerflow_workspace_bytes_mode(n_samples, n_bus, n_lines, n_pq, mode, route) is pfn_powerflow_workspace_bytes
 *                with the mode it is asked about (n_pq = the real count in every mode; modes 0 and 1 answer as the function above
 *                does): 0 exactly on the LDS route.
 * One owner per matrix row, sequential sums in stored line order, only max-reductions across threads, no float atomics: a
 * sample's result is a pure function of its own inputs, bit for bit, whatever the batch around it.                          */
int64_t pfn_powerflow_max_unknowns(void);
size_t pfn_powerflow_workspace_bytes(int64_t n_samples, int64_t n_bus, int64_t n_lines, int64_t n_pq, int route);
size_t pfn_powerflow_workspace_bytes_mode(int64_t n_samples, int64_t n_bus, int64_t n_lines, int64_t n_pq, int mode, int route);
int pfn_powerflow_solve_init(const int64_t* edge_index, int lines_per_sample, int64_t n_lines, const double* rx, const int32_t* bus_type,
                             const double* spec, const double* init, int64_t n_samples, int64_t n_bus, int64_t n_pv, int64_t n_pq, int mode,
                             double tol, int max_iter, int route, double* table, int32_t* status, double* residual, int32_t* flags,
                             void* ws, size_t ws_bytes, void* stream);
int pfn_powerflow_solve(const int64_t* edge_index, int lines_per_sample, int64_t n_lines, const double* rx, const int32_t* bus_type,
                        const double* spec, int64_t n_samples, int64_t n_bus, int64_t n_pv, int64_t n_pq, int mode, double tol,
                        int max_iter, int route, double* table, int32_t* status, double* residual, int32_t* flags, void* ws,
                        size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------- generator Q-limits, per-sample bus types
 * pfn_powerflow_solve_qlim (csrc/powerflow_qlim.hip): mode 0 of pfn_powerflow_solve_init on the dense route with the bus types the
 * SAMPLE's and the reference's enforce_q_lims loop inside the kernel.  ONE launch, one workgroup per sample, no host sync, no
 * allocation (capturable).  edge_index, lines_per_sample, rx, spec, init, tol, max_iter, table, status, residual, flags as there.
 *   bus_type     int32 [n_bus] (types_per_sample = 0) or [n_samples, n_bus] (1).  The workgroup copies its row into LDS and owns it:
 *                the host passes no counts.  A row that does not hold exactly one slack and only types 0, 1, 2 gives THAT sample
 *                status -5 (and sets bit 0 of flags[0]).
 *   q_limits     f64 [n_bus, 2] (limits_per_sample = 0) or [n_samples, n_bus, 2] (1) = (lo, hi) on the TABLE's Q column, i.e.
 *                demand-positive per-unit: a generator's [Qmin, Qmax] arrives as [-Qmax, -Qmin].  Read at PV buses only; NaN or
 *                +-inf: no limit on that side.  NULL: no limits at all (the plain solve with per-sample types).
 *   rounds       After an inner Newton loop converges, the line sum sq of every PV bus is tested: sq > hi + q_tol makes the bus PQ
 *                with Q = hi, sq < lo - q_tol with Q = lo.  All violators of a round switch together, none switches back, the slack
 *                is never limited.  No violator: done.  Otherwise the unknowns are numbered again and Newton goes on from the
 *                current state (a switched bus's Vm starts at the value it held).  max_iter bounds the solves of EACH inner loop,
 *                max_rounds the re-solves.
 *   table        as mode 0's; a switched bus holds its solved Vm and, bit for bit, the limit as Q; a bus still PV its line sum.
 *   bus_type_out int32 [n_samples, n_bus]: the final types;  rounds int32 [n_samples]: the re-solves (0: no limit was hit).
 *   status       >= 0: the Jacobian solves over all rounds; -1 ... -5 as above; -7: limits still violated after max_rounds
 *                re-solves.  A failed sample has NaN rows, its INPUT types in bus_type_out and the rounds it completed.
 *   route        0 auto, 1 LDS, 2 global.  Storage is sized for the worst case, every non-slack bus PQ: m_max = 2 (n_bus - 1)
 *                unknowns, whatever the types are.  LDS when the vectors (52 n_bus + 8 m_max bytes) and m_max rows of m_max | 1
 *                floats fit 160 KiB - 1 KiB -- 70 buses do, 118 do not --, else a per-sample slab of `ws`;
 *                pfn_powerflow_qlim_workspace_bytes(n_samples, n_bus, route) is what the route needs, 0 exactly on the LDS route.
 *                m_max > pfn_powerflow_max_unknowns() is PFN_EINVAL.                                                              */
size_t pfn_powerflow_qlim_workspace_bytes(int64_t n_samples, int64_t n_bus, int route);
int pfn_powerflow_solve_qlim(const int64_t* edge_index, int lines_per_sample, int64_t n_lines, const double* rx, const int32_t* bus_type,
                             int types_per_sample, const double* spec, const double* init, const double* q_limits, int limits_per_sample,
                             int64_t n_samples, int64_t n_bus, double tol, double q_tol, int max_iter, int max_rounds, int route,
                             double* table, int32_t* status, double* residual, int32_t* flags, int32_t* bus_type_out, int32_t* rounds,
                             void* ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------- sparse power-flow route
 * The same Newton / DC loop beyond pfn_powerflow_max_unknowns() (csrc/powerflow_sparse.hip), for ONE line list [2, n_lines] shared by
 * the samples: a static minimum-degree order and the filled pattern under it are planned once per grid on the host, the fp32
 * factor is sparse, left-looking by columns, not pivoted.  Modes 0 (AC) and 1 (DC); the fast-decoupled modes follow below.
 * pfn_powerflow_sparse_plan (csrc/powerflow_plan.cpp; HOST arrays in, HOST blob out, no device call): edge_index int64 [2, n_lines],
 *   bus_type int32 [n_bus].  pfn_powerflow_sparse_plan_bytes is the blob's size (0 on error); the blob is relocatable -- 32 int32
 *   header words (magic, version, n, e, m, mode, slab positions, nnz(L), the multiply-adds of one factor as lo / hi words, ...), then
 *   the sections csrc/powerflow_plan.hpp lists, by byte offset.  Unknowns: theta of the non-slack buses and Vm of the PQ buses (mode
 *   1: theta only) in a minimum-degree order of the bus graph (parallel lines collapse, ties to the lowest bus id: the plan is a pure
 *   function of its inputs), a bus's theta directly before its Vm.  PFN_EINVAL, nothing written: a line that names a bus outside
 *   [0, n_bus), not exactly one slack, a bus type outside 0, 1, 2, a plan whose offsets do not fit int32.  A bus without a line is no
 *   error: it is a zero pivot at solve time.
 * pfn_powerflow_solve_sparse: ONE launch, one workgroup per sample, no host sync, no allocation (capturable).  edge_index, rx,
 *   bus_type, spec, init, table, status, residual, flags, tol, max_iter as in pfn_powerflow_solve_init with lines_per_sample = 0;
 *   plan_header: the first 32 words of the blob on the HOST (sizes the launch); plan_dev: the whole blob on the DEVICE, 16-byte
 *   aligned; ws: pfn_powerflow_sparse_workspace_bytes(n_samples, plan_header) bytes (state, right-hand side and the factor's slab per
 *   sample), too little is PFN_ENOSPACE; threads: 0 (64 lanes per sample, 256 once the plan's longest column exceeds 128), or 64 /
 *   256 to force one.  PFN_EINVAL: a plan for another n_bus / n_lines / mode; a plan with 32-bit row ids (m > 65535) or whose
 *   work vector (4 m bytes) does not fit LDS.  Statuses as above, and -6: the device line list or
 *   bus types are not the ones the plan was built from (-5 with flag bit 0 for the types, as on the dense route).  Results are a pure
 *   function of the sample's inputs and the plan, bit for bit, whatever the batch.                                            */
#define PFN_POWERFLOW_STALE_PLAN (-6)
size_t pfn_powerflow_sparse_plan_bytes(const int64_t* edge_index, int64_t n_lines, const int32_t* bus_type, int64_t n_bus, int mode);
int pfn_powerflow_sparse_plan(const int64_t* edge_index, int64_t n_lines, const int32_t* bus_type, int64_t n_bus, int mode, void* plan,
                              size_t plan_bytes);
size_t pfn_powerflow_sparse_workspace_bytes(int64_t n_samples, const void* plan_header);
int pfn_powerflow_solve_sparse(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                               const double* init, int64_t n_samples, int64_t n_bus, int mode, double tol, int max_iter,
                               const void* plan_header, const void* plan_dev, int threads, double* table, int32_t* status,
                               double* residual, int32_t* flags, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------- sparse power-flow route, fast-decoupled modes
 * Modes 2 (fdxb) and 3 (fdbx) of pfn_powerflow_solve_init beyond pfn_powerflow_max_unknowns() (csrc/powerflow_sparse_fd.hip): B'
 * over the n_bus - 1 angle buses and B'' over the PQ buses are constant, so each is assembled and factored ONCE per sample (sparse,
 * fp32, left-looking, not pivoted) and a half-iteration is one mismatch walk and one pair of fp64 substitutions.  Half-iterations,
 * their count in `status`, the stopping rule, the warm start and the table are those of the dense fast-decoupled route.
 * pfn_powerflow_sparse_fd_plan (HOST arrays in, HOST blob out): ONE plan serves both variants -- an outer header of 32 int32 words
 *   (a magic of its own, n, e, m_p = n_bus - 1 in the usual words, m_q = the number of PQ buses in word 15, slab positions, nnz(L),
 *   multiply-adds and bytes as TOTALS over both halves, the longer of the two longest columns) and two embedded sub-plans at the
 *   byte offsets in words 16 and 17 -- P, byte for byte the mode-1 plan, and Q over the bus graph induced on the PQ buses under its
 *   own minimum-degree order (csrc/powerflow_plan.hpp).  pfn_powerflow_sparse_fd_plan_bytes is its size (0 on error).  PFN_EINVAL,
 *   nothing written: pfn_powerflow_sparse_plan's cases and a blob that is too small.  A grid without a PQ bus is valid (m_q = 0).
 * pfn_powerflow_solve_sparse_fd: ONE launch, one workgroup per sample, no host sync, no allocation (capturable); the arguments of
 *   pfn_powerflow_solve_sparse with mode 2 or 3, plan_header the outer header on the HOST, ws of
 *   pfn_powerflow_sparse_fd_workspace_bytes(n_samples, plan_header) bytes.  max_iter counts half-iterations.  Statuses as there:
 *   -2 a tiny or NaN pivot in either matrix, -5 (flag bit 0) bus types that disagree with either half, -6 another line list.   */
size_t pfn_powerflow_sparse_fd_plan_bytes(const int64_t* edge_index, int64_t n_lines, const int32_t* bus_type, int64_t n_bus);
int pfn_powerflow_sparse_fd_plan(const int64_t* edge_index, int64_t n_lines, const int32_t* bus_type, int64_t n_bus, void* plan,
                                 size_t plan_bytes);
size_t pfn_powerflow_sparse_fd_workspace_bytes(int64_t n_samples, const void* plan_header);
/* pfn_powerflow_sparse_plan_into (HOST arrays in, HOST blob out): the plan of mode 0, 1 or 2 (the fast-decoupled plan) built straight
 *   into a buffer the caller sized by a guess, ONE elimination per matrix where pfn_powerflow_sparse_plan_bytes + _plan run two (the
 *   fast-decoupled pair: six) -- for callers that plan often, as the per-sample-topology route does once per chunk.  *needed gets the
 *   plan's size whenever the inputs are valid.  PFN_OK: the blob, byte for byte the two-call path's, stands in plan[0, *needed);
 *   with plan_bytes < *needed (or plan null) it is PFN_ENOSPACE: come again with *needed bytes.  PFN_EINVAL: as the two-call path. */
int pfn_powerflow_sparse_plan_into(const int64_t* edge_index, int64_t n_lines, const int32_t* bus_type, int64_t n_bus, int mode, void* plan,
                                   size_t plan_bytes, size_t* needed);
int pfn_powerflow_solve_sparse_fd(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                                  const double* init, int64_t n_samples, int64_t n_bus, int mode, double tol, int max_iter,
                                  const void* plan_header, const void* plan_dev, int threads, double* table, int32_t* status,
                                  double* residual, int32_t* flags, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------- sparse power-flow routes, per-sample topologies
 * A factorisation under a static order without pivoting stays valid on any SUPERSET of a sample's pattern: a line the sample
 * lacks is a structural zero.  So a chunk of samples with their own line lists shares ONE plan, built by pfn_powerflow_sparse_plan
 * / _fd_plan on a COVER list that holds every line of every sample, and the kernels are told per sample which cover lines exist.
 * A line's key is its unordered bus pair, min * n_bus + max.
 * pfn_powerflow_cover_map (csrc/powerflow_cover.hip): ONE launch, one workgroup per sample, no host sync, no allocation
 *   (capturable), no atomics.  edge_index int64 [n_samples, 2, n_lines], rx [n_samples, n_lines, 2]; cover_keys int64 [n_cover]: the
 *   keys of the cover list sorted ascending, equal keys in cover order; cover_slot int32 [n_cover]: the cover line at each sorted
 *   position.  THE SLOT RULE: sample s's k-th line with key q, in stored order, takes the k-th cover line with key q, in cover
 *   order; its orientation does not matter (the line terms are symmetric in their ends).  line_mask uint8 [n_samples, n_cover]: 1
 *   where the sample has the cover line; rx_cover [n_samples, n_cover, 2]: the line's (r, x) at its cover line, NOT WRITTEN where
 *   the mask is 0; unplaced int32 [n_samples]: the sample's lines without a cover line -- a key the cover lacks or holds too few
 *   times, a bus outside [0, n_bus), one bus twice.  Every id is tested before it indexes anything; the assignment is the rule's on every run (where two lines of a
 *   sample meet at one cover line, the first in stored order keeps it).  rx and rx_cover 16-byte aligned.
 * pfn_powerflow_solve_sparse_masked / pfn_powerflow_solve_sparse_fd_masked: pfn_powerflow_solve_sparse / _fd with edge_index the
 *   COVER list [2, n_lines], rx = rx_cover, and line_mask uint8 [n_samples, n_lines] (or null: every line is there), unplaced int32
 *   [n_samples] (or null).  A masked-off line end adds nothing to the line sums, the mismatch, the Jacobian, B' or B'', and its rx
 *   is never read.  The plan is checked against the cover list as before; a sample with unplaced != 0 ends with -6 and NaN rows; a
 *   mask that leaves a bus without a line ends with -2 (a zero pivot), as a bus without a line does on every route.  With both
 *   pointers null these ARE the unmasked entries, bit for bit; with a mask a sample's result is a pure function of (its inputs,
 *   its mask row, the plan), bit for bit, whatever the batch and the workgroup size.  Under another cover the factor's pattern and
 *   order differ, so results agree to rounding, not bit for bit.                                                               */
int pfn_powerflow_cover_map(const int64_t* edge_index, int64_t n_lines, const double* rx, int64_t n_samples, int64_t n_bus,
                            const int64_t* cover_keys, const int32_t* cover_slot, int64_t n_cover, uint8_t* line_mask, double* rx_cover,
                            int32_t* unplaced, void* stream);
int pfn_powerflow_solve_sparse_masked(const int64_t* edge_index, int64_t n_lines, const double* rx, const uint8_t* line_mask,
                                      const int32_t* unplaced, const int32_t* bus_type, const double* spec, const double* init,
                                      int64_t n_samples, int64_t n_bus, int mode, double tol, int max_iter, const void* plan_header,
                                      const void* plan_dev, int threads, double* table, int32_t* status, double* residual,
                                      int32_t* flags, void* ws, size_t ws_bytes, void* stream);
int pfn_powerflow_solve_sparse_fd_masked(const int64_t* edge_index, int64_t n_lines, const double* rx, const uint8_t* line_mask,
                                         const int32_t* unplaced, const int32_t* bus_type, const double* spec, const double* init,
                                         int64_t n_samples, int64_t n_bus, int mode, double tol, int max_iter, const void* plan_header,
                                         const void* plan_dev, int threads, double* table, int32_t* status, double* residual,
                                         int32_t* flags, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------- sparse power-flow route, generator Q-limits and per-sample bus types
 * pfn_powerflow_solve_sparse_qlim (csrc/powerflow_sparse_qlim.hip): pfn_powerflow_solve_qlim beyond pfn_powerflow_max_unknowns().
 * ONE launch, one workgroup per sample, the rounds inside the kernel, no host sync, no allocation (capturable).  The plan is
 * pfn_powerflow_sparse_plan's, mode 0, for the type row in which EVERY non-slack bus is PQ: m = 2 (n_bus - 1) unknowns, a theta and
 * a Vm at every non-slack bus.  A sample's live types say which Vm unknowns are dead (the bus is PV now); a dead unknown is an
 * identity row and column (diagonal 1, right-hand side 0, its row and column structural zeros), so nothing is renumbered when a
 * bus switches, and a PV bus's Vm is never updated.
 *   edge_index, rx, line_mask, unplaced, spec, init, tol, max_iter, plan_header, plan_dev, threads, table, status, residual, flags:
 *   as pfn_powerflow_solve_sparse_masked with mode 0 (line_mask and unplaced null: one topology for all samples).
 *   bus_type, types_per_sample, q_limits, limits_per_sample, q_tol, max_rounds, bus_type_out, rounds, the round rule and the table:
 *   as pfn_powerflow_solve_qlim.
 *   status  as there: -5 (flag bit 0) for a row without exactly one slack or with a type outside 0, 1, 2, that sample alone; -6 for
 *           a slack at another bus than the plan's, a plan without theta and Vm at every non-slack bus, another line list, an
 *           unplaced line; -7 after max_rounds re-solves; -2 a tiny or NaN pivot.  A failed sample has NaN rows, its input types in
 *           bus_type_out and the rounds it completed.
 *   ws      pfn_powerflow_sparse_qlim_workspace_bytes(n_samples, plan_header) bytes: the sparse route's sample and its effective Q
 *           specification (8 n_bus bytes more per sample); too little is PFN_ENOSPACE.  The live types are n_bus bytes of LDS.
 *   refused with PFN_EINVAL: a plan with m != 2 (n_bus - 1) or another mode, for another n_bus / n_lines, with 32-bit row ids, or
 *   whose work vector and type bytes do not fit LDS.  A sample's bits are a function of (sample, plan), whatever the batch.    */
size_t pfn_powerflow_sparse_qlim_workspace_bytes(int64_t n_samples, const void* plan_header);
int pfn_powerflow_solve_sparse_qlim(const int64_t* edge_index, int64_t n_lines, const double* rx, const uint8_t* line_mask,
                                    const int32_t* unplaced, const int32_t* bus_type, int types_per_sample, const double* spec,
                                    const double* init, const double* q_limits, int limits_per_sample, int64_t n_samples, int64_t n_bus,
                                    double tol, double q_tol, int max_iter, int max_rounds, const void* plan_header, const void* plan_dev,
                                    int threads, double* table, int32_t* status, double* residual, int32_t* flags, int32_t* bus_type_out,
                                    int32_t* rounds, void* ws, size_t ws_bytes, void* stream);

/* --------------------------------------------------------------------------- topology perturbation
 * The reference's perturb_topology (utils/data_utils.py:12-59, behind dataset_generator.py -r / -a) drawn per sample on the device:
 * remove n_remove random lines, start over while a bus is left unsupplied, then add n_add lines between random bus pairs, each a copy
 * of a random existing line.  ONE launch, one workgroup per sample, the sample's state in LDS; no host sync, no allocation
 * (capturable), no atomic on global memory, no floating point.  What the solver's [n_samples, 2, e] line lists are made of.
 * THE DRAWING RULE (tests/topology_ref.py transcribes it in numpy and is held to it bit for bit).  Random words are Philox4x32-10
 * with key {seed[31:0], seed[63:32]} and counter {item, attempt, sample, stream}, sample = first_sample + s the GLOBAL sample
 * number: a sample's draw depends on (seed, sample) only, never on its batch.
 *   removal      stream 0; for attempt = 0 .. max_attempts - 1: base line j gets the key word 0 of philox({j, attempt, sample, 0});
 *                the n_remove lines with the smallest (key, j), compared lexicographically, are removed (a uniform subset, ties to
 *                the lower index); the draw is accepted when every bus is reachable from `root` over the kept lines -- the
 *                reference's unsupplied_buses == 0, checked before any line is added, as there.  The first accepted attempt ends it.
 *   addition     stream 1, attempt word 0; for k < n_add, w = philox({k, 0, sample, 1}): from = w0 mod n_bus,
 *                to = (from + 1 + w1 mod (n_bus - 1)) mod n_bus (never from; a duplicate of an existing line is allowed, as in the
 *                reference), source line = w2 mod n_lines.  The modulo bias is at most n / 2^32 (n = n_bus, n_lines).
 *   edge_index   DEVICE int64 [2, n_lines], the base list (local bus ids).
 *   edge_index_out  int64 [n_samples, 2, e_out], e_out = n_lines - n_remove + n_add for every sample: the kept base lines in base
 *                order (a stable compaction), then the added lines in draw order.
 *   source       int32 [n_samples, e_out]: the base line that output line j is, or whose parameters it copies.
 *   status       int32 [n_samples]: >= 1 the attempts used; -1 no connected draw in max_attempts (the reference gives up there);
 *                -4 a base line names a bus outside [0, n_bus) -- checked before any id is followed, hence for every sample; the
 *                solver's code.  Where status < 0 that sample's edge_index_out and source rows are all -1.
 * PFN_EINVAL, nothing launched: n_remove < 0, n_add < 0, n_remove > n_lines; n_lines - n_remove < n_bus - 1 (no such draw is
 * connected); n_add > 0 with n_bus < 2; root outside [0, n_bus); max_attempts outside [1, 1024]; first_sample < 0 or
 * first_sample + n_samples > 2^32; a shape whose state (8 n_lines + 4 n_remove + n_lines + n_bus bytes with 16-bit ids, up to
 * n_bus = 65536; 12 n_lines + ... beyond) exceeds the 159 KiB of LDS a workgroup may take -- 6470rte's (6470, 9005) needs 88 KB.
 *
 * pfn_topology_unsupplied: count[s] = the number of buses NOT reachable from `root` over the lines of sample s -- [2, n_lines]
 * for all samples (lines_per_sample == 0) or [n_samples, 2, n_lines] -- or -4 where a line of that sample names a bus outside
 * [0, n_bus).  The same reach routine: the check a stored dataset can be held to.  PFN_EINVAL: root outside [0, n_bus), a shape
 * beyond the LDS budget (4 n_lines + n_bus bytes with 16-bit ids).                                                              */
int pfn_topology_perturb(const int64_t* edge_index, int64_t n_lines, int64_t n_bus, int64_t n_samples, int64_t first_sample,
                         int64_t n_remove, int64_t n_add, uint64_t seed, int64_t root, int max_attempts, int64_t* edge_index_out,
                         int32_t* source, int32_t* status, void* stream);
int pfn_topology_unsupplied(const int64_t* edge_index, int lines_per_sample, int64_t n_lines, int64_t n_samples, int64_t n_bus,
                            int64_t root, int32_t* count, void* stream);

/* ------------------------------------------------------------------------------ N-1 line-outage screening
 * Which single line outages overload the rest of the grid (csrc/contingency.hip)?  Two launches over ONE line list [2, n_lines] for
 * all scenarios; no host sync, no allocation (capturable), no float atomics.  pfn_contingency_dc: n_bus - 1 <= pfn_powerflow_max_unknowns(); beyond it pfn_contingency_sparse, below.
 *
 * pfn_contingency_islands: islands[k] = the number of buses NOT reachable from `root` (the slack) when line k is removed -- one
 * workgroup per outage, pfn_topology_unsupplied's reach routine over the base list with line k skipped, nothing materialised.  > 0 is
 * a bridge: decided combinatorially, from the line list alone.  -4 for EVERY k where a line names a bus outside [0, n_bus) (never
 * followed).  PFN_EINVAL: root outside [0, n_bus), a shape beyond the LDS budget (5 n_lines + n_bus bytes with 16-bit ids).
 *
 * pfn_contingency_dc: one workgroup per scenario.  THE MODEL is mode 1's (pfn_powerflow_solve): B' the Laplacian of 1 / x over the
 * non-slack buses, B' theta = -P, theta refined under the fp64 residual to tol / max_iter from ONE fp32 inverse X = B'^-1 (Gauss-Jordan
 * in place, the fast-decoupled modes'); base flow of the stored line l = (a -> b): f_l = (theta_a - theta_b) / x_l, fp64.  The
 * outage of line k = (i -> j), with X extended by zeros at the slack:
 *     w_k = X[:, i] - X[:, j]    phi_{l,k} = (w_k[a] - w_k[b]) / x_l    den_k = 1 - phi_{k,k}
 *     f_l^(k) = f_l + phi_{l,k} / den_k * f_k  (l != k),   f_k^(k) = 0              -- fp32, every operation rounded on its own.
 *   rx, spec     DEVICE fp64 [n_samples, n_lines, 2] (r, x) and [n_samples, n_bus, 4] (Vm, Va, P, Q demand-positive), as the solver's.
 *   bus_type     DEVICE int32 [n_bus], exactly one slack (0); n_pv / n_pq are the host's counts of types 1 and 2.
 *   ratings      DEVICE fp64 per-unit current, [n_lines] (ratings_per_sample == 0) or [n_samples, n_lines]; null: 1.0 everywhere.  A
 *                rating whose fp32 value is not > 0 (zero, negative, NaN) leaves its line unmonitored: it enters no max and no count.
 *                Loading of line l is |f_l^(k)| / (float)rating_l (V = 1 under the DC model: |f| is the current).
 *   islands      DEVICE int32 [n_lines]: pfn_contingency_islands' output for this line list and slack.
 *   severity     fp32 [n_samples, n_lines]: per (scenario, outage) the largest loading over the monitored lines l != k; 0 where no
 *                line is monitored; NaN where a monitored loading is not finite.
 *   worst_line   int32 [n_samples, n_lines]: the line of that maximum, ties to the lowest l (a non-finite loading counts as the
 *                largest); -1 where no line is monitored.
 *   overloads    int32 [n_samples, n_lines]: the monitored lines with loading > 1.
 *                Where islands[k] != 0: severity +inf (islanding outages rank first), worst_line -1, overloads -1, a NaN table row.
 *   base_flow    fp64 [n_samples, n_lines].
 *   status       int32 [n_samples]: >= 0 the refinement solves used; -1 not converged in max_iter; -2 singular (a bus without a line
 *                in the base grid); -3 a non-finite residual (a NaN in P, x = 0); -4 a line names a bus outside [0, n_bus); -5 (and bit
 *                0 of flags[0]) bus_type disagrees with n_pv / n_pq.  A failed scenario's float outputs are NaN and its integer
 *                outputs -1; it touches nothing of another scenario.
 *   post_flow    fp32 [n_samples, n_lines, n_lines] (row = outage, column = line) or null: the full table.
 *   route        0 auto, 1 LDS, 2 global.  LDS: X sits behind the scenario's vectors (20 n_bus + 28 n_lines + 4 n_bus per wave
 *                bytes) in LDS while both fit the 159 KiB a workgroup may take (case118: yes); else X lives in a per-scenario slab of
 *                `ws`, same code, same bits.  pfn_contingency_workspace_bytes(n_samples, n_bus, n_lines, route) is what the call
 *                needs: 0 exactly for the LDS route.  256 threads up to 90 unknowns, 1024 beyond, as the solver.
 * A scenario's bits are a function of its own inputs, whatever the batch, the workgroup size or the route.  PFN_EINVAL: bad sizes or
 * counts, n_bus < 2, more unknowns than the dense cap, vectors beyond LDS, route 1 where it does not fit; PFN_ENOSPACE: too little ws. */
int pfn_contingency_islands(const int64_t* edge_index, int64_t n_lines, int64_t n_bus, int64_t root, int32_t* islands, void* stream);
size_t pfn_contingency_workspace_bytes(int64_t n_samples, int64_t n_bus, int64_t n_lines, int route);
int pfn_contingency_dc(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                       const double* ratings, int ratings_per_sample, const int32_t* islands, int64_t n_samples, int64_t n_bus,
                       int64_t n_pv, int64_t n_pq, double tol, int max_iter, int route, float* severity, int32_t* worst_line,
                       int32_t* overloads, double* base_flow, int32_t* status, float* post_flow, int32_t* flags, void* ws,
                       size_t ws_bytes, void* stream);

/* N-2: which PAIRS of line outages overload the rest of the grid (csrc/contingency_pairs.hip)?  The dense DC route only
 * (n_bus - 1 <= pfn_powerflow_max_unknowns(); beyond it pfn_contingency_pairs_sparse, below).  `lines`: DEVICE int32 [n_candidates], strictly increasing ids in [0, n_lines); pair
 * p = (lines[i], lines[j]), i < j, row-major in (i, j), P = n_candidates (n_candidates - 1) / 2; all n_lines lines stay monitored.
 * Three launches, no host sync, no allocation (capturable), no float atomics.
 *
 * pfn_contingency_pair_islands: islands[p] = the number of buses NOT reachable from `root` with BOTH lines of pair p removed -- one
 * workgroup per first candidate loops over the second, pfn_contingency_islands' reach routine with two keep flags cleared, nothing
 * materialised.  > 0 also where neither line is a bridge; decided combinatorially, never from a small determinant.  -4 for EVERY p
 * where a line names a bus outside [0, n_bus), and for a pair with a candidate outside [0, n_lines).  Fewer than 2 candidates: nothing
 * is launched.  PFN_EINVAL: root outside [0, n_bus), more candidates than lines, a shape beyond the LDS budget.
 *
 * pfn_contingency_pairs: the model, X, w_k and phi_{l,k} are pfn_contingency_dc's.  The outage of lines a and b:
 *     M = [[1 - phi_aa, -phi_ab], [-phi_ba, 1 - phi_bb]]      t = M^-1 (f_a, f_b)   (Cramer's rule)
 *     f_l^(a,b) = f_l + phi_la t_a + phi_lb t_b  (l != a, b),   f_a^(a,b) = f_b^(a,b) = 0     -- fp32, every operation rounded on its own.
 *   base   one workgroup per scenario: pfn_contingency_dc's base solve (the same code: base_flow and status carry its bits for the same
 *          inputs).  It leaves in the scenario's slab of `ws` X TRANSPOSED (the walk that forms w_k reads consecutive words; the element
 *          read is X[r][c] as in pfn_contingency_dc -- the fp32 inverse is not bitwise symmetric) and the staged per-line vectors.
 *   pairs  one workgroup per (scenario, first candidate): w_a once, its waves take the second candidates.
 *   severity, worst_line, overloads  [n_samples, P], pfn_contingency_dc's definitions with BOTH outaged lines unmonitored; where
 *          islands[p] != 0: +inf, -1, -1 and a NaN table row; a failed scenario: NaN, -1, -1.
 *   post_flow  fp32 [n_samples, P, n_lines] or null.
 *   route  0 auto, 1 LDS, 2 global: the pair launch copies X from the slab into LDS where it fits beside its vectors (16 n_lines +
 *          8 n_bus + 4 n_bus per wave bytes) in the 159 KiB a workgroup may take, else reads the slab; same code, same bits.
 * pfn_contingency_pairs_workspace_bytes(n_samples, n_bus, n_lines, n_candidates, route): what the call needs -- per scenario
 * 4 m (m | 1) rounded up to 16 (m = n_bus - 1) + 16 n_lines + 4 n_bus bytes, rounded up to 16 -- on EITHER route; 0 for arguments the
 * call would refuse, route 1 where X does not fit LDS among them (which is how a caller finds the threshold).
 * The bits of (scenario, a, b) are a function of the scenario's inputs and the two lines, whatever the batch, the candidate list, the
 * workgroup size or the route.  PFN_EINVAL: bad sizes or counts, more unknowns than the dense cap, vectors beyond LDS, route 1 where it
 * does not fit, null or misaligned pointers; PFN_ENOSPACE: too little ws.                                                          */
int pfn_contingency_pair_islands(const int64_t* edge_index, int64_t n_lines, int64_t n_bus, int64_t root, const int32_t* lines,
                                 int64_t n_candidates, int32_t* islands, void* stream);
size_t pfn_contingency_pairs_workspace_bytes(int64_t n_samples, int64_t n_bus, int64_t n_lines, int64_t n_candidates, int route);
int pfn_contingency_pairs(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                          const double* ratings, int ratings_per_sample, const int32_t* lines, int64_t n_candidates,
                          const int32_t* islands, int64_t n_samples, int64_t n_bus, int64_t n_pv, int64_t n_pq, double tol, int max_iter,
                          int route, float* severity, int32_t* worst_line, int32_t* overloads, double* base_flow, int32_t* status,
                          float* post_flow, int32_t* flags, void* ws, size_t ws_bytes, void* stream);

/* Generator outages, alone and followed by a line outage (csrc/contingency_units.hip): the dense DC route only
 * (n_bus - 1 <= pfn_powerflow_max_unknowns(); the sparse route is not built).  ONE launch, one workgroup per scenario (256 threads up
 * to 90 unknowns, 1024 beyond), behind pfn_contingency_islands where candidate lines are given; no host sync, no allocation
 * (capturable), no float atomics.  Inputs, model, X, base flows, ratings and statuses are pfn_contingency_dc's; added to them:
 *   units          DEVICE int32 [n_units], the bus of every unit: any bus type, the slack's included; a bus may appear more than once
 *                  (several units at one bus).  An id outside [0, n_bus) is never followed: EVERY scenario gets status -4.
 *   unit_p         DEVICE fp64 [n_units] (unit_p_per_sample == 0) or [n_samples, n_units]: the output lost with the unit,
 *                  generation-positive per-unit.
 *   participation  DEVICE fp64 [n_units] / [n_samples, n_units], a_h >= 0, or null: all zero (the slack picks up everything).
 *   lines          DEVICE int32 [n_candidates], strictly increasing ids in [0, n_lines), or null with n_candidates == 0: the unit x line
 *                  part.  islands: pfn_contingency_islands' output [n_lines] (read at the candidates only; null without candidates).
 * With c_g = X[:, b_g], A = sum_h a_h (fp64, stored order, one owner), rest_g = A - a_g (one fp64 subtraction) and the pickup vector
 * u = sum_h a_h c_h (fp32, once per scenario), the outage of unit g changes the generation-positive injection by -p_g at b_g and, if
 * rest_g > 0, by +p_g a_h / rest_g at b_h for every h != g (otherwise by nothing more: the slack absorbs p_g).  The angle change:
 *     d_g = p_g ((u - a_g c_g) / rest_g - c_g)   (rest_g > 0)        d_g = -p_g c_g   (otherwise)
 * evaluated as d_g = alpha_g u - beta_g c_g with alpha_g = p_g / rest_g and beta_g = p_g (a_g / rest_g + 1) formed in fp64 and rounded
 * once to fp32 (alpha_g = 0, beta_g = p_g otherwise), then per stored line l = (a -> b)
 *     f_l^(g) = f_l + (d_g[a] - d_g[b]) / x_l                                       -- fp32, every operation rounded on its own;
 * all n_lines lines are monitored, none is out.  p_g = 0 is an ordinary item whose flows are the base flows.
 * Unit x line (g, k), k = lines[j]: line k leaves the post-unit state,
 *     f_l^(g,k) = f_l^(g) + phi_{l,k} / den_k * f_k^(g)  (l != k),   0 at k          -- pfn_contingency_dc's phi, den and expression;
 * monitored are the lines l != k with a rating > 0; islands[k] != 0 gives (+inf, -1, -1) and a NaN row, never decided from den.
 *   severity, worst_line, overloads   [n_samples, n_units], pfn_contingency_dc's figures and rules; post_flow fp32
 *                  [n_samples, n_units, n_lines] or null.
 *   line_severity, line_worst_line, line_overloads   [n_samples, n_units, n_candidates]; line_post_flow fp32
 *                  [n_samples, n_units, n_candidates, n_lines] or null.  All four may be null with n_candidates == 0.
 *   base_flow, status   pfn_contingency_dc's BITS for the same inputs (the same base solve) where the unit inputs are good.  In
 *                  addition status -3 where a unit_p is not finite or a participation entry is not both finite and >= 0, and -4 as
 *                  above; a status the base solve set stands.  A failed scenario's float outputs are NaN and its integer outputs -1;
 *                  it touches nothing of another scenario.
 *   route          0 auto, 1 LDS, 2 global, as pfn_contingency_dc: the unit screen's own vectors (24 n_units + 8 n_bus + 4 n_lines
 *                  bytes, rounded up to 16) sit between that screen's vectors and X.  pfn_contingency_units_workspace_bytes(n_samples,
 *                  n_bus, n_lines, n_units, route) is what the call needs: 0 exactly for the LDS route, else a slab of 4 m (m | 1) bytes
 *                  (rounded up to 16, m = n_bus - 1) per scenario.
 * A scenario's bits are a function of its own inputs, whatever the batch, the workgroup size, the route, the tables or the candidate
 * lines: the unit figures are the same bits with and without lines.  PFN_EINVAL: bad sizes or counts (n_units < 1, more candidates
 * than lines), more unknowns than the dense cap, vectors beyond LDS, route 1 where it does not fit, null or misaligned pointers;
 * PFN_ENOSPACE: too little ws.  n_samples == 0 or n_lines == 0: PFN_OK, nothing is launched and NO output is written, as in
 * pfn_contingency_dc (a grid without lines has no flow to report; contingency_screen_units refuses it on the host).                 */
size_t pfn_contingency_units_workspace_bytes(int64_t n_samples, int64_t n_bus, int64_t n_lines, int64_t n_units, int route);
int pfn_contingency_units(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                          const double* ratings, int ratings_per_sample, const int32_t* units, int64_t n_units, const double* unit_p,
                          int unit_p_per_sample, const double* participation, int participation_per_sample, const int32_t* lines,
                          int64_t n_candidates, const int32_t* islands, int64_t n_samples, int64_t n_bus, int64_t n_pv, int64_t n_pq,
                          double tol, int max_iter, int route, float* severity, int32_t* worst_line, int32_t* overloads, double* base_flow,
                          int32_t* status, float* post_flow, float* line_severity, int32_t* line_worst_line, int32_t* line_overloads,
                          float* line_post_flow, int32_t* flags, void* ws, size_t ws_bytes, void* stream);

/* The same screen beyond the dense cap (csrc/contingency_sparse.hip): B' is kept as a sparse fp32 FACTOR under the mode-1 plan of the
 * sparse power-flow route (pfn_powerflow_sparse_plan(..., mode 1, ...): plan_header its first 32 words on the host, plan_dev the blob
 * on the device) where pfn_contingency_dc keeps its inverse.  Model, definitions, outputs and statuses are pfn_contingency_dc's, and
 * status -6 is added where the device line list is not the plan's.  Two launches behind pfn_contingency_islands, no host sync, no
 * allocation (capturable), no float atomics:
 *   base     one workgroup per scenario (64 threads, 256 where the plan's longest L column exceeds 128; `threads` 64 / 256 forces
 *            either, 0 the default): the fp64 residual first, B' at the planned positions factored ONCE in fp32, theta refined to
 *            tol / max_iter by column substitutions, the fp64 base flows; the factor stays in the scenario's workspace slab.
 *   outages  a lane per outage, a one-wave workgroup per tile of 64 consecutive outages: the tile's 64 right-hand sides e_i - e_j sit
 *            in one block [n_bus][64] fp32 (row = unknown in plan order, the last row the slack's zeros) and go through the forward
 *            and backward column substitutions together -- column bounds, row ids and factor values are read once per wave, a lane
 *            touches its own column only: no barrier, no shuffle, no atomic --, then den_k and one loop over the lines in ascending
 *            order with pfn_contingency_dc's per-line expression.  Workgroup g of G takes the items (scenario, tile) g, g + G, ...;
 *            groups = 0: G = min(n_samples * tiles, 16 * compute units), else G = min(n_samples * tiles, groups).  An item's bits do
 *            not depend on G.
 *   block_route  0 auto, 1 LDS, 2 global: the block sits in LDS where 256 n_bus bytes fit the 159 KiB a workgroup may take
 *            (n_bus <= 636), else in a per-workgroup block of `ws`; same code, same bits.
 * pfn_contingency_sparse_workspace_bytes(n_samples, n_lines, plan_header, block_route, groups): per scenario 8 (2 n_bus + m) +
 * 4 nnz + 20 n_lines bytes rounded up to 16, plus G blocks of 256 n_bus bytes on the global placement; 0 for arguments the call
 * would refuse.  A scenario's bits are a function of its own inputs and the plan, whatever the batch, `threads`, G or the placement.
 * PFN_EINVAL: bad sizes or counts, a plan that is no mode-1 plan or is for another n_bus / n_lines, 32-bit row ids, block_route 1
 * where the block does not fit, bad threads / groups, null or misaligned pointers; PFN_ENOSPACE: too little ws.                     */
size_t pfn_contingency_sparse_workspace_bytes(int64_t n_samples, int64_t n_lines, const void* plan_header, int block_route, int groups);
int pfn_contingency_sparse(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                           const double* ratings, int ratings_per_sample, const int32_t* islands, int64_t n_samples, int64_t n_bus,
                           int64_t n_pv, int64_t n_pq, double tol, int max_iter, float* severity, int32_t* worst_line,
                           int32_t* overloads, double* base_flow, int32_t* status, float* post_flow, int32_t* flags, void* ws,
                           size_t ws_bytes, const void* plan_header, const void* plan_dev, int threads, int block_route, int groups,
                           void* stream);

/* N-2 beyond the dense cap (csrc/contingency_pairs_sparse.hip): pfn_contingency_pairs' screen -- the same pairs of `lines` in the same
 * order, the same formulas, definitions and outputs -- from the sparse fp32 factor of pfn_contingency_sparse under the same mode-1
 * plan; statuses are pfn_contingency_sparse's (-6 where the device line list is not the plan's).  `islands`: DEVICE int32 [P],
 * pfn_contingency_pair_islands' output for this line list, slack and candidates.  Three launches behind it, no host sync, no
 * allocation (capturable after one eager call), no float atomics:
 *   base     pfn_contingency_sparse's base launch, the same kernel: base_flow and status carry its bits for the same inputs; `threads`
 *            as there.
 *   columns  a lane per candidate, a one-wave workgroup per tile of 64 consecutive candidates: pfn_contingency_sparse's tile
 *            substitution (the same function: column k has the bits its outage launch holds for outage lines[k]), then the tile is
 *            written into the scenario's column table [n_candidates][n_bus] fp32 (candidate-major, plan order, the last row the
 *            slack's zero).  block_route / groups as in pfn_contingency_sparse, the items being (scenario, tile of candidates):
 *            G = min(n_samples * ceil(n_candidates / 64), groups or 16 * compute units).
 *   pairs    one workgroup of `waves` waves (0: the default, 4; else 1, 2, 4, 8, 16) per (scenario, first candidate); a wave takes
 *            second candidates: M, t, then its lanes stride over the lines (the per-line vectors are read from the slab) and reduce
 *            as pfn_contingency_pairs does.
 *   column_route  0 auto, 1 LDS, 2 global: the pair launch copies w_a and one w_b per wave into LDS where 4 n_bus (1 + waves) bytes,
 *            rounded up to 16, fit the 159 KiB a workgroup may take, else gathers from the column table; same code, same bits.
 *   severity, worst_line, overloads  [n_samples, P]; post_flow fp32 [n_samples, P, n_lines] or null.
 * pfn_contingency_pairs_sparse_workspace_bytes(n_samples, n_lines, n_candidates, plan_header, block_route, groups, column_route,
 * waves): per scenario pfn_contingency_sparse's slab (8 (2 n_bus + m) + 4 nnz + 20 n_lines bytes rounded up to 16) plus the column
 * table, 4 n_candidates n_bus bytes rounded up to 16; plus G blocks of 256 n_bus bytes where the block sits in the workspace.  0 for
 * arguments the call would refuse -- block_route 1 where the block does not fit, column_route 1 where the columns do not fit (which is
 * how a caller finds the thresholds), waves that is none of the six, more candidates than lines, a plan of another mode or size.
 * The bits of (scenario, a, b) are a function of the scenario's inputs, the plan and the two lines, whatever the batch, the candidate
 * list, G, `threads`, `waves` or either placement.  PFN_EINVAL: what pfn_contingency_sparse refuses, bad candidate counts,
 * column_route 1 where it does not fit, bad waves, null or misaligned pointers; PFN_ENOSPACE: too little ws.                        */
size_t pfn_contingency_pairs_sparse_workspace_bytes(int64_t n_samples, int64_t n_lines, int64_t n_candidates, const void* plan_header,
                                                    int block_route, int groups, int column_route, int waves);
int pfn_contingency_pairs_sparse(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                                 const double* ratings, int ratings_per_sample, const int32_t* lines, int64_t n_candidates,
                                 const int32_t* islands, int64_t n_samples, int64_t n_bus, int64_t n_pv, int64_t n_pq, double tol,
                                 int max_iter, float* severity, int32_t* worst_line, int32_t* overloads, double* base_flow,
                                 int32_t* status, float* post_flow, int32_t* flags, void* ws, size_t ws_bytes, const void* plan_header,
                                 const void* plan_dev, int threads, int block_route, int groups, int column_route, int waves,
                                 void* stream);

/* N-1 with the NETWORK's prediction (csrc/contingency_model.hip): the two launches around a model forward.  Work item
 * t = s * n_lines + k is scenario s with line k out, islanding outages included, so every shape is static; a chunk is `chunk`
 * consecutive items from item0[0] -- a DEVICE int64 word, so that one captured chunk serves every chunk of a screen.  Inputs as
 * pfn_contingency_dc's (rx, spec DEVICE fp64, bus_type DEVICE int32, ONE line list); n_lines >= 2.  No host sync, no allocation
 * (capturable), no atomics; an item's bits are a function of its own inputs, whatever the chunk.
 *
 * pfn_contingency_model_batch: one workgroup per chunk position b; its item is item0[0] + b clamped to the last item (the tail of
 * the last chunk repeats it).  It writes what the dataset plus its collate produce for the graph "scenario s without line k":
 *   x            fp32 [chunk n_bus, 4] = (float(spec) * (1 - mask) - mean4) / div4, mask the bus type's row of (0,0,1,1) slack,
 *                (0,1,0,1) PV, (1,1,0,0) PQ; every operation rounded on its own, in this order: the dataset's bits.  div4 / mean4 /
 *                edge_div2 / edge_mean2 are HOST floats, div = std + 1e-7 formed in fp32 by the caller; null: 1 / 0.
 *   pred_mask    fp32 [chunk n_bus, 4]; bus_type_out int64 [chunk n_bus].
 *   edge_index_out  int64 [2, chunk (n_lines - 1)]: the lines l != k in stored order, bus ids offset by b n_bus, all sources then
 *                all targets (collate's layout).  A line that names a bus outside [0, n_bus) sets bit 1 of flags[0] and is written as
 *                the local pair (0, 0); pfn_contingency_islands reports -4 there.
 *   edge_attr    fp32 [chunk (n_lines - 1), 2] = (float(rx) - edge_mean2) / edge_div2.
 * The five tensors, spec and rx must be 16-byte aligned (16-byte stores and loads).
 *
 * pfn_contingency_model_loadings: one workgroup per chunk position; positions past the last item return at once.  `out` fp32
 * [chunk n_bus, 4] is the forward's output.  Per bus the row is merged: out * std4 + mean4 (HOST floats, std = the divisor above;
 * null: 1 / 0) where the mask says "predict", float(spec) where the entry is given.  (Vm, Va) become rectangular voltages with
 * pfn_branch_flows' arithmetic, loading of line l != k is I_l / (float)rating_l with r, x = float(rx) -- the bits of
 * pfn_branch_flows on the merged table and the reduced list -- and the reduction is pfn_contingency_dc's: severity fp32, worst_line
 * and overloads int32, each [n_samples n_lines]; ratings, monitoring and the non-finite rule as there.  Where islands[k] != 0:
 * +inf, -1, -1 and a NaN row.
 *   loading      optional fp32 [n_samples n_lines, n_lines] (row = item, column = line of the ORIGINAL list; NaN at line k).
 *   predictions  optional fp32 [n_samples n_lines, n_bus, 4]: the merged table (written for islanding items too).
 *   route        0 auto, 1 LDS, 2 direct.  LDS: one sincos per bus, 8 n_bus bytes, up to pfn_contingency_model_lds_max_bus() buses;
 *                direct: the phasors are formed per line end.  Same bits.
 * PFN_EINVAL: bad sizes (n_lines < 2, chunk < 1), route 1 where it does not fit, null or misaligned pointers.                      */
int64_t pfn_contingency_model_lds_max_bus(void);
int pfn_contingency_model_batch(const int32_t* bus_type, const double* spec, const int64_t* edge_index, const double* rx, int64_t n_samples,
                                int64_t n_bus, int64_t n_lines, const int64_t* item0, int64_t chunk, const float* div4, const float* mean4,
                                const float* edge_div2, const float* edge_mean2, float* x, float* pred_mask, int64_t* bus_type_out,
                                int64_t* edge_index_out, float* edge_attr, int32_t* flags, void* stream);
int pfn_contingency_model_loadings(const float* out, const int32_t* bus_type, const double* spec, const int64_t* edge_index, const double* rx,
                                   const double* ratings, int ratings_per_sample, const int32_t* islands, int64_t n_samples, int64_t n_bus,
                                   int64_t n_lines, const int64_t* item0, int64_t chunk, const float* std4, const float* mean4, int route,
                                   float* severity, int32_t* worst_line, int32_t* overloads, float* loading, float* predictions, void* stream);

/* AC N-1 screening, compensated 1P1Q on the dense route (csrc/contingency_ac.hip): for every scenario and every single line outage,
 * `halves` half-iterations of the fast-decoupled power flow from the scenario's AC base solution, the inverses of B' and B''
 * corrected for the missing line by a rank-1 update.  Inputs as pfn_contingency_dc's (ONE line list, bus_type DEVICE int32, spec
 * [S, n, 4] and rx [S, e, 2] DEVICE fp64, ratings [e] or [S, e] or null, islands from pfn_contingency_islands) plus `init`
 * [S, n, 2] = (Vm, Va in degrees) or null, the base solve's start.  variant 0: XB, 1: BX (pfn_powerflow_solve_init's modes 2 and
 * 3: their B' and B'' over the full list).  Two launches, no host sync, no allocation (capturable), no float atomics; n_bus - 1 <=
 * pfn_powerflow_max_unknowns().
 *
 * BASE, one workgroup per scenario: the fast-decoupled solve to tol within max_iter half-iterations -- the SAME code as
 * pfn_powerflow_solve_init's modes 2 / 3, so base_table fp64 [S, n, 4] (32-byte aligned), status int32 [S] and residual fp64 [S] carry
 * that call's bits.  It keeps X' = B'^-1 and X'' = B''^-1 (fp32), the fp64 base state and a per-bus list of line ends in the
 * scenario's slab of `ws` (pfn_contingency_ac_workspace_bytes, 16-byte aligned; PFN_ENOSPACE when short).
 *
 * OUTAGES, one wave per (scenario s, outage k = (i -> j)), `group` of them to a workgroup, for a non-islanding outage of a scenario
 * with status >= 0.  From the base state, for h = 0 .. halves - 1: F = the fp64 mismatch of the grid WITHOUT line k (a bus's terms
 * in stored line order); even h (every h where there is no PQ bus): theta -= X'_k (dP / Vm) over the angle buses; odd h:
 * Vm -= X''_k (dQ / Vm) over the PQ buses; X_k g = X g + w (w . g) / (1 / c_k - a^T w), a = e_i - e_j restricted to the matrix's
 * buses, w = X a, c_k the line's weight in the matrix (1 / x or x / (r^2 + x^2)); the fp32 entries in fp64 arithmetic, the corrected
 * matrix never formed.  Then
 *   mismatch      fp64 [S, e]: max |F| at the final state -- how far from converged the estimate is;
 *   severity, worst_line, overloads   fp32 / int32 / int32 [S, e]: pfn_contingency_dc's rules over the loadings I_l / (float)rating_l
 *                 of the lines l != k, I_l the fp32 current of pfn_branch_flows' arithmetic on the fp32-rounded final state;
 *   vm_min, vm_min_bus, v_violations  fp32 / int32 / int32 [S, e] over the PQ buses from the fp32-rounded final Vm: the lowest (ties to
 *                 the lowest bus; bus -1 and NaN without a PQ bus) and the count of Vm < v_lo or > v_hi, compared in fp32; a non-finite
 *                 Vm counts, is the lowest, and makes vm_min NaN;
 *   post_current  optional fp32 [S, e, e] (row = outage, column = line; NaN at l = k); post_state optional fp32 [S, e, n, 2] = (Vm, Va
 *                 in degrees), 8-byte aligned.
 * An islanding outage (islands[k] != 0): +inf, -1, -1; NaN voltage figures and mismatch with -1 integers; NaN rows.  A failed
 * scenario (status < 0, -1 .. -5 as in pfn_powerflow_solve_init): NaN floats and -1 integers for all its outages; flags[0] bit 0 with -5.
 * halves = 0: the figures of the base state with line k unmonitored.
 *   route   0 auto, 1 both inverses copied into LDS beside the waves' vectors (PFN_EINVAL where they do not fit), 2 read from the slab;
 *   group   0 auto, or the waves per workgroup, 1 .. 16.  No bit of any output depends on either.
 * pfn_contingency_ac_waves: the waves per workgroup a call with these arguments runs, *in_lds its placement; 0 where it is refused.
 * PFN_EINVAL: bad sizes or counts, halves < 0, variant outside {0, 1}, v_lo > v_hi or NaN, beyond the dense cap, route / group that do
 * not fit, null or misaligned pointers.                                                                                            */
size_t pfn_contingency_ac_workspace_bytes(int64_t n_samples, int64_t n_bus, int64_t n_lines, int64_t n_pq);
int pfn_contingency_ac_waves(int64_t n_bus, int64_t n_pq, int route, int group, int* in_lds);
int pfn_contingency_ac(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                       const double* init, const double* ratings, int ratings_per_sample, const int32_t* islands, int64_t n_samples,
                       int64_t n_bus, int64_t n_pv, int64_t n_pq, int variant, int halves, float v_lo, float v_hi, double tol, int max_iter,
                       int route, int group, float* severity, int32_t* worst_line, int32_t* overloads, float* vm_min, int32_t* vm_min_bus,
                       int32_t* v_violations, double* mismatch, double* base_table, int32_t* status, double* residual, float* post_current,
                       float* post_state, int32_t* flags, void* ws, size_t ws_bytes, void* stream);

/* AC N-1 screening beyond the dense cap (csrc/contingency_ac_sparse.hip): pfn_contingency_ac's screen -- the same definitions, outputs
 * and statuses -- from the sparse fp32 FACTORS of B' and B'' under the fast-decoupled plan of the sparse power-flow route
 * (pfn_powerflow_sparse_fd_plan: plan_header its first 32 words on the host, plan_dev the blob on the device) where
 * pfn_contingency_ac keeps their dense inverses: "X g" and "w = X a" are each one forward and one backward substitution in fp64 on
 * the fp32 factor (pfn_powerflow_solve_sparse_fd's expression and column order), w . g ONE serial fp64 sum in ascending unknown
 * order.  Status -6 is added where the device line list is not the plan's.  Arguments as pfn_contingency_ac's with `route, group`
 * replaced by the plan and the sparse route's options.  Two launches behind pfn_contingency_islands, no host sync, no allocation
 * (capturable), no atomics:
 *   base     pfn_powerflow_solve_sparse_fd's launch itself (mode 2 + variant; `threads` 0 / 64 / 256 as there): base_table, status
 *            and residual carry that call's bits; the fp64 base state and both factors stay in the scenario's slab of `ws`.
 *   outages  a lane per outage, a one-wave workgroup per tile of 64 consecutive outages of a scenario.  A lane's fp64 vectors --
 *            theta and Vm by bus, the half's right-hand side / solution and w by unknown -- are columns of one block
 *            [2 n_bus + 2 max(m_p, m_q)][64]; everything the lanes share is read wave-uniformly; no barrier, no shuffle.  w is
 *            formed anew in every half.  Workgroup g of G takes the items (scenario, tile) g, g + G, ...; groups = 0:
 *            G = min(n_samples * tiles, 4 * compute units), else G = min(n_samples * tiles, groups).
 *   block_route  0 auto, 1 LDS, 2 global: the block sits in LDS where pfn_contingency_ac_sparse_block_bytes(plan_header) =
 *            512 (2 n_bus + 2 max(m_p, m_q)) bytes fit the 159 KiB a workgroup may take (n_bus <= 80), else in a per-workgroup
 *            block of `ws`; same code, same bits.
 * pfn_contingency_ac_sparse_workspace_bytes(n_samples, n_lines, plan_header, block_route, groups): the scenarios' slabs first
 * (pfn_powerflow_sparse_fd_workspace_bytes), then G blocks on the global placement; 0 for arguments the call would refuse.  An
 * outage's bits are a function of its scenario's inputs and the plan, whatever the batch, `threads`, G or the placement.
 * n_pq that is not the plan's count of PQ buses: every scenario -5 and bit 0 of flags[0], as pfn_contingency_ac reports counts that
 * contradict bus_type.  PFN_EINVAL: no fast-decoupled plan or one for another n_bus / n_lines, bad sizes or counts, halves < 0,
 * variant outside {0, 1}, v_lo > v_hi or NaN, bad tol / max_iter / threads / block_route / groups, block_route 1 where the block does
 * not fit, 32-bit row ids, null or misaligned pointers; PFN_ENOSPACE: too little ws.                                               */
size_t pfn_contingency_ac_sparse_block_bytes(const void* plan_header);
size_t pfn_contingency_ac_sparse_workspace_bytes(int64_t n_samples, int64_t n_lines, const void* plan_header, int block_route, int groups);
int pfn_contingency_ac_sparse(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                              const double* init, const double* ratings, int ratings_per_sample, const int32_t* islands, int64_t n_samples,
                              int64_t n_bus, int64_t n_pv, int64_t n_pq, int variant, int halves, float v_lo, float v_hi, double tol, int max_iter,
                              const void* plan_header, const void* plan_dev, int threads, int block_route, int groups, float* severity,
                              int32_t* worst_line, int32_t* overloads, float* vm_min, int32_t* vm_min_bus, int32_t* v_violations, double* mismatch,
                              double* base_table, int32_t* status, double* residual, float* post_current, float* post_state, int32_t* flags, void* ws,
                              size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------- Diagnostic environment switches
 * The library reads these environment variables (each ONCE per process, through one function, pfn::diag_env).  They select
 * between kernels that compute the SAME result -- the parity tests use them to hold a fused kernel against the generic one it
 * replaces, the tuning scripts under tools/ to sweep a launch parameter -- and none of them is needed in production: unset, the
 * library behaves as DESIGN.md describes.  There is no switch that routes work off the GPU or through another backend.
 *   PFN_NO_SEG_EA=1         EdgeAggregation of small-graph batches: generic gemm_nt + edge walks instead of the graph-resident kernels
 *   PFN_NO_SEG_LIN_HOPS=1   small-graph batches: the Linear in front of a TAGConv's hops and the hops as two launches (gemm_nt + fused hops)
 *                           instead of one graph-resident launch (seg_lin_hops.hip; bit-identical results)
 *   PFN_NO_FUSED_FRONT=1    mask_embd + first P|Q as generic GEMMs instead of front.hip's one launch
 *   PFN_NO_SEG_FRONT=1      small-graph batches: front.hip's launch + the generic first edge walk instead of the one graph-resident
 *                           launch that does both (ea_seg.hip front_seg_fwd_kernel; bit-identical results)
 *   PFN_NO_SEG_GATES=1      small-graph training steps: the graph-resident forward walks write P | Q and the graph-resident backward
 *                           recomputes the pre-activations from them, instead of saving one ReLU gate bit per (edge, column) in the
 *                           forward and reading it back (ea_seg.hip "SAVED GATES"; bit-identical results)
 *   PFN_NO_FUSED_BACK=1     the last layer's Linear / dS outside the edge walks (generic GEMMs)
 *   PFN_NO_MSE_TAIL=1       pfn_mpn_mse_tail_ok answers 0: the output Linear, MSELoss and the backward pass as three calls
 *   PFN_FRONT_BLOCK_ROWS=1  front.hip: the block-per-row-group kernels instead of one row per wave
 *   PFN_NO_BIG_HOPS=1       TAGConv hops of large graphs (one LDS tile + registers per graph and column chunk, workgroups persistent over a graph's chunks): K generic hop launches instead
 *   PFN_NO_ROW_HOPS=1       TAGConv hops of big batches of small graphs: the two-tile column-slice kernel instead of whole rows per block
 *   PFN_NO_EDGE_ROWS=1      the edge stage of big inference batches of small graphs: the generic gather kernel instead of the LDS-resident one
 *   PFN_NO_L0_FLY=1         the front writes the first layer's P | Q and the edge walk gathers them (default: the walk forms them from x0)
 *   PFN_EDGE_FWD_BPC=N      workgroups per CU of the persistent generic forward edge walk (default 8; a large N = one workgroup per 256 items)
 *   PFN_FRONT_STORE_MEH=1   training beyond 32 k rows: mask_embd's hidden layer is stored and its weight gradients go through gemm_tn
 *                           (default: recomputed in the backward front, which forms those gradients itself)
 *   PFN_FRONT_NO_THREAD_ROWS=1   inference front: the row-per-wave / block kernels instead of one row per thread
 *   PFN_NO_SERPENTINE=1     the row-streaming kernels (gemm_nt, LDS-resident walks / hops, the generic forward walk) all visit their rows
 *                           first to last (default: consecutive launches alternate, so a consumer starts with what its producer wrote last)
 *   PFN_BRANCH_NO_LDS=1     pfn_branch_flows: the direct kernel (phasors per line end from global memory) for every size
 *   PFN_NT_CT=1|2           gemm_nt: quarters per wave
 *   PFN_NO_NT_ILF=1         gemm_nt, one-piece tiles at two quarters per wave: every tile flushed behind its own multiply (default: parked
 *                           and flushed inside the wave's next multiply, between its own MFMAs)
 *   PFN_NO_NT_PAIR=1        gemm_nt, products of >= 3 terms at one quarter per wave: ONE fp32 chain through all terms (default: every
 *                           term summed on its own, the terms added in order -- PyG's TAGConv dataflow)
 *   PFN_NT_TINY_MAX_TILES=<n> gemm_nt: the split-K small-batch kernel up to n row tiles of 32 rows (default 256; 0 = never)
 *   PFN_NT_WS_MIN_TILES=<n> gemm_nt: weight-streaming kernel from n row tiles per wave (default 2; 0 = never)                     */

/* --------------------------------------------------------------------------------------- profiling
 * Optional HIP-event bracket around every kernel launch (same stream), aggregated per kernel class with
 * the launch's algorithmic bytes / flops.  Inactive during hipGraph capture.
 * pfn_profile_report synchronises the device and writes a JSON object into `buf`.                  */
int pfn_profile_enable(int on);
int pfn_profile_report(char* buf, size_t buf_bytes, int reset);

#ifdef __cplusplus
}
#endif
#endif /* PFN_HIP_H */
