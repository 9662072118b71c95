"""The dispatch predicates of the forward and backward passes, restated in Python (a plain helper module for the tests).  The
whole-model ones are the lines of csrc/model.hip make_route (one Route per entry point), the rest live next to their kernels.

Every constant and formula here is a copy of one in csrc/; tests/test_host.py::test_regime_constants_are_still_in_the_source checks
that each of them is still written there, literally, so a threshold that moves fails on the CPU first.  The GPU tests
(tests/test_gpu_boundaries.py) pick their shapes on both sides of each edge from these functions and check the side they landed on
against the profile classes (pfn_profile_report).  `cus` is always the device's CU count (multi_processor_count), never a constant.
"""

# ---- seg_tile.hpp / ea_seg.hip: the graph-resident EdgeAggregation kernels (and seg_lin_hops.hip, front_seg_fwd_kernel)
SG_MAX_ROWS = 128          # rows of whole graphs per workgroup
SG_LDS_BYTES = 78 * 1024   # two workgroups per CU
SG_NCH = 17                # eight-wide k chunks: K8 <= 136
SG_TW = 36                 # LDS tile row stride (floats)
SG_W2A_CH = 34             # float4 chunks per W2 row kept for the MSELoss tail
SG_BWD_MAX_BLOCKS = 1024   # the backward kernel's dWe partial buffer
PER_CU = 4                 # ea_seg_fit / seg_lin_hops_fit: `per_cu = 4L` row-block columns per CU (the latency regime)
# ---- front.hip: the row-per-wave kernels
WAVE_MAX_ROWS = 32768      # wave_max_rows()
# ---- edge.hip
FH_LDS_BYTES = 156 * 1024  # fused_hops_kernel
BH_THREADS = 1024          # big_graph_hops_kernel
BH_RPT = 8
BH_HUB_DEG = 32
BH_HUB_CAP = 128
RH_THREADS = 512           # row_hops_kernel
RH_IPT = 8
ER_THREADS = 512           # edge rows kernel
ER_IPT = 8
# ---- gemm_nt.hip
NT_THREADS = 512
NT_WAVES = NT_THREADS // 64
NCH = 17
KP = 8 * NCH               # 136 k's per piece
NT_MAX_PIECES = 16
NT_LDS_BYTES = 160 * 1024
TINY_MAX_PIECES = 8
TINY_MAX_TILES = 256       # PFN_NT_TINY_MAX_TILES default
WS_MIN_ROUNDS = 2          # PFN_NT_WS_MIN_TILES default (whole rounds of the chip)


def ld_of(f):
    return (f + 3) // 4 * 4


def col_plan(ld):
    """pfn_internal.hpp col_plan: (remv trailing VALU columns, nq 32-column quarters)."""
    m = ld & 31
    remv = m if (m != 0 and m <= 4) else 0
    return remv, (ld - remv + 31) // 32


def k8_of(k):
    return (k + 7) & ~7 if k <= 136 else (k + 135) // 136 * 136


# ------------------------------------------------------------------------------------------ graph-resident EdgeAggregation
def seg_lds_bytes(trows, rows_pb, cap, bwd):
    f = ((3 if bwd else 2) * trows * SG_TW + (0 if bwd else 2 * SG_NCH * 256) + 2 * SG_TW
         + ((4 * SG_TW + 4 * SG_W2A_CH * 4 + 8 * 16 * 2 * 4) if bwd else 0) + (2 if bwd else 1) * 2 * cap)
    if bwd:
        f += max(trows * SG_TW, SG_NCH * 256) - trows * SG_TW     # seg_bwd_d_floats: the dS room also holds the W2 quarter
    i = (2 if bwd else 1) * (rows_pb + 1 + cap)
    return (f + i) * 4 + 16


def seg_plan(seg, n, ld, bwd_limits=True):
    """ea_seg.hip seg_plan: the plan dict, or None where it does not fit."""
    if seg <= 0 or seg > SG_MAX_ROWS or n <= 0 or n % seg != 0:
        return None
    gpb = max(1, SG_MAX_ROWS // seg)
    rows_pb = gpb * seg
    trows = (rows_pb + 31) // 32 * 32
    cap = rows_pb * 4
    nblocks = (n + rows_pb - 1) // rows_pb
    ny = col_plan(ld)[1]
    ok = (ny >= 1 and ld <= 8 * SG_NCH and (not bwd_limits or nblocks <= SG_BWD_MAX_BLOCKS)
          and seg_lds_bytes(trows, rows_pb, cap, True) <= SG_LDS_BYTES and seg_lds_bytes(trows, rows_pb, cap, False) <= SG_LDS_BYTES)
    return dict(rows_pb=rows_pb, trows=trows, cap=cap, nblocks=nblocks, ny=ny) if ok else None


def ea_seg_fit(seg, n, fe, ld, bwd, cus):
    p = seg_plan(seg, n, ld, bwd)
    return fe == 2 and p is not None and p["nblocks"] * p["ny"] <= PER_CU * cus


def ea_seg_bwd_out_ok(fo):
    """ea_seg.hip ea_seg_bwd_out_ok: the backward kernel's dS product takes the last layer's output width as ONE k piece."""
    return ((fo + 7) & ~7) <= 8 * SG_NCH


def ea_seg_bwd_fit(seg, n, fe, ld, cus, fo=4):
    """Route::ea_seg_bwd (model.hip make_route): ea_seg_fit's backward form AND the output-width clause."""
    return ea_seg_fit(seg, n, fe, ld, True, cus) and ea_seg_bwd_out_ok(fo)


def seg_lin_hops_shape_ok(ld, h):
    """seg_lin_hops_fit's operand-shape clause (K = ncols = H = 129-shaped layers only)."""
    remv, nq = col_plan(ld)
    return ((h + 7) & ~7) == 8 * SG_NCH and h - (8 * SG_NCH - 8) == 1 and ld == ld_of(h) and remv == 4 and h - 32 * nq == 1


def seg_lin_hops_fit(seg, n, ld, h, nhops, cus):
    """seg_lin_hops_fit without its LDS-size clause (slh_lds_bytes), which every seg <= SG_MAX_ROWS at H = 129 meets: the shape,
    fused_hops_fit and the ea_seg_fit grid bound (the same `per_cu`)."""
    if not (nhops > 0 and seg_lin_hops_shape_ok(ld, h) and fused_hops_fit(seg)):
        return False
    if seg <= 0 or seg > SG_MAX_ROWS or n <= 0 or n % seg != 0:
        return False
    rows_pb = max(1, SG_MAX_ROWS // seg) * seg
    return ((n + rows_pb - 1) // rows_pb) * col_plan(ld)[1] <= PER_CU * cus


# ------------------------------------------------------------------------------------------ front / last layer
def front_row_per_wave(nchunk, n):
    return nchunk <= 64 and n <= WAVE_MAX_ROWS


def front_latency_regime(h, n):
    return front_row_per_wave(ld_of(h) // 4, n)


def front_fused_ok(f0, h):
    return f0 == 4 and ld_of(h) // 4 <= 256


def lin_out4_ok(h, fo, ldo, n):
    return 1 <= fo <= 4 and ldo == 4 and ld_of(h) // 4 <= 64 and n <= WAVE_MAX_ROWS


def front_seg_fit(seg, n, h, fe, cus):
    ld = ld_of(h)
    return ld // 4 <= 64 and front_latency_regime(h, n) and ea_seg_fit(seg, n, fe, ld, False, cus)


def edge_fwd_out_ok(fe, h, fo, ldo):
    """edge.hip: the last layer's output Linear rides in its generic edge walk (edge_fwd_out_kernel)."""
    return fe == 2 and 1 <= fo <= 4 and ldo == 4 and ld_of(h) // 4 <= 256


def ea_saves_mask(train, n, fe, ld, seg, fused_front, i, cus, fo=4):
    generic_fwd = not ea_seg_fit(seg, n, fe, ld, False, cus) or (fused_front and i == 0)
    return train and fe == 2 and generic_fwd and not ea_seg_bwd_fit(seg, n, fe, ld, cus, fo)


def first_layer_fly(train, n, h, L, fe, seg, cus, f0=4, fo=4):
    fused_front = front_fused_ok(f0, h)
    return (fused_front and L > 1 and fe == 2 and f0 == 4 and not front_latency_regime(h, n)
            and (not train or ea_saves_mask(train, n, fe, ld_of(h), seg, fused_front, 0, cus, fo)))


def uses_seg_front(train, n, h, L, fe, seg, cus, f0=4, fo=4):
    ld = ld_of(h)
    return (front_fused_ok(f0, h) and ea_seg_fit(seg, n, fe, ld, False, cus) and not first_layer_fly(train, n, h, L, fe, seg, cus, f0, fo)
            and L > 1 and front_seg_fit(seg, n, h, fe, cus) and not (train and fe == 2 and not ea_seg_bwd_fit(seg, n, fe, ld, cus, fo)))


def mse_tail_ok(train, n, h, L, fe, seg, cus, fo=4):
    ld = ld_of(h)
    return (train and n > 0 and L > 1 and fe == 2 and fo == 4 and ld_of(fo) == 4 and lin_out4_ok(h, fo, ld_of(fo), n)
            and ea_seg_fit(seg, n, fe, ld, False, cus) and ea_seg_bwd_fit(seg, n, fe, ld, cus, fo) and ld // 4 <= 34)


def mse_tail_available(train, n, h, L, fe, seg, cus, fo=4):
    """pfn_mpn_mse_tail_ok: what the attached MSELoss / Masked_L2_loss need."""
    return mse_tail_ok(train, n, h, L, fe, seg, cus, fo) and uses_seg_front(train, n, h, L, fe, seg, cus, fo=fo)


# ------------------------------------------------------------------------------------------ TAGConv hops (edge.hip)
def fused_hops_fit(seg):
    return 0 < seg and 2 * seg * 4 * 4 + (2 * seg + 1) * 4 <= FH_LDS_BYTES // 2


def bh_hub_bytes():
    return BH_HUB_CAP * 16 + BH_HUB_CAP * 2 + 16


def big_hops_fit(seg, n):
    if seg <= 0 or n <= 0 or n % seg != 0 or seg > BH_RPT * BH_THREADS or seg >= 65536:
        return False
    return (seg + 1) * 16 + bh_hub_bytes() + ((seg + 2 + 7) & ~7) * 2 + 1024 <= 160 * 1024


def big_hops_nb_cap(seg, n, e_stored):
    """launch_big_graph_hops: the neighbour-list slots of a workgroup's LDS -- an equal share of the stored edges per graph with
    slack, within 160 KiB after the tile, the hub list and the row offsets."""
    ngraphs = n // seg
    fixed = (seg + 1) * 16 + bh_hub_bytes() + ((seg + 2 + 7) & ~7) * 2
    want_nb = (2 * e_stored // max(1, ngraphs) + 64) * 2
    lds_total = min(160 * 1024, fixed + want_nb)
    return (lds_total - fixed) // 2


def big_hops_staged(seg, n, e_stored, ne):
    """big_graph_hops_kernel: is the adjacency of a graph with `ne` edges (the in-edges of its rows) staged in LDS, or does the
    graph walk unstaged (bh_unstaged_graph)?  The kernel's `ne < 65536` clause never decides: nb_cap <= 62,776 slots wherever
    big_hops_fit applies (seg >= 1,997), so `ne + 4 <= nb_cap` fails first."""
    return ne + 4 <= big_hops_nb_cap(seg, n, e_stored) and ne < 65536


def hop_kernel(seg, n, K):
    """Which hop kernel a TAGConv over a graph with segment hint `seg` takes (model.hip hop_kind): 'fused' (two-tile / row
    kernels, profile class fused_hops_*), 'big' (big_graph_hops_kernel, ALSO profiled as fused_hops_*), 'generic' (K hop_norm)."""
    if K == 0:
        return None
    if seg > 0 and n % seg == 0 and fused_hops_fit(seg):
        return "fused"
    if big_hops_fit(seg, n):
        return "big"
    return "generic"


def row_hops_graphs_per_block(seg, nchunk):
    if seg <= 0 or seg > 1023 or seg * nchunk > RH_IPT * RH_THREADS:
        return 0
    gpb = min((RH_IPT * RH_THREADS) // (seg * nchunk), 1023 // seg)
    while gpb > 0 and gpb * seg * nchunk * 16 + ((gpb * seg + 2 + 7) & ~7) * 2 + 4096 > 78 * 1024:
        gpb -= 1
    return gpb


def edge_rows_graphs_per_block(seg, nchunk):
    if seg <= 0 or seg > 1023 or seg * nchunk > ER_IPT * ER_THREADS or 8 * nchunk > ER_THREADS:
        return 0
    gpb = min((ER_IPT * ER_THREADS) // (seg * nchunk), 1023 // seg)
    while gpb > 0 and gpb * seg * nchunk * 16 + 4096 > 66 * 1024:
        gpb -= 1
    return gpb


def row_hops_ok(seg, n, ld, cus):
    """launch_fused_hops' row_hops_kernel branch (forward data flow only): enough workgroups of whole graphs to fill the chip."""
    gpb = row_hops_graphs_per_block(seg, ld // 4)
    return gpb > 0 and n % seg == 0 and -(-(n // seg) // gpb) >= 4 * cus


def edge_rows_ok(seg, n, ld, cus):
    """launch_edge_fwd's edge-rows branch (inference: no ReLU masks, Fe = 2)."""
    gpb = edge_rows_graphs_per_block(seg, ld // 4)
    return seg > 0 and gpb > 0 and n % seg == 0 and -(-(n // seg) // gpb) >= 4 * cus


def first_graph_count(pred, hi=1 << 22):
    """The smallest graph count B >= 1 with pred(B) true, for a predicate that is monotone in B."""
    lo = 1
    assert pred(hi)
    while lo < hi:
        mid = (lo + hi) // 2
        if pred(mid):
            hi = mid
        else:
            lo = mid + 1
    assert pred(lo) and (lo == 1 or not pred(lo - 1))
    return lo


# ------------------------------------------------------------------------------------------ gemm_nt (the TAGConv products)
def gemm_nt_plan(M, cin, cout, nterm, cus):
    """The kernel launch_gemm_nt picks for a TAGConv forward product out = sum_k X_k W_k^T (+ bias): nterm = K + 1 terms of
    cin -> cout.  Returns dict(kind, tps, pieces, CT, rows_ws) with kind one of 'tiny', 'ws' (whole rounds only), 'ws+stationary',
    'wide', 'stationary' (one launch) or 'multi' (several accumulating stationary launches)."""
    ld = ld_of(cout)
    remv, nq = col_plan(ld)
    klen = k8_of(cin)
    per_term = 1 if klen <= KP else klen // KP
    piece_k = min(klen, KP)
    kmax_last = cin - (per_term - 1) * KP                      # the real k's of a term's last piece
    npieces = nterm * per_term
    nrem = max(0, min(remv, cout - 32 * nq))
    bias_bytes = (ld * 4 + 15) // 16 * 16
    budget = NT_LDS_BYTES - bias_bytes

    def piece_bytes(tps):
        return piece_k * (32 * tps + 4) * 4

    tps = 0
    if nq > 0:
        start = min(4 if nq >= 3 else nq, 4)
        tps = start
        while tps >= 1:
            if npieces * piece_bytes(tps) <= budget and npieces <= NT_MAX_PIECES:
                break
            tps >>= 1
        if tps < 1:
            tps = min(start, 2)
    nrt = (M + 31) // 32
    nslices = (nq + tps - 1) // tps if tps > 0 else 1
    last_step_one = piece_k == KP and kmax_last % 8 == 1        # (last_steps == 1: one real k in the last chunk)
    fast = (piece_k == KP and nrem <= 1) or (piece_k == KP - 8 and remv == 0)
    fast = fast and kmax_last >= piece_k - 12                    # (diet_ok: the straight-line variants)
    CT = 0 if tps == 0 else 1
    if fast and tps >= 2 and nrt * nslices * (tps // 2) >= 2 * cus * NT_WAVES:
        CT = 2
    out = dict(tps=tps, pieces=npieces, CT=CT, nrt=nrt, nslices=nslices, rows_ws=0)
    if (nrt <= TINY_MAX_TILES and nq == 4 and remv == 4 and nrem == 1 and npieces <= TINY_MAX_PIECES and piece_k == KP
            and per_term == 1 and last_step_one):
        return dict(out, kind="tiny")
    per_round = cus * NT_WAVES
    if (nq == 4 and remv == 4 and nrem == 1 and nslices > 2 and npieces <= NT_MAX_PIECES and nrt >= WS_MIN_ROUNDS * per_round
            and piece_k == KP and per_term == 1 and last_step_one):
        rows_ws = min(M, (nrt // per_round) * per_round * 32)
        return dict(out, kind="ws" if rows_ws == M else "ws+stationary", rows_ws=rows_ws)
    if remv == 0 and nq >= 8 and nq % 4 == 0 and npieces <= NT_MAX_PIECES and ld == 32 * nq and piece_k == KP:
        return dict(out, kind="wide")
    fits = npieces <= NT_MAX_PIECES and npieces * piece_bytes(max(tps, 1)) <= budget
    return dict(out, kind="stationary" if fits else "multi")


# ------------------------------------------------------------------------------------------ a whole MaskEmbdMultiMPN step
def route(n, seg, H, L, K, fe, train, cus, fo=4):
    """model.hip make_route for MaskEmbdMultiMPN(4, fe, fo, H, L, K) without the diagnostic switches: the Route's fields by name."""
    ld = ld_of(H)
    fused_front = front_fused_ok(4, H)
    r = dict(fused_front=fused_front, ea_seg_fwd=ea_seg_fit(seg, n, fe, ld, False, cus), ea_seg_bwd=ea_seg_bwd_fit(seg, n, fe, ld, cus, fo),
             mask0=ea_saves_mask(train, n, fe, ld, seg, fused_front, 0, cus, fo),
             mask1=ea_saves_mask(train, n, fe, ld, seg, fused_front, 1, cus, fo),
             l0_fly=first_layer_fly(train, n, H, L, fe, seg, cus, fo=fo), seg_front=uses_seg_front(train, n, H, L, fe, seg, cus, fo=fo),
             lin_out4=lin_out4_ok(H, fo, ld_of(fo), n), mse_tail=mse_tail_ok(train, n, H, L, fe, seg, cus, fo), hops=hop_kernel(seg, n, K))
    # saved gates (without its diagnostic switch): every EdgeAggregation graph-resident, forward and backward
    r["seg_gates"] = train and fe == 2 and r["ea_seg_fwd"] and r["ea_seg_bwd"] and (r["seg_front"] or not fused_front)
    # (front_recomputes_meh: me_h holds front_bwd_wg_kernel's partial sums -- a bound on the batch that is not restated; the check
    #  only needs that it is never set without l0_fly)
    r["meh_recompute"] = train and r["l0_fly"]
    r["masked_tail"] = r["mse_tail"] and r["seg_front"]
    r["big_cm"] = n if (K > 0 and not fused_hops_fit(seg) and big_hops_fit(seg, n)) else 0
    r["slh_fwd"] = r["slh_bwd"] = not r["big_cm"] and seg_lin_hops_fit(seg, n, ld, H, K, cus)
    return r


def route_contradictions(r):
    """The check make_route ends with: what forward, backward, the loss tails and the gate export take for granted of each other.
    Returns the names of the violated implications (empty: sound)."""
    checks = {
        "ea_seg_bwd -> ea_seg_fwd": not r["ea_seg_bwd"] or r["ea_seg_fwd"],
        "seg_front -> layer 0 saves no masks": not r["seg_front"] or not r["mask0"],
        "l0_fly -> fused_front and not seg_front": not r["l0_fly"] or (r["fused_front"] and not r["seg_front"]),
        "meh_recompute -> l0_fly": not r["meh_recompute"] or r["l0_fly"],
        "mse_tail -> ea_seg_fwd, ea_seg_bwd, lin_out4": not r["mse_tail"] or (r["ea_seg_fwd"] and r["ea_seg_bwd"] and r["lin_out4"]),
        "slh -> fused hops, row-major": not (r["slh_fwd"] or r["slh_bwd"]) or (r["hops"] == "fused" and not r["big_cm"]),
        "big_cm -> big hops": not r["big_cm"] or r["hops"] == "big",
        "seg_gates -> no generic walk": not r.get("seg_gates", False) or (
            r["ea_seg_fwd"] and r["ea_seg_bwd"] and not r["mask0"] and not r["mask1"] and not r["l0_fly"]
            and (r["seg_front"] or not r["fused_front"])),
    }
    return [name for name, ok in checks.items() if not ok]


def model_regime(n, seg, H, L, K, fe, train, cus, fo=4, gea=False):
    """The regime of every stage of MaskEmbdMultiMPN(4, fe, fo, H, L, K) on n rows of graphs of `seg` nodes, and the profile classes
    that must and must not appear in its forward (+ backward, when `train`).  `train` is the model's need_backward: a forward under
    autograd whose backward pass runs, with or without dropout.  `gea`: the backward pass is also asked for the edge-attribute
    gradient, which only the generic (recomputing) backward walks form (model_backward: `seg_bwd = r.ea_seg_bwd && !gea`).

    L is n_gnn_layers.  Only what the restated predicates decide is listed; the rest of a launch sequence is not pinned here."""
    ld = ld_of(H)
    fwd_seg = ea_seg_fit(seg, n, fe, ld, False, cus)
    bwd_seg = ea_seg_bwd_fit(seg, n, fe, ld, cus, fo) and not gea
    seg_front = uses_seg_front(train, n, H, L, fe, seg, cus, fo=fo)
    # the last layer's output Linear inside its generic edge walk (ea_forward's out_in_walk)
    out_in_walk = not fwd_seg and edge_fwd_out_ok(fe, H, fo, ld_of(fo))
    r = dict(ld=ld, ny=col_plan(ld)[1], ea_seg_fwd=fwd_seg, ea_seg_bwd=bwd_seg and train, seg_front=seg_front,
             front_latency=front_latency_regime(H, n), lin_out4=lin_out4_ok(H, fo, ld_of(fo), n), out_in_walk=out_in_walk,
             l0_fly=first_layer_fly(train, n, H, L, fe, seg, cus, fo=fo), mse_tail=mse_tail_available(train, n, H, L, fe, seg, cus, fo),
             hops=hop_kernel(seg, n, K), slh=seg_lin_hops_fit(seg, n, ld, H, K, cus) and L > 1,
             edge_rows=not train and fe == 2 and not fwd_seg and edge_rows_ok(seg, n, ld, cus),
             row_hops=K > 0 and hop_kernel(seg, n, K) == "fused" and row_hops_ok(seg, n, ld, cus))
    must, must_not = set(), set()
    if seg_front:
        must.add("front_seg_fwd+pack")
        must_not.add("front_fwd+pack")
    else:
        must_not.add("front_seg_fwd+pack")
        if front_fused_ok(4, H):
            must.add("front_fwd+pack")
    if not fwd_seg:
        must_not.add("ea_seg_fwd")
        must.add("edge_rows_fwd" if r["edge_rows"] else "edge_fwd")
    if not r["edge_rows"]:
        must_not.add("edge_rows_fwd")
    if train and bwd_seg:
        must.add("ea_seg_bwd")
    if not train or not bwd_seg:
        must_not.update({"ea_seg_bwd", "ea_seg_bwd+out+mse", "ea_seg_bwd+out+masked_l2"})
    if train and not bwd_seg:
        must.add("edge_bwd")
    if fwd_seg:
        must.add("ea_seg_fwd")           # (the last EdgeAggregation is never layer 0: never behind front_seg_fwd)
    # the output Linear: in the last layer's generic edge walk (edge_fwd_out_kernel: Fe = 2, Fo <= 4) unless that layer ran
    # graph-resident; else lin_out4 where lin_out4_ok holds (on the plain loss path: an attached loss tail forms the rows in the
    # backward's first launch); else gemm_nt with N = Fo
    if not out_in_walk and r["lin_out4"]:
        must.add("lin_out4")
    else:
        must_not.add("lin_out4")
        if not out_in_walk:
            must.add("gemm_nt")
    if K == 0:                           # no hop of any kind (HOPS_NONE): a TAGConv is its k = 0 product alone
        must_not.update({"hop_norm", "fused_hops_fwd", "fused_hops_bwd", "seg_lin_hops_fwd", "seg_lin_hops_bwd"})
    if not r["slh"]:
        must_not.update({"seg_lin_hops_fwd", "seg_lin_hops_bwd"})
    if K > 0 and r["hops"] in ("fused", "big") and not r["slh"]:
        must.add("fused_hops_fwd")
        must_not.add("hop_norm")
    if K > 0 and r["hops"] == "generic":
        must.add("hop_norm")
        must_not.update({"fused_hops_fwd", "fused_hops_bwd"})
    r["must"], r["must_not"] = must, must_not
    return r
