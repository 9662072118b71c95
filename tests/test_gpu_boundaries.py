"""Both sides of every dispatch threshold against the oracle.

The forward and backward passes choose among a dozen kernel families by predicates on the graph size, the row count, the batch
count relative to the CU count, the hidden width and the GEMM term count (restated in tests/regimes.py, pinned to csrc/ by
tests/test_host.py).  Each family below takes shapes just inside and just outside one edge, derived from the device's CU count,
checks the side it landed on from the profile classes (pfn_profile_report), and holds the forward output and every gradient to
north_star's 1e-5 against oracle/ref_cpu.py (the float64 oracle on the HIP path's own ReLU decisions for the gradients).
Where the profile classes cannot separate two kernels the restated predicate decides, and the test says so:
`fused_hops_*` covers the two-tile, row and big-graph hop kernels; `gemm_nt` covers the tiny, stationary, streaming and wide ones.
"""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from poweflownet_amd.data import Batch
from poweflownet_amd.networks.MPN import GraphCSR, MaskEmbdMultiMPN, TAGConv
from poweflownet_amd.synth import _MASK_TABLE, make_topology
from tests import regimes as R
from tests.util import RTOL, _assert_grads_on_hip_gates, _cpu_gates, _exported_masks, _fp64_truth, _to64, assert_close, record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _profiled(fn):
    from poweflownet_amd import _lib as L
    L.profile_report(reset=True)
    L.profile_enable(True)
    try:
        res = fn()
        torch.cuda.synchronize()
    finally:
        L.profile_enable(False)
    rep = L.profile_report(reset=True)
    return res, {k: v["count"] for k, v in rep.items() if not k.startswith("__")}


def _check_classes(launches, must, must_not, what):
    record(f"{what}: launches {sorted(launches.items())}", 0.0, 1.0, None)
    for k in sorted(must):
        assert launches.get(k, 0) > 0, (what, "missing", k, launches)
    for k in sorted(must_not):
        assert k not in launches, (what, "unexpected", k, launches)


def _batch(seg, B, seed, e=None):
    """B samples of one `seg`-node grid (a shared connected topology, make_graph's statistics), collated like the loader, built
    without a per-graph Python loop (tens of thousands of graphs)."""
    e = max(seg - 1, (3 * seg) // 2) if e is None else e
    topo = make_topology(seg, e, seed) if seg > 1 else torch.zeros(2, 0, dtype=torch.long)
    g = torch.Generator().manual_seed(seed)
    n = seg * B
    bus_type = torch.full((seg,), 2, dtype=torch.long)
    bus_type[::3] = 1
    bus_type[0] = 0
    bus_type = bus_type.repeat(B)
    pred_mask = _MASK_TABLE[bus_type]
    y = torch.randn(n, 4, generator=g)
    off = (torch.arange(B, dtype=torch.long) * seg).repeat_interleave(topo.shape[1])
    ei = topo.repeat(1, B) + off
    d = Batch()
    d.x, d.y, d.bus_type, d.pred_mask = y * (1 - pred_mask).float(), y, bus_type, pred_mask
    d.edge_index, d.edge_attr = ei, torch.randn(ei.shape[1], 2, generator=g)
    d.batch = torch.arange(B).repeat_interleave(seg)
    d.ptr = torch.arange(B + 1, dtype=torch.long) * seg
    return d


def _models(H, L_, K, p, seed):
    torch.manual_seed(seed)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, H, L_, K, p)
    with torch.no_grad():
        for mod in ref.layers:
            if hasattr(mod, "lins"):
                mod.bias.normal_(std=0.1)              # TAGConv bias is zero-initialised: exercise it
    m = MaskEmbdMultiMPN(4, 2, 4, H, L_, K, p)
    m.load_state_dict(ref.state_dict())
    return ref, m.to(DEV)


def _model_case(seg, B, H, L_, K, p, train, what, seed=0, data=None):
    """One model-level case: forward (and, when `train`, every parameter gradient of MSELoss) against the oracle; the profile
    classes against the restated predicates.  Dropout p > 0 trains against the oracle fed the exported keep masks."""
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    ref, m = _models(H, L_, K, p, seed)
    data = _batch(seg, B, seed) if data is None else data
    n = data.x.shape[0]
    reg = R.model_regime(n, seg, H, L_, K, 2, train, _cus())
    dd = data.to(DEV)
    m.train(p > 0)
    ref.train(p > 0)
    m.seed_dropout(1000 + seed)
    if train:
        def step():
            out = m(dd)
            torch.nn.MSELoss()(out, dd.y).backward()
            return out
        out, launches = _profiled(step)
    else:
        with torch.no_grad():
            out, launches = _profiled(lambda: m(dd))
    assert m._graphs._graph.seg_nodes == seg, (what, m._graphs._graph.seg_nodes)
    _check_classes(launches, reg["must"], reg["must_not"], what)
    if p > 0:
        ref.dropout_masks = [k.cpu() for k in _exported_masks(m, n)]
    if train:
        out_ref = ref(data)
        torch.nn.MSELoss()(out_ref, data.y).backward()
    else:
        with torch.no_grad():
            out_ref = ref(data)
    out64, _ = _fp64_truth(ref, data)
    assert_close(out, out_ref, RTOL, f"{what}: out")
    assert_close(out, out64.float(), RTOL, f"{what}: out vs fp64")
    if train:
        if n <= 2000:                                   # small: the plain fp32 oracle, no gate equalisation needed
            for (k, q_), q in zip(m.named_parameters(), ref.parameters()):
                assert_close(q_.grad, q.grad, RTOL, f"{what}: grad.{k}")
        _assert_grads_on_hip_gates(m, ref, data, what, out)
    return m, dd, reg, launches


# ------------------------------------------------------------------------------------------ graph size around the LDS tile
@pytest.mark.parametrize("seg,p", [(1, 0.0), (2, 0.2), (3, 0.0), (43, 0.0), (64, 0.2), (65, 0.0), (127, 0.0), (128, 0.2), (129, 0.0)])
def test_graph_resident_kernels_at_every_graph_size_edge(seg, p):
    """seg_plan (ea_seg.hip): graphs of <= SG_MAX_ROWS = 128 nodes, rows_pb = (128 // seg) * seg rows per workgroup, trows rounded
    up to 32.  seg 1 has no edges at all, 2 / 3 / 43 / 64 / 65 / 127 round rows_pb and trows differently, 128 fills the tile, 129 is
    the first size the graph-resident kernels refuse (the generic edge walks run).  The batch ends in a partial workgroup."""
    gpb = max(1, R.SG_MAX_ROWS // seg)
    B = 7 * gpb + 1
    _, _, reg, launches = _model_case(seg, B, 32, 2, 2, p, True, f"seg {seg}", seed=seg)
    assert reg["ea_seg_fwd"] == (seg <= R.SG_MAX_ROWS)
    if seg <= R.SG_MAX_ROWS:
        assert launches.get("ea_seg_bwd", 0) + launches.get("front_seg_fwd+pack", 0) > 0


@pytest.mark.parametrize("seg", [43, 48, 49, 65, 96, 97])
def test_graph_resident_backward_at_the_96_row_tile(seg):
    """ea_seg_bwd_kernel multiplies dS from a W2 quarter that first lies where the dS tile will be (seg_lds: B0 aliases D): up to
    17 * 256 floats, more than a 96-row tile of 36-float rows.  rows_pb <= 96, i.e. graphs of 43..48 nodes (two per workgroup) and
    of 65..96 (one), at H = 129 (K8 = 136): the room must be the larger of the two (seg_bwd_d_floats) -- sized by the tile alone
    the quarter's tail lay over the We slice, whose commit then wrote into the weights, and every gradient behind the layer was
    wrong by tens of per cent.  49 and 97 are the first sizes back on a 128-row tile."""
    gpb = max(1, R.SG_MAX_ROWS // seg)
    plan = R.seg_plan(seg, seg * (3 * gpb + 1), R.ld_of(129))
    assert plan is not None and (plan["trows"] == 96) == (seg in (43, 48, 65, 96)), plan
    what, B = f"seg {seg} at H 129", 3 * gpb + 1
    ref, m = _models(129, 2, 3, 0.0, seg)
    data = _batch(seg, B, seg)
    dd = data.to(DEV)
    dd.x.requires_grad_(True)

    def step():
        out = m(dd)
        torch.nn.MSELoss()(out, dd.y).backward()
        return out
    out, launches = _profiled(step)
    reg = R.model_regime(seg * B, seg, 129, 2, 3, 2, True, _cus())
    _check_classes(launches, reg["must"], reg["must_not"], what)
    assert reg["ea_seg_bwd"] and launches.get("ea_seg_bwd", 0) > 0, launches
    with torch.no_grad():
        assert_close(out, ref(data), RTOL, f"{what}: out")
    # (gradients on the HIP forward's own ReLU decisions: in a net this small ONE gate that differs from the fp32 oracle's moves a
    #  weight gradient by more than the tolerance, see _assert_grads_on_hip_gates)
    gates = _cpu_gates(m)
    _assert_grads_on_hip_gates(m, ref, data, what, out, gates)
    ref64 = copy.deepcopy(ref).double()
    ref64.gates = gates
    d64 = _to64(data)
    d64.x.requires_grad_(True)
    torch.nn.MSELoss()(ref64(d64), d64.y).backward()
    assert_close(dd.x.grad, d64.x.grad.float(), RTOL, f"{what}: grad x")


# ------------------------------------------------------------------------------------------ batch count at the latency-regime bound
@pytest.mark.parametrize("seg,H,partial", [(118, 129, False), (14, 129, True), (118, 32, False)])
def test_latency_regime_batch_bound_with_attached_losses(seg, H, partial):
    """ea_seg_fit / seg_lin_hops_fit / front_seg_fit / Route::mse_tail: ceil(n / rows_pb) * ny <= 4 * CUs (and <= 1024 row blocks in
    backward).  The largest graph count inside the bound and the first one past it (and, for 14-bus grids, one graph fewer, whose
    last workgroup is partial) -- 118-bus and 14-bus at H = 129 (ny = 4, the seg_lin_hops layers), 118-bus at H = 32 (ny = 1: the
    forward bound and the backward's 1,024 blocks coincide).  The H = 129 pairs stay within 32,768 rows, so front_seg_fwd and the
    graph-resident backward switch off together there: the check that ends model.hip make_route (front_seg_fwd never runs where layer 0's backward
    would read ReLU masks).  The H = 32 pair is above 32,768 rows: no front_seg_fwd and no loss tail on either side.  Training
    with dropout 0.2 against the oracle fed the exported masks; the attached MSELoss and Masked_L2_loss tails bit for bit equal to
    the three-call path inside, cleanly absent outside."""
    from poweflownet_amd.loss import MSELoss
    from poweflownet_amd.utils.custom_loss_functions import Masked_L2_loss
    from tests.util import _run, _run_masked
    cus = _cus()
    ld = R.ld_of(H)
    first_out = R.first_graph_count(lambda b: not R.ea_seg_fit(seg, seg * b, 2, ld, False, cus))
    counts = [first_out - 1, first_out] + ([first_out - 2] if partial else [])
    for B in counts:
        what = f"{seg}-bus x {B} at H {H}"
        inside = B < first_out
        m, dd, reg, launches = _model_case(seg, B, H, 2, 2, 0.2, True, what, seed=B)
        assert reg["ea_seg_fwd"] == inside and reg["ea_seg_bwd"] == inside
        assert reg["mse_tail"] == (inside and R.front_latency_regime(H, seg * B)), reg
        if H == 129:
            assert reg["slh"] == inside
            if inside:
                assert launches.get("seg_lin_hops_bwd", 0) + launches.get("seg_lin_hops_fwd", 0) > 0, launches
        m.train()
        for loss_fn, runner, tail in ((MSELoss(), _run, "ea_seg_bwd+out+mse"), (Masked_L2_loss(), _run_masked, "ea_seg_bwd+out+masked_l2")):
            plain = runner(m, dd, loss_fn, False)
            fused = runner(m, dd, loss_fn, True)
            assert tail not in plain["launches"]
            if reg["mse_tail"]:
                assert fused["launches"].get(tail) == 1 and "lin_out4" not in fused["launches"], (what, fused["launches"])
            else:
                assert tail not in fused["launches"], (what, fused["launches"])
            assert torch.equal(fused["out"], plain["out"]), what
            assert torch.equal(fused["g"], plain["g"]), (what, (fused["g"] - plain["g"]).abs().max().item())
            a, b = fused["loss"].item(), plain["loss"].item()
            assert abs(a - b) <= 2e-6 * abs(b), (what, a, b)


# ------------------------------------------------------------------------------------------ row-per-wave front / lin_out4
@pytest.mark.parametrize("train", [True, False])
def test_row_per_wave_front_at_its_row_bound(train):
    """front_row_per_wave / front_latency_regime / lin_out4_ok / Route::l0_fly (front.hip, model.hip make_route): n <= wave_max_rows() =
    32,768 rows.  16-node grids: 32,768 rows exactly (front_seg_fwd, the fused front + first edge stage) and one graph more
    (the block front; in inference layer 0's P | Q formed on the fly in the edge walk), in training and in inference."""
    seg = 16
    B_at = R.WAVE_MAX_ROWS // seg
    for B in (B_at, B_at + 1):
        what = f"{seg}-node x {B} ({seg * B} rows), {'training' if train else 'inference'}"
        _, _, reg, launches = _model_case(seg, B, 32, 2, 2, 0.2 if train else 0.0, train, what, seed=B)
        assert reg["front_latency"] == (B == B_at) and reg["lin_out4"] == (B == B_at)
        assert reg["seg_front"] == (B == B_at)
        assert reg["l0_fly"] == (B != B_at and not train), reg


@pytest.mark.parametrize("H", [256, 257])
def test_front_width_bound(H):
    """front_row_per_wave / lin_out4_ok: ld / 4 <= 64 chunks, i.e. H <= 256; H = 257 takes the block front.  Forward and every
    gradient against the oracle on both sides.  The profile cannot show the side: the row-per-wave and the block front are both
    front_fwd+pack / front_bwd, and lin_out4 runs at neither width -- above ld = 136 no layer is graph-resident, so the last
    layer's output Linear rides in its generic edge walk (edge_fwd_out_kernel).  The restated predicate decides."""
    _, _, reg, launches = _model_case(14, 20, H, 2, 2, 0.2, True, f"H {H}", seed=H)
    assert reg["lin_out4"] == (H <= 256) and reg["front_latency"] == (H <= 256)


# ------------------------------------------------------------------------------------------ inference: edge rows / row hops
def test_edge_rows_and_row_hops_first_admitting_graph_count():
    """launch_edge_fwd's edge-rows kernel and launch_fused_hops' row_hops_kernel: ceil(ngraphs / gpb) >= 4 * CUs (inference on
    big batches of small graphs).  14-bus grids at H = 32: one graph below and at the first count of each.  edge_rows_fwd is its
    own profile class; the row kernel shares fused_hops_fwd with the two-tile kernel, so the restated predicate decides there."""
    cus = _cus()
    seg, H = 14, 32
    ld = R.ld_of(H)
    b_er = R.first_graph_count(lambda b: R.edge_rows_ok(seg, seg * b, ld, cus))
    b_rh = R.first_graph_count(lambda b: R.row_hops_ok(seg, seg * b, ld, cus))
    for B in sorted({b_er - 1, b_er, b_rh - 1, b_rh}):
        what = f"{seg}-bus x {B} inference"
        _, _, reg, launches = _model_case(seg, B, H, 2, 2, 0.0, False, what, seed=B)
        assert reg["edge_rows"] == (B >= b_er) and reg["row_hops"] == (B >= b_rh)
        assert (launches.get("edge_rows_fwd", 0) > 0) == (B >= b_er), (what, launches)


# ------------------------------------------------------------------------------------------ TAGConv hops at layer level
def _tag_case(cin, cout, K, ei, n, seg, what, seed=0, mode=0):
    """TAGConv(cin, cout, K) over an already-built adjacency (GraphCSR with a segment hint) against the oracle TAGConv in float64:
    the output, grad_x, every lins.k.weight gradient and the bias gradient.  Returns the profile classes of forward + backward."""
    torch.manual_seed(seed)
    ref = ref_cpu.TAGConv(cin, cout, K=K)
    with torch.no_grad():
        ref.bias.normal_(std=0.1)
    layer = TAGConv(cin, cout, K=K)
    layer.load_state_dict(ref.state_dict())
    layer = layer.to(DEV)
    x = torch.randn(n, cin)
    g = torch.randn(n, cout)
    graph = GraphCSR(ei.to(DEV), n, mode=mode, seg_hint=seg)
    assert graph.seg_nodes == seg, (what, graph.seg_nodes)
    xd = x.to(DEV).requires_grad_(True)

    def step():
        out = layer.on_graph(graph, xd)
        out.backward(g.to(DEV))
        return out
    out, launches = _profiled(step)
    ref64 = ref.double()
    x64 = x.double().requires_grad_(True)
    out64 = ref64(x64, ei)
    out64.backward(g.double())
    assert_close(out, out64.float(), RTOL, f"{what}: out")
    assert_close(xd.grad, x64.grad.float(), RTOL, f"{what}: grad_x")
    for k in range(K + 1):
        assert_close(layer.lins[k].weight.grad, ref64.lins[k].weight.grad.float(), RTOL, f"{what}: grad lins.{k}.weight")
    assert_close(layer.bias.grad, ref64.bias.grad.float(), RTOL, f"{what}: grad bias")
    return launches


def _bidirectional(topo):
    return torch.cat([topo, topo.flip(0)], dim=1)


def _graphs(seg, B, e, seed):
    topo = _bidirectional(make_topology(seg, e, seed))
    off = (torch.arange(B, dtype=torch.long) * seg).repeat_interleave(topo.shape[1])
    return topo.repeat(1, B) + off


@pytest.mark.parametrize("seg", [1996, 1997, 8192, 8193])
def test_hop_kernels_at_their_graph_size_bounds(seg):
    """fused_hops_fit (edge.hip): two tiles of one float4 column plus offsets in half of FH_LDS_BYTES, 40 seg + 4 <= 78 KiB, i.e.
    seg <= 1,996; big_hops_fit: seg <= BH_RPT * BH_THREADS = 8,192.  1,996 -> the two-tile kernel, 1,997 and 8,192 ->
    big_graph_hops_kernel (both profiled as fused_hops_*: the restated predicate tells them apart), 8,193 -> K generic hop_norm
    launches although the segment hint is set.  With 1.5 x seg stored edges per graph, 1,997 stages its adjacency in LDS and
    8,192 walks unstaged (its edges exceed the neighbour list left after the tile); the staged kernel at 8,192 rows is
    test_big_graph_hops_lds_staging's."""
    K, B = 3, 2
    ei = _graphs(seg, B, (3 * seg) // 2, seg)
    kind = R.hop_kernel(seg, seg * B, K)
    assert kind == ("fused" if seg <= 1996 else "big" if seg <= 8192 else "generic")
    if kind == "big":
        assert R.big_hops_staged(seg, seg * B, ei.shape[1], ei.shape[1] // B) == (seg == 1997)
    launches = _tag_case(16, 16, K, ei, seg * B, seg, f"TAGConv hops, seg {seg} ({kind})", seed=seg)
    if kind == "generic":
        _check_classes(launches, {"hop_norm"}, {"fused_hops_fwd", "fused_hops_bwd"}, f"seg {seg}")
    else:
        _check_classes(launches, {"fused_hops_fwd", "fused_hops_bwd"}, {"hop_norm"}, f"seg {seg}")


def _staging_graph(kind):
    """(seg, one graph's edge list with both directions stored, staged?) of test_big_graph_hops_lds_staging."""
    gen = np.random.default_rng({"cap-in": 1, "cap-out": 2, "rows-8192": 3, "hubs": 4}[kind])
    if kind in ("cap-in", "cap-out"):
        # the neighbour list at its LDS limit: ne + 4 == nb_cap (staged) and one edge more (unstaged)
        seg = 2000
        cap = R.big_hops_nb_cap(seg, 2 * seg, 1 << 40)           # (the LDS bound: the equal share asks for more)
        ne = cap - 4 + (kind == "cap-out")
        ring = np.stack([np.arange(seg), (np.arange(seg) + 1) % seg])
        und = np.concatenate([ring, gen.integers(0, seg, size=(2, ne // 2 - seg))], axis=1)
        ei = torch.from_numpy(np.concatenate([und, und[::-1]], axis=1))
        if ne % 2:
            ei = torch.cat([ei, torch.tensor([[7], [7]])], dim=1)    # (a self loop: its own reverse)
        return seg, ei, kind == "cap-in"
    if kind == "rows-8192":
        # BH_RPT * BH_THREADS rows, staged: sparser than a spanning tree (isolated rows keep degree 0), edges on the last rows too
        seg = R.BH_RPT * R.BH_THREADS
        src = gen.integers(0, seg, size=3490)
        dst = gen.integers(0, seg, size=3490)
        src = np.concatenate([src, np.arange(seg - 10, seg)])
        dst = np.concatenate([dst, np.arange(seg - 1024 - 10, seg - 1024)])
        und = np.stack([src, dst])
        return seg, torch.from_numpy(np.concatenate([und, und[::-1]], axis=1)), True
    # more than BH_HUB_CAP rows of in-degree > BH_HUB_DEG, one of in-degree > 255, staged
    seg = 2000
    ring = np.stack([np.arange(seg), (np.arange(seg) + 1) % seg])
    hubs = gen.choice(seg, size=R.BH_HUB_CAP + 3, replace=False)
    parts = [ring]
    for i, h in enumerate(hubs):
        nb = gen.choice(np.setdiff1d(np.arange(seg), [h]), size=300 if i == 0 else 40, replace=False)
        parts.append(np.stack([nb, np.full(nb.shape[0], h)]))
    und = np.concatenate(parts, axis=1)
    return seg, torch.from_numpy(np.concatenate([und, und[::-1]], axis=1)), True


@pytest.mark.parametrize("kind", ["cap-in", "cap-out", "rows-8192", "hubs"])
def test_big_graph_hops_lds_staging(kind):
    """big_graph_hops_kernel stages a graph's adjacency in LDS when `ne + 4 <= nb_cap && ne < 65536` (edge.hip; nb_cap from
    launch_big_graph_hops' LDS share, restated in tests/regimes.py), else it walks unstaged (bh_unstaged_graph).  Both are
    profiled as fused_hops_*, so the restated predicate decides the side:
    - cap-in / cap-out: 2,000-node graphs with nb_cap - 4 and nb_cap - 3 edges, the last staged edge count and the first unstaged
      one.  (`ne < 65536` never decides: nb_cap <= 62,776 slots wherever big_hops_fit applies, so nb_cap fails first.)
    - rows-8192: 8,192 rows, staged -- the last thread's eighth row (t + 7 * 1024 = 8,191) carries edges;
    - hubs: 131 rows of in-degree > BH_HUB_DEG = 32, more than the BH_HUB_CAP = 128 listed (the rest stay with their owners),
      one of them of in-degree > 255 (the plan's 8-bit degree saturates), staged."""
    seg, one, staged = _staging_graph(kind)
    B, K = 2, 3
    ne = one.shape[1]
    ei = torch.cat([one, one + seg], dim=1)
    assert R.hop_kernel(seg, seg * B, K) == "big"
    assert R.big_hops_staged(seg, seg * B, ei.shape[1], ne) == staged, (kind, ne, R.big_hops_nb_cap(seg, seg * B, ei.shape[1]))
    indeg = torch.bincount(one[1], minlength=seg)
    if kind == "hubs":
        assert int((indeg > R.BH_HUB_DEG).sum()) > R.BH_HUB_CAP and int(indeg.max()) > 255
    if kind == "rows-8192":
        assert int(indeg[7 * R.BH_THREADS:].sum()) > 0 and int(indeg[seg - 1]) > 0
    launches = _tag_case(16, 16, K, ei, seg * B, seg, f"big-graph hops, {kind}: {ne} edges per graph, "
                         f"{'staged' if staged else 'unstaged'}", seed=seg + ne)
    _check_classes(launches, {"fused_hops_fwd", "fused_hops_bwd"}, {"hop_norm"}, kind)


# ------------------------------------------------------------------------------------------ gemm_nt at layer level
def _ring(n):
    i = torch.arange(n)
    return _bidirectional(torch.stack([i, (i + 1) % n]))


def _gemm_case(M, cin, cout, K, want_kind=None):
    plan = R.gemm_nt_plan(M, cin, cout, K + 1, _cus())
    what = f"TAGConv({cin}, {cout}, K={K}) at M = {M}: gemm_nt {plan['kind']}, {plan['pieces']} pieces, CT {plan['CT']}"
    if want_kind is not None:
        assert plan["kind"] == want_kind, (what, want_kind)
    launches = _tag_case(cin, cout, K, _ring(M), M, 0, what, seed=M + cin + cout)
    assert launches.get("gemm_nt", 0) > 0, launches
    return plan


def test_gemm_nt_tiny_kernel_row_tile_bound():
    """gemm_nt_tiny_kernel (gemm_nt.hip): ceil(M / 32) <= 256 row tiles, 129-wide output, 129-k terms, <= 8 pieces.  M = 8,192
    (256 tiles, tiny), 8,193 (one row past: stationary), 8,224 (a whole extra tile).  gemm_nt covers both kernels: the restated
    predicate decides the side."""
    tiles = R.TINY_MAX_TILES
    for M, kind in ((32 * tiles, "tiny"), (32 * tiles + 1, "stationary"), (32 * tiles + 32, "stationary")):
        _gemm_case(M, 129, 129, 3, kind)


def test_gemm_nt_weight_streaming_round_bounds():
    """gemm_nt_ws_kernel (>= 5 terms of 129, ceil(M / 32) >= 2 rounds of CUs x 8 row tiles) over whole rounds, the stationary
    kernel on the rest.  M one row below two rounds (stationary), 1 row into the last tile (streaming, a partial last tile),
    exactly two rounds, two rounds + 1 row (a one-row stationary tail) and 3 rounds + 33 rows."""
    per_round_rows = _cus() * R.NT_WAVES * 32
    r2 = R.WS_MIN_ROUNDS * per_round_rows
    for M, kind in ((r2 - 32, "stationary"), (r2 - 31, "ws"), (r2, "ws"), (r2 + 1, "ws+stationary"), (3 * per_round_rows + 33, "ws+stationary")):
        _gemm_case(M, 129, 129, 4, kind)


def test_gemm_nt_two_quarter_wave_tile_bound():
    """CT = 2 (two 32-column quarters per wave) from nrt * nslices * (tps / 2) >= 2 * CUs * NT_WAVES row tiles: a 2-term 129-wide
    product one row tile below and at that count."""
    cus = _cus()
    nrt = 2 * cus * R.NT_WAVES // 2                 # 2 terms: tps 4, one slice
    for M, ct in ((32 * (nrt - 1), 1), (32 * (nrt - 1) + 1, 2)):
        plan = _gemm_case(M, 129, 129, 1, "stationary")
        assert plan["CT"] == ct, plan


@pytest.mark.parametrize("cin,cout,K,kind", [(512, 512, 3, "wide"), (512, 512, 7, "multi"), (300, 129, 7, "multi")])
def test_gemm_nt_wide_and_multi_launch(cin, cout, K, kind):
    """The wide weight-streaming kernel (cout a multiple of 128 >= 256, <= NT_MAX_PIECES = 16 pieces: TAGConv(512, 512, 3) has
    exactly 16) and the accumulating multi-launch path (32 and 24 pieces)."""
    _gemm_case(1000, cin, cout, K, kind)


WIDTHS = [1, 4, 5, 31, 32, 33, 128, 129, 132, 136, 137, 260]


@pytest.mark.parametrize("side", ["cin", "cout"])
def test_gemm_nt_odd_widths_at_the_tiny_bound(side):
    """Widths around the column plan (trailing VALU columns, 32-column quarters, 136-k pieces) for cin and for cout, at M = 8,192
    and 8,193 -- the last row count of the tiny kernel's 129 x 129 admission and the first past it."""
    M0 = 32 * R.TINY_MAX_TILES
    for w in WIDTHS:
        for M in (M0, M0 + 1):
            cin, cout = (w, 129) if side == "cin" else (129, w)
            _gemm_case(M, cin, cout, 1)
