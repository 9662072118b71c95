"""NaN and Inf go through every ReLU and gate of the HIP path as they do through the reference.

The rule (csrc/device_prims.hpp relu_on / relu1 / relu4 / gate1 / clamp_lo): a unit is off iff its pre-activation compares <= 0, a
NaN is ON -- torch.relu and threshold_backward.  One entry of x or of edge_attr is replaced by NaN, +Inf or -Inf in a MIDDLE graph
of a batch of rings, and the HIP model is compared with oracle/ref_cpu.py on the same batch: the same entries are non-finite (NaN
against Inf is not distinguished), the finite ones agree to tests.util.RTOL, the loss is finite iff the oracle's is, and the other
graphs of the batch carry the BITS of the same batch without the poison.  One case per kernel route, the route confirmed from
the profile classes against tests/regimes.py as tests/test_gpu_boundaries.py does; then layers, loss kernels and the guarded
optimizer step the whole contract exists for.  tests/test_nonfinite_host.py pins what the oracle itself does.

What these tests see: with the ReLUs written fmaxf(v, 0) and the gates v > 0 (as they were), layer 0's edge stage turns a NaN
pre-activation P[i] + Q[src] + a_e We into "off, value 0", every output row is finite, and each NaN case fails at its first
comparison (`out`: all non-finite entries of the reference dropped).  fmaxf keeps +Inf, so the Inf cases would go non-finite on
that code too; they hold the rest of the rule (-Inf is off, Inf - Inf and 0 * Inf arise where the reference's do)."""
import copy
import math

import pytest
import torch

from oracle import ref_cpu
from poweflownet_amd.networks.MPN import EdgeAggregation, GraphCSR, TAGConv
from tests import regimes as R
from tests.nonfinite import VALUES, assert_covers_nonfinite, assert_same_nonfinite, nonfinite_rows, poison, ring_batch
from tests.test_gpu_boundaries import _check_classes, _cus, _graphs, _models, _profiled, _ring
from tests.util import RTOL, _cpu_gates, _to64, record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------ one model-level case
def _hip_step(m, dd, train, want_gea=False, gates=True):
    """Forward (+ MSELoss backward) of the HIP model: out, loss, grad x, grad edge_attr (when asked), the parameter gradients, the
    profile classes of forward + backward and (after them, outside the profile) the exported gates, all on the host."""
    if not train:
        with torch.no_grad():
            out, launches = _profiled(lambda: m(dd))
        return {"out": out.cpu(), "launches": launches}
    m.zero_grad(set_to_none=True)
    dd = dd.clone()
    dd.x.requires_grad_(True)
    dd.edge_attr.requires_grad_(want_gea)

    def step():
        out = m(dd)
        loss = torch.nn.MSELoss()(out, dd.y)
        loss.backward()
        return out, loss
    (out, loss), launches = _profiled(step)
    return {"out": out.detach().cpu(), "loss": loss.detach().cpu(), "gx": dd.x.grad.cpu(), "gates": _cpu_gates(m) if gates else None,
            "gea": dd.edge_attr.grad.cpu() if want_gea else None, "launches": launches,
            "grads": {k: p.grad.cpu().clone() for k, p in m.named_parameters()}}


def _oracle_on_gates(ref, data, gates):
    """The float64 oracle held to the HIP forward's ReLU decisions (tests.util._assert_grads_on_hip_gates's method): out, loss,
    grad x, grad edge_attr, parameter gradients."""
    ref64 = copy.deepcopy(ref).double()
    ref64.zero_grad(set_to_none=True)
    ref64.gates = gates
    d64 = _to64(data)
    d64.x.requires_grad_(True)
    d64.edge_attr.requires_grad_(True)
    out = ref64(d64)
    loss = torch.nn.MSELoss()(out, d64.y)
    loss.backward()
    return {"out": out.detach(), "loss": loss.detach(), "gx": d64.x.grad, "gea": d64.edge_attr.grad,
            "grads": {k: p.grad for k, p in ref64.named_parameters()}}


def _nf_case(data, seg, H, L_, K, where, row, value, what, train=True, mode="eval", want_gea=True, seed=0, route=True):
    """One poisoned batch through the HIP model and the oracle; returns (model regime, profile classes, HIP results)."""
    ref, m = _models(H, L_, K, 0.0, seed)
    ref.train(mode == "train")
    m.train(mode == "train")
    n = data.x.shape[0]
    g_bad = row // seg if where == "x" else row // (data.edge_index.shape[1] // (n // seg))
    others = torch.ones(n, dtype=torch.bool)
    others[g_bad * seg:(g_bad + 1) * seg] = False
    bad = poison(data, where, row, VALUES[value])
    clean = _hip_step(m, data.to(DEV), train, gates=False)
    got = _hip_step(m, bad.to(DEV), train)
    launches = got["launches"]
    assert m._graphs._graph.seg_nodes == seg, (what, m._graphs._graph.seg_nodes)
    reg = R.model_regime(n, seg, H, L_, K, 2, train, _cus())
    if route:
        _check_classes(launches, reg["must"], reg["must_not"], what)
    with torch.no_grad():
        out_ref = ref(bad)
    assert len(nonfinite_rows(out_ref)) > 0 and bool(torch.isfinite(out_ref[others]).all()), what
    # (the oracle on its OWN decisions: the gated float64 run below follows the HIP gates, so a gate that is wrongly off would go
    #  unnoticed there -- this comparison is the one that catches a dropped NaN, in every case)
    assert_same_nonfinite(got["out"], out_ref, f"{what}: out vs fp32 oracle", RTOL)
    assert torch.equal(got["out"][others], clean["out"][others]), f"{what}: the other graphs' out rows changed bits"
    if not train:
        return reg, launches, got
    want = _oracle_on_gates(ref, bad, got["gates"])
    assert_same_nonfinite(got["out"], want["out"].float(), f"{what}: out vs fp64 oracle on the HIP gates", RTOL)
    assert bool(torch.isfinite(got["loss"])) == bool(torch.isfinite(want["loss"])), (what, got["loss"], want["loss"])
    assert not bool(torch.isfinite(want["loss"])), what
    assert_same_nonfinite(got["gx"], want["gx"].float(), f"{what}: grad x", RTOL)
    assert torch.equal(got["gx"][others], clean["gx"][others]), f"{what}: the other graphs' grad x rows changed bits"
    for k, g in got["grads"].items():
        assert_covers_nonfinite(g, want["grads"][k].float(), f"{what}: grad.{k}", RTOL)
    if want_gea:
        # (asking for grad edge_attr takes the generic backward walks: a run of its own, not the one whose route was checked)
        again = _hip_step(m, bad.to(DEV), True, want_gea=True, gates=False)
        assert_same_nonfinite(again["gea"], want["gea"].float(), f"{what}: grad edge_attr", RTOL)
        assert_same_nonfinite(again["gx"], want["gx"].float(), f"{what}: grad x (with grad edge_attr)", RTOL)
    return reg, launches, got


def _mid(seg, B):
    """The poisoned entry: a node in the middle of the middle graph, or that graph's stored edge leaving it (rings: one stored edge
    per node, so the edge id is the node id)."""
    return (B // 2) * seg + seg // 2


# ------------------------------------------------------------------------------------------ routes
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("where", ["x", "edge_attr"])
def test_graph_resident_route(where, value, mode):
    """front_seg_fwd, ea_seg_*, seg_lin_hops_*: rings of 43 nodes, 7 graphs (two per workgroup: the last one partial),
    (H, L, K) = (129, 4, 3).  Radius 1 + 3 * (3 + 1) = 13: 27 of the middle graph's 43 rows are poisoned, 16 are not."""
    seg, B = 43, 7
    row = _mid(seg, B)
    reg, launches, got = _nf_case(ring_batch(seg, B, 1), seg, 129, 4, 3, where, row, value,
                                  f"graph-resident, {where} {value}, {mode}()", mode=mode)
    assert reg["seg_front"] and reg["ea_seg_fwd"] and reg["ea_seg_bwd"] and reg["slh"], reg
    assert launches.get("seg_lin_hops_fwd", 0) > 0 and launches.get("seg_lin_hops_bwd", 0) > 0, launches
    lo = row - 13 + (1 if where == "edge_attr" else 0)            # (the edge row -> row + 1 reaches rows row - 12 .. row + 13)
    assert nonfinite_rows(got["out"]) == list(range(lo, row + 14))


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("where", ["x", "edge_attr"])
def test_graph_resident_route_one_column_quarter(where, value):
    """The same at H = 32 (ny = 1: no seg_lin_hops, the two-tile hop kernel and gemm_nt between the graph-resident layers)."""
    seg, B = 43, 7
    reg, _, _ = _nf_case(ring_batch(seg, B, 2), seg, 32, 4, 3, where, _mid(seg, B), value, f"graph-resident ny = 1, {where} {value}")
    assert reg["seg_front"] and reg["ea_seg_fwd"] and reg["ea_seg_bwd"] and reg["ny"] == 1 and not reg["slh"], reg


@pytest.mark.parametrize("loss_name,attach", [("mse", False), ("mse", True), ("masked_l2", True)])
def test_graph_resident_route_with_the_loss_tails(loss_name, attach):
    """The project's own MSELoss with and without `attach`, Masked_L2_loss with `attach` (the backward's first launch forms out,
    loss and grad_out), on the first case with a NaN in x: out, loss and every gradient against the three-call torch path of
    _nf_case's HIP run -- non-finite where that is, the same bits elsewhere."""
    from poweflownet_amd.loss import MSELoss
    from poweflownet_amd.utils.custom_loss_functions import Masked_L2_loss
    from tests.util import _run, _run_masked
    seg, B = 43, 7
    data = poison(ring_batch(seg, B, 1), "x", _mid(seg, B), VALUES["nan"])
    ref, m = _models(129, 4, 3, 0.0, 0)
    m.train()
    dd = data.to(DEV)
    loss_fn, runner = (MSELoss(), _run) if loss_name == "mse" else (Masked_L2_loss(), _run_masked)
    plain = runner(m, dd, loss_fn, False)
    got = runner(m, dd, loss_fn, attach)
    tail = "ea_seg_bwd+out+mse" if loss_name == "mse" else "ea_seg_bwd+out+masked_l2"
    assert (got["launches"].get(tail, 0) == 1) == attach, got["launches"]
    with torch.no_grad():
        out_ref = ref(data)
    assert_same_nonfinite(got["out"], out_ref, f"{loss_name} attach {attach}: out", RTOL)
    assert not bool(torch.isfinite(got["loss"])) and not bool(torch.isfinite(plain["loss"]))
    fin = torch.isfinite(plain["g"])
    assert torch.equal(torch.isfinite(got["g"]), fin) and torch.equal(got["g"][fin], plain["g"][fin])
    assert int((~fin).sum()) > 0.9 * fin.numel(), int((~fin).sum())


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("where", ["x", "edge_attr"])
def test_generic_edge_walks_with_saved_masks(where, value):
    """Rings of 129 nodes (one past the graph-resident kernels): the generic edge walks, which save their ReLU masks in training,
    the fused front, the two-tile hops and gemm_nt's tiny kernel."""
    seg, B = 129, 3
    reg, launches, _ = _nf_case(ring_batch(seg, B, 3), seg, 129, 2, 3, where, _mid(seg, B), value, f"generic walks, {where} {value}")
    assert not reg["ea_seg_fwd"] and launches.get("edge_fwd", 0) > 0 and launches.get("edge_bwd", 0) > 0, launches
    assert R.ea_saves_mask(True, seg * B, 2, R.ld_of(129), seg, True, 1, _cus())
    assert R.gemm_nt_plan(seg * B, 129, 129, 4, _cus())["kind"] == "tiny" and launches.get("gemm_nt", 0) > 0


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("where", ["x", "edge_attr"])
def test_block_front(where, value):
    """H = 257: the block front (front_row_per_wave refuses 65 chunks), no graph-resident layer."""
    seg, B = 43, 3
    reg, _, _ = _nf_case(ring_batch(seg, B, 4), seg, 257, 2, 2, where, _mid(seg, B), value, f"block front, {where} {value}")
    assert not reg["front_latency"] and not reg["ea_seg_fwd"], reg


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("extra", [0, 1])
def test_row_per_wave_front_and_layer_0_on_the_fly_in_inference(extra, value):
    """16-node rings, inference: 32,768 rows (front_seg_fwd) and one graph more (the block front, layer 0's P | Q formed on the fly
    in the edge walk)."""
    seg = 16
    B = R.WAVE_MAX_ROWS // seg + extra
    data = ring_batch(seg, B, 5)
    for where in ("x", "edge_attr"):
        reg, _, _ = _nf_case(data, seg, 32, 2, 2, where, _mid(seg, B), value,
                             f"{seg * B} rows inference, {where} {value}", train=False)
        assert reg["seg_front"] == (extra == 0) and reg["l0_fly"] == (extra == 1), reg


@pytest.mark.parametrize("value", list(VALUES))
def test_gemm_nt_stationary(value):
    """8,193 rows (three rings of 2,731): one row past gemm_nt's tiny kernel -- the stationary kernel's ReLU epilogue and gate; the
    graphs are too large for the two-tile hops (big_graph_hops_kernel)."""
    seg, B = 2731, 3
    assert R.gemm_nt_plan(seg * B, 129, 129, 4, _cus())["kind"] == "stationary"
    _, launches, _ = _nf_case(ring_batch(seg, B, 6), seg, 129, 2, 3, "x", _mid(seg, B), value, f"gemm_nt stationary, x {value}", want_gea=False)
    assert launches.get("gemm_nt", 0) > 0, launches


@pytest.mark.parametrize("value", list(VALUES))
def test_gemm_nt_weight_streaming(value):
    """Five terms of 129 (K = 4): the smallest three-ring batch R.gemm_nt_plan reports as weight-streaming, in training, so the
    streaming kernel's ReLU epilogue and the backward's gate both run.  At this row count the restated plan also gives the ONE-term
    129-wide products of the EdgeAggregation layers (P | Q, S W2^T, dS) two quarters per wave (CT = 2), which is where launch_gemm_nt
    takes the interleaved flush (clamp_lo against 0 and against -inf) -- asserted as far as tests/regimes.py restates it; the flush's
    remaining clauses (the kernel variant, whole quarters, no group flags) are NOT restated and the profile class cannot show the
    flush, so that path is exercised here by supposition, not by confirmation."""
    cus, B = _cus(), 3
    seg = R.first_graph_count(lambda s: R.gemm_nt_plan(B * s, 129, 129, 5, cus)["kind"].startswith("ws"))
    plan = R.gemm_nt_plan(B * seg, 129, 129, 5, cus)
    record(f"weight streaming at {B} x {seg} rows: {plan}", 0.0, 1.0, None)
    assert R.gemm_nt_plan(B * seg, 129, 129, 1, cus)["CT"] == 2
    _, launches, _ = _nf_case(ring_batch(seg, B, 7), seg, 129, 2, 4, "x", _mid(seg, B), value, f"gemm_nt {plan['kind']}, x {value}",
                              want_gea=False)
    assert launches.get("gemm_nt", 0) > 0, launches


@pytest.mark.parametrize("value", list(VALUES))
def test_gemm_nt_wide_model(value):
    """H = 512: the wide weight-streaming kernel (16 pieces at K = 3) inside a model."""
    seg, B = 43, 3
    assert R.gemm_nt_plan(seg * B, 512, 512, 4, _cus())["kind"] == "wide"
    _, launches, _ = _nf_case(ring_batch(seg, B, 8), seg, 512, 2, 3, "x", _mid(seg, B), value, f"gemm_nt wide, H 512, x {value}", want_gea=False)
    assert launches.get("gemm_nt", 0) > 0, launches


@pytest.mark.parametrize("value", list(VALUES))
def test_edge_rows_and_row_hops_inference(value):
    """14-node rings at H = 32, inference, at the first graph count that admits the edge-rows kernel and at the first that admits
    row_hops_kernel."""
    cus, seg, H = _cus(), 14, 32
    ld = R.ld_of(H)
    b_er = R.first_graph_count(lambda b: R.edge_rows_ok(seg, seg * b, ld, cus))
    b_rh = R.first_graph_count(lambda b: R.row_hops_ok(seg, seg * b, ld, cus))
    for B in sorted({b_er, b_rh}):
        data = ring_batch(seg, B, 9)
        for where in ("x", "edge_attr"):
            reg, launches, _ = _nf_case(data, seg, H, 2, 2, where, _mid(seg, B), value,
                                        f"{seg}-node x {B} inference, {where} {value}", train=False)
            assert reg["edge_rows"] == (B >= b_er) and reg["row_hops"] == (B >= b_rh), reg
            assert (launches.get("edge_rows_fwd", 0) > 0) == (B >= b_er), launches


# ------------------------------------------------------------------------------------------ layers
@pytest.mark.parametrize("where", ["x", "edge_attr"])
def test_edge_aggregation_layer(where):
    """EdgeAggregation(7, 3, 65, 5) on 300 nodes (test_edge_aggregation_odd_shapes_vs_oracle's odd shape), forward and backward,
    with one NaN: every tensor non-finite exactly where the oracle layer's is."""
    fi, fe, h, fo, nodes = 7, 3, 65, 5, 300
    torch.manual_seed(fi * 1000 + h)
    ref = ref_cpu.EdgeAggregation(fi, fe, h, fo)
    ours = EdgeAggregation(fi, fe, h, fo)
    ours.load_state_dict(ref.state_dict())
    ours = ours.to(DEV)
    e = 3 * nodes
    ei = torch.randint(0, nodes, (2, e))
    x, ea, g = torch.randn(nodes, fi), torch.randn(e, fe), torch.randn(nodes, fo)
    (x if where == "x" else ea)[17, 1] = float("nan")

    def run(mod, x, ei, ea, g):
        x = x.clone().requires_grad_(True)
        ea = ea.clone().requires_grad_(True)
        y = mod(x, ei, ea)
        y.backward(g)
        return [y.detach(), x.grad, ea.grad] + [p.grad for p in mod.parameters()]

    want = run(ref.double(), x.double(), ei, ea.double(), g.double())
    got = run(ours, x.to(DEV), ei.to(DEV), ea.to(DEV), g.to(DEV))
    names = ["out", "grad x", "grad edge_attr"] + [f"grad.{k}" for k, _ in ref.named_parameters()]
    assert len(nonfinite_rows(want[0])) > 0
    for name, a, b in zip(names, got, want):
        assert_same_nonfinite(a, b.float(), f"EdgeAggregation, NaN in {where}: {name}", RTOL)


@pytest.mark.parametrize("seg", [1996, 1997, 8193])
def test_tagconv_hops_carry_a_nan(seg):
    """The hop kernels have no ReLU, but a sel4, a padded slot or a skipped zero could drop a NaN: TAGConv(8, 8, K = 3) over two
    graphs with a segment hint at 1,996 nodes (two-tile hops), 1,997 (big-graph hops, staged) and 8,193 (generic hop_norm), a NaN
    in x (forward) and one in the incoming gradient (backward), against the float64 oracle layer."""
    K, B, c = 3, 2, 8
    ei = _graphs(seg, B, (3 * seg) // 2, seg)
    n = seg * B
    kind = R.hop_kernel(seg, n, K)
    assert kind == ("fused" if seg <= 1996 else "big" if seg <= 8192 else "generic")
    torch.manual_seed(seg)
    ref = ref_cpu.TAGConv(c, c, K=K)
    layer = TAGConv(c, c, K=K)
    layer.load_state_dict(ref.state_dict())
    layer = layer.to(DEV)
    x, g = torch.randn(n, c), torch.randn(n, c)
    x[seg + seg // 2, 1] = float("nan")
    g[seg // 3, 2] = float("nan")
    graph = GraphCSR(ei.to(DEV), n, mode=0, seg_hint=seg)
    assert graph.seg_nodes == seg
    xd = x.to(DEV).requires_grad_(True)

    def step():
        out = layer.on_graph(graph, xd)
        out.backward(g.to(DEV))
        return out
    out, launches = _profiled(step)
    if kind == "generic":
        _check_classes(launches, {"hop_norm"}, {"fused_hops_fwd", "fused_hops_bwd"}, f"seg {seg}")
    else:
        _check_classes(launches, {"fused_hops_fwd", "fused_hops_bwd"}, {"hop_norm"}, f"seg {seg}")
    ref64 = ref.double()
    x64 = x.double().requires_grad_(True)
    out64 = ref64(x64, ei)
    out64.backward(g.double())
    what = f"TAGConv hops ({kind}), seg {seg}"
    assert 1 < len(nonfinite_rows(out64)) < seg and 1 < len(nonfinite_rows(x64.grad)) < seg
    assert_same_nonfinite(out, out64.float(), f"{what}: out", RTOL)
    assert_same_nonfinite(xd.grad, x64.grad.float(), f"{what}: grad x", RTOL)
    for k in range(K + 1):
        assert_covers_nonfinite(layer.lins[k].weight.grad, ref64.lins[k].weight.grad.float(), f"{what}: grad lins.{k}.weight", RTOL)


def test_gemm_nt_wide_layer():
    """TAGConv(512, 512, 3) at M = 1,000 (gemm_nt's wide kernel) under a ReLU, a NaN in one input entry."""
    M, c, K = 1000, 512, 3
    assert R.gemm_nt_plan(M, c, c, K + 1, _cus())["kind"] == "wide"
    torch.manual_seed(M)
    ref = ref_cpu.TAGConv(c, c, K=K)
    layer = TAGConv(c, c, K=K)
    layer.load_state_dict(ref.state_dict())
    layer = layer.to(DEV)
    ei = _ring(M)
    x, g = torch.randn(M, c), torch.randn(M, c)
    x[500, 3] = float("nan")
    graph = GraphCSR(ei.to(DEV), M, mode=0, seg_hint=0)
    xd = x.to(DEV).requires_grad_(True)
    out = torch.relu(layer.on_graph(graph, xd))
    out.backward(g.to(DEV))
    x64 = x.double().requires_grad_(True)
    out64 = torch.relu(ref.double()(x64, ei))
    out64.backward(g.double())
    assert nonfinite_rows(out64) == list(range(497, 504))
    assert_same_nonfinite(out, out64.float(), "wide TAGConv under a ReLU: out", RTOL)
    assert_same_nonfinite(xd.grad, x64.grad.float(), "wide TAGConv under a ReLU: grad x", RTOL)


# ------------------------------------------------------------------------------------------ loss kernels
def _loss_case(n, seed):
    g = torch.Generator().manual_seed(seed)
    out, y = torch.randn(n, 4, generator=g), torch.randn(n, 4, generator=g)
    mask = torch.randint(0, 2, (n, 4), generator=g)
    mask[5], mask[6] = torch.tensor([1, 0, 1, 0]), torch.tensor([0, 1, 0, 1])
    valid = torch.ones(n, dtype=torch.int32)
    valid[2::4] = 0                                     # rows 2, 6, 10, ...: invalid (row 5 counts)
    return out, y, mask, valid


def _hip_loss(fn, out, *rest, **kw):
    o = out.to(DEV).requires_grad_(True)
    loss = fn(o, *[r.to(DEV) for r in rest], **{k: v.to(DEV) for k, v in kw.items()})
    loss.backward()
    return loss.detach().cpu(), o.grad.cpu()


@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("n", [7, 1062])
def test_mse_loss_kernels_and_a_nan(n, rows):
    """pfn_mse_loss / pfn_mse_loss_rows: a NaN under a counted entry gives a NaN loss and a NaN at THAT gradient entry only (the
    others are the clean call's, bit for bit: 2 (o - y) / count); in an invalid row of a `_rows` call it changes nothing."""
    from poweflownet_amd.loss import MSELoss
    out, y, _, valid = _loss_case(n, 11)
    kw = {"valid": valid} if rows else {}
    l0, g0 = _hip_loss(MSELoss(), out, y, **kw)
    d = (out.double() - y.double())[valid.bool()] if rows else out.double() - y.double()
    assert abs(l0.item() - (d * d).mean().item()) <= 1e-6 * (d * d).mean().item()
    bad = out.clone()
    bad[5, 2] = float("nan")
    l1, g1 = _hip_loss(MSELoss(), bad, y, **kw)
    keep = torch.ones(n, 4, dtype=torch.bool)
    keep[5, 2] = False
    assert torch.isnan(l1) and torch.isnan(g1[5, 2]) and torch.equal(g1[keep], g0[keep])
    if rows:
        assert valid[6] == 0 and valid[5] == 1
        bad = out.clone()
        bad[6, 1] = float("nan")
        l2, g2 = _hip_loss(MSELoss(), bad, y, **kw)
        assert torch.equal(l2, l0) and torch.equal(g2, g0)


@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("regularize", [False, True])
def test_masked_l2_loss_kernels_and_a_nan(regularize, rows):
    """pfn_masked_l2_loss / pfn_masked_l2_loss_rows against ref_cpu.masked_l2_loss in float64: a NaN under a selected entry gives a
    NaN loss and a NaN at that gradient entry only; with regularize=False a NaN under an UNSELECTED entry leaves the loss and every
    gradient entry equal to the clean call's (masked_select semantics; with the regulariser it is selected by the second set); in
    an invalid row of a `_rows` call it changes nothing."""
    from poweflownet_amd.utils.custom_loss_functions import Masked_L2_loss
    n = 1062
    out, y, mask, valid = _loss_case(n, 12)
    kw = {"valid": valid} if rows else {}
    fn = Masked_L2_loss(regularize=regularize, regcoeff=0.5)
    l0, g0 = _hip_loss(fn, out, y, mask, **kw)
    k = valid.bool() if rows else torch.ones(n, dtype=torch.bool)
    o64 = out.double().requires_grad_(True)
    l64 = ref_cpu.masked_l2_loss(o64[k], y.double()[k], mask[k], regularize, 0.5)
    l64.backward()
    assert abs(l0.item() - l64.item()) <= 1e-6 * l64.item()
    assert float((g0.double() - o64.grad).abs().max()) <= 1e-6 * float(o64.grad.abs().max())
    assert mask[5, 0] == 1 and mask[5, 1] == 0 and valid[5] == 1
    sel, unsel = out.clone(), out.clone()
    sel[5, 0] = float("nan")
    unsel[5, 1] = float("nan")
    l1, g1 = _hip_loss(fn, sel, y, mask, **kw)
    keep = torch.ones(n, 4, dtype=torch.bool)
    keep[5, 0] = False
    assert torch.isnan(l1) and torch.isnan(g1[5, 0]) and torch.equal(g1[keep], g0[keep])
    l2, g2 = _hip_loss(fn, unsel, y, mask, **kw)
    if regularize:
        keep = torch.ones(n, 4, dtype=torch.bool)
        keep[5, 1] = False
        assert torch.isnan(l2) and torch.isnan(g2[5, 1]) and torch.equal(g2[keep], g0[keep])
    else:
        assert torch.equal(l2, l0) and torch.equal(g2, g0)
    if rows:
        assert valid[6] == 0
        inv = out.clone()
        inv[6] = float("nan")
        l3, g3 = _hip_loss(fn, inv, y, mask, **kw)
        assert torch.equal(l3, l0) and torch.equal(g3, g0)


def test_power_imbalance_and_a_nan():
    """pfn_power_imbalance on three rings of 40: a NaN in one node's x gives a NaN loss and NaN gradient rows at that node, its two
    neighbours (whose imbalance reads it) and THEIR neighbours (whose gradient reads that imbalance), as the float64 oracle does; the rest of the gradient keeps the clean call's bits."""
    from poweflownet_amd.utils.custom_loss_functions import PowerImbalance
    from tests.test_gpu_step_kernels import PI_STATS
    d = ring_batch(40, 3, 13)
    ea = d.edge_attr.clamp(-3, 3)
    loss_fn = PowerImbalance(*PI_STATS)

    def run(x):
        xd = x.to(DEV).requires_grad_(True)
        loss = loss_fn(xd, d.edge_index.to(DEV), ea.to(DEV))
        loss.backward(PowerImbalance.unit_grad(loss))
        return loss.detach().cpu(), xd.grad.cpu()
    l0, g0 = run(d.x)
    bad = d.x.clone()
    bad[50, 0] = float("nan")
    l1, g1 = run(bad)
    x64 = bad.double().requires_grad_(True)
    l64 = ref_cpu.power_imbalance(x64, d.edge_index, ea.double(), *PI_STATS)
    l64.backward()
    assert torch.isnan(l1) and torch.isnan(l64) and torch.isfinite(l0)
    assert nonfinite_rows(x64.grad) == [48, 49, 50, 51, 52]
    assert_same_nonfinite(g1, x64.grad.float(), "power imbalance: grad x", RTOL)
    rest = torch.ones(120, dtype=torch.bool)
    rest[48:53] = False
    assert torch.equal(g1[rest], g0[rest])


# ------------------------------------------------------------------------------------------ end to end
def test_guarded_training_epochs_skip_the_batch_with_a_nan_and_go_on_as_if_it_had_not_been_there():
    """What the whole contract is for, through the project's own loop: utils.training.train_epoch (eager steps, the project's
    MSELoss) on a model with per-batch topologies, whose optimizer step is guarded by the step's own loss (_guarded_opt_step ->
    FlatAdamW.guard).  A clean batch, the same batch with ONE NaN in x, another clean batch: the NaN reaches the loss, the update is
    skipped on the device (skipped_steps() == 1; flat_param, both moments and the step counter bit-unchanged), and the third
    batch ends in the bits of a run that never saw the bad one."""
    from poweflownet_amd.loss import MSELoss
    from poweflownet_amd.optim import FlatAdamW
    from poweflownet_amd.utils.training import train_epoch
    seg, B = 43, 7
    first, last = ring_batch(seg, B, 20), ring_batch(seg, B, 21)
    bad = poison(first, "x", _mid(seg, B), VALUES["nan"])
    _, m = _models(129, 4, 3, 0.0, 0)
    m2 = copy.deepcopy(m)
    for mm in (m, m2):
        mm.dynamic_topology = True            # adjacency checks stay on the device: the loop guards the update (_unverified_batch)
    o1, o2 = FlatAdamW(m, lr=1e-2), FlatAdamW(m2, lr=1e-2)
    loss_fn = MSELoss()
    assert math.isfinite(train_epoch(m, [first], loss_fn, o1, DEV))
    before = [t.clone() for t in (o1.flat_param, o1.exp_avg, o1.exp_avg_sq, o1.step_count)]
    assert math.isnan(train_epoch(m, [bad], loss_fn, o1, DEV))
    assert o1.skipped_steps() == 1 and o1.guard is None
    for t, b in zip((o1.flat_param, o1.exp_avg, o1.exp_avg_sq), before):
        assert torch.equal(t, b) and bool(torch.isfinite(t).all())
    assert int(o1.step_count[0]) == int(before[3][0]) == 1
    assert math.isfinite(train_epoch(m, [last], loss_fn, o1, DEV))
    assert math.isfinite(train_epoch(m2, [first, last], loss_fn, o2, DEV))
    assert o2.skipped_steps() == 0 and int(o1.step_count[0]) == int(o2.step_count[0]) == 2
    for a_, b_ in ((o1.flat_param, o2.flat_param), (o1.exp_avg, o2.exp_avg), (o1.exp_avg_sq, o2.exp_avg_sq)):
        assert torch.equal(a_, b_) and bool(torch.isfinite(a_).all())
