"""Parity tests proper (-m gpu): the HIP path, called through the C ABI, against (a) the golden vectors generated
from the reference and (b) the CPU oracle on seeded inputs.  Tolerance: north_star's 1e-5 relative fp32 (tests/util.RTOL)."""
import copy
import os

import pytest
import torch

from oracle import ref_cpu
from poweflownet_amd.networks.MPN import EdgeAggregation, GraphCSR, MaskEmbdMultiMPN, TAGConv
from poweflownet_amd.synth import make_batch
from tests.util import (RTOL, _assert_grads_on_hip_gates, _check_full_size, _cpu_gates, _exported_masks, _fp64_truth, _to64,
                        assert_close, data_from, load, params_from, record, record_elementwise, rel_err)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------ graph
def test_g1_is_directed_and_undirect_on_device():
    fx = load("g1_is_directed")
    m = MaskEmbdMultiMPN(4, 2, 4, 8, 2, 3, 0.0).to(DEV)
    for name in fx["names"]:
        ei, ea = fx[f"{name}.edge_index"].to(DEV), fx[f"{name}.edge_attr"].to(DEV)
        assert m.is_directed(ei) == bool(fx[f"{name}.directed"]), name
        ei2, ea2 = m.undirect_graph(ei, ea)
        assert torch.equal(ei2.cpu(), fx[f"{name}.out_edge_index"]), name
        assert torch.equal(ea2.cpu(), fx[f"{name}.out_edge_attr"]), name


def test_graph_rejects_out_of_range_ids():
    ei = torch.tensor([[0, 1, 7], [1, 2, 0]], device=DEV)
    with pytest.raises(RuntimeError, match="outside"):
        GraphCSR(ei, 5)


def test_scatter_add_matches_index_add_bitwise():
    import ctypes as C
    from poweflownet_amd import _lib as L
    b = make_batch("118", 4)
    ei = b.edge_index.to(DEV)
    n = b.x.shape[0]
    g = GraphCSR(ei, n, mode=1)
    eff = g.export_edges()
    x = torch.randn(n, 132, device=DEV)
    x[:, 129:] = 0
    out = torch.empty_like(x)
    L.check(L.load().pfn_scatter_add(g.ws.data_ptr(), n, ei.shape[1], x.data_ptr(), out.data_ptr(), 129, L.stream_ptr()), "sa")
    # sequential CPU scatter in edge-id order == our per-row edge-id-ordered sums, bit for bit
    want = torch.zeros(n, 132).index_add_(0, eff[1].cpu(), x.cpu()[eff[0].cpu()])
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("n,e", [(1, 0), (1025, 3000), (1_200_000, 1_500_000)])
def test_graph_build_degree_scan_over_many_blocks(n, e):
    """pfn_graph_build's row pointers come from a two-launch scan (per-block totals, then per-block scans; above 2^20 nodes a
    block walks several 1024-row chunks): the exported adjacency, in CSR order, must be the stable by-destination sort of
    the effective edge list, and a scatter-add over it must equal torch's index_add_ bit for bit."""
    import ctypes as C
    from poweflownet_amd import _lib as L
    gen = torch.Generator().manual_seed(n)
    ei = torch.randint(0, n, (2, e), generator=gen)
    g = GraphCSR(ei.to(DEV), n, mode=1)                      # directed: every stored edge also runs backwards
    eff = g.export_edges().cpu()
    want_src = torch.cat([ei[0], ei[1]])
    want_dst = torch.cat([ei[1], ei[0]])
    assert torch.equal(eff[0], want_src) and torch.equal(eff[1], want_dst)
    x = torch.randn(n, 4, device=DEV)
    out = torch.empty_like(x)
    L.check(L.load().pfn_scatter_add(g.ws.data_ptr(), n, e, x.data_ptr(), out.data_ptr(), 4, L.stream_ptr()), "sa")
    want = torch.zeros(n, 4).index_add_(0, want_dst, x.cpu()[want_src])
    assert torch.equal(out.cpu(), want)


# ------------------------------------------------------------------------------------------- single layers
@pytest.mark.parametrize("tag", ["4_8_8", "8_8_4", "129_129_129", "129_129_4"])
def test_g2_edge_aggregation_layer(tag):
    fx = load(f"g2_edge_aggregation_{tag}")
    fi, h, fo = (int(v) for v in tag.split("_"))
    layer = EdgeAggregation(fi, 2, h, fo).to(DEV)
    layer.load_state_dict({"edge_aggr.0.weight": fx["w1"], "edge_aggr.0.bias": fx["b1"],
                           "edge_aggr.2.weight": fx["w2"], "edge_aggr.2.bias": fx["b2"]})
    x = fx["x"].to(DEV).requires_grad_(True)
    ea = fx["edge_attr"].to(DEV).requires_grad_(True)
    out = layer(x, fx["edge_index"].to(DEV), ea)
    assert_close(out, fx["out"], RTOL, "out")
    out.backward(fx["grad_out"].to(DEV))
    assert_close(x.grad, fx["grad_x"], RTOL, "grad_x")
    assert_close(ea.grad, fx["grad_edge_attr"], RTOL, "grad_edge_attr")
    l1, l2 = layer.edge_aggr[0], layer.edge_aggr[2]
    for got, key in ((l1.weight.grad, "grad_w1"), (l1.bias.grad, "grad_b1"), (l2.weight.grad, "grad_w2"), (l2.bias.grad, "grad_b2")):
        assert_close(got, fx[key], RTOL, key)


@pytest.mark.parametrize("tag", ["K1_8_8", "K3_129_129", "K6_129_129", "K3_8_5"])
def test_g3_tagconv_layer(tag):
    fx = load(f"g3_tagconv_{tag}")
    K = int(fx["K"])
    cout, cin = fx["w0"].shape
    layer = TAGConv(cin, cout, K=K).to(DEV)
    sd = {f"lins.{k}.weight": fx[f"w{k}"] for k in range(K + 1)}
    sd["bias"] = fx["bias"]
    layer.load_state_dict(sd)
    x = fx["x"].to(DEV).requires_grad_(True)
    out = layer(x, fx["edge_index"].to(DEV))
    assert_close(out, fx["out"], RTOL, "out")
    out.backward(fx["grad_out"].to(DEV))
    assert_close(x.grad, fx["grad_x"], RTOL, "grad_x")
    assert_close(layer.bias.grad, fx["grad_bias"], RTOL, "grad_bias")
    for k in range(K + 1):
        assert_close(layer.lins[k].weight.grad, fx[f"grad_w{k}"], RTOL, f"grad_w{k}")


@pytest.mark.parametrize("fi,fe,h,fo,nodes", [(7, 3, 65, 5, 300), (64, 2, 64, 64, 257), (33, 1, 193, 130, 1000),
                                              (1, 2, 128, 1, 64), (129, 2, 300, 129, 513)])
def test_edge_aggregation_odd_shapes_vs_oracle(fi, fe, h, fo, nodes):
    """Shapes that exercise every tile / quadrant / remainder path of the GEMMs (64-multiples, 64k+1, >136 k's per
    piece, single columns) against the oracle layer on a random sparse graph."""
    torch.manual_seed(fi * 1000 + h)
    ref = ref_cpu.EdgeAggregation(fi, fe, h, fo)
    ours = EdgeAggregation(fi, fe, h, fo)
    ours.load_state_dict(ref.state_dict())
    ours = ours.to(DEV)
    e = 3 * nodes
    ei = torch.randint(0, nodes, (2, e))
    x, ea, g = torch.randn(nodes, fi), torch.randn(e, fe), torch.randn(nodes, fo)

    def run(mod, x, ei, ea, g):
        x = x.clone().requires_grad_(True)
        ea = ea.clone().requires_grad_(True)
        y = mod(x, ei, ea)
        y.backward(g)
        return [y.detach(), x.grad, ea.grad] + [p.grad for p in mod.parameters()]

    want = run(ref, x, ei, ea, g)
    got = run(ours, x.to(DEV), ei.to(DEV), ea.to(DEV), g.to(DEV))
    for i, (a, b) in enumerate(zip(got, want)):
        assert_close(a, b, RTOL, f"tensor {i}")


@pytest.mark.parametrize("cin,cout,K,nodes", [(33, 70, 2, 500), (64, 128, 1, 129), (193, 65, 3, 400), (5, 1, 4, 77)])
def test_tagconv_odd_shapes_vs_oracle(cin, cout, K, nodes):
    torch.manual_seed(cin * 100 + cout)
    ref = ref_cpu.TAGConv(cin, cout, K)
    with torch.no_grad():
        ref.bias.normal_(std=0.2)
    ours = TAGConv(cin, cout, K=K)
    ours.load_state_dict(ref.state_dict())
    ours = ours.to(DEV)
    ei = torch.randint(0, nodes, (2, 4 * nodes))
    x, g = torch.randn(nodes, cin), torch.randn(nodes, cout)

    def run(mod, x, ei, g):
        x = x.clone().requires_grad_(True)
        y = mod(x, ei)
        y.backward(g)
        return [y.detach(), x.grad] + [p.grad for p in mod.parameters()]

    want = run(ref, x, ei, g)
    got = run(ours, x.to(DEV), ei.to(DEV), g.to(DEV))
    for i, (a, b) in enumerate(zip(got, want)):
        assert_close(a, b, RTOL, f"tensor {i}")


@pytest.mark.parametrize("cin,cout,nodes", [(8, 5, 77), (129, 129, 300)])
def test_tagconv_without_hops_vs_oracle(cin, cout, nodes):
    """K = 0: out = x W_0^T + b, no hop of any kind (HOPS_NONE); the backward is tag_backward's K == 0 branch, one GEMM that
    writes grad_x itself.  Forward, grad_x, the weight and the bias gradient against the oracle layer."""
    torch.manual_seed(cin * 100 + cout)
    ref = ref_cpu.TAGConv(cin, cout, 0)
    with torch.no_grad():
        ref.bias.normal_(std=0.2)
    ours = TAGConv(cin, cout, K=0)
    ours.load_state_dict(ref.state_dict())
    ours = ours.to(DEV)
    ei = torch.randint(0, nodes, (2, 4 * nodes))
    x, g = torch.randn(nodes, cin), torch.randn(nodes, cout)

    def run(mod, x, ei, g):
        x = x.clone().requires_grad_(True)
        y = mod(x, ei)
        y.backward(g)
        return [y.detach(), x.grad] + [p.grad for p in mod.parameters()]

    want = run(ref, x, ei, g)
    got = run(ours, x.to(DEV), ei.to(DEV), g.to(DEV))
    assert len(got) == 4 and tuple(got[0].shape) == (nodes, cout)
    for i, (a, b) in enumerate(zip(got, want)):
        assert_close(a, b, RTOL, f"TAGConv({cin}, {cout}, K=0) tensor {i}")


# --------------------------------------------------------------------------------------------- whole model
def _model_from(fx, shared, dropout=0.0):
    params = params_from(load("g4_params_standard")) if shared else params_from(fx)
    cfg = [int(v) for v in fx["cfg"]]
    m = MaskEmbdMultiMPN(*cfg, dropout)
    m.load_state_dict(params)
    return m.to(DEV)


@pytest.mark.parametrize("name,shared", [("g4_model_tiny", False), ("g4_model_case14", True),
                                         ("g4_model_case118", True), ("g4_model_wideK6", False)])
def test_g4_whole_model_forward_and_grads(name, shared):
    fx = load(name)
    m = _model_from(fx, shared).eval()
    data = data_from(fx, device=DEV)
    out = m(data)
    assert out.shape == fx["out"].shape and out.dtype == torch.float32
    assert_close(out, fx["out"], RTOL, "out")
    loss = torch.nn.MSELoss()(out, data.y)
    assert_close(loss, fx["loss"], RTOL, "loss")
    loss.backward()
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        assert_close(p.grad, fx[f"grad.{k}"], RTOL, f"grad.{k}")
    flat = m.flat_grad()
    assert flat is not None and flat.numel() == sum(p.numel() for p in m.parameters())


def test_g6_three_adamw_steps():
    fx = load("g6_train_step")
    g4 = load("g4_model_case14")
    m = _model_from(g4, True).train()                     # dropout_rate 0 -> deterministic
    data = data_from(g4, device=DEV)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    loss_fn = torch.nn.MSELoss()
    for step in range(1, 4):
        opt.zero_grad()
        loss = loss_fn(m(data), data.y)
        loss.backward()
        opt.step()
        assert_close(loss, fx[f"loss.{step}"], RTOL, f"loss.{step}")
    # AdamW's first steps are ~lr*sign(g): entries whose gradient is rounding noise may flip, so compare the
    # well-conditioned entries tightly and bound the rest by 2*lr*steps.
    for k, p in m.named_parameters():
        ref, g = fx[f"param_after3.{k}"], g4[f"grad.{k}"]
        err = (p.detach().cpu() - ref).abs()
        solid = g.abs() > 1e-3 * g.abs().max()
        assert err.max().item() <= 6.5e-3, k
        if solid.any():
            assert err[solid].max().item() <= 2e-5, (k, err[solid].max().item())


def test_g6_flat_adamw_matches_reference_steps():
    """Same fixture, the flat single-kernel AdamW (poweflownet_amd.optim) instead of torch.optim.AdamW."""
    from poweflownet_amd.optim import FlatAdamW
    fx = load("g6_train_step")
    g4 = load("g4_model_case14")
    m = _model_from(g4, True).train()
    data = data_from(g4, device=DEV)
    opt = FlatAdamW(m, lr=1e-3)
    loss_fn = torch.nn.MSELoss()
    for step in range(1, 4):
        opt.zero_grad()
        loss = loss_fn(m(data), data.y)
        loss.backward()
        opt.step()
        assert_close(loss, fx[f"loss.{step}"], RTOL, f"loss.{step}")
    assert opt.step_count.tolist() == [3, 0, 0]
    for k, p in m.named_parameters():
        ref, g = fx[f"param_after3.{k}"], g4[f"grad.{k}"]
        err = (p.detach().cpu() - ref).abs()
        solid = g.abs() > 1e-3 * g.abs().max()
        assert err.max().item() <= 6.5e-3, k
        if solid.any():
            assert err[solid].max().item() <= 2e-5, (k, err[solid].max().item())
    assert sorted(m.state_dict().keys()) == sorted(params_from(load("g4_params_standard")).keys())


def test_fused_mse_loss_matches_torch():
    from poweflownet_amd.loss import MSELoss
    torch.manual_seed(0)
    a = torch.randn(1000, 4, device=DEV, requires_grad=True)
    b = torch.randn(1000, 4, device=DEV)
    l1 = MSELoss()(a, b)
    (3.0 * l1).backward()
    g1 = a.grad.clone()
    a.grad = None
    l2 = torch.nn.MSELoss()(a, b)
    (3.0 * l2).backward()
    assert_close(l1, l2, 1e-6, "loss")
    assert_close(g1, a.grad, 1e-6, "grad")


@pytest.mark.parametrize("rows", [15104, 414080])
def test_fused_mse_loss_handoff_is_never_stale(rows):
    """pfn_mse_loss sums per-block partials in the last-arriving block (write-through partial stores + ticket, no fence);
    300 back-to-back calls on changing data at the benchmark sizes (59 / 256 blocks): a stale partial -- the previous call's
    value -- would show up as a wrong loss."""
    from poweflownet_amd.loss import MSELoss
    torch.manual_seed(1)
    fn = MSELoss()
    y = torch.randn(rows, 4, device=DEV)
    outs = [torch.randn(rows, 4, device=DEV) * (1.0 + 0.37 * i) for i in range(6)]
    want = [((o.double() - y.double()) ** 2).mean().item() for o in outs]
    got = []
    for it in range(300):
        got.append(fn(outs[it % 6], y))
    torch.cuda.synchronize()
    for it, g in enumerate(got):
        assert abs(g.item() - want[it % 6]) <= 2e-6 * want[it % 6], (it, g.item(), want[it % 6])


def test_g8_masked_l2_loss_matches_reference_goldens():
    """pfn_masked_l2_loss vs outputs of the reference's own Masked_L2_loss (tests/golden/g8_masked_l2.npz), through the
    dispatching class the train loop uses; then against the oracle on a full-size input."""
    from poweflownet_amd.utils.custom_loss_functions import Masked_L2_loss
    fx = load("g8_masked_l2")
    for mname in ("int", "float", "allone", "odd"):
        for reg, coeff in ((True, 1), (True, 0.5), (False, 1)):
            o = fx["out"].to(DEV).requires_grad_(True)
            loss = Masked_L2_loss(regularize=reg, regcoeff=coeff)(o, fx["y"].to(DEV), fx[f"mask.{mname}"].to(DEV))
            want = fx[f"{mname}_{int(reg)}_{coeff}.loss"]
            if torch.isnan(want):
                assert torch.isnan(loss).item()
            else:
                assert_close(loss, want, 1e-6, f"loss {mname} {reg} {coeff}")
            loss.backward()
            assert_close(o.grad, fx[f"{mname}_{int(reg)}_{coeff}.grad"], 1e-6, f"grad {mname} {reg} {coeff}")
    d = make_batch("118v2", 128, seed=5)
    out = torch.randn_like(d.y)
    o_ref = out.clone().requires_grad_(True)
    l_ref = ref_cpu.masked_l2_loss(o_ref, d.y, d.pred_mask, True, 1)
    l_ref.backward()
    o = out.to(DEV).requires_grad_(True)
    loss = Masked_L2_loss()(o, d.y.to(DEV), d.pred_mask.to(DEV))
    loss.backward(Masked_L2_loss.unit_grad(loss))
    assert_close(loss, l_ref, 1e-6, "loss full size")
    assert_close(o.grad, o_ref.grad, 1e-6, "grad full size")


def test_powerflowdata_on_device_feeds_the_model(tmp_path):
    """A split resident on the GPU: batches assembled there equal the host collate of the same samples, the model output is
    identical, and equal-size batches reuse one cached edge_index (topology cache hit: no graph rebuild)."""
    import numpy as np
    from poweflownet_amd.data import Batch, DataLoader
    from poweflownet_amd.datasets import PowerFlowData
    from poweflownet_amd.synth import make_topology
    rng = np.random.default_rng(4)
    S, n = 12, 118
    ei = make_topology(118, 186).numpy()
    e = ei.shape[1]
    node = np.zeros((S, n, 6))
    node[:, :, 0] = np.arange(n)
    node[:, :, 1] = np.where(np.arange(n) == 0, 0, np.where(np.arange(n) % 3 == 0, 1, 2))
    node[:, :, 2:] = rng.normal(size=(S, n, 4))
    edge = np.zeros((S, e, 4))
    edge[:, :, :2] = ei.T
    edge[:, :, 2:] = np.abs(rng.normal(size=(S, e, 2)))
    (tmp_path / "raw").mkdir()
    np.save(tmp_path / "raw" / "case118v2_edge_features.npy", edge)
    np.save(tmp_path / "raw" / "case118v2_node_features.npy", node)
    host = PowerFlowData(root=str(tmp_path), case="118v2", split=[.5, .25, .25], task="train")
    dev = PowerFlowData(root=str(tmp_path), case="118v2", split=[.5, .25, .25], task="train", device=DEV)
    assert len(dev) == 6 and dev.device.type == "cuda"
    torch.manual_seed(0)
    m = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.0).to(DEV).eval()
    seen = []
    for bi, b in enumerate(DataLoader(dev, batch_size=3)):
        want = Batch.from_data_list([host[i] for i in range(3 * bi, 3 * bi + 3)])
        for k in ("x", "y", "pred_mask", "edge_index", "edge_attr", "ptr"):
            assert torch.equal(getattr(b, k).cpu(), getattr(want, k)), k
        out = m(b)
        assert_close(out, m(want.to(DEV)), 1e-6, "device batch vs host batch")
        seen.append(b.edge_index)
    assert seen[0] is seen[1]


def test_graphed_train_step_equals_eager_training(tmp_path):
    """train_epoch with a GraphedTrainStep (one hipGraph replay per batch -- the batch gathered from the device-resident dataset
    INSIDE the graph, a graph of its own for the short last batch, re-capture after a learning-rate change) leaves the same
    parameters and returns the same epoch loss as the eager loop."""
    import numpy as np
    from poweflownet_amd.data import DataLoader
    from poweflownet_amd.datasets import PowerFlowData
    from poweflownet_amd.optim import FlatAdamW
    from poweflownet_amd.synth import make_topology
    from poweflownet_amd.utils.custom_loss_functions import Masked_L2_loss
    from poweflownet_amd.utils.training import GraphedTrainStep, train_epoch
    rng = np.random.default_rng(11)
    S, n = 44, 14
    ei = make_topology(14, 20).numpy()
    node = np.zeros((S, n, 6))
    node[:, :, 1] = np.where(np.arange(n) == 0, 0, np.where(np.arange(n) % 3 == 0, 1, 2))
    node[:, :, 2:] = rng.normal(size=(S, n, 4))
    edge = np.zeros((S, 20, 4))
    edge[:, :, :2] = ei.T
    edge[:, :, 2:] = np.abs(rng.normal(size=(S, 20, 2)))
    (tmp_path / "raw").mkdir()
    np.save(tmp_path / "raw" / "case14_edge_features.npy", edge)
    np.save(tmp_path / "raw" / "case14_node_features.npy", node)
    ds = PowerFlowData(root=str(tmp_path), case="14", split=[.5, .25, .25], task="train", device=DEV)   # 22 samples

    def run(graphed):
        torch.manual_seed(5)
        m = MaskEmbdMultiMPN(4, 2, 4, 32, 3, 2, 0.0).to(DEV)
        opt = FlatAdamW(m, lr=1e-3)
        loss_fn = Masked_L2_loss()
        g = GraphedTrainStep(m, loss_fn, opt) if graphed else None
        losses = []
        for epoch in range(3):
            loader = DataLoader(ds, batch_size=8, shuffle=True, generator=torch.Generator().manual_seed(epoch))   # 8 + 8 + 6
            losses.append(train_epoch(m, loader, loss_fn, opt, DEV, graph=g))
            if epoch == 1:
                opt.param_groups[0]["lr"] = 5e-4                                   # what a scheduler does between epochs
        if g is not None:
            # device-resident dataset: every batch SIZE has its own captured step, which gathers its samples inside the graph
            # (utils/training.py step_indexed) -- also the epoch's short last batch
            assert sorted(g._children) == [6, 8] and all(ch.graph is not None and not ch.disabled for ch in g._children.values())
        return losses, [p.detach().clone() for p in m.parameters()]

    l_e, p_e = run(False)
    l_g, p_g = run(True)
    for a, b in zip(l_e, l_g):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), (l_e, l_g)
    for a, b in zip(p_e, p_g):
        assert_close(b, a, 1e-6, "parameters after 3 epochs")


def test_g10_power_imbalance_matches_reference_goldens():
    """pfn_power_imbalance vs outputs of the reference's own PowerImbalance / MixedMSEPoweImbalance (stored-once and
    already-symmetric edge lists), then against the oracle on a case118 batch."""
    from poweflownet_amd.utils.custom_loss_functions import MixedMSEPoweImbalance, PowerImbalance
    fx = load("g10_power_imbalance")
    st = (fx["xymean"], fx["xystd"], fx["edgemean"], fx["edgestd"])
    for tag, (ei, ea) in {"dir": (fx["edge_index"], fx["edge_attr"]), "sym": (fx["edge_index_sym"], fx["edge_attr_sym"])}.items():
        x = fx["x"].to(DEV).requires_grad_(True)
        loss = PowerImbalance(*st)(x, ei.to(DEV), ea.to(DEV))
        loss.backward()
        assert_close(loss, fx[f"pi_{tag}.loss"], RTOL, f"pi {tag} loss")
        assert_close(x.grad, fx[f"pi_{tag}.grad"], RTOL, f"pi {tag} grad")
        x = fx["x"].to(DEV).requires_grad_(True)
        loss = MixedMSEPoweImbalance(*st, alpha=0.9)(x, ei.to(DEV), ea.to(DEV), fx["y"].to(DEV))
        loss.backward()
        assert_close(loss, fx[f"mix_{tag}.loss"], RTOL, f"mix {tag} loss")
        assert_close(x.grad, fx[f"mix_{tag}.grad"], RTOL, f"mix {tag} grad")
    d = make_batch("118v2", 32, seed=2)
    stats = (torch.tensor([[1.0, -5.0, 25.0, 9.0]]), torch.tensor([[0.04, 12.0, 35.0, 14.0]]),
             torch.tensor([[0.05, 0.2]]), torch.tensor([[0.01, 0.05]]))
    ea = d.edge_attr.clamp(-3, 3)
    x_ref = d.x.clone().requires_grad_(True)
    l_ref = ref_cpu.power_imbalance(x_ref, d.edge_index, ea, *stats)
    l_ref.backward()
    x = d.x.to(DEV).requires_grad_(True)
    loss_fn = PowerImbalance(*stats)
    loss = loss_fn(x, d.edge_index.to(DEV), ea.to(DEV))
    loss.backward(PowerImbalance.unit_grad(loss))
    assert_close(loss, l_ref, RTOL, "loss, case118 x 32")
    assert_close(x.grad, x_ref.grad, RTOL, "grad, case118 x 32")


@pytest.mark.parametrize("tag", ["L3K2", "L2K3"])
def test_g11_mpn_simplenet_matches_reference(tag):
    """The sibling model that still runs on the dataset's 4-wide features (networks/MPN.py:753-792), composed from the two
    HIP layers, against the reference class's own output and parameter gradients."""
    from poweflownet_amd.data import Data
    from poweflownet_amd.networks.MPN import MPN_simplenet
    fx = load("g11_mpn_simplenet")
    L_, K, h = (int(v) for v in fx[f"{tag}.cfg"])
    m = MPN_simplenet(4, 2, 4, h, L_, K, 0.0)
    m.load_state_dict({k[len(tag) + 7:]: v for k, v in fx.items() if k.startswith(f"{tag}.param.")})
    m = m.to(DEV)
    d = Data(x=fx[f"{tag}.x"].to(DEV), edge_index=fx["edge_index"].to(DEV), edge_attr=fx[f"{tag}.edge_attr"].to(DEV))
    out = m(d)
    assert_close(out, fx[f"{tag}.out"], RTOL, "out")
    torch.nn.MSELoss()(out, fx[f"{tag}.y"].to(DEV)).backward()
    for k, p in m.named_parameters():
        assert_close(p.grad, fx[f"{tag}.grad.{k}"], RTOL, f"grad {k}")


@pytest.mark.parametrize("tag", ["MPN", "SkipMPN", "MaskEmbdMPN", "MultiMPN", "MaskEmbdMultiMPN_NoMP"])
def test_g12_sibling_models_match_reference(tag):
    """the reference's older model classes (networks/MPN.py:143-453, :562-650) as compositions of the two
    HIP layers (and the HIP GEMM for their mask embedding), against the reference classes' own outputs and parameter
    gradients on the 12-wide node layout they assert; on the dataset's 4-wide layout their first line raises, as there."""
    import poweflownet_amd.networks.MPN as M
    from poweflownet_amd.data import Data
    fx = load("g12_sibling_models")
    f, o, h, L_, K = (int(v) for v in fx[f"{tag}.cfg"])
    m = getattr(M, tag)(f, 2, o, h, L_, K, 0.0)
    m.load_state_dict({k[len(tag) + 7:]: v for k, v in fx.items() if k.startswith(f"{tag}.param.")})
    m = m.to(DEV)
    d = Data(x=fx[f"{tag}.x"].to(DEV), edge_index=fx["edge_index"].to(DEV), edge_attr=fx[f"{tag}.edge_attr"].to(DEV))
    out = m(d)
    assert_close(out, fx[f"{tag}.out"], RTOL, "out")
    torch.nn.MSELoss()(out, fx[f"{tag}.y"].to(DEV)).backward()
    for k, p in m.named_parameters():
        assert_close(p.grad, fx[f"{tag}.grad.{k}"], RTOL, f"grad {k}")
    assert m.is_directed(d.edge_index) is True
    with pytest.raises(AssertionError):                  # the stale-width assert, verbatim (:194 etc.)
        m(make_batch("14", 2).to(DEV))


def test_g7_batch_equals_concat_of_singles():
    fx = load("g7_collate")
    m = MaskEmbdMultiMPN(4, 2, 4, 8, 2, 3, 0.0)
    m.load_state_dict(params_from(fx))
    m = m.to(DEV).eval()
    big = data_from(fx, prefix="big.", device=DEV)
    assert_close(m(big), fx["batch_out"], RTOL, "batch_out")
    singles = []
    for b in range(3):
        d = data_from(fx, prefix=f"g{b}.", device=DEV)
        singles.append(m(d))
    assert_close(torch.cat(singles), fx["singles_out"], RTOL, "singles")


@pytest.mark.parametrize("case,B,cfg", [("14", 32, (129, 4, 3)), ("118", 16, (129, 4, 3)), ("118", 4, (129, 6, 6)),
                                        ("118", 3, (64, 2, 3)), ("14", 5, (512, 3, 2)),
                                        # hidden widths that walk the column plans of the graph-resident kernels (ea_seg.hip):
                                        # 33 / 36 -> one quarter + 1 / 4 trailing columns, 100 -> three quarters + 4, 132 -> four
                                        # + 4 real trailing columns, 136 -> five quarters, the last one 8 columns wide, K8 = 136
                                        ("118", 3, (33, 3, 2)), ("14", 20, (36, 3, 2)), ("118", 3, (100, 3, 2)),
                                        ("14", 20, (132, 3, 2)), ("118", 3, (136, 3, 2))])
def test_model_vs_oracle_seeded(case, B, cfg):
    torch.manual_seed(1234)
    h, L_, K = cfg
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, h, L_, K, 0.0).eval()
    with torch.no_grad():
        for mod in ref.layers:
            if hasattr(mod, "bias") and isinstance(mod.bias, torch.nn.Parameter):
                mod.bias.normal_(std=0.1)                  # TAGConv bias is zero-initialised: exercise it
    m = MaskEmbdMultiMPN(4, 2, 4, h, L_, K, 0.0)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    data = make_batch(case, B, seed=3)
    out_ref = ref(data)
    loss_ref = torch.nn.MSELoss()(out_ref, data.y)
    loss_ref.backward()
    dd = data.to(DEV)
    out = m(dd)
    assert_close(out, out_ref, RTOL, "out")
    torch.nn.MSELoss()(out, dd.y).backward()
    for (k, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        assert_close(p.grad, q.grad, RTOL, f"grad.{k}")


def test_fused_lds_hops_match_generic_path():
    """Batches with `ptr` take the graph-resident LDS kernels (fused hops, ea_seg); without it the generic per-hop / GEMM /
    edge kernels.  Same output to 1e-6;
    the gradients are two different fp32 formulations of a sum with cancellation (untrained weights: a ReLU decision within
    the forward rounding error of zero may differ between them), so EACH path is held at 1e-5 against the float64 oracle run
    on that path's own ReLU decisions (_assert_grads_on_hip_gates)."""
    torch.manual_seed(3)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 129, 3, 3, 0.0).eval()
    with torch.no_grad():
        for mod in ref.layers:
            if hasattr(mod, "lins"):
                mod.bias.normal_(std=0.1)
    m = MaskEmbdMultiMPN(4, 2, 4, 129, 3, 3, 0.0)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    for case, B in (("118", 6), ("14", 37)):
        data = make_batch(case, B)
        d = data.to(DEV)
        out_f = m(d)
        assert m._graphs._graph.seg_nodes == {"118": 118, "14": 14}[case]
        m.zero_grad()
        torch.nn.MSELoss()(out_f, d.y).backward()
        _assert_grads_on_hip_gates(m, ref, data, f"{case}: graph-resident", out_f)
        d2 = d.clone()
        del d2.__dict__["ptr"]; d2._keys.remove("ptr")
        out_g = m(d2)
        assert m._graphs._graph.seg_nodes == 0
        m.zero_grad()
        torch.nn.MSELoss()(out_g, d2.y).backward()
        _assert_grads_on_hip_gates(m, ref, data, f"{case}: generic", out_g)
        assert_close(out_f, out_g, 1e-6, "out")
    # a hint that the edges contradict is rejected on device: 5 graphs of 14 nodes claimed to be 7 graphs of 10
    d = make_batch("14", 5).to(DEV)
    d.ptr = torch.arange(0, 71, 10, device=DEV)
    m(d)
    assert m._graphs._graph.seg_nodes == 0


def test_graph_resident_kernels_with_more_edges_than_their_lds_slices():
    """Dense small graphs (16 nodes, 100 stored = 200 directed edges each): a workgroup of the graph-resident kernels owns 8
    graphs = 1,600 edge slots, more than its LDS adjacency slice holds (4 per row), so the walks read indices and attributes
    from global memory (csr_slot / seg_bwd_row_slow).  Output and all gradients against the CPU oracle."""
    from poweflownet_amd.data import Batch
    from poweflownet_amd.synth import make_graph, make_topology
    torch.manual_seed(11)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 129, 3, 2, 0.0).eval()
    m = MaskEmbdMultiMPN(4, 2, 4, 129, 3, 2, 0.0)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    topo = make_topology(16, 100, 0)
    data = Batch.from_data_list([make_graph(16, 100, seed=50 + b, edge_index=topo) for b in range(21)])
    out_ref = ref(data)
    torch.nn.MSELoss()(out_ref, data.y).backward()
    dd = data.to(DEV)
    out = m(dd)
    assert m._graphs._graph.seg_nodes == 16
    assert_close(out, out_ref, RTOL, "out")
    torch.nn.MSELoss()(out, dd.y).backward()
    for (k, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        assert_close(p.grad, q.grad, RTOL, f"grad.{k}")


@pytest.mark.parametrize("with_ptr", [True, False])
def test_model_input_and_edge_attr_gradients_vs_oracle(with_ptr):
    """Gradients with respect to x AND edge_attr through the whole model (pfn_mpn_backward's optional outputs).  The edge-attribute
    gradient needs the recomputing backward walks, whatever the forward pass ran: with `ptr` the graph-resident forward kernels
    (their P | Q must be in memory for it), without it the generic forward walks that also saved ReLU masks nobody reads."""
    torch.manual_seed(21)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 129, 3, 2, 0.0).eval()
    m = MaskEmbdMultiMPN(4, 2, 4, 129, 3, 2, 0.0)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    data = make_batch("118", 5, seed=9)
    data.x.requires_grad_(True)
    data.edge_attr.requires_grad_(True)
    torch.nn.MSELoss()(ref(data), data.y).backward()
    dd = data.clone().to(DEV)
    if not with_ptr:
        del dd.__dict__["ptr"]; dd._keys.remove("ptr")
    dd.x = dd.x.detach().requires_grad_(True)
    dd.edge_attr = dd.edge_attr.detach().requires_grad_(True)
    out = m(dd)
    assert (m._graphs._graph.seg_nodes == 118) == with_ptr
    torch.nn.MSELoss()(out, dd.y).backward()
    assert_close(dd.x.grad, data.x.grad, RTOL, "grad x")
    assert_close(dd.edge_attr.grad, data.edge_attr.grad, RTOL, "grad edge_attr")
    for (k, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        assert_close(p.grad, q.grad, RTOL, f"grad.{k}")


@pytest.mark.parametrize("fe", [1, 3])
def test_model_with_other_edge_feature_widths_vs_oracle(fe):
    """efeature_dim != 2 through the WHOLE model: the generic-width edge walks (runtime Fe), no ReLU masks, no graph-resident
    kernels -- the recomputing backward walks at model level."""
    torch.manual_seed(31 + fe)
    ref = ref_cpu.MaskEmbdMultiMPN(4, fe, 4, 64, 3, 2, 0.0).eval()
    m = MaskEmbdMultiMPN(4, fe, 4, 64, 3, 2, 0.0)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    data = make_batch("14", 6, seed=2)
    data.edge_attr = torch.randn(data.edge_index.shape[1], fe)
    torch.nn.MSELoss()(ref(data), data.y).backward()
    dd = data.to(DEV)
    out = m(dd)
    assert_close(out, ref(data), RTOL, "out")
    torch.nn.MSELoss()(out, dd.y).backward()
    for (k, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        assert_close(p.grad, q.grad, RTOL, f"grad.{k}")


def test_edge_cases_empty_edges_and_isolated_nodes():
    from poweflownet_amd.data import Data
    torch.manual_seed(0)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 8, 2, 3, 0.0).eval()
    m = MaskEmbdMultiMPN(4, 2, 4, 8, 2, 3, 0.0)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    n = 5
    for ei in (torch.zeros(2, 0, dtype=torch.long), torch.tensor([[0, 3], [1, 3]])):     # no edges; self loop + isolated
        d = Data(x=torch.randn(n, 4), y=torch.randn(n, 4), bus_type=torch.zeros(n, dtype=torch.long),
                 pred_mask=torch.randint(0, 2, (n, 4)), edge_index=ei, edge_attr=torch.randn(ei.shape[1], 2),
                 batch=torch.zeros(n, dtype=torch.long))
        assert_close(m(d.to(DEV)), ref(d), RTOL, f"E={ei.shape[1]}")


def test_ragged_batch_of_different_grids_vs_oracle():
    """A PyG batch may mix graphs of different sizes (14- and 118-bus grids here: the "graphs of n / B nodes" guess of the
    graph-resident kernels does not hold and the on-device segment check must send the batch down the generic path):
    forward and every parameter gradient against the oracle."""
    from poweflownet_amd.data import Batch
    from poweflownet_amd.synth import make_graph
    torch.manual_seed(11)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.0).eval()
    m = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.0)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    d = Batch.from_data_list([make_graph(14, 20, seed=1), make_graph(118, 186, seed=2), make_graph(14, 20, seed=3, topo_seed=4),
                              make_graph(118, 186, seed=5, topo_seed=6)])
    assert d.x.shape[0] == 264            # 4 graphs: the guess is 66 nodes per graph, and the 118-bus grids straddle its multiples
    out_ref = ref(d)
    torch.nn.MSELoss()(out_ref, d.y).backward()
    dd = d.to(DEV)
    out = m(dd)
    assert m._graphs._graph.seg_nodes == 0
    assert_close(out, out_ref, RTOL, "out")
    torch.nn.MSELoss()(out, dd.y).backward()
    for (k, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        assert_close(p.grad, q.grad, RTOL, f"grad.{k}")


def test_float_mask_and_nonsymmetric_input():
    """explain_epoch-style input: already-bidirectional, asymmetric edge list + float mask."""
    torch.manual_seed(5)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 16, 3, 2, 0.0).eval()
    m = MaskEmbdMultiMPN(4, 2, 4, 16, 3, 2, 0.0)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    d = make_batch("14", 2)
    ei = torch.cat([d.edge_index, d.edge_index.flip(0)[:, :25]], dim=1)   # first edge has its reverse; others may not
    d.edge_index, d.edge_attr = ei, torch.randn(ei.shape[1], 2)
    d.pred_mask = torch.rand(d.x.shape)                                    # arbitrary float mask
    out_ref = ref(d)
    out_ref.sum().backward()
    dd = d.to(DEV)
    out = m(dd)
    assert_close(out, out_ref, RTOL, "out")
    out.sum().backward()
    for (k, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        assert_close(p.grad, q.grad, RTOL, f"grad.{k}")


def test_forward_does_not_mutate_data_and_is_deterministic():
    m = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.0).to(DEV).eval()
    d = make_batch("118", 8).to(DEV)
    before = {k: getattr(d, k).clone() for k in d.keys()}
    a = m(d)
    b = m(d)
    assert torch.equal(a, b)                                # atomics-free segmented sums: bitwise reproducible
    for k, v in before.items():
        assert torch.equal(getattr(d, k), v), k


def test_dropout_mask_statistics_config2():
    """Row a10 (networks/MPN.py:496,546-547), the Bernoulli draw itself: at configs[1]'s size every hidden layer's keep-rate
    lies in a 4-sigma binomial band around 1 - p, so do the per-column and per-row marginals (5 sigma over 129 / 15,104
    cells), masks of different layers and of consecutive forwards are uncorrelated, the stream is reproducible from
    (seed, offset), and it never depends on the data."""
    p = 0.2
    m = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, p).to(DEV).train()
    d = make_batch("118v2", 128, seed=0).to(DEV)
    n = d.x.shape[0]
    m.seed_dropout(2024)
    with torch.no_grad():
        m(d)
    first = _exported_masks(m, n)
    cnt = n * 129
    sigma = (p * (1 - p) / cnt) ** 0.5
    for li, k in enumerate(first):
        assert ((k == 0) | (k == 1)).all()
        rate = k.mean().item()
        assert abs(rate - (1 - p)) <= 4 * sigma, (li, rate, sigma)
        col = k.mean(0)
        assert (col - (1 - p)).abs().max().item() <= 5 * (p * (1 - p) / n) ** 0.5, (li, "column marginal")
        row = k.mean(1)
        assert (row - (1 - p)).abs().max().item() <= 5.5 * (p * (1 - p) / 129) ** 0.5, (li, "row marginal")
        # neighbouring elements (the four words of one Philox call, and consecutive calls) are independent
        c = k - k.mean()
        for shift in (1, 4, 129):
            flat = c.flatten()
            corr = (flat[:-shift] * flat[shift:]).mean().item() / (p * (1 - p))
            assert abs(corr) <= 5 / cnt ** 0.5, (li, shift, corr)
    for a in range(len(first)):
        for b in range(a + 1, len(first)):
            corr = ((first[a] - (1 - p)) * (first[b] - (1 - p))).mean().item() / (p * (1 - p))
            assert abs(corr) <= 5 / cnt ** 0.5, (a, b, corr)
    with torch.no_grad():
        m(d)                                                     # offset advanced: a fresh, independent mask
    second = _exported_masks(m, n)
    for a, b in zip(first, second):
        assert not torch.equal(a, b)
        corr = ((a - (1 - p)) * (b - (1 - p))).mean().item() / (p * (1 - p))
        assert abs(corr) <= 5 / cnt ** 0.5
    m.seed_dropout(2024)                                         # same seed -> the same stream, whatever the input
    d2 = make_batch("118v2", 128, seed=7).to(DEV)
    with torch.no_grad():
        m(d2)
    for a, b in zip(first, _exported_masks(m, n)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("case,B,cfg", [("14", 4, (129, 4, 3)), ("118v2", 8, (129, 4, 3)), ("118v2", 128, (129, 4, 3)),
                                        ("118v2", 4, (129, 6, 6)),
                                        # 241,664 rows: the weight-streaming gemm_nt over whole rounds + the stationary kernel on
                                        # the remaining rows (its dropout counter continues at the global row)
                                        ("118v2", 2048, (129, 4, 3)),
                                        # K = 6 at 135,936 rows: the 7-term TAGConv products take the weight-STREAMING gemm_nt
                                        # (gemm_nt_ws_kernel) over whole rounds of row tiles + the stationary kernel on the tail
                                        ("118v2", 1152, (129, 2, 6))])
def test_train_mode_matches_oracle_fed_the_exported_masks(case, B, cfg):
    """Row a10 end to end: a TRAIN-mode pass (dropout 0.2) against the CPU oracle whose nn.Dropout is replaced by
    multiplication with the masks the HIP path exports (pfn_dropout_mask) and 1/(1-p).  Checks the three things SURVEY H4
    lists at once -- the kept set, the 1/(1-p) scale, and that backward uses the forward's mask: forward and ALL parameter
    gradients must agree with the oracle at 1e-5 (at every size against the float64 oracle on the HIP path's ReLU
    decisions, _assert_grads_on_hip_gates; below 2,000 nodes also against the plain fp32 oracle)."""
    h, L_, K = cfg
    p = 0.2
    torch.manual_seed(99)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, h, L_, K, p).train()
    m = MaskEmbdMultiMPN(4, 2, 4, h, L_, K, p)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).train()
    m.seed_dropout(31337)
    data = make_batch(case, B, seed=3)
    dd = data.to(DEV)
    out = m(dd)
    torch.nn.MSELoss()(out, dd.y).backward()
    ref.dropout_masks = [k.cpu() for k in _exported_masks(m, dd.x.shape[0])]
    torch.set_num_threads(min(32, os.cpu_count() or 8))
    out_ref = ref(data)
    torch.nn.MSELoss()(out_ref, data.y).backward()
    out64, _ = _fp64_truth(ref, data)                            # deepcopy carries the masks along
    assert_close(out, out_ref, RTOL, "train-mode out")
    assert_close(out, out64.float(), RTOL, "train-mode out vs fp64")
    if dd.x.shape[0] <= 2000:                                    # small: plain fp32 oracle, no gate equalisation needed
        for (k, q_), q in zip(m.named_parameters(), ref.parameters()):
            assert_close(q_.grad, q.grad, RTOL, f"train-mode grad.{k}")
    _assert_grads_on_hip_gates(m, ref, data, "train mode", out)
    # and the eval-mode pass of the same model ignores the stream entirely
    m.eval()
    ref.eval()
    ref.dropout_masks = None
    with torch.no_grad():
        assert_close(m(dd), ref(data), RTOL, "eval out")


def test_fused_front_and_back_equal_generic_gemm_path(tmp_path):
    """front.hip (mask_embd + residual + layer-0 P|Q in one launch, and its mirror in backward) and the last layer's fused
    walks (edge_fwd_out_kernel: out = S W2^T + deg b2 inside the edge walk; edge_bwd ds_row: dS rows formed from gout and
    W2 inside the walks) and the graph-resident EdgeAggregation kernels (ea_seg.hip: node GEMM + edge walk per 32-column
    quarter in one launch) against the generic tall-skinny GEMM + edge kernels they replace (PFN_NO_FUSED_FRONT=1 /
    PFN_NO_FUSED_BACK=1 / PFN_NO_SEG_EA=1; PFN_FRONT_BLOCK_ROWS=1 = the front's block-per-row-group kernels instead of one row per wave; read once per process -> child processes): same output and gradients up to fp32 summation
    order."""
    import os
    import subprocess
    import sys
    script = f"""
import sys, torch
sys.path.insert(0, {repr(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))})
from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
from poweflownet_amd.synth import make_batch
torch.manual_seed(3)
m = MaskEmbdMultiMPN(4, 2, 4, 129, 3, 2, 0.0).to("cuda:0").eval()
d = make_batch("118", 6, seed=4).to("cuda:0")
d.x.requires_grad_(True)
out = m(d)
torch.nn.MSELoss()(out, d.y).backward()
torch.save({{"out": out.detach().cpu(), "gx": d.x.grad.cpu(), "g": m.flat_grad().cpu()}}, sys.argv[1])
"""
    res = {}
    variants = (("fused", {}), ("no_front", {"PFN_NO_FUSED_FRONT": "1"}), ("no_back", {"PFN_NO_FUSED_BACK": "1"}),
                ("no_seg", {"PFN_NO_SEG_EA": "1"}), ("no_seg_no_back", {"PFN_NO_SEG_EA": "1", "PFN_NO_FUSED_BACK": "1"}),
                ("front_block_rows", {"PFN_FRONT_BLOCK_ROWS": "1"}),
                ("generic", {"PFN_NO_FUSED_FRONT": "1", "PFN_NO_FUSED_BACK": "1", "PFN_NO_SEG_EA": "1"}))
    for tag, env in variants:
        path = str(tmp_path / f"{tag}.pt")
        subprocess.run([sys.executable, "-c", script, path], check=True, env=dict(os.environ, **env), timeout=300)
        res[tag] = torch.load(path)
    for tag in ("fused", "no_front", "no_back", "no_seg", "no_seg_no_back", "front_block_rows"):
        assert_close(res[tag]["out"], res["generic"]["out"], RTOL, f"{tag}: out")
        assert_close(res[tag]["gx"], res["generic"]["gx"], RTOL, f"{tag}: grad x")
        assert_close(res[tag]["g"], res["generic"]["g"], RTOL, f"{tag}: flat parameter gradient")


def test_fused_linear_hops_are_bit_identical_to_two_launches(tmp_path):
    """seg_lin_hops.hip: for batches of small graphs the Linear in front of a TAGConv's hops -- forward `act(S W2^T + deg b2)`, backward
    `(dP W1i + dQ W1j)[gate]` -- and the K hops over its output run in ONE launch per (graph, 32-column quarter) (networks/MPN.py:541-547:
    the E -> act -> T loop).  It repeats gemm_nt's MFMA k / term order, trailing-column chains and epilogue expressions and
    fused_hops_kernel's edge order, so every output and every gradient carries the SAME BITS as the two-launch path
    (PFN_NO_SEG_LIN_HOPS=1; read once per process -> child processes): eval and train mode (dropout: the same Philox draw per
    (row, column group)), case118v2 x 128 (one graph per workgroup, gemm_nt's stationary kernel on the other side), case14 x 37 (nine
    graphs per workgroup, a last block with fewer rows), and dense 16-node graphs whose edges exceed the LDS adjacency slice."""
    import os
    import subprocess
    import sys
    script = f"""
import sys, torch
sys.path.insert(0, {repr(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))})
from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
from poweflownet_amd.synth import make_batch, make_graph, make_topology
from poweflownet_amd.data import Batch
from poweflownet_amd import _lib as L
res = {{}}
def run(tag, m, d):
    d = d.to("cuda:0")
    d.x.requires_grad_(True)
    L.profile_report(reset=True); L.profile_enable(True)
    out = m(d)
    torch.nn.MSELoss()(out, d.y).backward()
    torch.cuda.synchronize()
    L.profile_enable(False)
    rep = L.profile_report(reset=True)
    res[tag + ".launches"] = {{k: v["count"] for k, v in rep.items() if not k.startswith("__")}}
    res[tag + ".out"], res[tag + ".gx"], res[tag + ".g"] = out.detach().cpu(), d.x.grad.cpu(), m.flat_grad().cpu()
    m.zero_grad(set_to_none=True)
torch.manual_seed(5)
m = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.2).to("cuda:0")
m.seed_dropout(77)
m.train()
run("train118", m, make_batch("118v2", 128, seed=1))
m.eval()
run("eval118", m, make_batch("118v2", 128, seed=2))
run("eval14", m, make_batch("14", 37, seed=3))
topo = make_topology(16, 100, 0)
run("dense16", m, Batch.from_data_list([make_graph(16, 100, seed=50 + b, edge_index=topo) for b in range(21)]))
torch.save(res, sys.argv[1])
"""
    res = {}
    # (below 256 row tiles gemm_nt hands one-group products to its split-K kernel, whose per-term partial sums and `x + rs * b`
    #  epilogue are another fp32 order: PFN_NT_TINY_MAX_TILES=0 keeps the weight-stationary kernel on the two-launch side)
    for tag, env in (("fused", {"PFN_NT_TINY_MAX_TILES": "0"}), ("two", {"PFN_NT_TINY_MAX_TILES": "0", "PFN_NO_SEG_LIN_HOPS": "1"})):
        path = str(tmp_path / f"{tag}.pt")
        subprocess.run([sys.executable, "-c", script, path], check=True, env=dict(os.environ, **env), timeout=600)
        res[tag] = torch.load(path)
    for case in ("train118", "eval118", "eval14", "dense16"):
        lf, lt = res["fused"][case + ".launches"], res["two"][case + ".launches"]
        # L = 4: three E -> T transitions per direction ride in the fused launches; the two-launch path has none of them
        assert lf.get("seg_lin_hops_fwd") == 3 and lf.get("seg_lin_hops_bwd") == 3 and "fused_hops_fwd" not in lf, lf
        assert "seg_lin_hops_fwd" not in lt and lt.get("fused_hops_fwd") == 3 and lt.get("fused_hops_bwd") == 3, lt
        assert lf["gemm_nt"] == lt["gemm_nt"] - 6, (lf, lt)
        for key in ("out", "gx", "g"):
            a, b = res["fused"][f"{case}.{key}"], res["two"][f"{case}.{key}"]
            assert a.abs().max() > 0 and torch.isfinite(a).all()
            assert torch.equal(a, b), f"{case}.{key}: fused Linear + hops differs from gemm_nt + fused_hops by {(a - b).abs().max().item():.3e}"


def test_interleaved_flush_is_bit_identical_to_the_plain_flush(tmp_path):
    """gemm_nt_kernel's ILF (round 6): in large-M launches whose every K = 129 piece ends an output tile -- `act(S W2^T + deg b2)`
    without dropout, `P | Q = x [W1i | W1j]^T (+ b1)`, the backward `dS = g W2` products without a gate (networks/MPN.py:17-21,
    :28) -- a finished tile is parked in a second accumulator set and flushed one register group at a time between the MFMAs of the
    wave's NEXT multiply.  Same expressions in the same order (bias / row-scaled bias as one fma, ReLU as a max, the trailing column's
    two half-chains): every output and gradient carries the SAME BITS as the flush behind its own multiply (PFN_NO_NT_ILF=1; read
    once per process -> child processes).  case118v2 x 600 (row-major operands, 70,800 rows: a partial last row tile), eval and train
    mode (train: only P | Q qualifies in the forward pass), and case6470rte x 11 (chunk-major operands and outputs around the big-graph hops)."""
    import os
    import subprocess
    import sys
    script = f"""
import sys, torch
sys.path.insert(0, {repr(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))})
from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
from poweflownet_amd.synth import make_batch
res = {{}}
def run(tag, m, d, grad=True):
    d = d.to("cuda:0")
    if grad:
        d.x.requires_grad_(True)
        out = m(d)
        torch.nn.MSELoss()(out, d.y).backward()
        res[tag + ".gx"], res[tag + ".g"] = d.x.grad.cpu(), m.flat_grad().cpu()
        m.zero_grad(set_to_none=True)
    else:
        with torch.no_grad():
            out = m(d)
    torch.cuda.synchronize()
    res[tag + ".out"] = out.detach().cpu()
torch.manual_seed(9)
m = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.2).to("cuda:0")
m.seed_dropout(123)
m.eval()
run("infer118", m, make_batch("118v2", 600, seed=1), grad=False)
run("eval118", m, make_batch("118v2", 600, seed=2))
m.train()
run("train118", m, make_batch("118v2", 600, seed=3))
m.eval()
run("eval6470", m, make_batch("6470rte", 11, seed=4))
torch.save(res, sys.argv[1])
"""
    res = {}
    for tag, env in (("ilf", {}), ("plain", {"PFN_NO_NT_ILF": "1"})):
        path = str(tmp_path / f"{tag}.pt")
        subprocess.run([sys.executable, "-c", script, path], check=True, env=dict(os.environ, **env), timeout=900)
        res[tag] = torch.load(path)
    assert set(res["ilf"]) == set(res["plain"]) and len(res["ilf"]) == 10
    for key in sorted(res["ilf"]):
        a, b = res["ilf"][key], res["plain"][key]
        assert a.abs().max() > 0 and torch.isfinite(a).all(), key
        assert torch.equal(a, b), f"{key}: the interleaved flush differs from the plain one by {(a - b).abs().max().item():.3e}"


def test_fused_front_and_first_edge_stage_are_bit_identical_to_two_launches(tmp_path):
    """ea_seg.hip front_seg_fwd_kernel: for batches of small graphs mask_embd + residual (networks/MPN.py:533-537) AND the first
    EdgeAggregation's edge stage run in ONE graph-resident launch per (graph, 32-column quarter) -- front.hip's row-per-wave
    chains and butterfly row sum for x0 / me_h / P | Q, ea_seg's walk for S -- instead of front.hip's launch + the generic edge
    walk (PFN_NO_SEG_FRONT=1; read once per process -> child processes).  Same operands in the same order: outputs, input
    gradient and every parameter gradient carry the same bits; int64 and float masks, train and eval mode, a last block with
    fewer graphs (case14 x 37), dense 16-node graphs whose edges exceed the LDS adjacency slice, and a no_grad forward."""
    import os
    import subprocess
    import sys
    script = f"""
import sys, torch
sys.path.insert(0, {repr(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))})
from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
from poweflownet_amd.synth import make_batch, make_graph, make_topology
from poweflownet_amd.data import Batch
from poweflownet_amd import _lib as L
res = {{}}
def run(tag, m, d, float_mask=False, frac=False):
    d = d.to("cuda:0")
    if float_mask:
        d.pred_mask = d.pred_mask.float()
    if frac:     # entries that are neither 0 nor 1: the per-row evaluation behind the 16-pattern table of the fused launch
        d.pred_mask[::7] *= 0.5
        d.pred_mask[::5, 2] = 2.0
        d.pred_mask[3::11, 0] = -0.0
    d.x.requires_grad_(True)
    L.profile_report(reset=True); L.profile_enable(True)
    out = m(d)
    torch.nn.MSELoss()(out, d.y).backward()
    torch.cuda.synchronize()
    L.profile_enable(False)
    rep = L.profile_report(reset=True)
    res[tag + ".launches"] = {{k: v["count"] for k, v in rep.items() if not k.startswith("__")}}
    res[tag + ".out"], res[tag + ".gx"], res[tag + ".g"] = out.detach().cpu(), d.x.grad.cpu(), m.flat_grad().cpu()
    m.zero_grad(set_to_none=True)
    with torch.no_grad():
        res[tag + ".nograd"] = m(d).cpu()
torch.manual_seed(6)
m = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.2).to("cuda:0")
m.seed_dropout(78)
m.train()
run("train118", m, make_batch("118v2", 128, seed=1))
m.eval()
run("eval118f", m, make_batch("118v2", 16, seed=2), float_mask=True)
run("frac118", m, make_batch("118v2", 16, seed=4), float_mask=True, frac=True)
run("eval14", m, make_batch("14", 37, seed=3))
topo = make_topology(16, 100, 0)
run("dense16", m, Batch.from_data_list([make_graph(16, 100, seed=50 + b, edge_index=topo) for b in range(21)]))
torch.save(res, sys.argv[1])
"""
    res = {}
    for tag, env in (("fused", {}), ("two", {"PFN_NO_SEG_FRONT": "1"})):
        path = str(tmp_path / f"{tag}.pt")
        subprocess.run([sys.executable, "-c", script, path], check=True, env=dict(os.environ, **env), timeout=600)
        res[tag] = torch.load(path)
    for case in ("train118", "eval118f", "frac118", "eval14", "dense16"):
        lf, lt = res["fused"][case + ".launches"], res["two"][case + ".launches"]
        assert lf.get("front_seg_fwd+pack") == 1 and "front_fwd+pack" not in lf and "edge_fwd" not in lf, lf
        assert lt.get("front_fwd+pack") == 1 and lt.get("edge_fwd") == 1 and "front_seg_fwd+pack" not in lt, lt
        for key in ("out", "gx", "g", "nograd"):
            a, b = res["fused"][f"{case}.{key}"], res["two"][f"{case}.{key}"]
            assert a.abs().max() > 0 and torch.isfinite(a).all()
            assert torch.equal(a, b), f"{case}.{key}: fused front + edge stage differs from the two launches by {(a - b).abs().max().item():.3e}"


def test_first_layer_pq_from_x0_is_bit_identical_to_stored_pq(tmp_path):
    """Beyond the latency regime (> 32,768 rows) the first EdgeAggregation layer's P | Q rows are not written when nothing reads
    them from memory (inference; training whose backward walks read saved ReLU masks): the edge walk forms them from the 16-byte
    x0 rows with the front's own fma chains (edge.hip FLY, model.hip Route::l0_fly), and the inference front, left with 32
    bytes of output per row, runs one row per thread with the block kernel's summation order (front.hip).  Same operands in the
    same order -> the SAME BITS as the path that stores and gathers the rows (PFN_NO_L0_FLY=1) and as the block front
    (PFN_FRONT_NO_THREAD_ROWS=1; switches are read once per process -> child processes): outputs, every gradient, and the
    exported edge gates of layer 0 (which, like a backward pass asked for edge-attribute gradients, first writes the rows:
    launch_front_pq).  Covers the generic walk with and without mask saving (300 graphs x 118 buses, graph-resident kernels off)
    and the LDS-resident rows kernel (1,100 graphs)."""
    import os
    import subprocess
    import sys
    script = f"""
import sys, torch
sys.path.insert(0, {repr(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))})
from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
from poweflownet_amd.synth import make_batch
torch.manual_seed(3)
m = MaskEmbdMultiMPN(4, 2, 4, 129, 3, 2, 0.0).to("cuda:0").eval()
res = {{}}
d = make_batch("118", 300, seed=4).to("cuda:0")
d.x.requires_grad_(True)
out = m(d)                                        # training-mode autograd, masks saved (the graph-resident kernels are off)
_g = m.export_gates()
res["gates0"], res["gates_me"] = _g["edge"][0].cpu(), _g["mask_embd"].cpu()
torch.nn.MSELoss()(out, d.y).backward()
res["out"], res["gx"], res["g"] = out.detach().cpu(), d.x.grad.cpu(), m.flat_grad().cpu()
m.zero_grad(set_to_none=True)
d2 = make_batch("118", 300, seed=5).to("cuda:0")
d2.edge_attr.requires_grad_(True)                 # edge-attribute gradient: the backward recomputes pre-activations from P | Q
out2 = m(d2)
torch.nn.MSELoss()(out2, d2.y).backward()
res["out2"], res["gea"], res["g2"] = out2.detach().cpu(), d2.edge_attr.grad.cpu(), m.flat_grad().cpu()
with torch.no_grad():
    res["inf_generic"] = m(d).cpu()
    res["inf_rows"] = m(make_batch("118", 1100, seed=7).to("cuda:0")).cpu()
torch.save(res, sys.argv[1])
"""
    res = {}
    # (with layer 0 on the fly a training pass does not store mask_embd's hidden layer either: the backward front recomputes it and
    #  sums mask_embd's four weight gradients itself, in another order than gemm_tn -- PFN_FRONT_STORE_MEH=1 holds that off for the
    #  bit comparison; the default is compared below: outputs, input gradients and gates bit for bit, weight gradients to fp32 tolerance)
    keep = {"PFN_NO_SEG_EA": "1", "PFN_FRONT_STORE_MEH": "1"}
    for tag, env in (("fly", keep), ("stored", dict(keep, PFN_NO_L0_FLY="1")), ("block_front", dict(keep, PFN_FRONT_NO_THREAD_ROWS="1")),
                     ("default", {"PFN_NO_SEG_EA": "1"})):
        path = str(tmp_path / f"{tag}.pt")
        subprocess.run([sys.executable, "-c", script, path], check=True, env=dict(os.environ, **env), timeout=300)
        res[tag] = torch.load(path)
    for tag in ("stored", "block_front"):
        for key in res["fly"]:
            assert torch.equal(res["fly"][key], res[tag][key]), f"{key}: default path differs from {tag}"
    assert res["fly"]["gea"].abs().max() > 0 and res["fly"]["inf_rows"].abs().max() > 0
    assert torch.equal(res["fly"]["inf_generic"], res["fly"]["out"])   # (no_grad forward = training forward, bit for bit)
    n_me = 4 * 129 + 129 + 4 * 129 + 4                 # mask_embd's parameters are the last four of the flat gradient
    for key in res["fly"]:
        if key in ("g", "g2"):   # (the other weight gradients too: with two pairs fewer gemm_tn splits the rows differently)
            assert not torch.equal(res["default"][key][-n_me:], res["fly"][key][-n_me:])      # (the recomputing backward front did run)
            assert_close(res["default"][key][-n_me:], res["fly"][key][-n_me:], RTOL, f"{key}: mask_embd gradients formed in the backward front")
            assert_close(res["default"][key], res["fly"][key], RTOL, f"{key}: flat parameter gradient")
        else:
            assert torch.equal(res["default"][key], res["fly"][key]), f"{key}: recomputed mask_embd hidden layer"


# One child process per front route (the switches are read once per process); every child runs the same four small cases.
_FRONT_CHAIN_ROUTES = (("seg_front", {}),
                       ("wave", {"PFN_NO_SEG_FRONT": "1"}),
                       ("beyond", {"PFN_FRONT_BLOCK_ROWS": "1", "PFN_NO_SEG_EA": "1"}),
                       ("store_meh", {"PFN_FRONT_BLOCK_ROWS": "1", "PFN_NO_SEG_EA": "1", "PFN_FRONT_STORE_MEH": "1"}),
                       ("block", {"PFN_FRONT_BLOCK_ROWS": "1", "PFN_NO_SEG_EA": "1", "PFN_FRONT_NO_THREAD_ROWS": "1"}),
                       ("stored_pq", {"PFN_FRONT_BLOCK_ROWS": "1", "PFN_NO_SEG_EA": "1", "PFN_NO_L0_FLY": "1"}))
_FRONT_CHAIN_CASES = tuple(f"h{h}.{mk}" for h in (6, 129) for mk in ("int64", "float32"))
_FRONT_CHAIN_KEYS = ("out", "nograd", "gates_me", "gates0", "gx", "g")
_FRONT_CHAIN_CHILD = """
import sys, torch
sys.path.insert(0, {root!r})
from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
from poweflownet_amd.synth import make_batch
res = {{}}
for h in (6, 129):
    torch.manual_seed(11)
    m = MaskEmbdMultiMPN(4, 2, 4, h, 3, 2, 0.0).to("cuda:0").eval()
    for mk in ("int64", "float32"):
        d = make_batch("118", 3, seed=4).to("cuda:0")          # 354 rows
        if mk == "float32":
            d.pred_mask = d.pred_mask.float()
            d.pred_mask[5, 1] = 0.5                            # one non-binary row: front_seg_fwd_kernel's per-row tree
        d.x.requires_grad_(True)
        out = m(d)
        g = m.export_gates()
        res[f"h{{h}}.{{mk}}.gates_me"], res[f"h{{h}}.{{mk}}.gates0"] = g["mask_embd"].cpu(), g["edge"][0].cpu()
        torch.nn.MSELoss()(out, d.y).backward()
        res[f"h{{h}}.{{mk}}.out"], res[f"h{{h}}.{{mk}}.gx"], res[f"h{{h}}.{{mk}}.g"] = out.detach().cpu(), d.x.grad.cpu(), m.flat_grad().cpu()
        m.zero_grad(set_to_none=True)
        with torch.no_grad():
            res[f"h{{h}}.{{mk}}.nograd"] = m(d).cpu()
torch.save(res, sys.argv[1])
"""


def _front_chain_children(tmp_path):
    import subprocess
    import sys
    script = _FRONT_CHAIN_CHILD.format(root=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    # (the six children run side by side: each is mostly its import of torch)
    procs = [(tag, subprocess.Popen([sys.executable, "-c", script, str(tmp_path / f"{tag}.pt")], env=dict(os.environ, **env)))
             for tag, env in _FRONT_CHAIN_ROUTES]
    try:
        for tag, proc in procs:
            assert proc.wait(timeout=300) == 0, f"the child of route {tag} failed"
    finally:
        for _, proc in procs:
            if proc.poll() is None:
                proc.kill()
    return {tag: torch.load(str(tmp_path / f"{tag}.pt")) for tag, _ in _FRONT_CHAIN_ROUTES}


def test_front_chains_give_the_same_bits_on_every_route_at_small_shapes(tmp_path):
    """csrc/front_chains.hpp holds the front's arithmetic once -- mask row, clamped weight slice, hidden unit, Wb step, residual,
    P | Q unit, g0 step, dh unit, the two-level row sum -- and every front route calls it.  The cross-route tests above run
    H = 129 at >= 35,400 rows; this one pins the shared functions where they can go wrong cheaply: 3 x 118 = 354 rows (a multiple
    of neither the 4 rows per block of the row-per-wave kernels nor the 7-row group of the block kernels at H = 129: every
    kernel ends on a ragged trip), hidden_dim 6 (h % 4 != 0, h < 8: the clamp min(u, h - 1), exact-zero pad units, nchunk = 2)
    and 129 (nchunk = 33: the second level of row_sum, idle lanes 33..63, the c + 32 leg of front_seg_fwd_kernel's tree), int64
    and float32 masks, the float one with a non-binary row (front_seg_fwd_kernel's per-row tree next to its 16-pattern table).
    Six children, one per route (_FRONT_CHAIN_ROUTES).  What must agree bit for bit:
      * mask_embd's gates on ALL routes (the hidden unit depends on the mask row alone);
      * within {seg_front, wave} -- x0's chunk sums go through the xor-butterfly order -- everything, as the test of
        front_seg_fwd_kernel above asserts at the large shape: out, nograd, gx, g, and both gate exports;
      * within {beyond, store_meh, block, stored_pq} -- x0's chunk sums go through row_sum's two-level order -- out, nograd, gx and
        both gate exports; the flat parameter gradient g between store_meh and stored_pq as the P | Q test above does, and
        between beyond and block (both take the recomputing backward front where it fits its scratch, see below);
      * beyond against store_meh: g to RTOL (the recomputing backward front sums mask_embd's weight gradients in another order
        than gemm_tn; at the large shape the test above also shows that they differ bitwise);
      * a no_grad forward returns the bits of the training forward on every route.
    The two groups differ from each other in x0's summation order for nchunk > 2: out is held to RTOL across them; at hidden_dim 6
    both orders add the same two chunk sums (and exact zeros), so there out and gx agree bit for bit across the groups as well.
    Finding, measured on the commit before the header existed: at H = 129 the input gradient differs ACROSS the groups
    by 4.6e-4 of its largest entry (5.5e-7 against 1.2e-3) -- two summation orders take different ReLU decisions where a
    pre-activation lies within rounding of zero (tests/util._assert_grads_on_hip_gates) -- so gx is compared within a group only.
    Finding: at 354 rows front_bwd_wg_kernel runs for hidden_dim 6 only -- at H = 129 its per-workgroup partials
    (51 x 1,192 floats) exceed the unused me_h buffer (354 x 132), so make_route keeps me_h stored and `beyond` equals `store_meh`
    there; H = 129 through that kernel stays with the 35,400-row test above."""
    res = _front_chain_children(tmp_path)
    ref = res["seg_front"]
    for case in _FRONT_CHAIN_CASES:
        for key in _FRONT_CHAIN_KEYS:
            a = ref[f"{case}.{key}"]
            assert a.dtype == torch.bool or (torch.isfinite(a).all() and a.abs().max() > 0), f"{case}.{key}"
        for tag, _ in _FRONT_CHAIN_ROUTES:
            r = res[tag]
            assert torch.equal(r[f"{case}.gates_me"], ref[f"{case}.gates_me"]), f"{case}: mask_embd gates of {tag}"
            assert torch.equal(r[f"{case}.nograd"], r[f"{case}.out"]), f"{case}: no_grad forward of {tag} differs from its training forward"
        for key in _FRONT_CHAIN_KEYS:
            assert torch.equal(res["wave"][f"{case}.{key}"], ref[f"{case}.{key}"]), f"{case}.{key}: wave differs from seg_front"
        base = res["store_meh"]
        for tag in ("beyond", "block", "stored_pq"):
            for key in ("out", "nograd", "gates0", "gx"):
                assert torch.equal(res[tag][f"{case}.{key}"], base[f"{case}.{key}"]), f"{case}.{key}: {tag} differs from store_meh"
            if case.startswith("h6"):     # across the two summation orders: the same two addends at nchunk = 2
                for key in ("out", "gx"):
                    assert torch.equal(res[tag][f"{case}.{key}"], ref[f"{case}.{key}"]), f"{case}.{key}: {tag} differs from seg_front"
            else:
                assert_close(res[tag][f"{case}.out"], ref[f"{case}.out"], RTOL, f"{case}.out: {tag} against seg_front")
        assert torch.equal(res["stored_pq"][f"{case}.g"], base[f"{case}.g"]), f"{case}.g: stored_pq differs from store_meh"
        assert torch.equal(res["block"][f"{case}.g"], res["beyond"][f"{case}.g"]), f"{case}.g: block differs from beyond"
        assert_close(res["beyond"][f"{case}.g"], base[f"{case}.g"], RTOL, f"{case}: flat parameter gradient, recomputing backward front")
        n_me = 4 * 129 + 129 + 4 * 129 + 4 if case.startswith("h129") else 4 * 6 + 6 + 4 * 6 + 4
        assert_close(res["beyond"][f"{case}.g"][-n_me:], base[f"{case}.g"][-n_me:], RTOL, f"{case}: mask_embd gradients formed in the backward front")


def test_backward_after_an_inference_forward_gives_nan_gradients_not_garbage():
    """C-ABI misuse the host cannot see: `pfn_mpn_forward` with need_backward = 0 on a TRAINING-sized workspace,
    then `pfn_mpn_backward` with need_backward = 1 on it -- the forward saved nothing the backward reads.  The forward stamps the
    workspace on the device (a rider of its first launch) and the weight-gradient launch writes NaN unless the stamp says
    "training": every parameter gradient is NaN, no host sync, no extra launch; the proper sequence on the same workspace then
    gives the gradients of the autograd path, bit for bit."""
    import ctypes as C
    from poweflownet_amd import _lib as L
    from poweflownet_amd.networks.MPN import _padded
    lib = L.load()
    torch.manual_seed(9)
    m = MaskEmbdMultiMPN(4, 2, 4, 129, 3, 2, 0.0).to(DEV).eval()
    d = make_batch("118", 5, seed=3).to(DEV)
    out_ref = m(d)
    torch.nn.MSELoss()(out_ref, d.y).backward()
    g_ref = m.flat_grad().clone()
    graph = m._graphs._graph
    params = m._ordered_params()
    n = d.x.shape[0]
    cfg = m._config()
    cfg.need_backward = 1
    nbytes = lib.pfn_mpn_workspace_bytes(C.byref(cfg), n, graph.e_stored)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    out = torch.empty(n, _padded(4), dtype=torch.float32, device=DEV)
    gout = (2.0 * (out_ref.detach() - d.y) / out_ref.numel()).contiguous()
    sizes = [p.numel() for p in params]

    def fwd(need_backward):
        cfg.need_backward = need_backward
        L.check(lib.pfn_mpn_forward(C.byref(cfg), graph.ws.data_ptr(), n, graph.e_stored, L.ptr_table(params), d.x.data_ptr(),
                                    d.pred_mask.data_ptr(), 0 if d.pred_mask.dtype == torch.int64 else 1, d.edge_attr.data_ptr(),
                                    out.data_ptr(), ws.data_ptr(), nbytes, None, graph.seg_nodes, L.stream_ptr()), "pfn_mpn_forward")

    def bwd():
        cfg.need_backward = 1
        flat = torch.zeros(sum(sizes), dtype=torch.float32, device=DEV)
        grads = [g if p.dim() == 1 else g.view(p.shape) for g, p in zip(flat.split_with_sizes(sizes), params)]
        L.check(lib.pfn_mpn_backward(C.byref(cfg), graph.ws.data_ptr(), n, graph.e_stored, L.ptr_table(params), L.ptr_table(grads),
                                     d.x.data_ptr(), d.pred_mask.data_ptr(), 0 if d.pred_mask.dtype == torch.int64 else 1,
                                     d.edge_attr.data_ptr(), gout.data_ptr(), None, None, ws.data_ptr(), nbytes, graph.seg_nodes,
                                     L.stream_ptr()), "pfn_mpn_backward")
        torch.cuda.synchronize()
        return flat

    fwd(0)                                           # inference forward on the training-sized workspace
    assert torch.equal(out[:, :4], out_ref.detach())
    bad = bwd()
    assert torch.isnan(bad).all(), f"{int(torch.isnan(bad).sum())} of {bad.numel()} gradient entries are NaN"
    fwd(1)
    good = bwd()
    assert torch.equal(good, g_ref)
    fwd(1); fwd(0)                                   # the LAST forward on the workspace decides
    assert torch.isnan(bwd()).all()


def test_two_models_two_streams_two_threads_do_not_share_state():
    """The library holds no stream / event / device binding of its own (include/pfn_hip.h): two models, each on its own
    torch stream, driven (a) interleaved from one thread and (b) concurrently from two host threads, produce
    bit-for-bit the gradients each produces alone."""
    import threading
    torch.manual_seed(5)
    models = [MaskEmbdMultiMPN(4, 2, 4, 129, 3, 3, 0.0).to(DEV).train() for _ in range(2)]
    datas = [make_batch("118", 16, seed=s_).to(DEV) for s_ in (1, 2)]

    def run(i, reps=1):
        for _ in range(reps):
            models[i].zero_grad(set_to_none=True)
            torch.nn.MSELoss()(models[i](datas[i]), datas[i].y).backward()
        return models[i].flat_grad().clone()

    alone = [run(0), run(1)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    # (a) interleaved on two streams from one thread: forward 0, forward 1, backward 0, backward 1
    outs = []
    for i in range(2):
        streams[i].wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(streams[i]):
            models[i].zero_grad(set_to_none=True)
            outs.append(torch.nn.MSELoss()(models[i](datas[i]), datas[i].y))
    for i in range(2):
        with torch.cuda.stream(streams[i]):
            outs[i].backward()
    torch.cuda.synchronize()
    for i in range(2):
        assert torch.equal(models[i].flat_grad(), alone[i]), f"interleaved, model {i}"
    # (b) two host threads, each with its own stream, 20 steps each
    got, errs = [None, None], []

    def worker(i):
        try:
            with torch.cuda.stream(streams[i]):
                got[i] = run(i, reps=20)
            streams[i].synchronize()
        except Exception as exc:      # noqa: BLE001
            errs.append(exc)

    ts = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for i in range(2):
        assert torch.equal(got[i], alone[i]), f"threaded, model {i}"


# ------------------------------------------------------------------------------------ BASELINE.json full sizes
def test_config2_full_size_vs_oracle():
    """configs[1]: case118v2, batch 128, standard.json -- direct parity with the CPU oracle at the benchmark's size:
    forward and all 35 parameter gradients at 1e-5 (see _check_full_size)."""
    torch.manual_seed(1234)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.0).eval()
    m = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.0)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    _check_full_size(m, ref, make_batch("118v2", 128, seed=0), "config 2", ungated=True)


def _as_real_dataset(data, seed):
    """Give a synthetic batch the masked-entry statistics of the reference's datasets (datasets/PowerFlowData.py:126-139): x and y are
    z-scored with per-feature statistics AFTER x = y * (1 - mask), so a masked entry of x is the per-feature CONSTANT -mean/std,
    not 0, and y keeps a per-feature offset and scale."""
    g = torch.Generator().manual_seed(seed)
    mean = torch.tensor([1.0, 0.0, 0.3, 0.1]) + 0.2 * torch.randn(4, generator=g)
    std = torch.tensor([0.05, 8.0, 1.2, 0.6]) * (1.0 + 0.2 * torch.rand(4, generator=g))
    raw_y = data.y * std + mean                                 # "physical" values whose z-score is data.y
    raw_x = raw_y * (1.0 - data.pred_mask.float())
    data.x = (raw_x - mean) / std                               # masked entries: -mean / std, per feature
    data.y = (raw_y - mean) / std
    return data


def test_config2_with_real_dataset_masked_entry_statistics():
    """The metric configuration with inputs shaped like the reference's normalised datasets (masked entries of x = the constant
    -mean/std per feature, datasets/PowerFlowData.py:126-139) instead of synth's zeros: forward and all gradients at 1e-5."""
    torch.manual_seed(1234)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.0).eval()
    m = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.0)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    data = _as_real_dataset(make_batch("118v2", 128, seed=3), seed=11)
    assert (data.x[data.pred_mask.bool()].abs() > 1e-3).any()
    _check_full_size(m, ref, data, "config 2, real-dataset masked-entry statistics")


def test_new_edge_index_tensor_is_rebuilt_on_the_device_without_a_host_sync():
    """A PyG-style loader hands out a NEW `edge_index` tensor per batch (train.py:90-92) although every sample of a case shares one
    topology.  Round 5 compared the new tensor with the cached list on the device and READ THE VERDICT BACK -- a host sync per batch
    (1.14 ms against 0.58 for the cached step).  Now a new tensor of the cached shape takes the sync-free path: adjacency rebuilt on
    the device, id-range / segment checks left there, the forward ends with pfn_graph_poison_if_bad.  Same bits as the validated
    build for the same content; other content of the same shape is simply another graph; a bad id becomes a NaN output (the first
    build of a shape still validates with a read-back and raises); and NOTHING in that path synchronises: it runs under
    torch's sync-debug mode and inside a stream capture."""
    torch.manual_seed(9)
    m = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.0).to(DEV).eval()
    d = make_batch("118v2", 16, seed=4).to(DEV)
    with torch.no_grad():
        out0 = m(d)
        g0 = m._graphs._graph
        assert not g0.unverified and m._graphs.device_rebuilds == 0
        d2 = d.clone()                                       # every tensor new, the same values
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out1 = m(d2)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        g1 = m._graphs._graph
        assert m._graphs.device_rebuilds == 1 and g1 is not g0 and g1.unverified and g1.seg_nodes == g0.seg_nodes == 118
        assert torch.equal(out0, out1)
        out1b = m(d2)                                        # ... and from then on the identity path
        assert m._graphs.device_rebuilds == 1 and m._graphs._graph is g1 and torch.equal(out0, out1b)
        # the same call inside a stream capture: a host sync would abort the capture
        d2c = d.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(d2c)                                           # (allocator warm-up on the capture stream)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        d2c.edge_index = d.edge_index.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outc = m(d2c)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(outc, out0)
        d3 = d.clone()
        d3.edge_index = d.edge_index.flip(0).contiguous()    # every edge reversed: other content, same shape
        out2 = m(d3)
        ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.0).eval()
        ref.load_state_dict(m.state_dict())
        assert_close(out2, ref(d3.to("cpu")), RTOL, "reversed edge list: out vs oracle")
        d4 = d.clone()
        d4.edge_index[0, 0] = d4.x.shape[0] + 3              # a bad id in a new tensor of the cached shape: NaN, not a plausible output
        assert torch.isnan(m(d4)).all()
        d5 = d.clone()
        d5.edge_index[1, 7] = (int(d5.edge_index[1, 7]) + 118) % d5.x.shape[0]   # an edge between two graphs of the batch: NaN as well
        assert torch.isnan(m(d5)).all()
    m2 = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.0).to(DEV).eval()
    with torch.no_grad(), pytest.raises(RuntimeError):       # the FIRST build of a shape is validated with a read-back
        m2(d4)


@pytest.mark.parametrize("dtype", [torch.int32, torch.bool, torch.uint8, torch.float32, torch.float64, torch.int16])
def test_pred_mask_dtypes_go_through_float(dtype):
    """`pred_mask` may arrive in any int / float dtype: the reference applies `.float()` (networks/MPN.py:533).  int64 takes the
    kernel's own conversion, everything else `.float()` first -- the output and every gradient carry the int64 run's bits."""
    torch.manual_seed(3)
    m = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.0).to(DEV).eval()
    d = make_batch("14", 9, seed=2).to(DEV)
    assert d.pred_mask.dtype == torch.int64
    out0 = m(d)
    torch.nn.MSELoss()(out0, d.y).backward()
    g0 = m.flat_grad().clone()
    m.zero_grad(set_to_none=True)
    d2 = d.clone()
    d2.pred_mask = d.pred_mask.to(dtype)
    out1 = m(d2)
    torch.nn.MSELoss()(out1, d2.y).backward()
    assert torch.equal(out0, out1) and torch.equal(g0, m.flat_grad())


def test_large_json_h512_case118_batch128_vs_oracle():
    """The reference's own configs/large.json (hidden_dim 512, n_gnn_layers 5, K 3; train.py:52-58 takes the width from the JSON)
    at the metric's batch: case118v2 x 128.  H = 512 = 16 quarters, no trailing column, K = 512 = four 136-k pieces per term:
    none of the H = 129-shaped fast paths apply (weights stream through LDS / split launches, generic edge walks); forward and all
    44 parameter gradients at 1e-5 against the oracle (see _check_full_size)."""
    torch.manual_seed(1234)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 512, 5, 3, 0.0).eval()
    m = MaskEmbdMultiMPN(4, 2, 4, 512, 5, 3, 0.0)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    _check_full_size(m, ref, make_batch("118v2", 128, seed=0), "large.json (H512 L5 K3), case118v2 x 128")


def test_config3_size_training_step_vs_oracle():
    """configs[2]'s size (case118v2 x 2048 = 241,664 nodes) as a TRAINING step: the persistent gemm_nt + two-workgroups-per-CU
    fused-hop path with its backward, forward and all parameter gradients against the oracle (see _check_full_size)."""
    torch.manual_seed(1234)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.0).eval()
    m = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.0)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    _check_full_size(m, ref, make_batch("118v2", 2048, seed=5), "config 3 size, training")
    assert m._graphs._graph.seg_nodes == 118


def test_wide_k6_large_batch_streaming_gemm_vs_oracle():
    """wide.json's K = 6 (what the reference's runs.sh pairs with 6470rte) at 135,936 rows: the 7-term TAGConv products (forward
    and input gradient) run on gemm_nt_ws_kernel -- full rows per wave, weights streamed through LDS -- with the rows beyond the
    last whole round on the stationary kernel.  Forward and all gradients against the oracle (see _check_full_size)."""
    torch.manual_seed(77)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 129, 3, 6, 0.0).eval()
    m = MaskEmbdMultiMPN(4, 2, 4, 129, 3, 6, 0.0)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    _check_full_size(m, ref, make_batch("118v2", 1152, seed=9), "K = 6, 1152 graphs")


def test_config3_inference_batch2048_properties():
    """configs[2]: case118v2 inference, batch 2048 (takes the LDS-resident hop path).  Graphs of the batch against the CPU
    oracle run on that graph alone (fp32 and float64), and against the same graph alone on the HIP path (a different kernel
    selection); the result is bitwise reproducible."""
    torch.manual_seed(1234)
    m = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.2).to(DEV).eval()
    big = make_batch("118v2", 2048, seed=5)
    bd = big.to(DEV)
    with torch.no_grad():
        out = m(bd)
        assert m._graphs._graph.seg_nodes == 118
        assert torch.equal(out, m(bd))
        assert torch.isfinite(out).all()
        ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.2).eval()
        ref.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
        ref64 = copy.deepcopy(ref).double()
        for gidx in (0, 1, 1023, 2047):
            single = make_batch("118v2", 1, seed=5, first=gidx)
            assert torch.equal(single.x, big.x[gidx * 118:(gidx + 1) * 118])
            rows = out[gidx * 118:(gidx + 1) * 118]
            # the CPU oracle on that graph alone (fp32 and float64) against its rows of the 2048-graph HIP batch
            assert_close(rows, ref(single), RTOL, f"graph {gidx} of the batch vs fp32 oracle")
            assert_close(rows, ref64(_to64(single)).float(), RTOL, f"graph {gidx} of the batch vs fp64 oracle")
            assert_close(m(single.to(DEV)), rows, RTOL, f"graph {gidx} alone on the HIP path")


@pytest.mark.parametrize("batch", [4, 300])
def test_inference_forward_equals_training_forward_bitwise(batch):
    """A forward under torch.no_grad() announces need_backward = 0: the edge walks save no ReLU masks and the front kernel does
    not store mask_embd's hidden layer.  The output must not change by a bit (row-per-wave front at 4 graphs, block front at
    300 graphs = 35,400 rows)."""
    torch.manual_seed(7)
    m = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.0).to(DEV).eval()
    b = make_batch("118v2", batch, seed=3).to(DEV)
    with torch.no_grad():
        o_inf = m(b)
    o_grad = m(b)
    assert o_grad.requires_grad and not o_inf.requires_grad
    assert torch.equal(o_inf, o_grad.detach())
    torch.nn.MSELoss()(o_grad, b.y).backward()           # and the training forward's backward still has what it needs
    assert all(torch.isfinite(p.grad).all() and p.grad.abs().max() > 0 for p in m.parameters())


@pytest.mark.parametrize("hub,B", [(0.0, 64), (0.2, 64), (0.0, 16), (0.2, 16)])
def test_config4_case6470_batch64_vs_oracle(hub, B):
    """configs[3]: case6470rte training batch 64 (and the high-degree 'hub' variant) at FULL size against the CPU oracle:
    forward (fp32 and float64 oracle) and all parameter gradients at 1e-5 (see _check_full_size); graphs of the batch against
    the oracle on that graph alone; permuting the stored edge order leaves the output unchanged up to summation order."""
    import psutil
    torch.manual_seed(1234)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.0).eval()
    m = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.0)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    # the float64 oracle with autograd needs ~1.2 GB per graph of the batch: the full-size cases SKIP (visibly) on a small host --
    # round 3 shrank the batch silently -- and the 16-graph case (same kernels, same regime) runs everywhere
    avail = psutil.virtual_memory().available
    if B == 64 and avail < 160e9:
        pytest.skip(f"config 4 at batch 64 needs ~160 GB of host memory for the float64 oracle ({avail / 1e9:.0f} GB available); "
                    "the batch-16 case covers the same kernels")
    big = make_batch("6470rte", B, seed=2, hub_frac=hub)
    _check_full_size(m, ref, big, f"config 4 (batch {B}, hub {hub})")
    bd = big.to(DEV)
    with torch.no_grad():
        out = m(bd)
        assert out.shape == (B * 6470, 4) and torch.isfinite(out).all()
        ref64 = copy.deepcopy(ref).double()
        for gidx in (0, B - 1):
            single = make_batch("6470rte", 1, seed=2, first=gidx, hub_frac=hub)
            rows = out[gidx * 6470:(gidx + 1) * 6470]
            assert_close(rows, ref(single), RTOL, f"graph {gidx} of the batch vs fp32 oracle")
            assert_close(rows, ref64(_to64(single)).float(), RTOL, f"graph {gidx} of the batch vs fp64 oracle")
            assert_close(m(single.to(DEV)), rows, RTOL, f"graph {gidx} alone on the HIP path")
        # edge-order permutation invariance (sums are re-ordered -> tolerance, not bitwise)
        perm = torch.randperm(big.edge_index.shape[1])
        pd = big.clone()
        pd.edge_index, pd.edge_attr = big.edge_index[:, perm].contiguous(), big.edge_attr[perm].contiguous()
        if bool(ref_cpu.is_directed(pd.edge_index)) == bool(ref_cpu.is_directed(big.edge_index)):
            assert_close(m(pd.to(DEV)), out, RTOL, "edge permutation")


def test_wide_json_on_case6470rte_vs_oracle():
    """configs[3]'s WIDE variant on the real grid (runs.sh:4-12 pairs configs/wide.json -- H 129, L 6, K 6 -- with case6470rte): until
    round 6 K = 6 was only compared with the oracle on 2,500-node graphs and on case118 batches.  Six 6470-bus
    graphs (38,820 rows): the 7-term TAGConv products, the chunk-major big-graph hops with six hops per direction, eleven layers of
    compounding error.  Forward (fp32 and float64 oracle) and all 76 parameter gradients at 1e-5 (see _check_full_size)."""
    torch.manual_seed(1234)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 129, 6, 6, 0.0).eval()
    m = MaskEmbdMultiMPN(4, 2, 4, 129, 6, 6, 0.0)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    data = make_batch("6470rte", 6, seed=3)
    _check_full_size(m, ref, data, "wide.json (H129 L6 K6) on case6470rte x 6")
    assert m._graphs._graph.seg_nodes == 6470


def test_mse_loss_handoff_stress():
    """pfn_mse_loss's last-arriver hand-off (write-through partial, drained, relaxed ticket; csrc/util_kernels.hip mse_kernel) under
    load: grids from 1 to 256 blocks, back to back with other work in flight on a second stream, 300 launches each -- every
    launch must return bit for bit the value of the first (a stale partial would change the sum) and the float64 mean to 1e-6."""
    from poweflownet_amd import _lib as L
    lib = L.load()
    ws = torch.zeros(1028 // 4 + 3, dtype=torch.float32, device=DEV)
    noise_stream = torch.cuda.Stream()
    big = torch.randn(1 << 24, device=DEV)
    for count in (7, 1024, 5000, 60_416, 262_144, 1_656_320):
        g = torch.Generator(device=DEV).manual_seed(count)
        o, y = torch.randn(count, device=DEV, generator=g), torch.randn(count, device=DEV, generator=g)
        loss = torch.empty(300, device=DEV)
        grad = torch.empty(count, device=DEV)
        with torch.cuda.stream(noise_stream):
            for _ in range(20):
                big.mul_(1.0001)                                   # uneven load on the memory system while the hand-offs run
        for i in range(300):
            L.check(lib.pfn_mse_loss(o.data_ptr(), y.data_ptr(), count, loss[i:].data_ptr(), grad.data_ptr(), ws.data_ptr(),
                                     ws.numel() * 4, L.stream_ptr()), "pfn_mse_loss")
        torch.cuda.synchronize()
        assert (loss == loss[0]).all(), (count, loss.unique())
        want = ((o.double() - y.double()) ** 2).mean().item()
        assert abs(loss[0].item() - want) <= 1e-6 * want, (count, loss[0].item(), want)
        assert_close(grad, (2.0 * (o.double() - y.double()) / count).float(), 1e-6, f"mse grad, count {count}")


def test_in_degree_above_65535_saved_masks():
    """A bus with more than 65,535 incoming edges (a star: 70,000 leaves -> one hub, undirected on device): the by-source half of
    the mask-reading backward walk finds an edge's ReLU byte through {ceil(in-degree / 4), position among the destination's
    incoming edges} -- two full ints (graph.hip graph_mask_index_kernel); packed into 16 + 16 bits it read the wrong byte here.
    Forward and all gradients against the oracle (the float64 one, on the HIP path's ReLU decisions)."""
    from poweflownet_amd.data import Data
    n = 70_001
    g = torch.Generator().manual_seed(3)
    ei = torch.stack([torch.arange(1, n), torch.zeros(n - 1, dtype=torch.long)])        # leaf -> hub, stored once
    bus_type = torch.full((n,), 2, dtype=torch.long)
    bus_type[::3] = 1
    bus_type[0] = 0
    mask = torch.tensor([[0, 0, 1, 1], [0, 1, 0, 1], [1, 1, 0, 0]])[bus_type]
    y = torch.randn(n, 4, generator=g)
    data = Data(x=y * (1 - mask).float(), y=y, bus_type=bus_type, pred_mask=mask, edge_index=ei,
                edge_attr=torch.randn(n - 1, 2, generator=g), batch=torch.zeros(n, dtype=torch.long))
    torch.manual_seed(21)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 16, 2, 2, 0.0).eval()
    m = MaskEmbdMultiMPN(4, 2, 4, 16, 2, 2, 0.0)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    dd = data.to(DEV)
    out = m(dd)
    assert m._graphs._graph.info() == (True, 2 * (n - 1))
    torch.nn.MSELoss()(out, dd.y).backward()
    # The hub row is a SEQUENTIAL fp32 sum of 70,000 messages in edge order -- here as in torch's scatter_add -- whose rounding
    # error (~sqrt(d) eps .. d eps) is far above 1e-5 for ANY fp32 implementation, and the hub dominates every gradient.  So the
    # yardstick is the float64 oracle on the HIP path's ReLU decisions, and the bound is 4x the error the fp32 ORACLE itself makes
    # against it on the same decisions (or 1e-5).  A wrong mask byte is not subtle: it moves dQ, hence every gradient, by O(1).
    gates = _cpu_gates(m)
    torch.set_num_threads(8)
    ref64 = copy.deepcopy(ref).double()
    ref32 = copy.deepcopy(ref)
    ref64.gates = ref32.gates = gates
    d64 = _to64(data)
    o64 = ref64(d64)
    torch.nn.MSELoss()(o64, d64.y).backward()
    o32 = ref32(data)
    torch.nn.MSELoss()(o32, data.y).backward()

    def check(what, ours, fp32, truth):
        e_ours, scale = rel_err(ours, truth)
        e_ref, _ = rel_err(fp32, truth)
        record(f"star graph: {what} vs fp64 oracle on the HIP gates (fp32 oracle: {e_ref / max(scale, 1e-300):.2e})", e_ours, scale, None)
        assert e_ours <= max(RTOL * scale, 4 * e_ref), (what, e_ours, e_ref, scale)
    check("out", out, o32, o64)
    for (k, p), q, t in zip(m.named_parameters(), ref32.parameters(), ref64.parameters()):
        check(f"grad.{k}", p.grad, q.grad, t.grad)


def opt_steps_counted(g):
    return int(g.opt.step_count[0].item())


@pytest.mark.parametrize("loss_kind", ["mse", "mixed_mse_power_imbalance"])
def test_graphed_train_step_with_a_new_topology_in_every_batch(tmp_path, loss_kind):
    """The reference's `perturbed` datasets (dataset_generator.py:250-253, utils/data_utils.py:12-59) give every SAMPLE its own
    line set: every batch brings a new edge_index.  GraphedTrainStep switches to its dynamic mode -- the adjacency build (device
    is_directed / undirect / CSRs / degrees / segment check) is captured INSIDE the step's hipGraph and replays from the copied-in
    edge_index -- and must (a) replay every full batch, (b) never synchronise with the host for the topology (pfn_graph_info /
    pfn_graph_segments are not called once the step is captured), (c) end on the parameters of the eager loop, which rebuilds
    and validates the adjacency per batch with a host sync like the reference (networks/MPN.py:498-504).
    `mixed_mse_power_imbalance`: a loss that walks the grid itself (PowerImbalance keeps its OWN adjacency per edge_index: with
    its cache a replayed loss walked the capture-time topology for ever -- ADVICE r03; the dynamic mode now rebuilds it inside the
    graph too).  Afterwards neither the model nor the loss is left in its unverified mode."""
    import numpy as np
    from poweflownet_amd import _lib as L
    from poweflownet_amd.data import DataLoader
    from poweflownet_amd.datasets import PowerFlowData
    from poweflownet_amd.loss import MSELoss
    from poweflownet_amd.optim import FlatAdamW
    from poweflownet_amd.synth import make_topology
    from poweflownet_amd.utils.training import GraphedTrainStep, train_epoch
    rng = np.random.default_rng(5)
    S, n, e = 96, 118, 186
    node = np.zeros((S, n, 6))
    node[:, :, 0] = np.arange(n)
    node[:, :, 1] = np.where(np.arange(n) == 0, 0, np.where(np.arange(n) % 3 == 0, 1, 2))
    node[:, :, 2:] = rng.normal(size=(S, n, 4))
    edge = np.zeros((S, e, 4))
    for s_ in range(S):
        edge[s_, :, :2] = make_topology(n, e, seed=100 + s_).numpy().T          # every sample: its own spanning tree + chords
    edge[:, :, 2:] = np.abs(rng.normal(size=(S, e, 2))) * 0.1 + 0.01
    (tmp_path / "raw").mkdir()
    np.save(tmp_path / "raw" / "case118_edge_features.npy", edge)
    np.save(tmp_path / "raw" / "case118_node_features.npy", node)
    ds = PowerFlowData(root=str(tmp_path), case="118", split=[.5, .25, .25], task="train", device=DEV)      # 48 samples
    assert not ds._blocks[0].static_topology

    lib = L.load()
    calls = {"info": 0, "segments": 0}
    real_info, real_seg = lib.pfn_graph_info, lib.pfn_graph_segments

    from poweflownet_amd.utils.custom_loss_functions import MixedMSEPoweImbalance

    def make_loss():
        if loss_kind == "mse":
            return MSELoss()
        return MixedMSEPoweImbalance(*[t.cpu() for t in ds.get_data_means_stds()], alpha=0.9)

    def run(graphed):
        torch.manual_seed(5)
        m = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.0).to(DEV)
        opt = FlatAdamW(m, lr=1e-3)
        loss_fn = make_loss()
        g = GraphedTrainStep(m, loss_fn, opt) if graphed else None
        losses = []
        for epoch in range(3):
            loader = DataLoader(ds, batch_size=16, shuffle=True, generator=torch.Generator().manual_seed(epoch))   # 3 x 16
            if graphed and epoch == 1:          # captured by now (first batch eager-captured static, second switched to dynamic)
                assert g.dynamic and g.graph is not None and not g.disabled

                def count_info(*a):
                    calls["info"] += 1
                    return real_info(*a)

                def count_seg(*a):
                    calls["segments"] += 1
                    return real_seg(*a)
                lib.pfn_graph_info, lib.pfn_graph_segments = count_info, count_seg
            losses.append(train_epoch(m, loader, loss_fn, opt, DEV, graph=g))
        lib.pfn_graph_info, lib.pfn_graph_segments = real_info, real_seg
        assert not m.dynamic_topology and not any(getattr(x, "dynamic_topology", False) for x in loss_fn.modules())
        return losses, opt.flat_param.detach().clone(), g

    try:
        l_g, p_g, g = run(True)
    finally:
        lib.pfn_graph_info, lib.pfn_graph_segments = real_info, real_seg
    assert calls == {"info": 0, "segments": 0}, calls            # no topology read-back in two epochs of per-batch topologies
    assert g.graph.mode == "one graph"
    l_e, p_e, _ = run(False)
    for a, b in zip(l_e, l_g):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), (l_e, l_g)
    assert_close(p_g, p_e, 1e-6, "parameters after 3 epochs of per-batch topologies")
    assert opt_steps_counted(g) == 9                            # (the guarded update skipped nothing: every batch was sound)


def test_dynamic_topology_bad_batches_give_nan_not_garbage():
    """With the checks left on the device (model.dynamic_topology: no host sync) a node id outside [0, N) or a `ptr` hint the
    edges contradict cannot raise -- the forward ends with pfn_graph_poison_if_bad, so the output (hence the loss) is NaN.  The
    default mode raises for the same inputs (test_graph_rejects_out_of_range_ids) or rejects the hint."""
    torch.manual_seed(2)
    m = MaskEmbdMultiMPN(4, 2, 4, 32, 2, 2, 0.0).to(DEV).eval()
    m.dynamic_topology = True
    good = make_batch("14", 5).to(DEV)
    with torch.no_grad():
        ok = m(good)
        assert torch.isfinite(ok).all() and m._graphs._graph.unverified and m._graphs._graph.seg_nodes == 14
        bad = good.clone()
        bad.edge_index = good.edge_index.clone()
        bad.edge_index[0, 3] = 70                              # one id past the last node
        assert torch.isnan(m(bad)).all()
        cross = good.clone()
        cross.edge_index = good.edge_index.clone()
        cross.edge_index[1, 0] = 20                            # an edge from graph 0 into graph 1: the ptr hint is wrong
        assert torch.isnan(m(cross)).all()
        m.dynamic_topology = False
        assert_close(m(good), ok, 1e-6, "same batch, validated build")


def test_guarded_adamw_step_skips_a_poisoned_batch():
    """`pfn_adamw_step_guarded` (FlatAdamW.guard): the captured step of a per-batch-topology run cannot raise for a bad batch, the
    batch arrives as a NaN loss -- the update is then skipped ON THE DEVICE (parameters, moments and step counter untouched) instead
    of turning every parameter NaN for good; with a finite loss it is the plain update, bit for bit."""
    from poweflownet_amd.optim import FlatAdamW
    torch.manual_seed(4)
    m = MaskEmbdMultiMPN(4, 2, 4, 32, 2, 2, 0.0).to(DEV)
    m2 = copy.deepcopy(m)
    d = make_batch("14", 6, seed=1).to(DEV)
    o1, o2 = FlatAdamW(m, lr=1e-2), FlatAdamW(m2, lr=1e-2)
    for guard_value, expect_step in ((1.25, True), (float("nan"), False), (float("inf"), False), (0.5, True)):
        for mm, oo in ((m, o1), (m2, o2)):
            oo.zero_grad(set_to_none=True)
            torch.nn.MSELoss()(mm(d), d.y).backward()
        before = o1.flat_param.clone()
        o1.guard = torch.tensor(guard_value, device=DEV)
        o1.step()
        o1.guard = None
        if expect_step:
            o2.step()
            assert torch.equal(o1.flat_param, o2.flat_param) and torch.equal(o1.exp_avg_sq, o2.exp_avg_sq)
        else:
            assert torch.equal(o1.flat_param, before) and torch.isfinite(o1.flat_param).all()
        assert int(o1.step_count[0].item()) == int(o2.step_count[0].item()) and int(o1.step_count[1].item()) == 0


def test_big_graph_hops_with_unequal_edge_counts():
    """Graphs too large for the two-tile LDS hop kernel (2,500 nodes) take big_graph_hops_kernel (one LDS tile + registers per graph
    and column chunk, hop outputs chunk-major, read back by gemm_nt / gemm_tn through GemmTerm::cm_rows / TnPair::b_cm_rows).  The
    staged 16-bit neighbour list is sized for an EQUAL share of the edges per graph; here the first graph has three times the edges
    of the others, so its blocks read their indices from global memory instead.  Forward and all gradients against the oracle."""
    from poweflownet_amd.data import Batch
    from poweflownet_amd.synth import make_graph, make_topology
    torch.manual_seed(8)
    n = 2500
    graphs = [make_graph(n, e, seed=40 + i, edge_index=make_topology(n, e, seed=7 + i)) for i, e in enumerate((9000, 3000, 3000))]
    data = Batch.from_data_list(graphs)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 16, 3, 3, 0.0).eval()
    m = MaskEmbdMultiMPN(4, 2, 4, 16, 3, 3, 0.0)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    dd = data.to(DEV)
    out = m(dd)
    assert m._graphs._graph.seg_nodes == n
    torch.nn.MSELoss()(out, dd.y).backward()
    with torch.no_grad():
        assert_close(out, ref(data), RTOL, "big-graph hops: out vs fp32 oracle")
    _assert_grads_on_hip_gates(m, ref, data, "big-graph hops, unequal edge counts", out)


def test_big_graph_hops_one_workgroup_per_graph_walks_every_chunk():
    """big_graph_hops_kernel's workgroups are persistent over the column chunks of ONE graph; the launcher deals `CUs / graphs`
    workgroups to a graph.  With more graphs than a third of the CUs a single workgroup walks ALL chunks of its graph (H = 20: five
    chunks, the last one partly padding), in more than one round of the chip -- and 139 graphs leave 5 idle workgroups in the last
    group of eight.  Forward and all gradients against the oracle (K = 2 and the K = 1 edge case: no tile refill at all)."""
    from poweflownet_amd.data import Batch
    from poweflownet_amd.synth import make_graph, make_topology
    n, e = 2500, 3400
    topo = make_topology(n, e, seed=11)
    data = Batch.from_data_list([make_graph(n, e, seed=60 + i, edge_index=topo) for i in range(139)])
    for K in (2, 1):
        torch.manual_seed(9 + K)
        ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 20, 2, K, 0.0).eval()
        m = MaskEmbdMultiMPN(4, 2, 4, 20, 2, K, 0.0)
        m.load_state_dict(ref.state_dict())
        m = m.to(DEV).eval()
        dd = data.to(DEV)
        out = m(dd)
        assert m._graphs._graph.seg_nodes == n
        torch.nn.MSELoss()(out, dd.y).backward()
        with torch.no_grad():
            assert_close(out, ref(data), RTOL, f"big-graph hops, 139 graphs, K={K}: out vs fp32 oracle")
        _assert_grads_on_hip_gates(m, ref, data, f"big-graph hops, one workgroup per graph, K={K}", out)


def test_rows_kernels_with_unequal_edge_counts(tmp_path):
    """Big inference batches of small graphs take the whole-rows LDS kernels (row_hops_kernel, edge_rows_fwd_kernel -- the first
    layer's launch forming P | Q from x0).  Their staged adjacency / attribute lists are sized for an EQUAL share of the edges per
    graph; here ten of 2,100 fifty-bus graphs have four times the edges of the others, so the blocks that hold them read indices
    and attributes from global memory instead.  Against the generic kernels (PFN_NO_ROW_HOPS=1 PFN_NO_EDGE_ROWS=1; switches are
    read once per process -> child processes) on the whole batch, and against the CPU oracle on the first (heavy) graph alone."""
    import os
    import subprocess
    import sys
    from poweflownet_amd.synth import make_graph, make_topology
    script = f"""
import sys, torch
sys.path.insert(0, {repr(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))})
from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
from poweflownet_amd.data import Batch
from poweflownet_amd.synth import make_graph, make_topology
torch.manual_seed(11)
m = MaskEmbdMultiMPN(4, 2, 4, 129, 3, 3, 0.0).to("cuda:0").eval()
n = 50
graphs = [make_graph(n, 240 if i < 10 else 60, seed=300 + i, edge_index=make_topology(n, 240 if i < 10 else 60, seed=900 + i)) for i in range(2100)]
d = Batch.from_data_list(graphs).to("cuda:0")
with torch.no_grad():
    out = m(d)
assert m._graphs._graph.seg_nodes == n
torch.save({{"out": out.cpu(), "state": {{k: v.cpu() for k, v in m.state_dict().items()}}}}, sys.argv[1])
"""
    res = {}
    for tag, env in (("rows", {}), ("generic", {"PFN_NO_ROW_HOPS": "1", "PFN_NO_EDGE_ROWS": "1"})):
        path = str(tmp_path / f"{tag}.pt")
        subprocess.run([sys.executable, "-c", script, path], check=True, env=dict(os.environ, **env), timeout=600)
        res[tag] = torch.load(path)
    assert_close(res["rows"]["out"], res["generic"]["out"], RTOL, "whole-rows LDS kernels vs generic kernels, unequal edge counts")
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 129, 3, 3, 0.0).eval()
    ref.load_state_dict(res["rows"]["state"])
    g0 = make_graph(50, 240, seed=300, edge_index=make_topology(50, 240, seed=900))
    with torch.no_grad():
        assert_close(res["rows"]["out"][:50], ref(g0), RTOL, "heavy graph 0 of the batch vs the CPU oracle on that graph alone")


def test_k6_big_graphs_streaming_gemm_reads_chunk_major_hops():
    """K = 6 on 56 graphs of 2,500 nodes (140,000 rows): the hops run in big_graph_hops_kernel and come out CHUNK-major; the
    7-term TAGConv products then take gemm_nt_ws_kernel (weight streaming, whole rounds) plus the stationary kernel on the tail rows,
    both reading six of their seven A operands through GemmTerm::cm_rows, and gemm_tn reads them as B operands through
    TnPair::b_cm_rows.  Forward and all gradients against the oracle, eval mode and train mode (dropout masks exported)."""
    from poweflownet_amd.data import Batch
    from poweflownet_amd.synth import make_graph, make_topology
    torch.manual_seed(12)
    n, e, B = 2500, 3400, 56
    topo = make_topology(n, e, seed=3)
    data = Batch.from_data_list([make_graph(n, e, seed=500 + i, edge_index=topo) for i in range(B)])
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 129, 2, 6, 0.0).eval()
    m = MaskEmbdMultiMPN(4, 2, 4, 129, 2, 6, 0.0)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    _check_full_size(m, ref, data, "K = 6, 56 graphs of 2,500 nodes")
    assert m._graphs._graph.seg_nodes == n
    # train mode: the tail launch's dropout counter continues at the global row
    p = 0.2
    ref2 = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 129, 2, 6, p).train()
    ref2.load_state_dict(ref.state_dict())
    m2 = MaskEmbdMultiMPN(4, 2, 4, 129, 2, 6, p)
    m2.load_state_dict(ref.state_dict())
    m2 = m2.to(DEV).train()
    m2.seed_dropout(99)
    dd = data.to(DEV)
    out = m2(dd)
    torch.nn.MSELoss()(out, dd.y).backward()
    ref2.dropout_masks = [k.cpu() for k in _exported_masks(m2, dd.x.shape[0])]
    _assert_grads_on_hip_gates(m2, ref2, data, "K = 6 big graphs, train mode", out)
