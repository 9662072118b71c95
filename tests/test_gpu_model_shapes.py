"""The whole model against the oracle at every feature width it accepts.

csrc/model.hip (make_route, ea_forward, ea_backward) chooses kernels on `efeature_dim == 2`, `output_dim == 4`, `output_dim <= 4` and
`K > 0`; tests/test_gpu_boundaries.py pins the SIZE thresholds for MaskEmbdMultiMPN(4, 2, 4, ...) only.  Here the size regimes are
few and the widths vary: MaskEmbdMultiMPN(4, fe, fo, H, L, K) for fe 1..6, fo 1..200, H 3..129, K 0..3 in four regimes --

  R1  graph-resident: 14-node grids x 6 with `ptr` (ea_seg_fwd / ea_seg_bwd, front_seg_fwd, seg_lin_hops at H = 129);
  R2  the generic walks and hop_norm: the R1 batch without `ptr` (no segment hint);
  R3  generic EdgeAggregation with fused hops: 129-node grids x 2 with `ptr` (one node past SG_MAX_ROWS);
  R4  one row past WAVE_MAX_ROWS: 14-node grids x 2,341 = 32,774 rows at H = 16 (no lin_out4, the block front).

A cell's batch is tests/test_gpu_boundaries._batch with edge_attr = randn(E, fe) and y = randn(N, fo).  Every cell checks the output
shape, the forward against the fp32 and the fp64 oracle, every parameter gradient of MSELoss against the fp32 oracle (below 2,000
rows) and against the fp64 oracle on the HIP path's own ReLU decisions, that a second identical step gives the same bits, and the
profile classes against tests/regimes.model_regime(fo=, gea=).

What the cells reach that nothing else does: lin_out4_wave_kernel, edge_fwd_out_kernel's output Linear, edge_bwd's ds_row and the
last-layer form of ea_seg_bwd_kernel with fo < 4; gemm_nt with N = fo and the non-last form of ea_seg_bwd_kernel with K = fo and
ldgo != ld for fo > 4 (fo = 129..136: the async-fragment form); fo = 137 and 200, which the graph-resident backward must refuse
(its dS product is one 136-k piece: Route::ea_seg_bwd, ea_seg_bwd_out_ok) -- R1 then pairs the graph-resident forward with the
generic backward; fe = 4, 5, 6; K = 0 (HOPS_NONE, the K == 0 branch of tag_backward).

Tolerance: tests/util.RTOL = 1e-5 normwise, no exclusions.  The oracle alone, fp32 against fp64 on the CPU, differs by at most
4.7e-7 (forward) and 8.7e-7 (any gradient) on 13 of these cells (fe 1..6, fo 1..130, K = 0 among them): more than 10x inside.
Worst error achieved on an MI355X (parity_report.json, 49 cells): forward 7.2e-7 ((2, 1, 129, 2, 3) in R3), any gradient 1.9e-6
(grad mask_embd.0.weight of (4, 4, 64, 3, 2) in R1) of the tensor's largest entry.
"""
import copy
import os

import pytest
import torch

from oracle import ref_cpu
from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
from tests import regimes as R
from tests.test_gpu_boundaries import _batch as _usual_batch
from tests.test_gpu_boundaries import _check_classes, _cus, _profiled
from tests.util import (RTOL, _assert_grads_on_hip_gates, _cpu_gates, _exported_masks, _fp64_truth, _run, _to64, assert_close)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# regime -> (nodes per graph, graphs, carries `ptr`)
REGIMES = {"R1": (14, 6, True), "R2": (14, 6, False), "R3": (129, 2, True), "R4": (14, 2341, True)}


def _cell_batch(regime, fe, fo, seed):
    seg, B, with_ptr = REGIMES[regime]
    d = _usual_batch(seg, B, seed)
    g = torch.Generator().manual_seed(7919 * seed + 13)
    d.edge_attr = torch.randn(d.edge_index.shape[1], fe, generator=g)
    d.y = torch.randn(d.x.shape[0], fo, generator=g)
    if not with_ptr:
        del d.__dict__["ptr"]
        d._keys.remove("ptr")
    return d, (seg if with_ptr else 0)


def _models(fe, fo, H, L_, K, p, seed):
    torch.manual_seed(seed)
    ref = ref_cpu.MaskEmbdMultiMPN(4, fe, fo, H, L_, K, p)
    with torch.no_grad():
        for mod in ref.layers:
            if hasattr(mod, "lins"):
                mod.bias.normal_(std=0.1)              # TAGConv bias is zero-initialised: exercise it
    m = MaskEmbdMultiMPN(4, fe, fo, H, L_, K, p)
    m.load_state_dict(ref.state_dict())
    return ref, m.to(DEV)


def _cell(fe, fo, H, L_, K, regime, p=0.0, train=True, input_grads=False, seed=None):
    """One cell (see the module docstring).  `input_grads`: the step also asks for the gradients of x and edge_attr (the
    edge-attribute gradient forces the recomputing generic backward walks and the dS GEMM with K = fo), held to the same oracles."""
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    seed = (fe * 1000 + fo * 7 + H + 31 * K) if seed is None else seed
    what = f"({fe}, {fo}, {H}, {L_}, {K}) {regime}{' train p=%g' % p if p else ''}{'' if train else ' inference'}{' +input grads' if input_grads else ''}"
    ref, m = _models(fe, fo, H, L_, K, p, seed)
    data, seg = _cell_batch(regime, fe, fo, seed)
    n = data.x.shape[0]
    reg = R.model_regime(n, seg, H, L_, K, fe, train, _cus(), fo=fo, gea=input_grads)
    dd = data.to(DEV)
    if input_grads:
        dd.x = dd.x.detach().requires_grad_(True)
        dd.edge_attr = dd.edge_attr.detach().requires_grad_(True)
    m.train(p > 0)
    ref.train(p > 0)

    def step():
        m.seed_dropout(1000 + seed)
        m.zero_grad(set_to_none=True)
        if not train:
            with torch.no_grad():
                return m(dd)
        dd.x.grad = dd.edge_attr.grad = None
        out = m(dd)
        torch.nn.MSELoss()(out, dd.y).backward()
        return out
    out, launches = _profiled(step)
    assert m._graphs._graph.seg_nodes == seg, (what, m._graphs._graph.seg_nodes)
    assert tuple(out.shape) == (n, fo) and out.dtype == torch.float32, (what, tuple(out.shape))
    _check_classes(launches, reg["must"], reg["must_not"], what)
    if p > 0:
        ref.dropout_masks = [k.cpu() for k in _exported_masks(m, n)]
    if input_grads:
        data.x.requires_grad_(True)
        data.edge_attr.requires_grad_(True)
    if train:
        out_ref = ref(data)
        torch.nn.MSELoss()(out_ref, data.y).backward()
    else:
        with torch.no_grad():
            out_ref = ref(data)
    out64, _ = _fp64_truth(ref, data)
    assert_close(out, out_ref, RTOL, f"{what}: out")
    assert_close(out, out64.float(), RTOL, f"{what}: out vs fp64")
    first = {"out": out.detach().clone()}
    if train:
        first["g"] = m.flat_grad().clone()
        if n <= 2000:                                   # small: the plain fp32 oracle, no gate equalisation needed
            for (k, q_), q in zip(m.named_parameters(), ref.parameters()):
                assert_close(q_.grad, q.grad, RTOL, f"{what}: grad.{k}")
            if input_grads:
                assert_close(dd.x.grad, data.x.grad, RTOL, f"{what}: grad x")
                assert_close(dd.edge_attr.grad, data.edge_attr.grad, RTOL, f"{what}: grad edge_attr")
        gates = _cpu_gates(m)
        if input_grads:                                 # (the oracle's fp32 input gradients are compared: cut its inputs loose)
            data.x, data.edge_attr = data.x.detach(), data.edge_attr.detach()
        _assert_grads_on_hip_gates(m, ref, data, what, out, gates)
        if input_grads:
            first["gx"], first["gea"] = dd.x.grad.clone(), dd.edge_attr.grad.clone()
            ref64 = copy.deepcopy(ref).double()
            ref64.zero_grad(set_to_none=True)
            ref64.gates = gates
            d64 = _to64(data.clone())
            d64.x = d64.x.detach().requires_grad_(True)
            d64.edge_attr = d64.edge_attr.detach().requires_grad_(True)
            torch.nn.MSELoss()(ref64(d64), d64.y).backward()
            assert_close(dd.x.grad, d64.x.grad.float(), RTOL, f"{what}: grad x vs fp64 oracle on the HIP gates")
            assert_close(dd.edge_attr.grad, d64.edge_attr.grad.float(), RTOL, f"{what}: grad edge_attr vs fp64 oracle on the HIP gates")
    # a second identical step: the same bits (ordered reductions everywhere, the dropout stream re-seeded)
    out2 = step()
    torch.cuda.synchronize()
    assert torch.equal(out2, first["out"]), f"{what}: the second step's output differs"
    if train:
        assert torch.equal(m.flat_grad(), first["g"]), f"{what}: the second step's parameter gradients differ"
        if input_grads:
            assert torch.equal(dd.x.grad, first["gx"]) and torch.equal(dd.edge_attr.grad, first["gea"]), f"{what}: input gradients differ"
    return reg, launches


# ------------------------------------------------------------------------------------------ narrow output
@pytest.mark.parametrize("regime", ["R1", "R2", "R3"])
@pytest.mark.parametrize("fo", [1, 2, 3])
def test_narrow_output_across_regimes(fo, regime):
    """fo < 4 at H = 129: lin_out4 behind the graph-resident walk and the last-layer form of ea_seg_bwd_kernel (R1); the output
    Linear inside edge_fwd_out_kernel and the dS rows formed in the generic backward walks (R2, R3)."""
    reg, launches = _cell(2, fo, 129, 2, 3, regime)
    assert reg["ea_seg_fwd"] == (regime == "R1") and reg["ea_seg_bwd"] == (regime == "R1")
    assert ("lin_out4" in launches) == (regime == "R1") and reg["out_in_walk"] == (regime != "R1")
    assert reg["hops"] == ("generic" if regime == "R2" else "fused")


def test_narrow_output_one_row_past_the_wave_kernels():
    """32,774 rows at H = 16: no lin_out4 and no front_seg_fwd (the block front), while the 261 row blocks still run the
    EdgeAggregation layers graph-resident -- so gemm_nt forms the output with N = 3."""
    reg, launches = _cell(2, 3, 16, 2, 1, "R4")
    assert not reg["lin_out4"] and not reg["front_latency"] and not reg["seg_front"] and "lin_out4" not in launches
    assert reg["out_in_walk"] == (not reg["ea_seg_fwd"])
    if reg["ea_seg_fwd"]:
        assert launches.get("gemm_nt", 0) > 0 and launches.get("ea_seg_fwd", 0) > 0


# ------------------------------------------------------------------------------------------ wide output
@pytest.mark.parametrize("regime", ["R1", "R2"])
@pytest.mark.parametrize("fo", [5, 8, 129, 136, 137, 200])
def test_wide_output_on_the_graph_resident_backward_and_past_it(fo, regime):
    """fo > 4: gemm_nt forms the output (N = fo); in R1 the last layer's backward is the NON-last form of ea_seg_bwd_kernel with
    K = fo and ldgo = ld_of(fo) != ld -- fo = 129 and 136 give K8 = 136, the async-fragment form -- up to fo = 136.  fo = 137 and
    200 are more than its one k piece: make_route sends the whole backward down the generic walks (edge_bwd, no ea_seg_bwd)
    while the forward stays graph-resident."""
    reg, launches = _cell(2, fo, 129, 2, 3, regime)
    assert reg["ea_seg_fwd"] == (regime == "R1") and not reg["lin_out4"] and not reg["out_in_walk"]
    assert reg["ea_seg_bwd"] == (regime == "R1" and fo <= 136)
    if regime == "R1":
        assert launches.get("ea_seg_fwd", 0) > 0
        if fo <= 136:
            assert launches.get("ea_seg_bwd", 0) > 0 and "edge_bwd" not in launches, launches
        else:
            assert launches.get("edge_bwd", 0) > 0 and "ea_seg_bwd" not in launches, launches


def test_wide_output_async_fragment_at_another_hidden_width():
    """fo = 130 (K8 = 136, lda = ldgo = 132) over H = 65 (two quarters + one trailing column)."""
    reg, launches = _cell(2, 130, 65, 2, 1, "R1")
    assert reg["ea_seg_bwd"] and launches.get("ea_seg_bwd", 0) > 0


# ------------------------------------------------------------------------------------------ edge widths
@pytest.mark.parametrize("fe,regime", [(1, "R1"), (3, "R1"), (4, "R1"), (5, "R1"), (6, "R1"), (1, "R2"), (6, "R2"), (1, "R3"), (6, "R3")])
def test_edge_feature_widths(fe, regime):
    """efeature_dim != 2: the runtime-width generic walks in every regime (nothing graph-resident, no ReLU masks)."""
    reg, launches = _cell(fe, 4, 64, 3, 2, regime)
    assert not reg["ea_seg_fwd"] and not reg["ea_seg_bwd"] and not reg["seg_front"] and not reg["out_in_walk"]
    assert reg["lin_out4"] and launches.get("lin_out4", 0) > 0


@pytest.mark.parametrize("fo", [3, 5])
def test_edge_feature_width_3_with_other_output_widths(fo):
    reg, launches = _cell(3, fo, 64, 3, 2, "R1")
    assert ("lin_out4" in launches) == (fo == 3) and not reg["out_in_walk"]


@pytest.mark.parametrize("train", [False, True])
def test_edge_feature_width_3_one_row_past_the_wave_kernels(train):
    """32,774 rows, fe = 3: no lin_out4 (rows) and no edge_fwd_out_kernel (fe), so gemm_nt forms the 4-wide output."""
    reg, launches = _cell(3, 4, 16, 2, 1, "R4", train=train)
    assert not reg["lin_out4"] and not reg["out_in_walk"] and "lin_out4" not in launches and launches.get("gemm_nt", 0) > 0


# ------------------------------------------------------------------------------------------ small hidden widths
@pytest.mark.parametrize("H", [3, 7, 33])
def test_small_hidden_widths(H):
    """H = 3 (ld 4: no 32-column quarter, so nothing graph-resident), 7 (ld 8: one quarter, K8 = 8), 33 (a quarter + one trailing
    column), with fo = 3."""
    reg, launches = _cell(2, 3, H, 3, 2, "R1")
    assert reg["ny"] == (0 if H == 3 else 1)
    assert reg["ea_seg_fwd"] == (H != 3) and reg["ea_seg_bwd"] == (H != 3)
    if H == 3:
        assert "ea_seg_fwd" not in launches and "ea_seg_bwd" not in launches and "front_seg_fwd+pack" not in launches


# ------------------------------------------------------------------------------------------ gradients of x and edge_attr
@pytest.mark.parametrize("fe,fo,H,L_,K,regime", [(2, 3, 129, 2, 3, "R1"), (2, 3, 129, 2, 3, "R2"), (2, 5, 129, 2, 3, "R1"),
                                                 (2, 5, 129, 2, 3, "R2"), (3, 4, 64, 3, 2, "R1")])
def test_input_and_edge_attribute_gradients(fe, fo, H, L_, K, regime):
    """An edge-attribute gradient takes the recomputing generic backward walks whatever the forward ran (after a graph-resident
    forward with saved gates P | Q are written first), and with them the dS GEMM with K = fo."""
    reg, launches = _cell(fe, fo, H, L_, K, regime, input_grads=True)
    assert not reg["ea_seg_bwd"] and launches.get("edge_bwd", 0) > 0 and "ea_seg_bwd" not in launches


# ------------------------------------------------------------------------------------------ dropout
def test_train_mode_with_dropout_at_other_widths():
    """Train mode, p = 0.2, at (3, 3, 64, 3, 2): against the oracle fed the exported keep masks."""
    _cell(3, 3, 64, 3, 2, "R1", p=0.2)


# ------------------------------------------------------------------------------------------ K = 0
@pytest.mark.parametrize("fe,fo,H,L_,regime", [(2, 4, 129, 2, "R1"), (2, 4, 129, 2, "R2"), (2, 4, 7, 3, "R1"), (3, 3, 33, 3, "R2")])
def test_tagconv_without_hops_in_the_whole_model(fe, fo, H, L_, regime):
    """K = 0 (HOPS_NONE): a TAGConv is its k = 0 product alone; its backward is the K == 0 branch of tag_backward (one gated GEMM)."""
    reg, launches = _cell(fe, fo, H, L_, 0, regime)
    assert reg["hops"] is None and not reg["slh"]
    for k in ("hop_norm", "fused_hops_fwd", "fused_hops_bwd", "seg_lin_hops_fwd", "seg_lin_hops_bwd"):
        assert k not in launches, (k, launches)


# ------------------------------------------------------------------------------------------ loss plumbing at fo != 4
@pytest.mark.parametrize("fo", [3, 5])
def test_attached_mse_is_transparent_at_other_output_widths(fo):
    """MSELoss.attach on a model with output_dim != 4, in the regime where the tail would otherwise run: the announcement is
    consumed, the plain path runs -- the same launches and the same bits, no ea_seg_bwd+out+mse."""
    from poweflownet_amd.loss import MSELoss
    _, m = _models(2, fo, 129, 2, 3, 0.2, 40 + fo)
    m.train()
    data, seg = _cell_batch("R1", 2, fo, 40 + fo)
    assert not R.mse_tail_available(True, data.x.shape[0], 129, 2, 2, seg, _cus(), fo=fo)
    assert R.mse_tail_available(True, data.x.shape[0], 129, 2, 2, seg, _cus(), fo=4)
    d = data.to(DEV)
    loss_fn = MSELoss()
    plain = _run(m, d, loss_fn, attach=False, x_grad=True)
    fused = _run(m, d, loss_fn, attach=True, x_grad=True)
    assert m._mse_attach is None
    assert "ea_seg_bwd+out+mse" not in fused["launches"] and fused["launches"] == plain["launches"], (fused["launches"], plain["launches"])
    assert tuple(fused["out"].shape) == (data.x.shape[0], fo) and torch.isfinite(fused["out"]).all()
    for k in ("out", "loss", "g", "gx"):
        assert torch.equal(fused[k], plain[k]), k


def test_graphed_train_step_matches_the_eager_loop_at_other_widths():
    """GraphedTrainStep at (3, 3, 64, 3, 2) with dropout 0.2: three replayed AdamW steps land on the parameters of the same three
    steps run call by call, bit for bit."""
    from poweflownet_amd.loss import MSELoss
    from poweflownet_amd.optim import FlatAdamW
    from poweflownet_amd.utils.training import GraphedTrainStep
    data, _ = _cell_batch("R1", 3, 3, 77)
    d = data.to(DEV)
    finals, losses = [], []
    for graphed in (True, False):
        _, m = _models(3, 3, 64, 3, 2, 0.2, 11)
        m.train()
        m.seed_dropout(5)
        opt = FlatAdamW(m, lr=1e-3)
        loss_fn = MSELoss()
        step = GraphedTrainStep(m, loss_fn, opt) if graphed else None
        ls = []
        for _ in range(3):
            if graphed:
                ls.append(step(d).item())
            else:
                opt.zero_grad()
                loss = loss_fn(m(d), d.y)
                loss.backward(loss_fn.unit_grad(loss))
                opt.step()
                ls.append(loss.item())
        if graphed:
            assert step.graph is not None and not step.disabled
        finals.append(opt.flat_param.detach().clone())
        losses.append(ls)
    assert torch.isfinite(finals[0]).all()
    assert torch.equal(finals[0], finals[1]), (finals[0] - finals[1]).abs().max().item()
    for a, b in zip(*losses):
        assert abs(a - b) <= 2e-6 * abs(b), (a, b)
