"""`GraphedEvalStep` / `evaluate_epoch(graph=)` / `evaluate_epoch_v2(graph=)` / `evaluate_report` (utils/evaluation.py): an
evaluation epoch replayed from one hipGraph per batch size is held to FLOAT EQUALITY with the eager loop -- which in turn is held to
the host arithmetic of the loop it replaces (`loss.item() * len(data)` per batch) -- and the one-pass report to float64 formulas
applied to the eager model's own fp32 outputs.  Sets: case 14 (14 buses, 20 branches) written by tools/make_raw_dataset.py; the
validation split holds 22 samples, batches of 8, 8 and 6."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from poweflownet_amd.data import DataLoader
from poweflownet_amd.datasets import PowerFlowData, denormalize
from poweflownet_amd.loss import MSELoss
from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
from poweflownet_amd.optim import FlatAdamW
from poweflownet_amd.synth import make_topology
from poweflownet_amd.utils.custom_loss_functions import Masked_L2_loss, MaskedL1, MaskedL2V2, PowerImbalance
from poweflownet_amd.utils.evaluation import (GraphedEvalStep, evaluate_epoch, evaluate_epoch_v2, evaluate_report, report_keys)
from poweflownet_amd.utils.training import GraphedTrainStep, train_epoch
from tests.test_segpack_host import _mixed_root
from tests.util import RTOL, record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    root = tmp_path_factory.mktemp("case14")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_raw_dataset.py"), "--root", str(root), "--case", "14",
                    "--samples", "110"], check=True, capture_output=True)
    train = PowerFlowData(root=str(root), case="14", split=[.5, .2, .3], task="train", device=DEV)
    kw = dict(xymean=train.xymean, xystd=train.xystd, edgemean=train.edgemean, edgestd=train.edgestd)
    val = PowerFlowData(root=str(root), case="14", split=[.5, .2, .3], task="val", device=DEV, **kw)
    assert len(train) == 55 and len(val) == 22 and val.can_gather()
    return train, val


def _model(dropout=0.0, seed=7):
    torch.manual_seed(seed)
    return MaskEmbdMultiMPN(4, 2, 4, 32, 3, 2, dropout).to(DEV)


def _loader(ds):
    return DataLoader(ds, batch_size=8, shuffle=False)


def _loss(kind, ds):
    if kind == "masked_l2":
        return Masked_L2_loss(regularize=False)
    if kind == "mse":
        return MSELoss()
    return PowerImbalance(*[t.cpu() for t in ds.get_data_means_stds()])


@torch.no_grad()
def _host_loop(model, loader, loss_fn):
    """The loop `evaluate_epoch` replaces, with its arithmetic on the host: sum(loss.item() * len(data)) / sum(len(data))."""
    model.eval()
    total, n = 0.0, 0
    for data in loader:
        out = model(data)
        if isinstance(loss_fn, Masked_L2_loss):
            loss = loss_fn(out, data.y, data.pred_mask)
        elif isinstance(loss_fn, PowerImbalance):
            loss = loss_fn(out * data.pred_mask + data.pred_mask * (1 - data.pred_mask), data.edge_index, data.edge_attr)
        else:
            loss = loss_fn(out, data.y)
        n += len(data)
        total += loss.item() * len(data)
    return total / max(n, 1)


@pytest.mark.parametrize("kind", ["masked_l2", "mse", "power_imbalance"])
def test_graphed_epoch_equals_the_eager_epoch(sets, kind):
    _, val = sets
    model, loss_fn, loader = _model(), _loss(kind, val), _loader(val)
    step = GraphedEvalStep(model, loss_fn)
    model.train()
    eager = evaluate_epoch(model, loader, loss_fn, DEV)
    assert eager == _host_loop(model, loader, loss_fn) and math.isfinite(eager) and eager > 0
    model.train()
    assert evaluate_epoch(model, loader, loss_fn, DEV, graph=step) == eager
    assert step.captures == 2 and step.eager_batches == 0 and not step.disabled           # one per batch size: 8 and 6
    assert model.training, "the step leaves the model in the mode it found it in"
    assert all(p.grad is None for p in model.parameters())
    with torch.no_grad():                                                                   # values change in place: no new capture
        for p in model.parameters():
            p.mul_(1.03)
    eager2 = evaluate_epoch(model, loader, loss_fn, DEV)
    assert eager2 != eager
    assert evaluate_epoch(model, loader, loss_fn, DEV, graph=step) == eager2 and step.captures == 2
    FlatAdamW(model)                                                                        # the parameters' storage moves
    eager3 = evaluate_epoch(model, loader, loss_fn, DEV)
    assert eager3 == eager2
    assert evaluate_epoch(model, loader, loss_fn, DEV, graph=step) == eager3 and step.captures == 4
    assert evaluate_epoch(model, loader, loss_fn, DEV, graph=step) == eager3 and step.captures == 4


@pytest.mark.parametrize("denorm", [False, True])
def test_graphed_epoch_v2_equals_the_eager_epoch(sets, denorm):
    train, val = sets
    model, loss_fn, loader = _model(), MaskedL2V2(), _loader(val)
    pre = None
    if denorm:
        mean, std = train.xymean.to(DEV), train.xystd.to(DEV)
        pre = lambda t: denormalize(t, mean, std)                                            # noqa: E731
    eager = evaluate_epoch_v2(model, loader, loss_fn, DEV, pre_loss_fn=pre)
    # the loop it replaces, on the host, with its quirk: the FIRST batch unweighted, later ones by len(data)
    want, n = None, 0
    with torch.no_grad():
        for data in loader:
            out = model(data)
            terms = loss_fn(out, data.y, data.pred_mask) if pre is None else loss_fn(pre(out), pre(data.y), data.pred_mask)
            n += len(data)
            want = {k: v.item() for k, v in terms.items()} if want is None else {k: v + terms[k].item() * len(data) for k, v in want.items()}
    want = {k: v / n for k, v in want.items()}
    assert list(eager) == ["total", "balanced total", "vm", "va", "p", "q"] and eager == want
    step = GraphedEvalStep(model, loss_fn, pre)
    assert evaluate_epoch_v2(model, loader, loss_fn, DEV, pre_loss_fn=pre, graph=step) == eager
    assert step.captures == 2 and step.eager_batches == 0
    assert evaluate_epoch_v2(model, loader, loss_fn, DEV, pre_loss_fn=pre, graph=step) == eager and step.captures == 2
    # PowerImbalance: 'total' on the mixed rows, 'ref' on the ground truth
    if not denorm:
        pi = _loss("power_imbalance", val)
        e2 = evaluate_epoch_v2(model, loader, pi, DEV)
        assert list(e2) == ["total", "ref"]
        assert evaluate_epoch_v2(model, loader, pi, DEV, graph=GraphedEvalStep(model, pi)) == e2


def test_training_is_untouched_by_graphed_evaluation_in_between(sets):
    """graphed train epoch -> eval -> train -> eval: training losses and every parameter bit-identical whether the evaluation in
    between is graphed or eager; the model comes back in train mode with the same dropout RNG state."""
    train, val = sets

    def run(graphed_eval):
        model = _model(dropout=0.1, seed=11)
        model.seed_dropout(99)
        opt = FlatAdamW(model, lr=1e-3)
        loss_fn, eval_loss = MSELoss(), Masked_L2_loss(regularize=False)
        gt = GraphedTrainStep(model, loss_fn, opt)
        ge = GraphedEvalStep(model, eval_loss) if graphed_eval else None
        seq = []
        for epoch in range(2):
            loader = DataLoader(train, batch_size=8, shuffle=True, generator=torch.Generator().manual_seed(epoch))
            seq.append(train_epoch(model, loader, loss_fn, opt, DEV, graph=gt))
            model.train()
            seq.append(evaluate_epoch(model, _loader(val), eval_loss, DEV, graph=ge))
            if graphed_eval:
                assert model.training
        torch.cuda.synchronize()
        return seq, [p.detach().clone() for p in model.parameters()], model._rng_state.clone(), torch.cuda.get_rng_state(0), ge

    seq_e, params_e, rng_e, trng_e, _ = run(False)
    seq_g, params_g, rng_g, trng_g, ge = run(True)
    assert seq_g == seq_e, (seq_g, seq_e)
    assert all(torch.equal(a, b) for a, b in zip(params_g, params_e))
    assert torch.equal(rng_g, rng_e) and torch.equal(trng_g, trng_e)
    assert ge.captures == 2 and ge.eager_batches == 0


def test_a_list_backed_loader_is_copied_into_the_captured_inputs(sets):
    _, val = sets
    model, loss_fn = _model(), Masked_L2_loss(regularize=False)
    items = [val[i] for i in range(len(val))]
    loader = DataLoader(items, batch_size=8, shuffle=False)                                 # Batch.from_data_list: a new edge_index per batch
    eager = evaluate_epoch(model, loader, loss_fn, DEV)
    step = GraphedEvalStep(model, loss_fn)
    assert evaluate_epoch(model, loader, loss_fn, DEV, graph=step) == eager
    first = step.captures
    assert step.eager_batches == 0 and sorted(ch.static.x.shape[0] for ch in step._children.values()) == [6 * 14, 8 * 14]
    assert all(ch.graph is not None and ch.dynamic for ch in step._children.values())     # the short last batch has its own graph
    assert evaluate_epoch(model, loader, loss_fn, DEV, graph=step) == eager and step.captures == first
    # CPU batches are moved and copied the same way
    cpu_loader = DataLoader([d.to("cpu") for d in items], batch_size=8, shuffle=False)
    assert evaluate_epoch(model, cpu_loader, loss_fn, DEV, graph=step) == eager and step.captures == first


def test_a_mixed_split_runs_the_eager_body(tmp_path):
    ds = PowerFlowData(root=_mixed_root(tmp_path, samples=24), case="mixed", split=[.5, .25, .25], task="train", device=DEV)
    model, loss_fn = _model(), Masked_L2_loss(regularize=False)
    loader = DataLoader(ds, batch_size=8, shuffle=True, generator=torch.Generator().manual_seed(0))
    eager = evaluate_epoch(model, loader, loss_fn, DEV)
    loader = DataLoader(ds, batch_size=8, shuffle=True, generator=torch.Generator().manual_seed(0))
    step = GraphedEvalStep(model, loss_fn)
    assert evaluate_epoch(model, loader, loss_fn, DEV, graph=step) == eager
    assert step.eager_batches > 0


def test_per_sample_topologies(tmp_path):
    """One line set per sample: gathered and built inside the graph (gather_topologies_into); graphed and eager epoch values
    agree within RTOL (whether bit for bit is recorded)."""
    rng = np.random.default_rng(5)
    S, n, e = 44, 14, 20
    node = np.zeros((S, n, 6))
    node[:, :, 0] = np.arange(n)
    node[:, :, 1] = np.where(np.arange(n) == 0, 0, np.where(np.arange(n) % 3 == 0, 1, 2))
    node[:, :, 2:] = rng.normal(size=(S, n, 4))
    edge = np.zeros((S, e, 4))
    for s_ in range(S):
        edge[s_, :, :2] = make_topology(n, e, seed=100 + s_).numpy().T
    edge[:, :, 2:] = np.abs(rng.normal(size=(S, e, 2))) * 0.1 + 0.01
    (tmp_path / "raw").mkdir()
    np.save(tmp_path / "raw" / "case14_edge_features.npy", edge)
    np.save(tmp_path / "raw" / "case14_node_features.npy", node)
    ds = PowerFlowData(root=str(tmp_path), case="14", split=[.5, .25, .25], task="train", device=DEV)
    assert len(ds) == 22 and ds.can_gather_topologies() and not ds.can_gather()
    model, loss_fn = _model(), Masked_L2_loss(regularize=False)
    seg_before, dyn_before = model.segment_build, model.dynamic_topology
    eager = evaluate_epoch(model, _loader(ds), loss_fn, DEV)
    step = GraphedEvalStep(model, loss_fn)
    got = evaluate_epoch(model, _loader(ds), loss_fn, DEV, graph=step)
    assert math.isfinite(eager) and math.isfinite(got)
    record(f"per-sample topologies: graphed vs eager epoch value (bit for bit: {got == eager})", abs(got - eager), abs(eager), RTOL)
    print(f"per-sample topologies: graphed {got!r} eager {eager!r} bit for bit: {got == eager}")
    assert abs(got - eager) <= RTOL * abs(eager)
    assert step.captures == 2 and step.eager_batches == 0
    assert all(ch.topo_graph is not None for ch in step._children.values())
    assert (model.segment_build, model.dynamic_topology) == (seg_before, dyn_before)
    assert evaluate_epoch(model, _loader(ds), loss_fn, DEV, graph=step) == got and step.captures == 2


def _f64_report(model, loader, std, mean, pi):
    """The report from float64 formulas applied to the eager model's own fp32 outputs per batch, with the v2 weighting."""
    tot, n = {}, 0
    with torch.no_grad():
        for b, data in enumerate(loader):
            out = model(data)
            w = 1.0 if b == 0 else float(len(data))
            n += len(data)
            o, y, m, x = out.double().cpu(), data.y.double().cpu(), data.pred_mask.cpu(), data.x.double().cpu()
            s, mu = (std.float().cpu() + 1e-7).double(), mean.double().cpu()          # denormalize's fp32 factor, widened
            terms = {}
            for title, loss, a, c in (("MaskedL2", MaskedL2V2(), o, y), ("MaskedL2(denorm)", MaskedL2V2(), o * s + mu, y * s + mu),
                                      ("MaskedL1(denorm)", MaskedL1(), o * s + mu, y * s + mu)):
                terms.update({f"{title} {k}": float(v) for k, v in loss(a, c, m).items()})
            mixed = out * data.pred_mask + data.x * (1 - data.pred_mask)
            terms["PowerImbalance"] = float(pi(mixed, data.edge_index, data.edge_attr).item())
            terms["PowerImbalance(ref)"] = float(pi(data.y, data.edge_index, data.edge_attr).item())
            d2 = (o - y) ** 2
            terms["Masked_L2_loss"] = float(d2[m != 0].mean())
            terms["MSE"] = float(d2.mean())
            for k, v in terms.items():
                tot[k] = tot.get(k, 0.0) + v * w
    return {k: v / n for k, v in tot.items()}


@pytest.mark.parametrize("graphed", [False, True])
def test_report_in_one_pass(sets, graphed):
    train, val = sets
    model, loader = _model(), _loader(val)
    model.eval()
    pi = _loss("power_imbalance", val)
    step = GraphedEvalStep(model) if graphed else None
    rep = evaluate_report(model, loader, DEV, xystd=train.xystd, power_imbalance=pi, graph=step)
    assert list(rep) == report_keys()
    want = _f64_report(model, loader, train.xystd, train.xymean, pi)
    for k in report_keys():
        rel = abs(rep[k] - want[k]) / abs(want[k])
        record(f"evaluate_report {k} against float64", abs(rep[k] - want[k]), abs(want[k]), RTOL)
        assert rel <= RTOL, f"{k}: {rep[k]!r} against float64 {want[k]!r}: {rel:.2e}"
    if graphed:
        assert step.captures == 2 and step.eager_batches == 0
        assert evaluate_report(model, loader, DEV, xystd=train.xystd, power_imbalance=pi, graph=step) == rep and step.captures == 2
        assert rep == evaluate_report(model, loader, DEV, xystd=train.xystd, power_imbalance=pi)     # the eager pass: same bits
    # against the six passes of test.py: the normalised lines within RTOL; the de-normalised ones are recorded only (the eager
    # fp32 path subtracts two de-normalised values and is itself up to 7.6e-5 off there)
    mean, std = train.xymean.to(DEV), train.xystd.to(DEV)
    de = lambda t: denormalize(t, mean, std)                                                 # noqa: E731
    six = {}
    for title, loss, pre in (("MaskedL2", MaskedL2V2(), None), ("MaskedL2(denorm)", MaskedL2V2(), de), ("MaskedL1(denorm)", MaskedL1(), de)):
        six.update({f"{title} {k}": v for k, v in evaluate_epoch_v2(model, loader, loss, DEV, pre_loss_fn=pre).items()})
    t = evaluate_epoch_v2(model, loader, pi, DEV)
    six["PowerImbalance"], six["PowerImbalance(ref)"] = t["total"], t["ref"]
    six["Masked_L2_loss"] = evaluate_epoch_v2(model, loader, Masked_L2_loss(regularize=False), DEV)["total"]
    six["MSE"] = evaluate_epoch_v2(model, loader, MSELoss(), DEV)["total"]
    for k in report_keys():
        rel = abs(rep[k] - six[k]) / abs(six[k])
        record(f"evaluate_report {k} against the six passes", abs(rep[k] - six[k]), abs(six[k]), None if "denorm" in k else RTOL)
        if "denorm" not in k:
            assert rel <= RTOL, f"{k}: {rep[k]!r} against the six passes' {six[k]!r}: {rel:.2e}"
