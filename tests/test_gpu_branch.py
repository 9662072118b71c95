"""Per-line branch flows on the device: `pfn_branch_flows` (csrc/branch_flows.hip) against the float64 yardstick of
tests/branch_ref.py -- every value within C * 2^-24 * (S_q + |ref|) with C = 32, the error table bit-equal to the fp32 difference of the
two written tables, counts / min / max of the moments exact and their double sums within bus_errors_ref.sum_bound -- and
`branch_error_epoch` / error_per_feature.py --branch-errors end to end (graphed == eager bit for bit).

Worst measured |dev - ref64| / (2^-24 (S_q + |ref64|)) on an MI355X over the value tests below (C = 32 is the bound):
I 1.24, P 0.67, Q 0.74, loss 1.61 (each test prints its own)."""
import contextlib
import copy
import io
import os

import numpy as np
import pytest
import torch

from poweflownet_amd.data import DataLoader
from poweflownet_amd.datasets import PowerFlowData
from poweflownet_amd.loss import branch_flows, branch_flows_lds_max_bus, branch_moments, reset_bus_error_moments
from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
from poweflownet_amd.utils.branch_analysis import branch_error_epoch
from poweflownet_amd.utils.error_analysis import bus_error_epoch
from poweflownet_amd.utils.evaluation import GraphedEvalStep
from tests import branch_ref as R
from tests import bus_errors_ref as BR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, GUARD_WORDS = -777.25, 64
NAMES = ("I", "P", "Q", "loss")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Case:
    """Shared inputs of one shape: a normalised prediction table, a truth table (normalised or physical), one line list or one per
    sample, shared or per-sample attributes -- and the yardstick's flows of both tables, computed once."""

    def __init__(self, n, e, S, seed, per_sample_attr=False, truth_normalised=True, per_sample_lines=False, touch_ends=False):
        rng = np.random.default_rng(seed)
        self.n, self.e, self.S = n, e, S
        self.truth_normalised = truth_normalised
        if per_sample_lines:
            self.ei = np.stack([R.topology(n, e, rng) for _ in range(S)])
        elif touch_ends:                               # fewer lines than a tree needs: random pairs, three of them on bus 0 / n - 1
            a = rng.integers(0, n, e)
            self.ei = np.stack([a, (a + rng.integers(1, n, e)) % n])
            self.ei[:, 0], self.ei[:, 1], self.ei[:, 2] = (0, n - 1), (n - 1, 1), (2, 0)
        else:
            self.ei = R.topology(n, e, rng)
        self.pred = R.bus_table(S, n, rng, normalised=True)
        self.truth = R.bus_table(S, n, rng, normalised=truth_normalised)
        self.ea = R.edge_attrs((S, e) if per_sample_attr else (e,), rng)
        self.rx = R.physical_rx(self.ea, R.EDGE_STD, R.EDGE_MEAN)
        self.ref_pred, self.scale_pred = R.flows(R.denorm_rows(self.pred, R.STD4, R.MEAN4), self.ei, self.rx)
        self.ref_true, self.scale_true = R.flows(R.denorm_rows(self.truth, R.STD4, R.MEAN4) if truth_normalised else self.truth,
                                                 self.ei, self.rx)

    def run(self, moments=None, flags=None, rows=slice(None), pred=None, ei=None):
        pred = self.pred if pred is None else pred
        ei = self.ei if ei is None else ei
        sub = lambda a, per: a[rows] if per else a                                       # noqa: E731
        return branch_flows(_dev(pred[rows]), _dev(sub(ei, ei.ndim == 3)), _dev(sub(self.ea, self.ea.ndim == 3)), truth=_dev(self.truth[rows]),
                            pred_normalised=True, truth_normalised=self.truth_normalised, std=R.STD4, mean=R.MEAN4, edge_std=R.EDGE_STD,
                            edge_mean=R.EDGE_MEAN, flows_pred=True, flows_true=True, errors=True, moments=moments, flags=flags)


def _ratios(dev, ref, scale):
    """worst |dev - ref64| / (2^-24 (S_q + |ref64|)) per quantity."""
    return (np.abs(dev.astype(np.float64) - ref) / (R.EPS * (scale + np.abs(ref)))).reshape(-1, 4).max(axis=0)


def _check_values(case, fp, ft, err, what):
    fp, ft, err = fp.cpu().numpy(), ft.cpu().numpy(), err.cpu().numpy()
    assert fp.shape == ft.shape == err.shape == (case.S, case.e, 4) and fp.dtype == np.float32
    worst = np.maximum(_ratios(fp, case.ref_pred, case.scale_pred), _ratios(ft, case.ref_true, case.scale_true))
    print(f"{what}: worst ratio " + ", ".join(f"{q} {w:.2f}" for q, w in zip(NAMES, worst)) + f" (bound {R.C_BOUND:.0f})")
    assert (worst <= R.C_BOUND).all(), (what, worst)
    assert (fp[..., 3] >= 0).all() and (ft[..., 3] >= 0).all()                          # r >= 0 everywhere: the loss is never negative
    assert (fp[..., 0] >= 0).all() and (ft[..., 0] >= 0).all()
    assert np.array_equal(err, fp - ft)                                                  # ONE fp32 subtraction of the written tables
    return worst


# ------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("truth_normalised", [True, False])
@pytest.mark.parametrize("per_sample_attr", [False, True])
@pytest.mark.parametrize("n,e,S", [(14, 20, 3), (118, 186, 37), (300, 600, 8)])
def test_values_against_the_yardstick(n, e, S, per_sample_attr, truth_normalised):
    case = _Case(n, e, S, seed=n * 7 + S + 2 * per_sample_attr + truth_normalised, per_sample_attr=per_sample_attr,
                 truth_normalised=truth_normalised)
    fp, ft, err, flags = case.run()
    _check_values(case, fp, ft, err, f"n {n} e {e} S {S} attr/sample {per_sample_attr} truth normalised {truth_normalised}")
    assert int(flags[0]) == 0
    # one table only: the same flows of the prediction, bit for bit, and nothing else
    only, none_t, none_e, _ = branch_flows(_dev(case.pred), _dev(case.ei), _dev(case.ea), pred_normalised=True, std=R.STD4, mean=R.MEAN4,
                                           edge_std=R.EDGE_STD, edge_mean=R.EDGE_MEAN)
    assert torch.equal(only, fp) and none_t is None and none_e is None


def test_per_sample_topologies():
    case = _Case(30, 45, 5, seed=11, per_sample_lines=True, per_sample_attr=True)
    assert len({case.ei[s].tobytes() for s in range(5)}) == 5
    fp, ft, err, flags = case.run()
    _check_values(case, fp, ft, err, "five line lists")
    for s in range(5):                                                                  # ... and per sample, against its own list
        ref, scale = R.flows(R.denorm_rows(case.pred[s:s + 1], R.STD4, R.MEAN4), case.ei[s], case.rx[s])
        assert (_ratios(fp[s:s + 1].cpu().numpy(), ref, scale) <= R.C_BOUND).all(), s
    assert int(flags[0]) == 0


def test_the_direct_path_just_above_the_lds_limit():
    n = branch_flows_lds_max_bus() + 1
    case = _Case(n, 64, 2, seed=13, touch_ends=True)
    assert {0, n - 1} <= set(case.ei.reshape(-1).tolist()) and (case.ei[0] != case.ei[1]).all()
    fp, ft, err, flags = case.run()
    _check_values(case, fp, ft, err, f"direct path, n {n}")
    assert int(flags[0]) == 0
    # the same lines on a grid that fits the LDS path: the same values bit for bit (the two kernels share every expression)
    small = copy.copy(case)
    small.n, small.ei, small.pred, small.truth = n - 1, np.minimum(case.ei, n - 2), case.pred[:, :n - 1], case.truth[:, :n - 1]
    keep = (case.ei < n - 1).all(axis=0)
    fp2 = small.run()[0]
    assert keep.sum() >= 60 and torch.equal(fp2[:, _dev(keep)], fp[:, _dev(keep)])


# ----------------------------------------------------------------------------------------------------- moments
def _check_moments(mom, err, valid, n_terms, what):
    """`mom` [e, 4, 6] against the float64 moments of the kernel's own error table."""
    count, s, sa, sq, mn, mx, terms = R.moments(err, valid)
    assert np.array_equal(mom[..., 0], count), what
    assert np.array_equal(mom[..., 4], mn) and np.array_equal(mom[..., 5], mx), what
    for k, want in ((1, s), (2, sa), (3, sq)):
        got, bound = mom[..., k], BR.sum_bound(n_terms, terms[..., k - 1])
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (what, k)
        diff = np.abs(got - want)[~nan]
        if diff.size:
            print(f"{what} {BR_VALUE[k]}: worst |difference| {diff.max():.3e}, bound there {bound[~nan].reshape(-1)[diff.argmax()]:.3e}")
        assert (diff <= bound[~nan]).all(), (what, k)


BR_VALUE = ("count", "sum e", "sum |e|", "sum e^2", "min", "max")


def _guarded_moments(e):
    buf = torch.full((e * 24 + GUARD_WORDS,), GUARD, dtype=torch.float64, device=DEV)
    mom = buf[:e * 24].view(e, 4, 6)
    mom.copy_(branch_moments(DEV, e))
    return buf, mom


def test_moments_of_the_error_table():
    case = _Case(118, 186, 37, seed=21)
    buf, mom = _guarded_moments(case.e)
    err = case.run(moments=mom)[2]
    assert bool((buf[case.e * 24:] == GUARD).all())
    assert (mom[..., 0] == 37).all()
    _check_moments(mom.cpu().numpy(), err.cpu().numpy(), None, 37, "one call")
    # samples [0, 20) and then [20, 37): the same counts and extremes, the sums within the bound of two orders of the same terms
    _, two = _guarded_moments(case.e)
    e1 = case.run(moments=two, rows=slice(0, 20))[2]
    e2 = case.run(moments=two, rows=slice(20, 37))[2]
    assert torch.equal(torch.cat([e1, e2]), err)
    _check_moments(two.cpu().numpy(), err.cpu().numpy(), None, 37, "two calls")
    # two identical calls from identical moments: bit-identical
    _, again = _guarded_moments(case.e)
    case.run(moments=again)
    assert torch.equal(again, mom)
    # without an error table of the caller's the moments are the same (the table goes to a workspace)
    _, bare = _guarded_moments(case.e)
    out = branch_flows(_dev(case.pred), _dev(case.ei), _dev(case.ea), truth=_dev(case.truth), pred_normalised=True, truth_normalised=True,
                       std=R.STD4, mean=R.MEAN4, edge_std=R.EDGE_STD, edge_mean=R.EDGE_MEAN, errors=False, moments=bare)
    assert out[2] is None and torch.equal(bare, mom)


# --------------------------------------------------------------------------------------------------- bad input
def test_lines_outside_the_grid_are_flagged_nan_and_left_out():
    case = _Case(14, 20, 6, seed=31)
    _, clean_m = _guarded_moments(case.e)
    clean = case.run(moments=clean_m)
    bad = case.ei.copy()
    bad[1, 3], bad[0, 17] = -1, case.n                                                   # endpoint -1, endpoint n
    _, mom = _guarded_moments(case.e)
    flags = torch.zeros(2, dtype=torch.int32, device=DEV)
    fp, ft, err, _ = case.run(moments=mom, flags=flags, ei=bad)
    assert flags.tolist() == [1, 0]
    other = np.ones(case.e, dtype=bool)
    other[[3, 17]] = False
    for got, want in zip((fp, ft, err), clean[:3]):
        assert torch.isnan(got[:, [3, 17]]).all()
        assert torch.equal(got[:, _dev(other)], want[:, _dev(other)])
    m = mom.cpu().numpy()
    assert (m[[3, 17], :, 0] == 0).all() and (m[[3, 17], :, 1:4] == 0).all()
    assert (m[[3, 17], :, 4] == np.inf).all() and (m[[3, 17], :, 5] == -np.inf).all()
    assert torch.equal(mom[_dev(other)], clean_m[_dev(other)])
    # per-sample lists: only the samples that name the bad bus are left out
    lists = np.stack([case.ei] * case.S)
    lists[2, 0, 5], lists[4, 1, 5] = case.n + 7, np.iinfo(np.int64).min
    _, mom2 = _guarded_moments(case.e)
    flags.zero_()
    out = case.run(moments=mom2, flags=flags, ei=lists)
    assert int(flags[0]) == 1 and torch.isnan(out[2][[2, 4], 5]).all() and not torch.isnan(out[2][[0, 1, 3, 5], 5]).any()
    assert (mom2[5, :, 0] == 4).all() and (mom2[_dev(np.arange(case.e) != 5), :, 0] == 6).all()
    valid = np.ones((case.S, case.e), dtype=bool)
    valid[[2, 4], 5] = False
    _check_moments(mom2.cpu().numpy(), out[2].cpu().numpy(), valid, case.S, "per-sample bad ids")


def test_a_nan_prediction_reaches_exactly_its_lines():
    case = _Case(14, 20, 5, seed=37)
    pred = case.pred.copy()
    pred[2, 6, 0] = np.nan                                                               # sample 2, bus 6
    touching = (case.ei == 6).any(axis=0)
    assert 0 < touching.sum() < case.e
    _, mom = _guarded_moments(case.e)
    fp, ft, err, flags = case.run(moments=mom, pred=pred)
    nan = torch.isnan(err).all(dim=2).cpu().numpy()
    want = np.zeros((5, case.e), dtype=bool)
    want[2, touching] = True
    assert np.array_equal(nan, want) and np.array_equal(torch.isnan(err).any(dim=2).cpu().numpy(), want)
    assert not torch.isnan(ft).any() and int(flags[0]) == 0
    m = mom.cpu().numpy()
    assert (m[..., 0] == 5).all()
    assert np.isnan(m[touching][..., 1:4]).all() and not np.isnan(m[~touching]).any()
    assert np.isfinite(m[touching][..., 4:]).all() and (m[touching][..., 4] <= m[touching][..., 5]).all()
    _check_moments(m, err.cpu().numpy(), None, 5, "NaN prediction")


def test_nothing_to_do_writes_nothing():
    case = _Case(14, 20, 3, seed=41)
    buf, mom = _guarded_moments(case.e)
    before = buf.clone()
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = case.run(moments=mom, flags=flags, rows=slice(0, 0))                           # S = 0
    assert tuple(out[2].shape) == (0, 20, 4) and torch.equal(buf, before) and int(flags[0]) == 0
    empty = torch.full((GUARD_WORDS,), GUARD, dtype=torch.float64, device=DEV)           # e = 0
    out = branch_flows(_dev(case.pred), torch.zeros(2, 0, dtype=torch.long, device=DEV), torch.zeros(0, 2, device=DEV),
                       truth=_dev(case.truth), moments=empty[:0], flags=flags)
    assert tuple(out[2].shape) == (3, 0, 4) and bool((empty == GUARD).all()) and int(flags[0]) == 0


def test_zero_impedance_gives_nan_not_a_fault():
    case = _Case(14, 20, 2, seed=43)
    ea = case.ea.copy()
    ea[4] = (-1.0, -1.0)                                                                 # r = x = fma(-1, std, std) = 0
    fp = branch_flows(_dev(case.pred), _dev(case.ei), _dev(ea), pred_normalised=True, std=R.STD4, mean=R.MEAN4, edge_std=R.EDGE_STD,
                      edge_mean=R.EDGE_MEAN)[0]
    assert torch.isnan(fp[:, 4, 1:]).all() and not torch.isfinite(fp[:, 4, 0]).any()
    assert torch.isfinite(fp[:, [0, 1, 2, 3, 5]]).all()


# ----------------------------------------------------------------------------------------------------- capture
def test_a_captured_call_replays_bit_for_bit():
    case = _Case(118, 186, 37, seed=51)
    _, want_m = _guarded_moments(case.e)
    want = case.run(moments=want_m)
    pred, truth, ei, ea = _dev(case.pred), _dev(case.truth), _dev(case.ei), _dev(case.ea)
    outs = [torch.full((37, case.e, 4), GUARD, device=DEV) for _ in range(3)]
    buf, mom = _guarded_moments(case.e)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)

    def launch():
        branch_flows(pred, ei, ea, truth=truth, pred_normalised=True, truth_normalised=True, std=R.STD4, mean=R.MEAN4, edge_std=R.EDGE_STD,
                     edge_mean=R.EDGE_MEAN, flows_pred=outs[0], flows_true=outs[1], errors=outs[2], moments=mom, flags=flags)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                                         # warm-up
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for _ in range(2):
        for o in outs:
            o.fill_(GUARD)
        reset_bus_error_moments(mom)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o, w) for o, w in zip(outs, want[:3])) and torch.equal(mom, want_m)
        assert bool((buf[case.e * 24:] == GUARD).all()) and int(flags[0]) == 0


# -------------------------------------------------------------------------------------------------- end to end
S_TEST, BATCH, N118, E118 = 40, 16, 118, 186


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    """A synthetic 118-bus test split of 40 samples (batches of 16, 16 and 8), device-resident, and the same samples as a list."""
    root = tmp_path_factory.mktemp("branch_case118")
    rng = np.random.default_rng(19)
    S = 2 * S_TEST
    node = np.zeros((S, N118, 6), dtype=np.float32)
    node[:, :, 0] = np.arange(N118)
    node[:, :, 1] = np.where(np.arange(N118) == 0, 0, np.where(np.arange(N118) % 3 == 0, 1, 2))
    node[:, :, 2:] = R.bus_table(S, N118, rng, normalised=False)
    edge = np.zeros((S, E118, 4), dtype=np.float32)
    edge[:, :, :2] = R.topology(N118, E118, rng).T
    edge[:, :, 2] = rng.uniform(0.01, 0.1, (S, E118))
    edge[:, :, 3] = rng.uniform(0.05, 0.5, (S, E118))
    os.makedirs(root / "raw")
    np.save(root / "raw" / "case118_edge_features.npy", edge)
    np.save(root / "raw" / "case118_node_features.npy", node)
    ds = PowerFlowData(root=str(root), case="118", split=[.5, .0, .5], task="test", device=DEV)
    assert len(ds) == S_TEST and ds.can_gather()
    return ds, [ds[i] for i in range(len(ds))]


def _model(seed=7):
    torch.manual_seed(seed)
    return MaskEmbdMultiMPN(4, 2, 4, 32, 3, 2, 0.0).to(DEV).eval()


@pytest.mark.parametrize("kind", ["device_resident", "list"])
def test_branch_error_epoch_eager_and_graphed(split, kind):
    ds, items = split
    loader = DataLoader(ds if kind == "device_resident" else items, batch_size=BATCH, shuffle=False)
    model = _model()
    stats = dict(xymean=ds.xymean, xystd=ds.xystd, edgemean=ds.edgemean, edgestd=ds.edgestd)
    eager = branch_error_epoch(model, loader, DEV, keep_flows=True, **stats)
    graphed = branch_error_epoch(model, loader, DEV, graph=GraphedEvalStep(model), keep_flows=True, **stats)
    for a, b in ((eager.errors, graphed.errors), (eager.flows_pred, graphed.flows_pred), (eager.flows_true, graphed.flows_true),
                 (eager.moments, graphed.moments)):
        assert torch.equal(a, b)
    assert eager.num_samples == graphed.num_samples == S_TEST and eager.flags == graphed.flags == 0
    assert tuple(eager.errors.shape) == (S_TEST, E118, 4) and tuple(eager.moments.shape) == (E118, 4, 6)
    assert torch.equal(eager.lines0, ds[0].edge_index.cpu()) and torch.isfinite(eager.errors).all() and float(eager.errors.abs().max()) > 0
    # == branch_flows on the predictions bus_error_epoch returns, against the dataset's own tables
    bus = bus_error_epoch(model, loader, DEV, xymean=ds.xymean, xystd=ds.xystd, keep_errors=False, keep_predictions=True)
    assert bus.rows_by_index == (kind == "device_resident")
    b = ds._blocks[0]
    std4 = (ds.xystd.reshape(-1)[:4].float() + 1e-7).tolist()
    estd = (ds.edgestd.reshape(-1)[:2].float() + 1e-7).tolist()
    mom = branch_moments(DEV, E118)
    fp, ft, err, _ = branch_flows(bus.predictions, b.edge_index[0], b.edge_attr, truth=b.y, truth_normalised=True, std=std4,
                                  mean=ds.xymean.reshape(-1)[:4].tolist(), edge_std=estd, edge_mean=ds.edgemean.reshape(-1)[:2].tolist(),
                                  flows_pred=True, flows_true=True, moments=mom)
    assert torch.equal(err, eager.errors) and torch.equal(fp, eager.flows_pred) and torch.equal(ft, eager.flows_true)
    assert torch.equal(mom.cpu(), eager.moments)
    # the truth's flows are those of the raw file's voltages and impedances, up to the normalisation's fp32 round trip
    raw_y = R.denorm_rows(b.y.cpu().numpy(), np.asarray(std4, np.float32), ds.xymean.reshape(-1)[:4].numpy())
    rx = R.physical_rx(b.edge_attr.cpu().numpy(), np.asarray(estd, np.float32), ds.edgemean.reshape(-1)[:2].numpy())
    ref, scale = R.flows(raw_y, b.edge_index[0].cpu().numpy(), rx)
    assert (_ratios(ft.cpu().numpy(), ref, scale) <= R.C_BOUND).all()
    # a shuffling loader: the device-resident split fills its rows by sample index, a list-backed one cannot be aligned
    shuffled = DataLoader(loader.dataset, batch_size=BATCH, shuffle=True, generator=torch.Generator().manual_seed(3))
    if kind == "device_resident":
        assert torch.equal(branch_error_epoch(model, shuffled, DEV, **stats).errors, eager.errors)
    else:
        with pytest.raises(ValueError, match="shuffling"):
            branch_error_epoch(model, shuffled, DEV, **stats)


def _run_script(argv):
    import error_per_feature
    torch.manual_seed(0)                                                                 # (no checkpoint: the same random model per call)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert error_per_feature.main(list(argv)) == 0
    return out.getvalue()


def test_error_per_feature_branch_errors(tmp_path):
    base = ["--case", "118", "--synthetic-samples", "40", "--batch-size", "8"]
    plain_dir, branch_dir = tmp_path / "plain", tmp_path / "branch"
    plain = _run_script(base + ["--results-dir", str(plain_dir)])
    text = _run_script(base + ["--branch-errors", "--results-dir", str(branch_dir)])
    S = 12                                                                               # 40 samples: the last 30 % are the test split
    shapes = {"i_error_table": (S, E118), "branch_errors": (S, E118, 4), "lines": (2, E118), "branch_error_hist": (E118, 4, 300),
              "branch_error_hist_edges": (4, 301)}
    got = {k: np.load(branch_dir / f"118_{k}.npy") for k in shapes}
    assert {k: v.shape for k, v in got.items()} == shapes
    assert np.array_equal(got["i_error_table"], got["branch_errors"][..., 0], equal_nan=True)
    assert got["branch_errors"].dtype == np.float32 and got["lines"].dtype == np.int64
    assert not (branch_dir / "118_branch_flows_pred.npy").exists() and not (branch_dir / "118_predictions.npy").exists()
    for b in range(0, E118, 37):
        for f in range(4):
            col = got["branch_errors"][:, b, f].astype(np.float64)
            assert np.array_equal(got["branch_error_hist"][b, f], np.histogram(col[~np.isnan(col)], bins=got["branch_error_hist_edges"][f])[0])
    assert "i_error_table mean:" in text and "Absolute Average of Active Loss:" in text and "Largest error of Line Current: line:" in text
    # without the flag: none of the files, and the output of the same call is the head of the flagged one's
    assert sorted(p.name for p in plain_dir.iterdir()) == sorted(f"118_{k}.npy" for k in ("errors", "masks", "types", "error_hist",
                                                                                           "error_hist_edges"))
    assert "i_error_table" not in plain and "Line Current" not in plain
    assert text.startswith(plain.replace(str(plain_dir), str(branch_dir)))
    flows = _run_script(base + ["--branch-errors", "--save-flows", "--results-dir", str(tmp_path / "flows")])
    fp, ft = np.load(tmp_path / "flows" / "118_branch_flows_pred.npy"), np.load(tmp_path / "flows" / "118_branch_flows_true.npy")
    assert fp.shape == ft.shape == (S, E118, 4)
    assert np.array_equal(fp - ft, np.load(tmp_path / "flows" / "118_branch_errors.npy"), equal_nan=True) and "branch_flows_true" in flows
