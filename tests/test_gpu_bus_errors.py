"""Per-bus error analysis on the device: `pfn_bus_errors_accumulate` / `pfn_bus_errors_histogram` (csrc/bus_errors.hip) against the
numpy yardsticks of tests/bus_errors_ref.py -- tables bit for bit, counts / min / max exact, the double sums within the derived bound
2 * S * 2^-53 * sum |terms|, histograms with integer equality to np.histogram -- and `bus_error_epoch` / `report_lines` /
error_per_feature.py end to end (eager per-batch loop bit for bit, graphed == eager bit for bit)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.data import DataLoader
from poweflownet_amd.datasets import PowerFlowData, denormalize
from poweflownet_amd.loss import bus_error_moments, bus_errors_accumulate, bus_errors_histogram
from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
from poweflownet_amd.synth import _MASK_TABLE, make_topology
from poweflownet_amd.utils.custom_loss_functions import PowerImbalance
from poweflownet_amd.utils.error_analysis import (bus_error_epoch, bus_error_histograms, histogram_edges, mask_scale, report_lines)
from poweflownet_amd.utils.evaluation import GraphedEvalStep, evaluate_report
from tests import bus_errors_ref as R
from tests.test_segpack_host import _mixed_root

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, GUARD_WORDS = -777.25, 64
STD, MEAN = (0.05, 10.0, 50.0, 20.0), (1.0, 0.5, 30.0, -10.0)
SHAPES = [(1, 1), (14, 3), (37, 128), (118, 5), (6470, 2)]


# ------------------------------------------------------------------------------------------------ accumulate
def _masks(kind, n_bus, G, rng):
    types = np.full(n_bus, 2, dtype=np.int64)
    types[::3] = 1
    types[0] = 0
    table = np.tile(_MASK_TABLE.numpy()[types], (G, 1))                       # the bus-type table, one mask for every graph
    if kind == "table":
        return torch.from_numpy(table)
    if kind == "zero_column":
        table[:, 0] = 0                                                      # nothing of Vm is predicted: group 0 stays empty there
        return torch.from_numpy(table)
    return torch.from_numpy((rng.random((G * n_bus, 4)) < 0.5).astype(np.float32))       # float32 0 / 1, differing per sample


def _batch(n_bus, G, seed):
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(G * n_bus, 4)).astype(np.float32)
    y = (o + rng.normal(size=o.shape) * 0.3).astype(np.float32)
    return o, y, rng


class _Guarded:
    """The outputs of an accumulate call, each with guard words behind it: tables [rows, n, 4] pre-filled with the guard value."""

    def __init__(self, rows, n_bus):
        self.rows, self.n = rows, n_bus
        self.err_buf = torch.full((rows * n_bus * 4 + GUARD_WORDS,), GUARD, device=DEV)
        self.pred_buf = torch.full((rows * n_bus * 4 + GUARD_WORDS,), GUARD, device=DEV)
        self.mom_buf = torch.full((n_bus * 48 + GUARD_WORDS,), GUARD, dtype=torch.float64, device=DEV)
        self.err = self.err_buf[:rows * n_bus * 4].view(rows, n_bus, 4)
        self.pred = self.pred_buf[:rows * n_bus * 4].view(rows, n_bus, 4)
        self.moments = self.mom_buf[:n_bus * 48].view(n_bus, 4, 2, 6)
        self.moments.copy_(bus_error_moments(DEV, n_bus))
        self.flags = torch.zeros(2, dtype=torch.int32, device=DEV)

    def call(self, o, y, mask, idx, std=STD, mean=MEAN):
        bus_errors_accumulate(torch.as_tensor(o).to(DEV), torch.as_tensor(y).to(DEV), mask.to(DEV), self.n,
                              torch.as_tensor(np.asarray(idx, dtype=np.int64)).to(DEV), self.moments, self.flags, std=std, mean=mean,
                              err_table=self.err, pred_table=self.pred)

    def guards_intact(self):
        tail = self.rows * self.n * 4
        return (bool((self.err_buf[tail:] == GUARD).all()) and bool((self.pred_buf[tail:] == GUARD).all())
                and bool((self.mom_buf[self.n * 48:] == GUARD).all()))


def _check(out: _Guarded, calls, n_terms_note=""):
    """`calls`: [(o, y, mask, idx)] accumulated into `out` one after the other."""
    err, pred, mom = out.err.cpu().numpy(), out.pred.cpu().numpy(), out.moments.cpu().numpy()
    assert out.guards_intact()
    addressed = set()
    total = None
    n_terms = 0
    for o, y, mask, idx in calls:
        written, mo = R.accumulate(o, y, mask.numpy(), out.n, idx, out.rows, STD, MEAN)
        n_terms += len(written)
        for g, (row, e, p) in written.items():
            addressed.add(row)
            assert np.array_equal(err[row], e, equal_nan=True), (g, row)
            assert np.array_equal(pred[row], p, equal_nan=True), (g, row)
        if total is None:
            total = list(mo)
        else:
            for k in (0, 1, 2, 3, 6):
                total[k] = total[k] + mo[k]
            total[4], total[5] = np.minimum(total[4], mo[4]), np.maximum(total[5], mo[5])
    for row in range(out.rows):
        if row not in addressed:
            assert (err[row] == GUARD).all() and (pred[row] == GUARD).all(), row
    count, s, sa, sq, mn, mx, terms = total
    assert np.array_equal(mom[..., 0], count) and np.array_equal(mom[..., 4], mn) and np.array_equal(mom[..., 5], mx)
    worst = 0.0
    for k, want in ((1, s), (2, sa), (3, sq)):
        got, bound = mom[..., k], R.sum_bound(n_terms, terms[..., k - 1])
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), BUS_VALUE[k]
        diff = np.abs(got - want)[~nan]
        print(f"{BUS_VALUE[k]}{n_terms_note}: worst |difference| {diff.max():.3e}, bound there {bound[~nan].reshape(-1)[diff.argmax()]:.3e}")
        assert (diff <= bound[~nan]).all(), BUS_VALUE[k]
        worst = max(worst, float(diff.max()))
    return mom, worst


BUS_VALUE = ("count", "sum e", "sum |e|", "sum e^2", "min", "max")


@pytest.mark.parametrize("mask_kind", ["table", "zero_column", "float01"])
@pytest.mark.parametrize("n_bus,G", SHAPES)
def test_accumulate_against_numpy(n_bus, G, mask_kind):
    o, y, rng = _batch(n_bus, G, seed=n_bus * 131 + G)
    mask = _masks(mask_kind, n_bus, G, rng)
    rows = G + 3
    idx = rng.permutation(rows)[:G]                                           # a permutation into a table with more rows than graphs
    out = _Guarded(rows, n_bus)
    out.call(o, y, mask, idx)
    mom, _ = _check(out, [(o, y, mask, idx)])
    assert int(out.flags[0]) == 0
    if mask_kind == "zero_column":
        assert (mom[:, 0, 0, 0] == 0).all() and (mom[:, 0, 0, 4] == np.inf).all() and (mom[:, 0, 0, 5] == -np.inf).all()
        assert (mom[:, 0, 1, 0] == G).all()


def test_out_of_range_indices_are_flagged_and_left_out():
    n_bus, G, rows = 14, 6, 9
    o, y, rng = _batch(n_bus, G, seed=5)
    mask = _masks("table", n_bus, G, rng)
    idx = np.array([4, -1, 0, rows, 8, 2])
    out = _Guarded(rows, n_bus)
    out.call(o, y, mask, idx)
    assert int(out.flags[0]) & 1
    mom, _ = _check(out, [(o, y, mask, idx)])
    assert mom[..., 0].sum() == 4 * n_bus * 4                                 # four of the six graphs were counted
    # a clean batch afterwards leaves the bit set and nothing else behind
    good = np.array([1, 3, 5, 6, 7, 2])
    out.call(o, y, mask, good)
    assert int(out.flags[0]) == 1
    _check(out, [(o, y, mask, idx), (o, y, mask, good)])


def test_nan_poisons_the_sums_of_its_own_group_only():
    n_bus, G = 14, 5
    o, y, rng = _batch(n_bus, G, seed=9)
    mask = _masks("table", n_bus, G, rng)
    m = mask.numpy().reshape(G, n_bus, 4)
    assert m[2, 5, 0] == 1 and m[3, 6, 2] == 0                                # bus 5 (load) predicts Vm; bus 6 (generator) is given P
    o.reshape(G, n_bus, 4)[2, 5, 0] = np.nan                                  # under a predicted entry
    o.reshape(G, n_bus, 4)[3, 6, 2] = np.nan                                  # under a given entry
    out = _Guarded(G, n_bus)
    out.call(o, y, mask, np.arange(G))
    mom, _ = _check(out, [(o, y, mask, np.arange(G))])
    for (b, f, g) in ((5, 0, 0), (6, 2, 1)):
        assert mom[b, f, g, 0] == G and np.isnan(mom[b, f, g, 1:4]).all()
        assert np.isfinite(mom[b, f, g, 4:]).all() and mom[b, f, g, 4] <= mom[b, f, g, 5]
    clean = np.ones((n_bus, 4, 2), dtype=bool)
    clean[5, 0, 0] = clean[6, 2, 1] = False
    assert not np.isnan(mom[clean]).any()
    assert np.isnan(out.err.cpu().numpy()).sum() == 2 and np.isnan(out.pred.cpu().numpy()).sum() == 2


def test_two_batches_equal_the_concatenation_and_replays_equal_eager_calls():
    n_bus, G, rows = 37, 24, 80
    batches = []
    for b in range(3):
        o, y, rng = _batch(n_bus, G, seed=40 + b)
        batches.append((o, y, _masks("float01", n_bus, G, rng), np.arange(b * G, (b + 1) * G) + 3))
    # (a) one after the other == one call on the concatenation, within the bound of two orders of the same double sums
    seq, cat = _Guarded(rows, n_bus), _Guarded(rows, n_bus)
    for o, y, mask, idx in batches[:2]:
        seq.call(o, y, mask, idx)
    o2, y2 = np.concatenate([batches[0][0], batches[1][0]]), np.concatenate([batches[0][1], batches[1][1]])
    m2, i2 = torch.cat([batches[0][2], batches[1][2]]), np.concatenate([batches[0][3], batches[1][3]])
    cat.call(o2, y2, m2, i2)
    _check(seq, batches[:2], " (two calls)")
    _check(cat, [(o2, y2, m2, i2)], " (one call)")
    a, c = seq.moments.cpu().numpy(), cat.moments.cpu().numpy()
    assert torch.equal(seq.err, cat.err) and torch.equal(seq.pred, cat.pred)
    assert np.array_equal(a[..., 0], c[..., 0]) and np.array_equal(a[..., 4:], c[..., 4:])
    _, (_, _, _, _, _, _, terms) = R.accumulate(o2, y2, m2.numpy(), n_bus, i2, rows, STD, MEAN)
    for k in (1, 2, 3):
        assert (np.abs(a[..., k] - c[..., k]) <= R.sum_bound(2 * G, terms[..., k - 1])).all(), BUS_VALUE[k]
    # (b) three replays of ONE captured launch over three batches == three eager calls, bit for bit
    eager, graphed = _Guarded(rows, n_bus), _Guarded(rows, n_bus)
    for o, y, mask, idx in batches:
        eager.call(o, y, mask, idx)
    so, sy = torch.zeros(G * n_bus, 4, device=DEV), torch.zeros(G * n_bus, 4, device=DEV)
    sm, si = torch.zeros(G * n_bus, 4, device=DEV), torch.zeros(G, dtype=torch.long, device=DEV)

    def launch():
        bus_errors_accumulate(so, sy, sm, n_bus, si, graphed.moments, graphed.flags, std=STD, mean=MEAN, err_table=graphed.err,
                              pred_table=graphed.pred)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                              # warm-up (on zeros, into row 0)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    fresh = _Guarded(rows, n_bus)                                             # the warm-up leaves no trace
    for dst, src in ((graphed.err_buf, fresh.err_buf), (graphed.pred_buf, fresh.pred_buf), (graphed.mom_buf, fresh.mom_buf)):
        dst.copy_(src)
    for o, y, mask, idx in batches:
        so.copy_(torch.from_numpy(o)); sy.copy_(torch.from_numpy(y)); sm.copy_(mask); si.copy_(torch.from_numpy(idx))     # noqa: E702
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(graphed.moments, eager.moments) and torch.equal(graphed.err, eager.err) and torch.equal(graphed.pred, eager.pred)
    assert graphed.guards_intact() and int(graphed.flags[0]) == 0
    _check(graphed, batches, " (three replays)")


# -------------------------------------------------------------------------------------------------- histogram
def _planted_table(S, n_bus, edges, rng):
    t = rng.uniform(-1.3, 2.6, size=(S, n_bus, 4)).astype(np.float32)
    flat = t.reshape(-1, 4)
    for f in range(4):
        e = edges[f]
        nb = e.size - 1
        planted = [np.float32(e[0]), np.float32(e[nb // 2]), np.float32(e[-1]), np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan),
                   np.nextafter(np.float32(e[0]), np.float32(-np.inf)), np.nextafter(np.float32(e[-1]), np.float32(np.inf)),
                   np.float32(e[min(1, nb)]), np.float32(e[max(nb - 1, 0)])]
        where = rng.permutation(flat.shape[0])[:len(planted)]
        flat[where, f] = planted[:len(where)]
    return t


@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("nbins", [1, 7, 300, 2048])
def test_histogram_against_np_histogram(nbins, with_scale):
    rng = np.random.default_rng(1000 * nbins + with_scale)
    edges = np.stack([np.linspace(-0.9 - 0.1 * f, 2.1 + 0.2 * f, nbins + 1) for f in range(4)])      # asymmetric ranges
    edges_dev = torch.from_numpy(edges).to(DEV)
    for S in (1, 37, 1000):
        for n_bus in (1, 9, 14, 17, 33, 118):       # 33: one past a 32-bus tile; 9 / 17: one past the 8- / 16-bus tiles; 14, 118: partial
            if S == 1000 and n_bus in (9, 17):
                continue
            table = _planted_table(S, n_bus, edges, rng)
            scale = None
            if with_scale:
                scale = rng.uniform(0.5, 2.0, size=(n_bus, 4)).astype(np.float32)
                scale[rng.random((n_bus, 4)) < 0.3] = 1.0
                scale[rng.random((n_bus, 4)) < 0.2] = np.float32(0.00001)
            hbuf = torch.full((n_bus * 4 * nbins + GUARD_WORDS,), -7, dtype=torch.int32, device=DEV)
            obuf = torch.full((n_bus * 12 + GUARD_WORDS,), -7, dtype=torch.int32, device=DEV)
            tdev = torch.from_numpy(table).to(DEV)
            sdev = None if scale is None else torch.from_numpy(scale).to(DEV)
            L.check(L.load().pfn_bus_errors_histogram(tdev.data_ptr(), S, n_bus, L.ptr(sdev), edges_dev.data_ptr(), nbins,
                                                      hbuf.data_ptr(), obuf.data_ptr(), L.stream_ptr()), "pfn_bus_errors_histogram")
            hist = hbuf[:n_bus * 4 * nbins].view(n_bus, 4, nbins).cpu().numpy()
            outside = obuf[:n_bus * 12].view(n_bus, 4, 3).cpu().numpy()
            assert bool((hbuf[n_bus * 4 * nbins:] == -7).all()) and bool((obuf[n_bus * 12:] == -7).all())
            v = table if scale is None else table * scale[None]
            assert v.dtype == np.float32
            what = f"S {S} n_bus {n_bus} nbins {nbins} scale {with_scale}"
            assert ((hist.sum(axis=2) + outside.sum(axis=2)) == S).all(), what
            for b in range(n_bus):
                for f in range(4):
                    col = v[:, b, f].astype(np.float64)
                    want, _ = np.histogram(col[~np.isnan(col)], bins=edges[f])
                    assert np.array_equal(hist[b, f], want), (what, b, f)
                    _, below, above, nan = R.edge_rule(col, edges[f])
                    assert tuple(outside[b, f]) == (below, above, nan), (what, b, f)
            # the wrapper: the same counts, overwritten on every call
            h2, o2 = bus_errors_histogram(tdev, edges, sdev)
            assert np.array_equal(h2.cpu().numpy(), hist) and np.array_equal(o2.cpu().numpy(), outside)


def test_bad_bin_counts_are_errors_not_faults():
    lib = L.load()
    table = torch.zeros(3, 2, 4, device=DEV)
    edges = torch.linspace(-1, 1, 4096, dtype=torch.float64, device=DEV)
    hist, outside = torch.zeros(2 * 4 * 4096, dtype=torch.int32, device=DEV), torch.zeros(24, dtype=torch.int32, device=DEV)
    for nbins in (0, 2049, -3):
        rc = lib.pfn_bus_errors_histogram(table.data_ptr(), 3, 2, None, edges.data_ptr(), nbins, hist.data_ptr(), outside.data_ptr(), L.stream_ptr())
        assert rc == -1 and b"nbins must be in 1..2048" in lib.pfn_last_error(), (nbins, rc, lib.pfn_last_error())
    with pytest.raises(RuntimeError, match="nbins must be in 1..2048"):
        bus_errors_histogram(table, np.zeros((4, 1)))
    # ... and the process goes on
    h, o = bus_errors_histogram(table, np.stack([np.linspace(-1, 1, 3)] * 4))
    assert h.cpu().tolist() == [[[0, 3]] * 4] * 2 and int(o.sum()) == 0
    assert int(hist.sum()) == 0


# ------------------------------------------------------------------------------------------------- end to end
S_TEST, BATCH = 40, 16


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    """A synthetic case14 test split of 40 samples (batches of 16, 16 and 8), device-resident, and the same samples as a list."""
    root = tmp_path_factory.mktemp("bus_errors_case14")
    rng = np.random.default_rng(17)
    S, n, e = 2 * S_TEST, 14, 20
    node = np.zeros((S, n, 6), dtype=np.float32)
    node[:, :, 0] = np.arange(n)
    node[:, :, 1] = np.where(np.arange(n) == 0, 0, np.where(np.arange(n) % 3 == 0, 1, 2))
    node[:, :, 2:] = rng.normal(size=(S, n, 4)) * np.array([0.05, 10.0, 50.0, 20.0]) + np.array([1.0, 0.0, 30.0, 10.0])
    edge = np.zeros((S, e, 4), dtype=np.float32)
    edge[:, :, :2] = make_topology(n, e).numpy().T
    edge[:, :, 2:] = np.abs(rng.normal(size=(S, e, 2))) * 0.1 + 0.01
    os.makedirs(root / "raw")
    np.save(root / "raw" / "case14_edge_features.npy", edge)
    np.save(root / "raw" / "case14_node_features.npy", node)
    ds = PowerFlowData(root=str(root), case="14", split=[.5, .0, .5], task="test", device=DEV)
    assert len(ds) == S_TEST and ds.can_gather()
    return ds, [ds[i] for i in range(len(ds))]


def _model(seed=7):
    torch.manual_seed(seed)
    return MaskEmbdMultiMPN(4, 2, 4, 32, 3, 2, 0.0).to(DEV).eval()


@torch.no_grad()
def _per_batch_loop(model, loader, ds):
    """The loop written by hand: (out - y) * (std + 1e-7) and denormalize(out) per batch, in torch."""
    std, mean = ds.xystd.to(DEV), ds.xymean.to(DEV)
    errs, preds = [], []
    for data in loader:
        data = data.to(DEV)
        out = model(data)
        errs.append(((out - data.y) * (std + 1e-7)).view(-1, 14, 4))
        preds.append(denormalize(out, mean, std).view(-1, 14, 4))
    return torch.cat(errs), torch.cat(preds)


@pytest.mark.parametrize("kind", ["device_resident", "list"])
def test_eager_epoch_equals_the_per_batch_loop(split, kind):
    ds, items = split
    loader = DataLoader(ds if kind == "device_resident" else items, batch_size=BATCH, shuffle=False)
    model = _model()
    res = bus_error_epoch(model, loader, DEV, xymean=ds.xymean, xystd=ds.xystd, keep_predictions=True)
    want_e, want_p = _per_batch_loop(model, loader, ds)
    assert res.num_samples == S_TEST and res.flags == 0 and tuple(res.errors.shape) == (S_TEST, 14, 4)
    assert torch.equal(res.errors, want_e) and torch.equal(res.predictions, want_p)
    assert float(res.errors.abs().max()) > 0 and torch.isfinite(res.errors).all()
    assert torch.equal(res.mask0, ds[0].pred_mask.cpu()) and torch.equal(res.types0, ds[0].bus_type.cpu())
    # the moments are those of the table
    _, mo = R.accumulate(np.zeros((S_TEST * 14, 4), np.float32), -res.errors.cpu().numpy().reshape(-1, 4),
                         np.tile(res.mask0.numpy(), (S_TEST, 1)), 14, np.arange(S_TEST), S_TEST, None, None)
    m = res.moments.numpy()
    assert np.array_equal(m[..., 0], mo[0]) and np.array_equal(m[..., 4], mo[4]) and np.array_equal(m[..., 5], mo[5])
    for k in (1, 2, 3):
        assert (np.abs(m[..., k] - mo[k]) <= R.sum_bound(S_TEST, mo[6][..., k - 1])).all()
    # without tables: the same moments, nothing kept
    bare = bus_error_epoch(model, loader, DEV, xymean=ds.xymean, xystd=ds.xystd, keep_errors=False)
    assert bare.errors is None and bare.predictions is None and torch.equal(bare.moments, res.moments)
    # a shuffling loader over the device-resident split fills the same rows (the row is the sample index)
    if kind == "device_resident":
        shuffled = DataLoader(ds, batch_size=BATCH, shuffle=True, generator=torch.Generator().manual_seed(3))
        again = bus_error_epoch(model, shuffled, DEV, xymean=ds.xymean, xystd=ds.xystd)
        assert torch.equal(again.errors, res.errors)


@pytest.mark.parametrize("kind", ["device_resident", "list"])
def test_graphed_epoch_equals_the_eager_epoch_and_the_report(split, kind):
    ds, items = split
    loader = DataLoader(ds if kind == "device_resident" else items, batch_size=BATCH, shuffle=False)
    model = _model()
    eager = bus_error_epoch(model, loader, DEV, xymean=ds.xymean, xystd=ds.xystd, keep_predictions=True)
    step = GraphedEvalStep(model)
    for _ in range(2):                                                        # the second epoch replays what the first captured
        got = bus_error_epoch(model, loader, DEV, xymean=ds.xymean, xystd=ds.xystd, graph=step, keep_predictions=True)
        # one capture per batch size (16 and 8); the list-backed loader hands out a new edge_index per batch, which the step sees
        # at its second batch and answers by capturing that size once more with the adjacency build inside the graph
        assert step.captures == (2 if kind == "device_resident" else 3) and step.eager_batches == 0 and not step.disabled
        assert torch.equal(got.errors, eager.errors) and torch.equal(got.predictions, eager.predictions)
        assert torch.equal(got.moments, eager.moments) and got.num_samples == S_TEST and got.flags == 0
    # the report against the reference's lines computed from the read-back arrays
    errors = got.errors.cpu().numpy()
    masks = np.broadcast_to(got.mask0.numpy(), (S_TEST, 14, 4))
    types = np.broadcast_to(got.types0.numpy(), (S_TEST, 14))
    want, lines = R.report(errors, masks, types), report_lines(got.moments, got.mask0, got.types0)
    assert list(lines) == list(want)
    for k, w in want.items():
        if isinstance(w, int):
            assert lines[k] == w, k
        elif math.isnan(w):
            assert math.isnan(lines[k]), k
        else:
            print(f"{k}: {lines[k]!r} against {w!r}: {abs(lines[k] - w) / abs(w):.2e}")
            assert abs(lines[k] - w) <= 1e-9 * abs(w), (k, lines[k], w)
    # the histograms of the scaled errors, edges from the moments: the reference's n x 4 np.histogram calls
    scale = mask_scale(got.mask0)
    edges = histogram_edges(got.moments, scale)
    scaled = errors * scale.numpy()[None]
    assert np.array_equal(edges, R.range_rule(scaled))
    hist, outside = bus_error_histograms(got.errors, edges, scale)
    hist = hist.cpu().numpy()
    for b in range(14):
        for f in range(4):
            assert np.array_equal(hist[b, f], np.histogram(scaled[:, b, f].astype(np.float64), bins=edges[f])[0]), (b, f)
    assert ((hist.sum(axis=2) + outside.cpu().numpy().sum(axis=2)) == S_TEST).all()


def test_restrictions_and_the_kinds_take_turns(split, tmp_path):
    ds, items = split
    model = _model()
    step = GraphedEvalStep(model)
    mixed = PowerFlowData(root=_mixed_root(tmp_path, samples=24), case="mixed", split=[.5, .25, .25], task="train", device=DEV)
    with pytest.raises(ValueError, match="mixed split"):
        bus_error_epoch(model, DataLoader(mixed, batch_size=8), DEV, graph=step)
    with pytest.raises(ValueError, match="mixed split"):
        bus_error_epoch(model, DataLoader([mixed[i] for i in range(len(mixed))], batch_size=8), DEV, graph=step)
    odd = [d.clone() for d in items[:8]]
    odd[5].pred_mask = 1 - odd[5].pred_mask
    with pytest.raises(ValueError, match="pred_mask differs"):
        bus_error_epoch(model, DataLoader(odd, batch_size=4), DEV, graph=step)
    # the step serves an errors epoch, then a report, then an errors epoch again: each as a fresh step would
    loader = DataLoader(ds, batch_size=BATCH, shuffle=False)
    first = bus_error_epoch(model, loader, DEV, xymean=ds.xymean, xystd=ds.xystd, graph=step)
    pi = PowerImbalance(*[t.cpu() for t in ds.get_data_means_stds()])
    rep = evaluate_report(model, loader, DEV, xystd=ds.xystd, power_imbalance=pi, graph=step)
    assert rep == evaluate_report(model, loader, DEV, xystd=ds.xystd, power_imbalance=pi, graph=GraphedEvalStep(model))
    again = bus_error_epoch(model, loader, DEV, xymean=ds.xymean, xystd=ds.xystd, graph=step)
    assert torch.equal(again.errors, first.errors) and torch.equal(again.moments, first.moments)
    assert torch.equal(first.errors, bus_error_epoch(model, loader, DEV, xymean=ds.xymean, xystd=ds.xystd).errors)


def test_error_per_feature_script_in_a_fresh_process(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "error_per_feature.py"), "--case", "14", "--synthetic-samples", "40",
                        "--batch-size", "8", "--save-predictions"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "Absolute Average of Voltage Magnitude:" in r.stdout and "Number of Loads: 9" in r.stdout and "Loads: Average of all errors:" in r.stdout
    shapes = {"errors": (12, 14, 4), "masks": (12, 14, 4), "types": (12, 14), "error_hist": (14, 4, 300), "error_hist_edges": (4, 301),
              "predictions": (12, 14, 4)}                                      # 40 samples: the last 30 % are the test split
    got = {k: np.load(tmp_path / "results" / f"14_{k}.npy") for k in shapes}
    assert {k: v.shape for k, v in got.items()} == shapes
    assert np.isfinite(got["errors"]).all() and got["errors"].dtype == np.float32 and got["error_hist_edges"].dtype == np.float64
    scaled = got["errors"] * np.where(got["masks"] == 0, np.float32(0.00001), got["masks"]).astype(np.float32)
    assert np.array_equal(got["error_hist_edges"], R.range_rule(scaled))
    for b in range(14):
        for f in range(4):
            assert np.array_equal(got["error_hist"][b, f], np.histogram(scaled[:, b, f].astype(np.float64), bins=got["error_hist_edges"][f])[0])
