"""csrc/topology.hip on the device against the float-free numpy yardstick (tests/topology_ref.py, itself checked without a GPU by
tests/test_topology_host.py): every output of `perturb_topology` and `unsupplied_buses` bit for bit, the draw's independence of
its batch, containment of bad input, and the loop the kernel closes -- generate a solved perturbed set, check it, train on it."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

from poweflownet_amd.synth import make_physical_inputs, make_topology
from poweflownet_amd.utils.topology import perturb_topology, unsupplied_buses
from tests import branch_ref as R
from tests import topology_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _base(n, e):
    return make_topology(n, e).numpy()


def _equal(got, want):
    out, source, status = want
    assert got.edge_index.dtype == torch.int64 and got.source.dtype == torch.int32 and got.status.dtype == torch.int32
    assert torch.equal(got.status.cpu(), torch.from_numpy(status))
    assert torch.equal(got.source.cpu(), torch.from_numpy(source))
    assert torch.equal(got.edge_index.cpu(), torch.from_numpy(out))


# ------------------------------------------------------------------------------------------------ bit equality
@pytest.mark.parametrize("n, e, r, a, S", [(5, 6, 1, 0, 64),          # the smallest grid
                                           (14, 20, 2, 1, 256),       # the structure case of the host tests
                                           (8, 10, 3, 0, 256),        # the give-up path
                                           (118, 186, 3, 2, 16),      # case118
                                           (300, 520, 5, 3, 8),       # lines and buses beyond one pass of the 256-thread block
                                           (6470, 9005, 3, 2, 2)])    # the big-LDS shape, 1024 threads (a draw is connected with
                                                                      # probability ~0.48: no draw in 20 is ~2e-6 per sample)
def test_draw_is_the_yardsticks_bit_for_bit(n, e, r, a, S):
    base = _base(n, e)
    want = T.perturb(base, n, S, r, a, seed=7)
    got = perturb_topology(_dev(base), n, num_samples=S, remove=r, add=a, seed=7)
    assert tuple(got.edge_index.shape) == (S, 2, e - r + a)
    _equal(got, want)
    status = want[2]
    print(f"({n}, {e}) r {r} a {a}: {int((status == -1).sum())} of {S} without a draw, mean attempts {status[status > 0].mean():.2f}")
    if (n, e) == (8, 10):
        assert 0 < (status == -1).sum() < S                                   # both outcomes, on the device
    else:
        assert (status >= 1).all()
    # the second opinion: the kept lines of an accepted sample supply every bus (the added ones come behind them)
    kept = got.edge_index[:, :, :e - r]
    count = unsupplied_buses(kept[got.status >= 1], n)
    assert count.dtype == torch.int32 and int(count.abs().sum()) == 0


def test_options_reach_the_kernel():
    """seed beyond 32 bits, a root that is not bus 0, one attempt only, a large first_sample: all part of the counter / key."""
    n, e = 14, 20
    base = _base(n, e)
    for kw in (dict(seed=(0xDEADBEEF << 32) | 5), dict(root=9), dict(max_attempts=1), dict(first_sample=2 ** 32 - 64)):
        args = dict(dict(seed=3, first_sample=0, root=0, max_attempts=20), **kw)
        _equal(perturb_topology(_dev(base), n, num_samples=64, remove=3, add=2, **args), T.perturb(base, n, 64, 3, 2, **args))


# ---------------------------------------------------------------------------------------- many relaxation rounds
def test_ring_needs_hundreds_of_rounds():
    n = 300
    ring = np.stack([np.arange(n), (np.arange(n) + 1) % n]).astype(np.int64)
    got = perturb_topology(_dev(ring), n, num_samples=32, remove=1, seed=11)
    assert bool((got.status == 1).all())                                      # a ring less one line is a path: always connected
    assert int(unsupplied_buses(got.edge_index, n).abs().sum()) == 0
    _equal(got, T.perturb(ring, n, 32, 1, 0, seed=11))
    with pytest.raises(ValueError, match="cannot connect"):                   # r = 2: 298 lines cannot connect 300 buses
        perturb_topology(_dev(ring), n, num_samples=1, remove=2)
    chord = np.concatenate([ring, np.array([[0], [150]])], axis=1)
    # two lines of one arc cut the buses between them off, about half of the draws: with two attempts a quarter of the samples
    # finds none (with twenty, one in a million)
    want = T.perturb(chord, n, 64, 2, 0, seed=11, max_attempts=2)
    assert (want[2] == -1).sum() > 0 and (want[2] == 1).sum() > 0 and (want[2] == 2).sum() > 0
    _equal(perturb_topology(_dev(chord), n, num_samples=64, remove=2, seed=11, max_attempts=2), want)


# ------------------------------------------------------------------------------------------------ unsupplied_buses
def test_unsupplied_buses_counts():
    n = 12
    grid = _base(n, 16)
    island = grid.copy()
    cut = np.isin(island, [9, 10, 11]).any(axis=0)                            # buses 9, 10, 11 keep the lines among themselves only
    island = np.concatenate([island[:, ~cut], np.array([[9, 10], [10, 11]])], axis=1)
    pad = 16 - island.shape[1]
    assert pad >= 0
    island = np.concatenate([island, np.repeat(island[:, :1], pad, axis=1)], axis=1)    # (a repeated line changes nothing)
    lonely = np.where(grid == 0, 1, grid)                                     # no line touches bus 0: an isolated root
    bad = grid.copy()
    bad[1, 5] = n                                                             # a line to bus n
    neg = grid.copy()
    neg[0, 0] = -1
    lists = np.stack([grid, island, lonely, bad, grid, neg])
    want = T.unsupplied_batch(lists, n)
    assert want.tolist()[:2] == [0, 3] and want[2] == n - 1 and want.tolist()[3:] == [-4, 0, -4]
    got = unsupplied_buses(_dev(lists), n)
    assert torch.equal(got.cpu(), torch.from_numpy(want))                     # -4 for the samples with the bad line only
    for k, one in enumerate(lists):                                           # [2, e] against [S, 2, e]
        assert unsupplied_buses(_dev(one), n).tolist() == [int(want[k])]
    for root in (3, 10):
        assert torch.equal(unsupplied_buses(_dev(lists), n, root=root).cpu(), torch.from_numpy(T.unsupplied_batch(lists, n, root)))
    assert unsupplied_buses(torch.zeros(2, 2, 0, dtype=torch.int64, device=DEV), 4).tolist() == [3, 3]    # no line at all
    big = _base(6470, 9005)                                                   # the 1024-thread shape
    assert unsupplied_buses(_dev(big), 6470).tolist() == [0]
    assert unsupplied_buses(_dev(big[:, :6000]), 6470).tolist() == [int(T.unsupplied(big[:, :6000], 6470))]


# ------------------------------------------------------------------------------------------------ independence
def test_a_draw_does_not_depend_on_its_batch():
    n, e = 118, 186
    base = _dev(_base(n, e))
    kw = dict(remove=3, add=2, seed=5)
    whole = perturb_topology(base, n, num_samples=64, **kw)
    lo, hi = perturb_topology(base, n, num_samples=32, **kw), perturb_topology(base, n, num_samples=32, first_sample=32, **kw)
    for name in ("edge_index", "source", "status"):
        assert torch.equal(getattr(whole, name), torch.cat([getattr(lo, name), getattr(hi, name)])), name
    other = perturb_topology(base, n, num_samples=64, remove=3, add=2, seed=6)
    assert not torch.equal(other.source, whole.source) and not torch.equal(other.edge_index[:, :, -2:], whole.edge_index[:, :, -2:])


# ------------------------------------------------------------------------------------------------ containment
def test_bad_base_line_and_the_empty_perturbation():
    n, e = 14, 20
    base = _base(n, e)
    bad = base.copy()
    bad[1, 7] = n
    got = perturb_topology(_dev(bad), n, num_samples=16, remove=2, add=1)
    assert bool((got.status == -4).all()) and bool((got.edge_index == -1).all()) and bool((got.source == -1).all())
    _equal(got, T.perturb(bad, n, 16, 2, 1))
    same = perturb_topology(_dev(base), n, num_samples=8)
    assert bool((same.status == 1).all())
    assert torch.equal(same.edge_index.cpu(), torch.from_numpy(base).expand(8, 2, e))
    assert torch.equal(same.source.cpu(), torch.arange(e, dtype=torch.int32).expand(8, e))
    none = perturb_topology(_dev(base), n, num_samples=0, remove=1)
    assert tuple(none.edge_index.shape) == (0, 2, 19) and tuple(none.status.shape) == (0,)


def test_the_draw_is_capturable():
    """No sync, no allocation inside the call's launch: a hipGraph holding it replays the same draw into the same tensors."""
    n, e = 14, 20
    base = _dev(_base(n, e))
    want = perturb_topology(base, n, num_samples=32, remove=2, add=1, seed=9)
    torch.cuda.synchronize()
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            got = perturb_topology(base, n, num_samples=32, remove=2, add=1, seed=9)
            count = unsupplied_buses(got.edge_index, n)
    got.edge_index.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got.edge_index, want.edge_index) and torch.equal(got.source, want.source) and torch.equal(got.status, want.status)
    assert int(count.abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ end to end
def _imbalance_bound(table32, ei, rx):
    """The bound tests/test_gpu_powerflow.py holds solved tables to, re-stated: every line message the physics kernel forms in fp32
    is within C_BOUND EPS scale of its exact value (tests/branch_ref.py: the bound the branch-flow kernel is held to for the same
    expressions, scale = column 1 of the yardstick's scales), a bus sums the messages of the lines at it, P_i and Q_i carry their
    own fp32 rounding, and dP^2 + dQ^2 has two such terms: mean over (sample, bus) of
    2 (C_BOUND EPS sum of the scales at the bus + EPS (|P_i| + |Q_i|))^2.  `ei` is [S, 2, e] here: a line list per sample."""
    S, n = table32.shape[:2]
    _, scales = R.flows(table32, ei, rx)
    at_bus = np.zeros((S, n))
    for s in range(S):
        np.add.at(at_bus[s], ei[s, 0], scales[s, :, 1])
        np.add.at(at_bus[s], ei[s, 1], scales[s, :, 1])
    t = table32.astype(np.float64)
    return float(np.mean(2 * (R.C_BOUND * R.EPS * at_bus + R.EPS * (np.abs(t[:, :, 2]) + np.abs(t[:, :, 3]))) ** 2))


def test_generate_check_and_train_on_a_perturbed_set(tmp_path):
    import dataset_generator
    from poweflownet_amd.data import DataLoader
    from poweflownet_amd.datasets import PowerFlowData
    from poweflownet_amd.loss import MSELoss
    from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
    from poweflownet_amd.optim import FlatAdamW
    from poweflownet_amd.utils.custom_loss_functions import PowerImbalance
    from poweflownet_amd.utils.training import GraphedTrainStep, train_epoch
    root = str(tmp_path / "set")
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        assert dataset_generator.main(["--case", "14", "--samples", "32", "-r", "1", "-a", "1", "--root", root]) == 0
    print(text.getvalue())
    assert "dropped: 0" in text.getvalue() and "drawn again: 0" in text.getvalue()
    node = np.load(tmp_path / "set" / "raw" / "case14perturbed1r1a_node_features.npy")
    edge = np.load(tmp_path / "set" / "raw" / "case14perturbed1r1a_edge_features.npy")
    assert node.shape == (32, 14, 6) and edge.shape == (32, 20, 4) and np.isfinite(node).all() and np.isfinite(edge).all()
    S, n, e = 32, 14, 20
    ei = np.ascontiguousarray(edge[:, :, :2].transpose(0, 2, 1)).astype(np.int64)
    assert (ei == edge[:, :, :2].transpose(0, 2, 1)).all()
    # the stored lines are the draw of (seed 0, samples 0..31), with the parameters of the lines they are or copy
    want = T.perturb(_base(n, e), n, S, 1, 1, seed=0)
    assert (want[2] >= 1).all() and (ei == want[0]).all()
    rx0 = make_physical_inputs(n, e, S, 0)[2].numpy()
    assert (edge[:, :, 2:] == np.take_along_axis(rx0, want[1][:, :, None].astype(np.int64), axis=1)).all()
    assert int(unsupplied_buses(_dev(ei), n).abs().sum()) == 0

    ds = PowerFlowData(root=root, case="14perturbed1r1a", split=[.5, .25, .25], task="train", device=DEV)
    assert len(ds) == 16 and not ds._blocks[0].static_topology and ds.can_gather_topologies()

    # PowerImbalance of the whole set, formed from the file's fp64 values cast to fp32
    table32, rx32 = node[:, :, 2:].astype(np.float32), edge[:, :, 2:].astype(np.float32)
    loss_fn = PowerImbalance(torch.zeros(1, 4), torch.ones(1, 4), torch.zeros(1, 2), torch.ones(1, 2))
    flat_ei = _dev((ei + n * np.arange(S)[:, None, None]).transpose(1, 0, 2).reshape(2, S * e))
    got = float(loss_fn(_dev(table32.reshape(S * n, 4)), flat_ei, _dev(rx32.reshape(S * e, 2))))
    bound = _imbalance_bound(table32, ei, rx32.astype(np.float64))
    # ... and of the same tables on the UNPERTURBED grid: what a set that ignored its own line lists would show
    base_ei = np.broadcast_to(_base(n, e), (S, 2, e))
    flat_base = _dev((base_ei + n * np.arange(S)[:, None, None]).transpose(1, 0, 2).reshape(2, S * e))
    wrong = float(loss_fn(_dev(table32.reshape(S * n, 4)), flat_base, _dev(rx32.reshape(S * e, 2))))
    print(f"PowerImbalance: generated perturbed set {got:.3e}, bound {bound:.3e}; on the base grid's lines {wrong:.3e}")
    assert got < bound and wrong > 1e3 * bound

    torch.manual_seed(3)
    model = MaskEmbdMultiMPN(4, 2, 4, 32, 3, 2, 0.0).to(DEV)
    mse, opt = MSELoss(), FlatAdamW(model, lr=1e-3)
    step = GraphedTrainStep(model, mse, opt, per_sample_topology=True)
    assert step.topologies_supported(ds, DEV)
    loss = train_epoch(model, DataLoader(ds, batch_size=8, shuffle=False), mse, opt, DEV, graph=step)
    assert np.isfinite(loss) and list(step._topo_children) == [8]


def test_generator_without_perturbation_is_unchanged(tmp_path):
    """r = a = 0: the files, their names and their content are those of the generator as it was (one grid for all samples)."""
    import dataset_generator
    with contextlib.redirect_stdout(io.StringIO()):
        assert dataset_generator.main(["--case", "14", "--samples", "8", "--root", str(tmp_path)]) == 0
    edge = np.load(tmp_path / "raw" / "case14_edge_features.npy")
    assert edge.shape == (8, 20, 4) and (edge[:, :, :2] == _base(14, 20).T).all()
    with pytest.raises(SystemExit):
        with contextlib.redirect_stderr(io.StringIO()):
            dataset_generator.main(["--case", "14", "--samples", "8", "--root", str(tmp_path), "-r", "-1"])
