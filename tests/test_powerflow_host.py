"""The float64 yardstick of the power-flow solver (tests/powerflow_ref.py) and the generator's file layout, without a GPU: the
yardstick converges where tests/test_gpu_powerflow.py holds the kernel to it, fails where that file expects failures, and a table it
solved round-trips through the raw files into `PowerFlowData`."""
import numpy as np
import pytest
import torch

from poweflownet_amd.datasets import PowerFlowData
from poweflownet_amd.synth import make_graph, make_physical_inputs, make_topology
from tests import powerflow_ref as P


def _inputs(n, e, S, seed, load=0.2):
    ei, bt, rx, spec = make_physical_inputs(n, e, S, seed, load)
    return ei.numpy(), bt.numpy(), rx.numpy(), spec.numpy()


def test_make_physical_inputs_layout():
    ei, bt, rx, spec = make_physical_inputs(14, 20, 3, seed=5)
    assert torch.equal(ei, make_topology(14, 20)) and torch.equal(bt, make_graph(14, 20).bus_type)
    assert rx.dtype == spec.dtype == torch.float64 and tuple(rx.shape) == (3, 20, 2) and tuple(spec.shape) == (3, 14, 4)
    rx, spec, bt = rx.numpy(), spec.numpy(), bt.numpy()
    assert (rx[..., 0] >= 0.005).all() and (rx[..., 0] <= 0.03).all() and (rx[..., 1] >= 0.03).all() and (rx[..., 1] <= 0.15).all()
    assert (spec[:, bt != 2, 0] >= 1.0).all() and (spec[:, bt != 2, 0] <= 1.05).all() and (spec[:, bt == 2, 0] == 0).all()
    assert (spec[:, :, 1] == 0).all() and (spec[:, bt != 2, 3] == 0).all() and (spec[:, bt == 0, 2] == 0).all()
    assert (spec[:, bt == 2, 2] > 0).all() and (spec[:, bt == 1, 2] < 0).all()
    # generation within +-20 % of the demand; the first samples do not depend on how many are drawn
    assert np.allclose(-spec[:, bt == 1, 2].sum(axis=1), spec[:, bt == 2, 2].sum(axis=1), rtol=0.2)
    again = make_physical_inputs(14, 20, 2, seed=5)
    assert np.array_equal(again[2].numpy(), rx[:2]) and np.array_equal(again[3].numpy(), spec[:2])


@pytest.mark.parametrize("n,e,S,load", [(5, 6, 8, 0.2), (14, 20, 16, 0.2), (118, 186, 4, 0.2), (14, 20, 16, 0.5)])
def test_the_yardstick_converges(n, e, S, load):
    ei, bt, rx, spec = _inputs(n, e, S, seed=n + 1, load=load)
    for s in range(S):
        table, status, res = P.newton(bt, spec[s], ei, rx[s], tol=1e-10, max_iter=10)
        assert 1 <= status <= 10 and res < 1e-10, (s, status, res)
        dp, dq = P.mismatch(table, ei, rx[s])
        bound = 1e-10 + 64 * P.EPS64 * P.scale(table, ei, rx[s])
        assert (np.abs(dp) <= bound).all() and (np.abs(dq) <= bound).all()
        # given entries are kept, the rest is solved
        assert np.array_equal(table[bt != 2, 0], spec[s][bt != 2, 0]) and np.array_equal(table[bt != 0, 2], spec[s][bt != 0, 2])
        assert np.array_equal(table[bt == 2, 3], spec[s][bt == 2, 3]) and table[bt == 0, 1] == 0


def test_an_fp32_solve_reaches_the_same_solution():
    ei, bt, rx, spec = _inputs(14, 20, 4, seed=3)
    f32 = lambda A, F: np.linalg.solve(A.astype(np.float32), F.astype(np.float32)).astype(np.float64)      # noqa: E731
    for s in range(4):
        want, _, _ = P.newton(bt, spec[s], ei, rx[s], tol=1e-10)
        got, status, _ = P.newton(bt, spec[s], ei, rx[s], tol=1e-10, solve=f32)
        bound = 2e-10 * P.jacobian_inverse_norm(want, bt, ei, rx[s])
        assert 1 <= status <= 10 and np.abs(got[:, 0] - want[:, 0]).max() <= bound and np.abs(got[:, 1] - want[:, 1]).max() * P.RAD <= bound


def test_the_jacobian_is_the_derivative_of_the_line_sums():
    ei, bt, rx, spec = _inputs(14, 20, 1, seed=9)
    table, _, _ = P.newton(bt, spec[0], ei, rx[0])
    ang, mag = P.unknowns(bt)
    A = P.flow_jacobian(table[:, 0].copy(), table[:, 1] * P.RAD, bt, ei, rx[0])

    def sums(x):
        t = table.copy()
        t[ang, 1] = x[:len(ang)] / P.RAD
        t[mag, 0] = x[len(ang):]
        sp, sq = P.line_sums(t, ei, rx[0])
        return np.concatenate([sp[ang], sq[mag]])
    x0 = np.concatenate([table[ang, 1] * P.RAD, table[mag, 0]])
    h = 1e-6
    num = np.stack([(sums(x0 + h * np.eye(len(x0))[k]) - sums(x0 - h * np.eye(len(x0))[k])) / (2 * h) for k in range(len(x0))], axis=1)
    assert np.abs(num - A).max() <= 1e-6 * np.abs(A).max()


def test_too_much_load_converges_for_none():
    ei, bt, rx, spec = _inputs(14, 20, 32, seed=2, load=2.0)
    assert [P.newton(bt, spec[s], ei, rx[s], tol=1e-10)[1] for s in range(32)] == [-1] * 32


def test_a_bus_without_a_line_is_singular():
    ei, bt, rx, spec = _inputs(14, 20, 1, seed=4)
    lone = 13
    ei = np.where(ei == lone, 1, ei)                                          # its lines go to bus 1 instead
    assert not (ei == lone).any()
    vm, th, _ = P.flat_start(bt, spec[0])
    A = P.flow_jacobian(vm, th, bt, ei, rx[0])
    assert (A == 0).all(axis=1).sum() == 2 and np.linalg.matrix_rank(A) == A.shape[0] - 2      # its P row and its Q row
    assert P.newton(bt, spec[0], ei, rx[0])[1] == -2


def test_dc_yardstick():
    ei, bt, rx, spec = _inputs(118, 186, 2, seed=6)
    for s in range(2):
        table, inv_norm = P.dc_solve(bt, spec[s], ei, rx[s])
        F = P.dc_mismatch(table, ei, rx[s], bt)
        assert (np.abs(F) <= 64 * P.EPS64 * P.dc_scale(table, ei, rx[s])).all() and inv_norm > 0
        assert np.isnan(table[:, 3]).all() and (table[bt == 2, 0] == 1).all() and np.array_equal(table[bt != 2, 0], spec[s][bt != 2, 0])


def test_the_raw_files_round_trip_through_powerflowdata(tmp_path):
    import dataset_generator
    ei, bt, rx, spec = _inputs(14, 20, 10, seed=8)
    tables = np.stack([P.newton(bt, spec[s], ei, rx[s])[0] for s in range(10)])
    node_path, edge_path = dataset_generator.write_raw(str(tmp_path), "14", bt, ei, rx, tables)
    node, edge = np.load(node_path), np.load(edge_path)
    assert node.shape == (10, 14, 6) and edge.shape == (10, 20, 4)
    assert np.array_equal(node[:, :, 0], np.broadcast_to(np.arange(14), (10, 14))) and np.array_equal(node[:, :, 1], np.broadcast_to(bt, (10, 14)))
    assert np.array_equal(node[:, :, 2:], tables) and np.array_equal(edge[:, :, :2], np.broadcast_to(ei.T, (10, 20, 2))) and np.array_equal(edge[:, :, 2:], rx)
    ds = PowerFlowData(root=str(tmp_path), case="14", split=[.5, .2, .3], task="test", normalize=False)
    assert len(ds) == 3
    d = ds[0]
    assert torch.equal(d.edge_index, torch.from_numpy(ei)) and torch.equal(d.bus_type, torch.from_numpy(bt))
    assert torch.equal(d.y, torch.from_numpy(tables[7]).float()) and torch.equal(d.edge_attr, torch.from_numpy(rx[7]).float())
    assert torch.equal(d.x, d.y * (1 - d.pred_mask))


def test_no_cpu_path():
    from poweflownet_amd.utils.powerflow import solve_power_flow
    ei, bt, rx, spec = make_physical_inputs(5, 6, 2, seed=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        solve_power_flow(bt, spec, ei, rx)
