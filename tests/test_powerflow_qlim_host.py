"""Pins the float64 yardstick of the Q-limited solve (tests/powerflow_qlim_ref.py) and the host side of `solve_power_flow_qlim`
(utils/powerflow.py) and `dataset_generator.write_raw` without a GPU: infinite limits are the plain Newton solve; a switched bus ends
at its limit with every mismatch under tol; the bus that stays PV keeps its limits; max_rounds exhaustion is -7; and the arguments
the function refuses before anything touches a device."""
import numpy as np
import pytest
import torch

from poweflownet_amd.datasets import PowerFlowData
from poweflownet_amd.synth import make_physical_inputs
from tests import powerflow_qlim_ref as Q
from tests import powerflow_ref as P

TOL = 1e-10


def _inputs(n, e, S, seed=1, load=0.2):
    ei, bt, rx, spec = make_physical_inputs(n, e, S, seed, load)
    return ei.numpy(), bt.numpy(), rx.numpy(), spec.numpy()


def test_infinite_limits_are_the_plain_newton_solve():
    ei, bt, rx, spec = _inputs(14, 20, 4)
    for s in range(4):
        table, status, res = P.newton(bt, spec[s], ei, rx[s], tol=TOL)
        for limits in (None, np.full((14, 2), np.inf) * [-1, 1], np.full((14, 2), np.nan)):
            got = Q.solve(bt, spec[s], ei, rx[s], limits, tol=TOL)
            assert np.array_equal(got.table, table) and got.status == status and got.residual == res
            assert got.rounds == 0 and np.array_equal(got.bus_type, bt) and got.history == [(status, 0, 0)]


@pytest.mark.parametrize("n,e,S", [(14, 20, 16), (70, 100, 4)])
def test_a_switched_bus_ends_at_its_limit_and_the_rest_within_theirs(n, e, S):
    ei, bt, rx, spec = _inputs(n, e, S)
    switched = 0
    for s in range(S):
        free, _, _ = P.newton(bt, spec[s], ei, rx[s], tol=TOL)
        limits = Q.band_limits(bt, free)
        got = Q.solve(bt, spec[s], ei, rx[s], limits, tol=TOL)
        assert got.status >= got.rounds + 1 and got.rounds >= 1 and got.status == sum(h[0] for h in got.history)
        assert len(got.history) == got.rounds + 1 and got.history[-1][1:] == (0, 0) and all(h[1] + h[2] > 0 for h in got.history[:-1])
        moved = got.bus_type != bt
        switched += int(moved.sum())
        assert (bt[moved] == 1).all() and (got.bus_type[moved] == 2).all()
        q = got.table[:, 3]
        assert np.isin(q[moved], limits[0]).all()                             # the limit, bit for bit
        dp, dq = P.mismatch(got.table, ei, rx[s])
        assert max(np.abs(dp).max(), np.abs(dq).max()) < TOL + 64 * P.EPS64 * P.scale(got.table, ei, rx[s]).max()
        still = got.bus_type == 1
        assert (q[still] <= limits[still, 1] + TOL).all() and (q[still] >= limits[still, 0] - TOL).all()
        assert np.array_equal(got.table[got.bus_type != 2, 0], spec[s][got.bus_type != 2, 0])      # a switched bus's Vm is solved
        assert got.margin > 1e-4
    assert switched > S


def test_exhausted_rounds_are_status_minus_seven():
    ei, bt, rx, spec = _inputs(14, 20, 16)
    full = [Q.solve(bt, spec[s], ei, rx[s], Q.band_limits(bt, P.newton(bt, spec[s], ei, rx[s], tol=TOL)[0]), tol=TOL) for s in range(16)]
    two = [s for s in range(16) if full[s].rounds == 2]
    assert two
    for s in two:
        limits = Q.band_limits(bt, P.newton(bt, spec[s], ei, rx[s], tol=TOL)[0])
        short = Q.solve(bt, spec[s], ei, rx[s], limits, tol=TOL, max_rounds=1)
        assert short.status == Q.PF_QLIM_ROUNDS == -7 and short.table is None and short.rounds == 1 and np.array_equal(short.bus_type, bt)
        assert Q.solve(bt, spec[s], ei, rx[s], limits, tol=TOL, max_rounds=2).status == full[s].status
    none = Q.solve(bt, spec[0], ei, rx[0], Q.band_limits(bt, P.newton(bt, spec[0], ei, rx[0], tol=TOL)[0]), tol=TOL, max_rounds=0)
    assert none.status == -7 and none.rounds == 0


def test_status_text():
    from poweflownet_amd.utils.powerflow import STATUS
    assert "max_rounds" in STATUS[-7] and sorted(STATUS) == [-7, -6, -5, -4, -3, -2, -1]


def test_host_side_refusals():
    from poweflownet_amd.utils.powerflow import max_unknowns, solve_power_flow_qlim
    ei, bt, rx, spec = make_physical_inputs(5, 6, 2, seed=1)
    with pytest.raises(ValueError, match="sparse route"):
        solve_power_flow_qlim(bt, spec, ei, rx, route="sparse")
    with pytest.raises(ValueError, match="route"):
        solve_power_flow_qlim(bt, spec, ei, rx, route="cover")
    with pytest.raises(RuntimeError, match="bus_type must be"):
        solve_power_flow_qlim(bt[None].expand(3, 5), spec, ei, rx)
    with pytest.raises(RuntimeError, match="bus_type must be"):
        solve_power_flow_qlim(bt.double(), spec, ei, rx)
    with pytest.raises(RuntimeError, match="q_limits must be"):
        solve_power_flow_qlim(bt, spec, ei, rx, torch.zeros(5, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="q_limits must be"):
        solve_power_flow_qlim(bt, spec, ei, rx, torch.zeros(5, 2))
    with pytest.raises(RuntimeError, match="rx must be"):
        solve_power_flow_qlim(bt, spec, ei, rx[:, :5])
    with pytest.raises(RuntimeError, match="init must be"):
        solve_power_flow_qlim(bt, spec, ei, rx, init=torch.zeros(2, 5, 1))
    with pytest.raises(ValueError, match="max_rounds"):
        solve_power_flow_qlim(bt, spec, ei, rx, max_rounds=-1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        solve_power_flow_qlim(bt[None].expand(2, 5), spec, ei, rx, torch.zeros(2, 5, 2, dtype=torch.float64))
    # every non-slack bus may end PQ: 2 (n - 1) unknowns are what the launch is sized for, whatever the types are
    cap = max_unknowns()
    n = cap // 2 + 2
    all_pv = torch.ones(n, dtype=torch.int64)
    all_pv[0] = 0
    args = (torch.zeros(1, n, 4, dtype=torch.float64), torch.zeros(2, 1, dtype=torch.int64), torch.ones(1, 1, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="sparse factorisation"):
        solve_power_flow_qlim(all_pv, *args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                 # one bus fewer passes the cap
        solve_power_flow_qlim(all_pv[:n - 1], args[0][:, :n - 1], *args[1:])


def test_the_library_sizes_the_worst_case():
    from poweflownet_amd import _lib as L
    lib = L.load()
    assert lib.pfn_powerflow_qlim_workspace_bytes(8, 70, 0) == 0                # (70, 100) runs in LDS

    def slab(n):                                                               # m_max rows of m_max | 1 floats, rounded to 4 floats
        m = 2 * (n - 1)
        return (m * (m | 1) + 3) // 4 * 4 * 4
    assert lib.pfn_powerflow_qlim_workspace_bytes(4, 118, 0) == 4 * slab(118) > 0            # 118 leaves it
    assert lib.pfn_powerflow_qlim_workspace_bytes(4, 118, 1) == 0 and lib.pfn_powerflow_qlim_workspace_bytes(4, 14, 2) == 4 * slab(14)
    assert lib.pfn_powerflow_qlim_workspace_bytes(4, L.load().pfn_powerflow_max_unknowns() // 2 + 2, 2) == 0


def test_per_sample_types_round_trip_through_powerflowdata(tmp_path):
    import dataset_generator
    ei, bt, rx, spec = _inputs(14, 20, 10, seed=8)
    out = [Q.solve(bt, spec[s], ei, rx[s], Q.band_limits(bt, P.newton(bt, spec[s], ei, rx[s])[0])) for s in range(10)]
    tables, types = np.stack([o.table for o in out]), np.stack([o.bus_type for o in out])
    assert len({t.tobytes() for t in types}) > 1 and (types != bt).any()
    node_path, _ = dataset_generator.write_raw(str(tmp_path), "14", types, ei, rx, tables)
    node = np.load(node_path)
    assert np.array_equal(node[:, :, 1], types) and np.array_equal(node[:, :, 2:], tables)
    ds = PowerFlowData(root=str(tmp_path), case="14", split=[.5, .2, .3], task="test", normalize=False)
    assert len(ds) == 3
    masks = torch.tensor(PowerFlowData.bus_type_mask)
    for k in range(3):
        d = ds[k]
        assert torch.equal(d.bus_type, torch.from_numpy(types[7 + k])) and torch.equal(d.pred_mask, masks[d.bus_type].to(d.pred_mask.dtype))
        assert torch.equal(d.x, d.y * (1 - d.pred_mask))
    with pytest.raises(AssertionError):
        dataset_generator.write_raw(str(tmp_path), "14", types[:9], ei, rx, tables)
