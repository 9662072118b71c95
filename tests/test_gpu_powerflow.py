"""The batched power-flow solver on the device: `pfn_powerflow_solve` (csrc/powerflow.hip) through `solve_power_flow`, held to the
float64 yardstick of tests/powerflow_ref.py with tol = 1e-10 and max_iter = 10 --
  residual   the yardstick's mismatch of the WRITTEN table, at all buses, <= tol + 64 * 2^-52 * scale_i: the kernel stopped under tol in
             its own fp64, the rest is the rounding of evaluating the sums again;
  solution   Vm and Va (radians) within 2 tol ||J^-1||_inf of the yardstick's own solution, J at that solution: two points whose
             mismatch is under tol each are that close to first order;
-- on the LDS route, the global route and the shape that no longer fits LDS; bit-for-bit independence of a sample from its batch;
failures that stay local; the DC mode; and the closed loop against the existing physics kernel (`PowerImbalance` on the solved table,
with tests/branch_ref.py's C_BOUND, EPS and per-line scales as they stand) and the tools on top (dataset_generator.py, dc_error.py).

Worst ratios measured on an MI355X (bound 1; each test prints its own): residual 0.85 at (14, 20, 64), 3.4e-4 at m = 115 and m = 195;
distance to the yardstick's solution 5.8e-3; DC 0.022 / 7.3e-4; PowerImbalance of the solved table 8.5e-12 against a bound of 3.6e-7
(flat start 0.48).  3-4 Jacobian solves everywhere, 2 in DC mode.  DESIGN.md section 7h."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.synth import make_physical_inputs, make_topology
from poweflownet_amd.utils.powerflow import solve_power_flow
from tests import powerflow_ref as P
from tests.powerflow_checks import DEV, TOL, _check_given, _dev, _distance, _imbalance_bound, _residual_ratio, _run

pytestmark = pytest.mark.gpu
MAX_ITER = 10


class _Case:
    """Inputs of one shape on the host, the yardstick's solutions and ||J^-1|| computed once."""

    def __init__(self, n, e, S, seed, load=0.2, types=None):
        ei, bt, rx, spec = make_physical_inputs(n, e, S, seed, load)
        self.n, self.e, self.S = n, e, S
        self.ei, self.bt, self.rx, self.spec = ei.numpy(), bt.numpy().copy(), rx.numpy(), spec.numpy().copy()
        if types == "no_pv":                                   # the PV buses become PQ buses: their P stays, their Q is 0
            self.bt[self.bt == 1] = 2
        elif types == "no_pq":                                 # the PQ buses become PV buses that hold 1.02
            self.spec[:, self.bt == 2, 0] = 1.02
            self.bt[self.bt == 2] = 1
        self.m = (n - 1) + int((self.bt == 2).sum())

    @functools.cached_property
    def ref(self):
        out = [P.newton(self.bt, self.spec[s], self.ei, self.rx[s], tol=TOL, max_iter=MAX_ITER) for s in range(self.S)]
        assert all(1 <= st <= MAX_ITER for _, st, _ in out), [st for _, st, _ in out]
        return np.stack([t for t, _, _ in out])

    @functools.cached_property
    def inv_norm(self):
        return np.array([P.jacobian_inverse_norm(self.ref[s], self.bt, self.ei, self.rx[s]) for s in range(self.S)])

    def solve(self, rows=slice(None), ei=None, **kw):
        ei = self.ei if ei is None else ei
        kw = {"tol": TOL, "max_iter": MAX_ITER, **kw}
        return solve_power_flow(_dev(self.bt), _dev(self.spec[rows]), _dev(ei[rows] if ei.ndim == 3 else ei), _dev(self.rx[rows]), **kw)


@functools.lru_cache(maxsize=None)
def _case(n, e, S, seed=1, load=0.2, types=None):
    return _Case(n, e, S, seed, load, types)


def _check_ac(case, res, what):
    table, status = res.table.cpu().numpy(), res.status.cpu().numpy()
    assert table.shape == (case.S, case.n, 4) and table.dtype == np.float64 and int(res.flags.item()) == 0
    assert ((status >= 1) & (status <= MAX_ITER)).all(), (what, status)
    assert torch.equal(res.iterations, res.status) and bool((res.residual < TOL).all())
    worst_f = _residual_ratio(case, table)
    worst_x = max(float(_distance(table[s], case.ref[s]) / (2 * TOL * case.inv_norm[s])) for s in range(case.S))
    _check_given(case, table)
    print(f"{what}: route {res.route}, solves {status.min()}..{status.max()} (mean {status.mean():.2f}), worst |mismatch| / bound {worst_f:.3g}, "
          f"worst |x - yardstick| / (2 tol ||J^-1||) {worst_x:.3g}")
    assert worst_f <= 1.0 and worst_x <= 1.0, (what, worst_f, worst_x)


# ------------------------------------------------------------------------------------------------- residual, routes
@pytest.mark.parametrize("n,e,S", [(5, 6, 3), (14, 20, 64), (70, 100, 16), (118, 186, 8)])
def test_residual_and_solution_on_the_lds_route(n, e, S):
    case = _case(n, e, S)
    assert case.m == {5: 7, 14: 22, 70: 115, 118: 195}[n]
    res = case.solve()
    assert res.route == "lds"
    _check_ac(case, res, f"n {n} e {e} S {S} m {case.m}")
    assert torch.equal(case.solve(route="lds").table, res.table)


@pytest.mark.parametrize("n,e,S", [(14, 20, 64), (70, 100, 16)])
def test_the_global_route_meets_the_same_bounds(n, e, S):
    case = _case(n, e, S)
    res = case.solve(route="global")
    assert res.route == "global"
    _check_ac(case, res, f"global route, n {n} e {e} S {S} m {case.m}")


def test_beyond_lds_auto_takes_the_global_route():
    case = _case(130, 200, 4)
    assert case.m == 215
    res = case.solve()
    assert res.route == "global"
    _check_ac(case, res, "n 130 e 200 S 4 m 215")
    with pytest.raises(RuntimeError, match=r"code -1.*LDS"):
        case.solve(route="lds")


def test_more_unknowns_than_the_dense_cap_is_refused():
    from poweflownet_amd.utils.powerflow import max_unknowns
    cap = max_unknowns()
    assert cap >= 1024
    n = cap + 2                                                # one slack, the rest PV: m = n - 1 = cap + 1
    bt = torch.ones(n, dtype=torch.int32, device=DEV)
    bt[0] = 0
    with pytest.raises(RuntimeError, match="sparse factorisation"):
        solve_power_flow(bt, torch.zeros(1, n, 4, dtype=torch.float64, device=DEV), torch.zeros(2, 1, dtype=torch.int64, device=DEV),
                         torch.ones(1, 1, 2, dtype=torch.float64, device=DEV))


@pytest.mark.parametrize("types,m", [("no_pv", 26), ("no_pq", 13)])
def test_block_edge_cases(types, m):
    case = _case(14, 20, 8, seed=2, types=types)
    assert case.m == m
    _check_ac(case, case.solve(), types)
    _check_ac(case, case.solve(route="global"), types + ", global route")


# ---------------------------------------------------------------------------------------------------- independence
def test_a_sample_does_not_depend_on_its_batch():
    case = _case(14, 20, 8, seed=3)
    lists = np.stack([make_topology(14, 20, seed=k).numpy() for k in range(4)])
    assert len({lists[k].tobytes() for k in range(4)}) == 4
    batch = case.solve(rows=slice(0, 4), ei=lists)
    assert bool((batch.status >= 1).all())
    for k in range(4):                                         # [S, 2, e] against four single-sample calls in [2, e] form
        one = case.solve(rows=slice(k, k + 1), ei=lists[k])
        assert torch.equal(one.table[0], batch.table[k]) and int(one.status[0]) == int(batch.status[k])
        assert torch.equal(one.residual[0], batch.residual[k])
    whole = case.solve()
    a, b = case.solve(rows=slice(0, 3)), case.solve(rows=slice(3, 8))
    assert torch.equal(torch.cat([a.table, b.table]), whole.table) and torch.equal(torch.cat([a.status, b.status]), whole.status)
    assert torch.equal(torch.cat([a.residual, b.residual]), whole.residual)
    assert torch.equal(case.solve().table, whole.table)


# -------------------------------------------------------------------------------------------------------- failures
def test_failures_stay_local():
    n, e = 14, 20
    good, heavy = _case(n, e, 8, seed=4), _case(n, e, 8, seed=4, load=2.0)
    lists = np.stack([good.ei] * 8)
    spec, rx = good.spec.copy(), good.rx.copy()
    lists[2] = np.where(lists[2] == 13, 1, lists[2])           # sample 2: bus 13 has no line
    spec[5], rx[5] = heavy.spec[5], heavy.rx[5]                # sample 5: ten times the load
    lists[6, 1, 7] = n                                         # sample 6: a line to bus id n
    bt = _dev(good.bt)
    res = solve_power_flow(bt, _dev(spec), _dev(lists), _dev(rx), tol=TOL, max_iter=MAX_ITER)
    clean = solve_power_flow(bt, _dev(good.spec), _dev(np.stack([good.ei] * 8)), _dev(good.rx), tol=TOL, max_iter=MAX_ITER)
    status = res.status.tolist()
    assert [status[k] for k in (2, 5, 6)] == [-2, -1, -4] and int(res.flags.item()) == 0
    assert res.iterations.tolist() == [s if s >= 0 else -1 for s in status]
    assert torch.isnan(res.table[[2, 5, 6]]).all() and float(res.residual[5]) >= TOL
    keep = [0, 1, 3, 4, 7]
    assert bool((clean.status >= 1).all())
    assert torch.equal(res.table[keep], clean.table[keep]) and torch.equal(res.status[keep], clean.status[keep])
    assert torch.equal(res.residual[keep], clean.residual[keep])
    for route in ("global",):
        again = solve_power_flow(bt, _dev(spec), _dev(lists), _dev(rx), tol=TOL, max_iter=MAX_ITER, route=route)
        assert [again.status.tolist()[k] for k in (2, 5, 6)] == [-2, -1, -4] and torch.isnan(again.table[[2, 5, 6]]).all()


def test_counts_that_contradict_bus_type_raise_the_flag():
    case = _case(14, 20, 8, seed=4)
    n_pv, n_pq = int((case.bt == 1).sum()), int((case.bt == 2).sum())
    bt, spec, ei, rx = _dev(case.bt.astype(np.int32)), _dev(case.spec), _dev(case.ei), _dev(case.rx)
    guard = -7.5
    table = torch.full((case.S + 1, case.n, 4), guard, dtype=torch.float64, device=DEV)
    status = torch.full((case.S,), 99, dtype=torch.int32, device=DEV)
    residual = torch.zeros(case.S, dtype=torch.float64, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    # one PQ bus fewer, one PV bus more than the device array holds: the launch is sized for the smaller m and must not obey it
    rc = L.load().pfn_powerflow_solve(ei.data_ptr(), 0, case.e, rx.data_ptr(), bt.data_ptr(), spec.data_ptr(), case.S, case.n, n_pv + 1,
                                      n_pq - 1, 0, C.c_double(TOL), MAX_ITER, 0, table.data_ptr(), status.data_ptr(), residual.data_ptr(),
                                      flags.data_ptr(), None, 0, L.stream_ptr())
    assert rc == 0
    assert int(flags.item()) & 1 and status.tolist() == [-5] * case.S
    assert torch.isnan(table[:case.S]).all() and bool((table[case.S] == guard).all())


# -------------------------------------------------------------------------------------------------------------- DC
@pytest.mark.parametrize("n,e,S,route", [(14, 20, 64, "auto"), (118, 186, 8, "auto"), (70, 100, 16, "global")])
def test_dc_mode(n, e, S, route):
    case = _case(n, e, S)
    res = case.solve(mode="dc", route=route)
    table, status = res.table.cpu().numpy(), res.status.cpu().numpy()
    assert ((status >= 1) & (status <= MAX_ITER)).all() and int(res.flags.item()) == 0 and res.route == ("global" if route == "global" else "lds")
    worst_f = worst_x = 0.0
    for s in range(S):
        want, inv_norm = P.dc_solve(case.bt, case.spec[s], case.ei, case.rx[s])
        F = P.dc_mismatch(table[s], case.ei, case.rx[s], case.bt)
        worst_f = max(worst_f, float((np.abs(F) / (TOL + 64 * P.EPS64 * P.dc_scale(table[s], case.ei, case.rx[s]))).max()))
        worst_x = max(worst_x, float(np.abs(table[s, :, 1] - want[:, 1]).max() * P.RAD / (2 * TOL * inv_norm)))
        assert np.isnan(table[s, :, 3]).all() and np.array_equal(table[s, :, 0], want[:, 0])
        others = case.bt != 0
        assert np.array_equal(table[s, others, 2], want[others, 2])
        # the slack's line sum is minus the sum of the others up to the residuals of the others' equations
        assert abs(table[s, ~others, 2][0] - want[~others, 2][0]) <= (n - 1) * TOL + 64 * P.EPS64 * np.abs(want[:, 2]).sum()
    print(f"dc n {n} S {S} route {res.route}: solves {status.min()}..{status.max()} (mean {status.mean():.2f}), worst |mismatch| / bound {worst_f:.3g}, "
          f"worst |theta - fp64 solve| / (2 tol ||B'^-1||) {worst_x:.3g}")
    assert worst_f <= 1.0 and worst_x <= 1.0


# ------------------------------------------------------------------------------- closed loop: the physics kernel
def test_power_imbalance_of_the_solved_table_is_rounding():
    from poweflownet_amd.utils.custom_loss_functions import PowerImbalance
    case = _case(14, 20, 64)
    S, n, e = case.S, case.n, case.e
    solved = case.solve().table.cpu().numpy().astype(np.float32)
    vm, th, _ = zip(*(P.flat_start(case.bt, case.spec[s]) for s in range(S)))
    flat = np.stack([np.stack(vm), np.stack(th) / P.RAD, case.spec[:, :, 2], case.spec[:, :, 3]], axis=-1).astype(np.float32)
    rx32 = case.rx.astype(np.float32)
    loss_fn = PowerImbalance(torch.zeros(1, 4), torch.ones(1, 4), torch.zeros(1, 2), torch.ones(1, 2))
    ei = _dev((case.ei[None] + n * np.arange(S)[:, None, None]).transpose(1, 0, 2).reshape(2, S * e))
    ea = _dev(rx32.reshape(S * e, 2))
    got = float(loss_fn(_dev(solved.reshape(S * n, 4)), ei, ea))
    start = float(loss_fn(_dev(flat.reshape(S * n, 4)), ei, ea))
    bound = _imbalance_bound(solved, case.ei, rx32.astype(np.float64))
    print(f"PowerImbalance: solved table {got:.3e}, bound {bound:.3e}, flat start {start:.3e}")
    assert got < bound
    assert start > 1e3 * bound                                                 # ... so the bound cannot pass vacuously


# ------------------------------------------------------------------------------------------------------ end to end
def test_generator_dataset_report_and_dc_error(tmp_path):
    import dataset_generator
    import dc_error
    from poweflownet_amd.data import DataLoader
    from poweflownet_amd.datasets import PowerFlowData
    from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
    from poweflownet_amd.utils.custom_loss_functions import PowerImbalance
    from poweflownet_amd.utils.evaluation import evaluate_report
    root, split = str(tmp_path / "solved"), [.5, .25, .25]
    text = _run(dataset_generator.main, ["--case", "14", "--samples", "32", "--root", root])
    assert "Failed to converge and drawn again: 0" in text
    node, edge = np.load(tmp_path / "solved" / "raw" / "case14_node_features.npy"), np.load(tmp_path / "solved" / "raw" / "case14_edge_features.npy")
    assert node.shape == (32, 14, 6) and edge.shape == (32, 20, 4) and np.isfinite(node).all()

    def ref_imbalance(where):
        ds = PowerFlowData(root=where, case="14", split=split, task="test", device=DEV)
        assert len(ds) == 8
        torch.manual_seed(7)
        model = MaskEmbdMultiMPN(4, 2, 4, 32, 3, 2, 0.0).to(DEV).eval()
        stats = [t.cpu() for t in ds.get_data_means_stds()]
        report = evaluate_report(model, DataLoader(ds, batch_size=4, shuffle=False), DEV, xystd=ds.xystd, power_imbalance=PowerImbalance(*stats))
        return report["PowerImbalance(ref)"]
    got = ref_imbalance(root)
    # the same bound on the rows the test split holds: the file's fp64 values cast to fp32.  The normalisation round trip moves a
    # voltage by a few EPS of itself and (r, x) by 1e-7 of their spread -- relative to the FLOWS (a hundredth of the scales) that is
    # well inside C_BOUND EPS of the scales.
    bound = _imbalance_bound(node[24:, :, 2:].astype(np.float32), edge[0, :, :2].T.astype(np.int64), edge[24:, :, 2:].astype(np.float32).astype(np.float64))
    # a set of the same shape whose rows satisfy no physical law (tools/make_raw_dataset.py's draw)
    rng = np.random.default_rng(0)
    fake = node.copy()
    fake[:, :, 2:] = rng.normal(size=(32, 14, 4)) * np.array([0.05, 10.0, 50.0, 20.0]) + np.array([1.0, 0.0, 30.0, 10.0])
    (tmp_path / "fake" / "raw").mkdir(parents=True)
    np.save(tmp_path / "fake" / "raw" / "case14_node_features.npy", fake)
    np.save(tmp_path / "fake" / "raw" / "case14_edge_features.npy", edge)
    unphysical = ref_imbalance(str(tmp_path / "fake"))
    print(f"PowerImbalance(ref): generated set {got:.3e} (bound {bound:.3e}), unphysical set {unphysical:.3e}")
    assert got < bound and unphysical > 1.0
    text = _run(dc_error.main, ["--case", "14", "--data-dir", root, "--split", "0.5", "0.25", "0.25"])
    lines = [l for l in text.splitlines() if " losses: " in l]
    assert [l.split(" losses: ")[0] for l in lines] == ["Average", "Std", "Max", "Min", "Median", "25th percentile", "75th percentile",
                                                        "95th percentile", "99th percentile"]
    values = [float(l.split(" losses: ")[1]) for l in lines]
    assert np.isfinite(values).all() and values[3] > 0 and values[2] >= values[0] >= values[3] and "8 samples" in text
