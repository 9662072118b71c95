"""The sparse route of the batched power-flow solver on the device: `pfn_powerflow_solve_sparse` (csrc/powerflow_sparse.hip) through
`solve_power_flow(route="sparse")`, held to the float64 yardstick of tests/powerflow_ref.py with tol = 1e-10 and max_iter = 10, the
bounds of tests/test_gpu_powerflow.py re-stated here --
  residual   the yardstick's mismatch of the WRITTEN table, at all buses, <= tol + 64 * 2^-52 * scale_i;
  solution   Vm and Va (radians) within 2 tol ||J^-1||_inf of the yardstick's own solution and of the dense route's table;
-- at the shapes the dense routes take too, at (1100, 1530) which they refuse (m = 1832), in DC mode, bit-for-bit independence of a
sample from its batch and of a result from who built the plan, failures that stay local, one sample of the workload size
(6470, 9005), and dataset_generator.py with the route forced.

Worst ratios measured on an MI355X (bound 1; each test prints its own): residual 0.56 at (5, 6, 3), 3.2e-4 at m = 195, 7.6e-3 at
m = 1832, 3.9e-4 at m = 10782; distance to the yardstick's solution 1.2e-2, to the dense route's 7.4e-3; DC 0.039 / 3.6e-5;
PowerImbalance of the generated set 1.1e-12 against a bound of 2.9e-7.  3-4 solves (5 at 6470, in 1.9 s), 2 in DC mode.  DESIGN.md
section 7k."""
import functools
import time

import numpy as np
import pytest
import torch

from poweflownet_amd.synth import make_physical_inputs
from poweflownet_amd.utils import powerflow as PF
from poweflownet_amd.utils.powerflow import max_unknowns, solve_power_flow, sparse_plan
from tests import powerflow_ref as P
from tests.powerflow_checks import DEV, TOL, _check_given, _dev, _distance, _imbalance_bound, _residual_ratio, _run

pytestmark = pytest.mark.gpu
MAX_ITER = 10


class _Case:
    """Inputs of one shape on the host; the yardstick's solutions and ||J^-1|| computed once, where a test asks for them."""

    def __init__(self, n, e, S, seed, load=0.2):
        ei, bt, rx, spec = make_physical_inputs(n, e, S, seed, load)
        self.n, self.e, self.S = n, e, S
        self.ei, self.bt, self.rx, self.spec = ei.numpy(), bt.numpy().copy(), rx.numpy(), spec.numpy().copy()
        self.m = (n - 1) + int((self.bt == 2).sum())

    @functools.cached_property
    def ref(self):
        out = [P.newton(self.bt, self.spec[s], self.ei, self.rx[s], tol=TOL, max_iter=MAX_ITER) for s in range(self.S)]
        assert all(1 <= st <= MAX_ITER for _, st, _ in out), [st for _, st, _ in out]
        return np.stack([t for t, _, _ in out])

    @functools.cached_property
    def inv_norm(self):
        return np.array([P.jacobian_inverse_norm(self.ref[s], self.bt, self.ei, self.rx[s]) for s in range(self.S)])

    @functools.cached_property
    def plan(self):
        return sparse_plan(_dev(self.bt), _dev(self.ei))

    @functools.cached_property
    def plan_dc(self):
        return sparse_plan(_dev(self.bt), _dev(self.ei), "dc")

    def solve(self, rows=slice(None), **kw):
        kw = {"tol": TOL, "max_iter": MAX_ITER, "route": "sparse", **kw}
        if kw["route"] == "sparse" and "plan" not in kw:
            kw["plan"] = self.plan_dc if kw.get("mode") == "dc" else self.plan
        threads = kw.pop("threads", None)
        args = (_dev(self.bt), _dev(self.spec[rows]), _dev(self.ei), _dev(self.rx[rows]))
        if threads is not None:                                 # the workgroup size forced: the module's internal entry
            return PF._solve(*args, kw.get("mode", "ac"), kw["tol"], kw["max_iter"], kw["route"], kw.get("init"), kw["plan"], threads)
        return solve_power_flow(*args, **kw)


@functools.lru_cache(maxsize=None)
def _case(n, e, S, seed=1, load=0.2):
    return _Case(n, e, S, seed, load)


# ------------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("n,e,S", [(5, 6, 3), (14, 20, 8), (70, 100, 4), (118, 186, 4)])
def test_residual_and_solution_against_the_yardstick_and_the_dense_route(n, e, S):
    case = _case(n, e, S)
    res = case.solve()
    assert res.route == "sparse"
    table, status = res.table.cpu().numpy(), res.status.cpu().numpy()
    assert table.shape == (S, n, 4) and table.dtype == np.float64 and int(res.flags.item()) == 0
    assert ((status >= 1) & (status <= MAX_ITER)).all(), status
    assert torch.equal(res.iterations, res.status) and bool((res.residual < TOL).all())
    dense = case.solve(route="auto")
    assert dense.route in ("lds", "global") and bool((dense.status >= 1).all())
    dense_table = dense.table.cpu().numpy()
    worst_f, worst_x, worst_d = _residual_ratio(case, table), 0.0, 0.0
    for s in range(S):
        for other, which in ((case.ref[s], "yardstick"), (dense_table[s], "dense")):
            ratio = float(_distance(table[s], other) / (2 * TOL * case.inv_norm[s]))
            if which == "dense":
                worst_d = max(worst_d, ratio)
            else:
                worst_x = max(worst_x, ratio)
    _check_given(case, table)
    print(f"sparse n {n} e {e} S {S} m {case.m}: nnz(L) {case.plan.nnz_l}, solves {status.min()}..{status.max()} (mean {status.mean():.2f}), "
          f"worst |mismatch| / bound {worst_f:.3g}, |x - yardstick| / (2 tol ||J^-1||) {worst_x:.3g}, |x - dense route| / same {worst_d:.3g}")
    assert worst_f <= 1.0 and worst_x <= 1.0 and worst_d <= 1.0


@pytest.mark.parametrize("threads", [64, 256])
def test_both_workgroup_sizes_meet_the_bounds(threads):
    case = _case(118, 186, 4)
    res = case.solve(threads=threads)
    assert bool(((res.status >= 1) & (res.status <= MAX_ITER)).all())
    assert _residual_ratio(case, res.table.cpu().numpy()) <= 1.0


# -------------------------------------------------------------------------- the shape the dense routes refuse
def test_beyond_the_dense_cap_the_sparse_route_solves_what_auto_refuses():
    case = _case(1100, 1530, 2)
    assert case.m == 1832 > max_unknowns()
    res = case.solve()
    status = res.status.cpu().numpy()
    table = res.table.cpu().numpy()
    assert res.route == "sparse" and ((status >= 1) & (status <= MAX_ITER)).all(), status
    worst = _residual_ratio(case, table)
    _check_given(case, table)
    print(f"sparse n 1100 m {case.m}: nnz(L) {case.plan.nnz_l}, longest column {case.plan.max_col}, {case.plan.madds} multiply-adds per factor, "
          f"plan built in {case.plan.build_s * 1e3:.1f} ms, solves {status.tolist()}, worst |mismatch| / bound {worst:.3g}")
    assert worst <= 1.0
    with pytest.raises(RuntimeError, match="sparse factorisation"):
        case.solve(route="auto")


# -------------------------------------------------------------------------------------------------------------- DC
@pytest.mark.parametrize("n,e,S", [(14, 20, 8), (1100, 1530, 2)])
def test_dc_mode(n, e, S):
    case = _case(n, e, S)
    res = case.solve(mode="dc")
    table, status = res.table.cpu().numpy(), res.status.cpu().numpy()
    assert ((status >= 1) & (status <= MAX_ITER)).all() and int(res.flags.item()) == 0 and res.route == "sparse"
    worst_f = worst_x = 0.0
    for s in range(S):
        F = P.dc_mismatch(table[s], case.ei, case.rx[s], case.bt)
        worst_f = max(worst_f, float((np.abs(F) / (TOL + 64 * P.EPS64 * P.dc_scale(table[s], case.ei, case.rx[s]))).max()))
        assert np.isnan(table[s, :, 3]).all()
        if n == 14:
            want, inv_norm = P.dc_solve(case.bt, case.spec[s], case.ei, case.rx[s])
            worst_x = max(worst_x, float(np.abs(table[s, :, 1] - want[:, 1]).max() * P.RAD / (2 * TOL * inv_norm)))
            others = case.bt != 0
            assert np.array_equal(table[s, :, 0], want[:, 0]) and np.array_equal(table[s, others, 2], want[others, 2])
    print(f"sparse dc n {n} S {S}: solves {status.min()}..{status.max()}, worst |mismatch| / bound {worst_f:.3g}, "
          f"worst |theta - fp64 solve| / (2 tol ||B'^-1||) {worst_x:.3g}")
    assert worst_f <= 1.0 and worst_x <= 1.0


# ---------------------------------------------------------------------------------------------------- independence
def test_a_sample_depends_on_neither_its_batch_nor_who_built_the_plan():
    case = _case(14, 20, 8, seed=3)
    whole = case.solve()
    assert bool((whole.status >= 1).all())
    a, b = case.solve(rows=slice(0, 4)), case.solve(rows=slice(4, 8))
    assert torch.equal(torch.cat([a.table, b.table]), whole.table) and torch.equal(torch.cat([a.status, b.status]), whole.status)
    assert torch.equal(torch.cat([a.residual, b.residual]), whole.residual)
    fresh = case.solve(plan=None)                               # builds its own plan
    assert torch.equal(fresh.table, whole.table) and torch.equal(fresh.status, whole.status) and torch.equal(fresh.residual, whole.residual)
    assert torch.equal(sparse_plan(_dev(case.bt), _dev(case.ei)).blob, case.plan.blob)
    wide = case.solve(threads=256)                             # ... nor on the workgroup size
    assert torch.equal(wide.table, whole.table) and torch.equal(wide.status, whole.status)
    # a start already under tol: nothing is solved and the table comes back.  Vm and everything given return bit for bit; Va makes the
    # trip degrees -> radians -> degrees that every warm start makes (taken as on the dense route: x * RAD, then * (1 / RAD)): three
    # roundings of half an ulp each, so it returns within 4 * 2^-52 of itself, not bit for bit; the slack's P, Q and the PV buses' Q
    # are line sums re-formed from those angles and are held to the residual bound again
    again = case.solve(init=whole.table)
    assert again.status.tolist() == [0] * 8 and bool((again.residual < TOL).all())
    got, want = again.table.cpu().numpy(), whole.table.cpu().numpy()
    assert np.array_equal(got[:, :, 0], want[:, :, 0])
    assert (np.abs(got[:, :, 1] - want[:, :, 1]) <= 4 * P.EPS64 * np.abs(want[:, :, 1])).all()
    _check_given(case, got)
    assert _residual_ratio(case, got) <= 1.0


def test_what_does_not_fit_the_route_raises():
    case = _case(14, 20, 8, seed=3)
    for mode in ("fdxb", "fdbx"):
        with pytest.raises(ValueError, match="dense"):
            case.solve(mode=mode, plan=None)
    with pytest.raises(RuntimeError, match="one topology"):
        solve_power_flow(_dev(case.bt), _dev(case.spec), _dev(np.stack([case.ei] * 8)), _dev(case.rx), route="sparse")
    with pytest.raises(RuntimeError, match="the plan is for"):
        case.solve(plan=_case(5, 6, 3).plan)
    with pytest.raises(RuntimeError, match="the plan is for"):
        case.solve(plan=case.plan_dc)
    with pytest.raises(ValueError, match="route='sparse' only"):
        case.solve(route="auto", plan=case.plan)
    # a plan for other lines of the same size: the kernel notices, nothing is followed
    other = case.ei.copy()
    other[:, [0, 1]] = other[:, [1, 0]]
    stale = solve_power_flow(_dev(case.bt), _dev(case.spec), _dev(other), _dev(case.rx), route="sparse", plan=case.plan)
    assert stale.status.tolist() == [-6] * 8 and torch.isnan(stale.table).all()


# -------------------------------------------------------------------------------------------------------- failures
def test_failures_stay_local():
    n, e = 14, 20
    good, heavy = _case(n, e, 6, seed=4), _case(n, e, 6, seed=4, load=2.0)      # tests/test_gpu_powerflow.py's recipe: ten times the load
    spec, rx = good.spec.copy(), good.rx.copy()
    spec[5], rx[5] = heavy.spec[5], heavy.rx[5]
    bt, ei = _dev(good.bt), _dev(good.ei)
    res = solve_power_flow(bt, _dev(spec), ei, _dev(rx), tol=TOL, max_iter=MAX_ITER, route="sparse", plan=good.plan)
    clean = good.solve()
    status = res.status.tolist()
    assert status[5] == -1 and int(res.flags.item()) == 0 and float(res.residual[5]) >= TOL
    assert res.iterations.tolist() == [s if s >= 0 else -1 for s in status] and torch.isnan(res.table[5]).all()
    keep = [0, 1, 2, 3, 4]
    assert bool((clean.status >= 1).all())
    assert torch.equal(res.table[keep], clean.table[keep]) and torch.equal(res.status[keep], clean.status[keep])
    assert torch.equal(res.residual[keep], clean.residual[keep])
    # the grid variant in which bus 13 (a PQ bus) has no line: a zero pivot, as on the dense route
    assert good.bt[13] == 2
    alone = np.where(good.ei == 13, 1, good.ei)
    res = solve_power_flow(bt, _dev(good.spec), _dev(alone), _dev(good.rx), tol=TOL, max_iter=MAX_ITER, route="sparse")
    assert res.status.tolist() == [-2] * 6 and torch.isnan(res.table).all() and int(res.flags.item()) == 0
    dense = solve_power_flow(bt, _dev(good.spec), _dev(alone), _dev(good.rx), tol=TOL, max_iter=MAX_ITER)
    assert dense.status.tolist() == [-2] * 6


# --------------------------------------------------------------------------------------------------- workload size
def test_one_sample_of_the_workload_size():
    """(6470, 9005), m = 10782: the residual bound alone (a dense yardstick solve of that order is not a test's business)."""
    case = _case(6470, 9005, 1)
    assert case.m == 10782
    plan = case.plan
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = case.solve()
    status = res.status.tolist()
    seconds = time.perf_counter() - t0
    table = res.table.cpu().numpy()
    worst = _residual_ratio(case, table)
    print(f"sparse n 6470 m {case.m}: nnz(L) {plan.nnz_l}, longest column {plan.max_col}, {plan.madds / 1e6:.1f} M multiply-adds per factor, "
          f"plan {plan.bytes / 1e6:.2f} MB built in {plan.build_s:.3f} s, {status[0]} solves in {seconds:.3f} s, worst |mismatch| / bound {worst:.3g}")
    assert 1 <= status[0] <= MAX_ITER and worst <= 1.0
    _check_given(case, table)


# ------------------------------------------------------------------------------------------------------ end to end
def test_generator_with_the_route_forced_writes_a_balanced_set(tmp_path):
    import dataset_generator
    from poweflownet_amd.data import DataLoader
    from poweflownet_amd.datasets import PowerFlowData
    from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
    from poweflownet_amd.utils.custom_loss_functions import PowerImbalance
    from poweflownet_amd.utils.evaluation import evaluate_report
    root, split = str(tmp_path / "solved"), [.5, .25, .25]
    text = _run(dataset_generator.main, ["--case", "14", "--samples", "16", "--root", root, "--route", "sparse"])
    assert "Failed to converge and drawn again: 0" in text and "Solved on the sparse route" in text
    node, edge = np.load(tmp_path / "solved" / "raw" / "case14_node_features.npy"), np.load(tmp_path / "solved" / "raw" / "case14_edge_features.npy")
    assert node.shape == (16, 14, 6) and edge.shape == (16, 20, 4) and np.isfinite(node).all()
    ds = PowerFlowData(root=root, case="14", split=split, task="test", device=DEV)
    assert len(ds) == 4
    torch.manual_seed(7)
    model = MaskEmbdMultiMPN(4, 2, 4, 32, 3, 2, 0.0).to(DEV).eval()
    stats = [t.cpu() for t in ds.get_data_means_stds()]
    report = evaluate_report(model, DataLoader(ds, batch_size=4, shuffle=False), DEV, xystd=ds.xystd, power_imbalance=PowerImbalance(*stats))
    got = report["PowerImbalance(ref)"]
    bound = _imbalance_bound(node[12:, :, 2:].astype(np.float32), edge[0, :, :2].T.astype(np.int64), edge[12:, :, 2:].astype(np.float32).astype(np.float64))
    print(f"PowerImbalance(ref) of the set generated on the sparse route: {got:.3e} (bound {bound:.3e})")
    assert got < bound
