"""The Q-limited, per-sample-types power-flow solve on the SPARSE route: `pfn_powerflow_solve_sparse_qlim`
(csrc/powerflow_sparse_qlim.hip) through `solve_power_flow_qlim(route="sparse", plan=qlim_plan(...))`, held to what
tests/test_gpu_powerflow_qlim.py holds the dense kernel to -- the same fixtures (`_qcase`), the same checks (`_check_fixture`,
`_check_against`), tol = 1e-10, max_iter = 10, the 1e-4 margin condition on the inputs and the bounds of tests/powerflow_checks.py;
no tolerance of its own:
  decisions  the final bus types and the number of re-solves equal the float64 yardstick's (tests/powerflow_qlim_ref.py) EXACTLY;
  residual   the yardstick's mismatch of the WRITTEN table, at all buses, <= tol + 64 * 2^-52 * scale_i;
  solution   Vm and Va (radians) within 2 tol ||J^-1||_inf of the yardstick's table, J at the FINAL type set;
  given      what the final types give comes back bit for bit, a switched bus's Q being its limit.
The plan is ONE plan per grid, for the type row with every non-slack bus PQ: the Vm of a bus that is PV is a dead unknown.  Then:
beyond the dense cap at (1100, 1530), no limits, no PV bus, per-sample PV sets under one plan, independence from the batch, failures
that stay local, every PV bus switching, per-sample line lists under a cover plan, one sample of (6470, 9005), and the closed loop
through dataset_generator.py --route sparse --enforce-q-lims.  Every test but the two without limits fails where route="sparse"
raises.  DESIGN.md section 7r."""
import re
import types

import numpy as np
import pytest
import torch

from poweflownet_amd.synth import make_physical_inputs
from poweflownet_amd.utils import powerflow as PF
from poweflownet_amd.utils.powerflow import CoverPlan, SparsePlan, qlim_plan, solve_power_flow_qlim, sparse_plan
from tests import powerflow_cover_ref as CR
from tests import powerflow_qlim_ref as Q
from tests import powerflow_ref as P
from tests.powerflow_checks import DEV, TOL, _dev, _imbalance_bound, _residual_ratio, _run
from tests.test_gpu_powerflow import _case as _plain_case
from tests.test_gpu_powerflow import _check_ac
from tests.test_gpu_powerflow_cover import _case as _cover_case
from tests.test_gpu_powerflow_qlim import MAX_ITER, MIN_MARGIN, _cat, _check_against, _check_fixture, _Grid, _own_types, _qcase, _same
from tests.test_gpu_powerflow_sparse import _case as _sparse_case

pytestmark = pytest.mark.gpu


def _solve(bt, spec, ei, rx, limits, plan, threads=0, max_rounds=8, init=None, max_iter=MAX_ITER):
    """`solve_power_flow_qlim(route="sparse")` on host arrays, with the workgroup size exposed"""
    return PF._solve_qlim(_dev(bt), _dev(spec), _dev(ei), _dev(rx), None if limits is None else _dev(limits), TOL, max_iter, max_rounds, None,
                          "sparse", None if init is None else _dev(init), plan, threads)


_PLANS = {}


def _plan(case):
    """the ONE plan of a fixture's grid"""
    key = (case.n, case.ei.tobytes(), int(np.flatnonzero(case.bt == 0)[0]))
    if key not in _PLANS:
        _PLANS[key] = qlim_plan(_dev(case.bt), _dev(case.ei))
        assert isinstance(_PLANS[key], SparsePlan) and _PLANS[key].m == 2 * (case.n - 1)
    return _PLANS[key]


def _run_case(case, rows=slice(None), bt=None, limits="fixture", **kw):
    bt = case.bt if bt is None else bt
    limits = case.limits[rows] if isinstance(limits, str) else limits
    return _solve(bt[rows] if bt.ndim == 2 else bt, case.spec[rows], case.ei, case.rx[rows], limits, _plan(case), **kw)


# ------------------------------------------------------------------------------------------- 1. decisions and solution
@pytest.mark.parametrize("n,e,S", [(5, 6, 3), (14, 20, 16), (70, 100, 8), (118, 186, 4)])
def test_decisions_and_solution(n, e, S):
    case = _qcase(n, e, S)
    res = solve_power_flow_qlim(_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), _dev(case.limits), tol=TOL, max_iter=MAX_ITER,
                                route="sparse", plan=_plan(case))
    assert res.route == "sparse"
    _check_fixture(case, res, f"sparse, n {n} e {e} S {S}")
    if n == 5:
        assert not (res.bus_type == 1).any() and res.rounds.tolist() == [1] * S
    else:
        assert max(r.rounds for r in case.ref) >= 2
    if n == 14:
        narrow, wide = _run_case(case, threads=64), _run_case(case, threads=256)
        _check_fixture(case, narrow, "sparse, 64 threads, n 14")
        _check_fixture(case, wide, "sparse, 256 threads, n 14")
        print(f"64 against 256 threads: tables bit-equal {torch.equal(narrow.table, wide.table)}, status equal {torch.equal(narrow.status, wide.status)}")


# -------------------------------------------------------------------------------------------- 2. beyond the dense cap
def test_beyond_the_dense_cap():
    case = _qcase(1100, 1530, 2)
    assert 2 * (case.n - 1) == 2198 > PF.max_unknowns()
    with pytest.raises(RuntimeError, match="sparse factorisation"):
        solve_power_flow_qlim(_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), _dev(case.limits), tol=TOL, max_iter=MAX_ITER)
    plan = _plan(case)
    res = _run_case(case)
    _check_fixture(case, res, f"sparse, n 1100 m_max 2198 (plan: {plan.nnz} slab positions, {plan.madds} multiply-adds, built in {plan.build_s * 1e3:.0f} ms)")
    print(f"switched buses {((res.bus_type.cpu().numpy() != case.bt).sum(axis=1)).tolist()}")


# ------------------------------------------------------------------------------------------------------ 3. no limits
@pytest.mark.parametrize("n,e,S", [(14, 20, 64), (118, 186, 8)])
def test_without_limits_it_is_the_newton_solve(n, e, S):
    case = _plain_case(n, e, S)
    res = _solve(case.bt, case.spec, case.ei, case.rx, None, _plan(case))
    _check_ac(case, res, f"sparse, no limits, n {n} e {e} S {S}")
    assert res.route == "sparse" and res.rounds.tolist() == [0] * S and torch.equal(res.bus_type, _dev(case.bt.astype(np.int32)).expand(S, n))
    own = case.solve(route="sparse", plan=sparse_plan(_dev(case.bt), _dev(case.ei)))
    print(f"no limits, n {n}: table bit-equal to solve_power_flow(route='sparse') on the own-types plan: {torch.equal(res.table, own.table)}, "
          f"status equal: {torch.equal(res.status, own.status)} (the order differs: it need not be)")
    wide = np.tile([-1e9, 1e9], (n, 1))
    again = _solve(case.bt, case.spec, case.ei, case.rx, wide, _plan(case))
    assert torch.equal(again.table, res.table) and torch.equal(again.status, res.status) and again.rounds.tolist() == [0] * S


# ------------------------------------------------------------------------------------------------------ 4. no PV bus
def test_a_grid_without_a_pv_bus():
    case = _plain_case(14, 20, 8, seed=2, types="no_pv")
    plan, own = qlim_plan(_dev(case.bt), _dev(case.ei)), sparse_plan(_dev(case.bt), _dev(case.ei))
    assert torch.equal(plan.blob, own.blob)                           # every non-slack bus PQ: the all-PQ plan IS the own-types plan
    res = _solve(case.bt, case.spec, case.ei, case.rx, np.zeros((14, 2)), plan)       # (nobody reads the limits: they belong to PV buses)
    _check_ac(case, res, "sparse, no PV bus, limits given")
    assert res.rounds.tolist() == [0] * 8 and torch.equal(res.bus_type, _dev(case.bt.astype(np.int32)).expand(8, 14))
    sparse = case.solve(route="sparse", plan=own)
    print(f"no PV bus: table bit-equal to solve_power_flow(route='sparse'): {torch.equal(res.table, sparse.table)}, "
          f"status equal: {torch.equal(res.status, sparse.status)}")


# ------------------------------------------------------------------------------- 5. per-sample PV sets under ONE plan
@pytest.mark.parametrize("limited", [False, True])
def test_per_sample_types_under_one_plan(limited):
    n, e, S = 14, 20, 8
    ei, types_, rx, spec = _own_types(n, e, S, seed=5)
    assert len({t.tobytes() for t in types_}) == 3
    limits = None
    if limited:
        limits = np.stack([Q.band_limits(types_[s], P.newton(types_[s], spec[s], ei, rx[s], tol=TOL, max_iter=MAX_ITER)[0]) for s in range(S)])
    refs = [Q.solve(types_[s], spec[s], ei, rx[s], None if limits is None else limits[s], tol=TOL, max_iter=MAX_ITER) for s in range(S)]
    plan = qlim_plan(_dev(types_), _dev(ei))
    res = _solve(types_, spec, ei, rx, limits, plan)
    if limited:
        assert min(r.margin for r in refs) >= MIN_MARGIN and all(r.rounds >= 1 for r in refs)
    _check_against(refs, res, ei, rx, spec, f"sparse, per-sample types, limits {limited}")
    if not limited:
        assert torch.equal(res.bus_type, _dev(types_.astype(np.int32))) and res.rounds.tolist() == [0] * S
    # a sample with its own row against the same sample under that row shared
    for s in (0, 1, 2):
        one = _solve(types_[s], spec[s:s + 1], ei, rx[s:s + 1], None if limits is None else limits[s], plan)
        assert torch.equal(one.table[0], res.table[s]) and int(one.status[0]) == int(res.status[s]) and torch.equal(one.bus_type[0], res.bus_type[s])


# --------------------------------------------------------------------------------------------------- 6. independence
def test_a_sample_does_not_depend_on_its_batch():
    case = _qcase(14, 20, 16)
    whole = _run_case(case)
    assert bool((whole.status >= 1).all()) and len(set(whole.rounds.tolist())) > 1
    assert _same(_cat([_run_case(case, rows=slice(k, k + 1)) for k in range(case.S)]), whole)
    assert _same(_cat([_run_case(case, rows=slice(0, 5)), _run_case(case, rows=slice(5, 16))]), whole)
    assert _same(_run_case(case), whole)
    # shared [n, 2] limits against the same limits repeated per sample; shared [n] types against the row repeated
    shared = _run_case(case, limits=case.limits[3])
    assert bool((shared.rounds >= 1).all()) and bool((shared.status >= 1).all())
    assert _same(_run_case(case, limits=np.stack([case.limits[3]] * case.S)), shared)
    assert _same(_run_case(case, bt=np.stack([case.bt] * case.S)), whole)


# ------------------------------------------------------------------------------------------------------- 7. failures
def test_failures_stay_local():
    case = _qcase(14, 20, 16)
    S, n = case.S, case.n
    rounds = [r.rounds for r in case.ref]
    two, one = [s for s in range(S) if rounds[s] == 2], [s for s in range(S) if rounds[s] == 1]
    assert len(two) >= 1 and len(one) >= 4 and len(two) + len(one) == S
    a, b, c = one[0], one[1], one[2]                                  # a: two slacks; b: a non-finite start; c: the slack elsewhere
    slack, other = int(np.flatnonzero(case.bt == 0)[0]), int(np.flatnonzero(case.bt == 2)[0])
    types_ = np.stack([case.bt] * S)
    types_[a, other] = 0
    types_[c, slack], types_[c, other] = 2, 0
    init = np.zeros((S, n, 2))
    init[:, :, 0] = 1.0                                               # the flat start, spelled out
    clean = _run_case(case, bt=np.stack([case.bt] * S), init=init)
    assert _same(clean, _run_case(case)) and int(clean.flags.item()) == 0
    init[b, other, 0] = np.nan
    res = _run_case(case, bt=types_, init=init, max_rounds=1)
    status = res.status.tolist()
    assert status[a] == -5 and status[b] == -3 and status[c] == -6 and [status[s] for s in two] == [-7] * len(two), status
    assert int(res.flags.item()) == 1                                 # bit 0: a type row was refused
    failed = [a, b, c] + two
    assert torch.isnan(res.table[failed]).all() and torch.equal(res.bus_type[failed], _dev(types_[failed].astype(np.int32)))
    assert res.rounds[[a, b, c]].tolist() == [0, 0, 0] and res.rounds[two].tolist() == [1] * len(two)
    assert res.iterations.tolist() == [s if s >= 0 else -1 for s in status]
    assert torch.isnan(res.residual[[a, b, c]]).all() and bool((res.residual[two] < TOL).all())
    keep = one[3:]
    for f in ("table", "status", "rounds", "bus_type", "residual"):
        assert torch.equal(getattr(res, f)[keep], getattr(clean, f)[keep]), f
    # max_rounds = 0 with a violated limit, beside samples nobody limits
    limits = np.stack([np.tile([-np.inf, np.inf], (n, 1))] * S)
    limits[a] = case.limits[a]
    free = _run_case(case, limits=limits)
    assert free.rounds.tolist() == [int(s == a) for s in range(S)]
    res = _run_case(case, limits=limits, max_rounds=0)
    assert res.status.tolist()[a] == -7 and int(res.rounds[a]) == 0 and torch.isnan(res.table[a]).all() and int(res.flags.item()) == 0
    assert torch.equal(res.bus_type[a], _dev(case.bt.astype(np.int32))) and float(res.residual[a]) < TOL
    keep = [s for s in range(S) if s != a]
    for f in ("table", "status", "rounds", "bus_type", "residual"):
        assert torch.equal(getattr(res, f)[keep], getattr(free, f)[keep]), f
    # what the host refuses: the grid's own-types plan, and the route without a plan
    args = (_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), _dev(case.limits))
    with pytest.raises(RuntimeError, match="every non-slack bus PQ"):
        solve_power_flow_qlim(*args, route="sparse", plan=sparse_plan(_dev(case.bt), _dev(case.ei)))
    with pytest.raises(ValueError, match="sparse route"):
        solve_power_flow_qlim(*args, route="sparse")


# ---------------------------------------------------------------------------------------- 8. every PV bus switches
def test_every_pv_bus_switches():
    case = _qcase(14, 20, 16)
    S, n = 8, case.n
    pv = case.bt == 1
    limits = np.stack([np.tile([-np.inf, case.free[s, pv, 3].min() - 0.05], (n, 1)) for s in range(S)])
    refs = [Q.solve(case.bt, case.spec[s], case.ei, case.rx[s], limits[s], tol=TOL, max_iter=MAX_ITER) for s in range(S)]
    assert min(r.margin for r in refs) >= MIN_MARGIN and all(r.rounds == 1 and not (r.bus_type == 1).any() for r in refs)
    res = _run_case(case, rows=slice(0, S), limits=limits)
    _check_against(refs, res, case.ei, case.rx[:S], case.spec[:S], f"sparse, every PV bus switches (m live = m_max = {2 * (n - 1)})")
    assert int((res.bus_type == 2).sum()) == S * (n - 1) and not (res.bus_type == 1).any()


# ------------------------------------------------------------------------ 9. per-sample line lists with Q-limits
def _row(res, s):
    """sample s of a result as a result of one sample"""
    return types.SimpleNamespace(table=res.table[s:s + 1], status=res.status[s:s + 1], iterations=res.iterations[s:s + 1],
                                 residual=res.residual[s:s + 1], bus_type=res.bus_type[s:s + 1], rounds=res.rounds[s:s + 1], flags=res.flags,
                                 route=res.route)


@pytest.mark.parametrize("n,e,S,ra", [(14, 20, 8, 1), (70, 100, 4, 1), (118, 186, 4, 2)])
def test_per_sample_line_lists_with_limits(n, e, S, ra):
    case = _cover_case(n, e, S, ra, ra)
    free = [P.newton(case.bt, case.spec[s], case.lists[s], case.rx[s], tol=TOL, max_iter=MAX_ITER)[0] for s in range(S)]
    limits = np.stack([Q.band_limits(case.bt, free[s]) for s in range(S)])
    refs = [Q.solve(case.bt, case.spec[s], case.lists[s], case.rx[s], limits[s], tol=TOL, max_iter=MAX_ITER) for s in range(S)]
    margin = min(r.margin for r in refs)
    assert margin >= MIN_MARGIN and all(r.rounds >= 1 for r in refs), margin
    plan = qlim_plan(_dev(case.bt), _dev(case.lists), _dev(case.ei))
    assert isinstance(plan, CoverPlan) and plan.plan.m == 2 * (n - 1)
    res = _solve(case.bt, case.spec, case.lists, case.rx, limits, plan)
    assert res.route == "sparse" and int(res.flags.item()) == 0
    for s in range(S):                                                # each sample against the yardstick on ITS OWN list
        _check_against([refs[s]], _row(res, s), case.lists[s], case.rx[s:s + 1], case.spec[s:s + 1],
                       f"cover, n {n} R = A = {ra}, sample {s} (smallest margin {margin:.3g}, {plan.extras} extra lines)")
    if n != 14:
        return
    assert _same(_solve(case.bt, case.spec[3:4], case.lists[3:4], case.rx[3:4], limits[3:4], plan), _row(res, 3))
    # a line the cover lacks fails its sample alone
    lists = case.lists.copy()
    have = {CR.key(a, b) for a, b in plan.cover.cpu().numpy().T}
    a, b = next((a, b) for a in range(n) for b in range(a + 1, n) if (a, b) not in have)
    lists[2, :, 0] = (b, a)
    bad = _solve(case.bt, case.spec, lists, case.rx, limits, plan)
    assert bad.status.tolist()[2] == -6 and torch.isnan(bad.table[2]).all() and int(bad.flags.item()) == 0
    assert torch.equal(bad.bus_type[2], _dev(case.bt.astype(np.int32))) and int(bad.rounds[2]) == 0
    keep = [0, 1, 3, 4, 5, 6, 7]
    for f in ("table", "status", "rounds", "bus_type", "residual"):
        assert torch.equal(getattr(bad, f)[keep], getattr(res, f)[keep]), f


# ------------------------------------------------------------------------------- 10. one sample of the workload size
def test_one_sample_of_the_workload_size():
    """(6470, 9005), m_max = 12938.  No dense yardstick (1.3 GB): the limits are the band of the sample's own unconstrained sparse
    solve, and the assertions are those that hold whatever a close decision came to.  A solve of ONE sample of this size is a chain
    of 12938 column steps, 0.4-0.7 s: the case and its own-types plan are tests/test_gpu_powerflow_sparse.py's (built once per
    session), and the Q-limited solve starts from the unconstrained table, so its first inner loop costs no solve."""
    n, e = 6470, 9005
    case = _sparse_case(n, e, 1)
    ei, bt, rx, spec = case.ei, case.bt, case.rx, case.spec
    free = case.solve()
    assert int(free.status[0]) >= 1
    limits = Q.band_limits(bt, free.table[0].cpu().numpy())
    plan = qlim_plan(_dev(bt), _dev(ei))
    assert plan.m == 2 * (n - 1) == 12938
    res = _solve(bt, spec, ei, rx, limits, plan, init=free.table[:, :, :2].cpu().numpy())
    status, rounds = int(res.status[0]), int(res.rounds[0])
    table, types_ = res.table.cpu().numpy(), res.bus_type[0].cpu().numpy()
    worst = _residual_ratio(_Grid(ei, rx), table) if status >= 0 else float("nan")
    moved = types_ != bt
    print(f"sparse Q-limits n 6470 m_max {plan.m}: {plan.nnz} slab positions, {plan.madds / 1e6:.1f} M multiply-adds per factor, plan built in "
          f"{plan.build_s:.3f} s; status {status}, rounds {rounds}, {int(moved.sum())} of {int((bt == 1).sum())} PV buses switched, "
          f"worst |mismatch| / bound {worst:.3g}")
    assert status >= 0 and rounds >= 1 and int(res.flags.item()) == 0
    assert worst <= 1.0
    assert moved.any() and (bt[moved] == 1).all() and (types_[moved] == 2).all()
    q = table[0, :, 3]
    assert (np.equal(q[moved], limits[moved, 0]) | np.equal(q[moved], limits[moved, 1])).all()     # its limit, bit for bit
    still = types_ == 1
    assert (q[still] >= limits[still, 0] - TOL).all() and (q[still] <= limits[still, 1] + TOL).all()
    assert np.array_equal(table[0, types_ != 2, 0], spec[0, types_ != 2, 0]) and np.array_equal(table[0, types_ != 0, 2], spec[0, types_ != 0, 2])


# ------------------------------------------------------------------------------------------------- 11. closed loop
def test_generator_with_enforced_q_limits_on_the_sparse_route(tmp_path):
    import dataset_generator
    from poweflownet_amd.data import DataLoader
    from poweflownet_amd.datasets import PowerFlowData
    from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
    from poweflownet_amd.utils.custom_loss_functions import PowerImbalance
    from poweflownet_amd.utils.evaluation import evaluate_report
    S, n, e = 32, 14, 20
    ei, bt, rx, spec = (t.numpy() for t in make_physical_inputs(n, e, S, 0, 0.2))         # the generator's first draw (seed 0)
    gen_tol = 1e-8                                                     # the generator's tolerance
    free = np.stack([P.newton(bt, spec[s], ei, rx[s], tol=gen_tol)[0] for s in range(S)])
    worst = np.sort(np.abs(free[:, bt == 1, 3]).max(axis=1))
    cap = float(0.5 * (worst[S // 2 - 1] + worst[S // 2]))             # half of the samples reach beyond it in round 0
    limits = np.tile([-cap, cap], (n, 1))
    refs = [Q.solve(bt, spec[s], ei, rx[s], limits, tol=gen_tol) for s in range(S)]
    assert all(r.table is not None for r in refs) and min(r.margin for r in refs) >= MIN_MARGIN, min(r.margin for r in refs)
    want = np.stack([r.bus_type for r in refs])
    assert 0 < int((want != bt).any(axis=1).sum()) < S

    root, split = str(tmp_path / "qlim"), [.5, .25, .25]
    text = _run(dataset_generator.main, ["--case", "14", "--samples", str(S), "--root", root, "--route", "sparse", "--enforce-q-lims",
                                         "--q-limit", repr(cap)])
    assert "Failed to converge and drawn again: 0" in text and "Solved on the sparse route" in text
    node = np.load(tmp_path / "qlim" / "raw" / "case14_node_features.npy")
    edge = np.load(tmp_path / "qlim" / "raw" / "case14_edge_features.npy")
    assert node.shape == (S, n, 6) and edge.shape == (S, e, 4) and np.isfinite(node).all()
    direct = solve_power_flow_qlim(_dev(bt), _dev(spec), _dev(ei), _dev(rx), _dev(limits), tol=gen_tol, route="sparse",
                                   plan=qlim_plan(_dev(bt), _dev(ei)))
    types_ = node[:, :, 1].astype(np.int64)
    assert np.array_equal(types_, direct.bus_type.cpu().numpy()) and np.array_equal(node[:, :, 2:], direct.table.cpu().numpy())
    assert np.array_equal(types_, want) and len({t.tobytes() for t in types_}) > 1
    said = re.search(r"(\d+) sample\(s\) had a bus switched to a load bus, at most (\d+) re-solve", text)
    assert said and int(said.group(1)) == int((types_ != bt).any(axis=1).sum()) and int(said.group(2)) == int(direct.rounds.max())
    q = node[:, :, 5]
    assert (np.abs(q[types_ == 1]) <= cap + gen_tol).all() and (np.abs(q[(types_ == 2) & (bt == 1)]) == cap).all()

    seen = []
    for task in ("train", "val", "test"):
        ds = PowerFlowData(root=root, case="14", split=split, task=task, device=DEV)
        seen += [ds[k].bus_type.cpu().numpy() for k in range(len(ds))]
    assert np.array_equal(np.stack(seen), types_)
    ds = PowerFlowData(root=root, case="14", split=split, task="test", device=DEV)
    torch.manual_seed(7)
    model = MaskEmbdMultiMPN(4, 2, 4, 32, 3, 2, 0.0).to(DEV).eval()
    stats = [t.cpu() for t in ds.get_data_means_stds()]
    report = evaluate_report(model, DataLoader(ds, batch_size=4, shuffle=False), DEV, xystd=ds.xystd, power_imbalance=PowerImbalance(*stats))
    got = report["PowerImbalance(ref)"]
    bound = _imbalance_bound(node[24:, :, 2:].astype(np.float32), edge[0, :, :2].T.astype(np.int64), edge[24:, :, 2:].astype(np.float32).astype(np.float64))
    print(f"--route sparse --enforce-q-lims --q-limit {cap:.6g}: {said.group(0)}; PowerImbalance(ref) {got:.3e} (bound {bound:.3e})")
    assert got < bound

    # with -r / -a: one cover plan of the all-PQ row and one Q-limited solve per chunk; every sample balanced on its own list
    root = str(tmp_path / "perturbed")
    text = _run(dataset_generator.main, ["--case", "14", "--samples", "8", "-r", "1", "-a", "1", "--route", "sparse", "--enforce-q-lims",
                                         "--q-limit", repr(cap), "--root", root])
    assert "Solved on the sparse route" in text and "Cover plans:" in text and "switched to a load bus" in text
    node = np.load(tmp_path / "perturbed" / "raw" / "case14perturbed1r1a_node_features.npy")
    edge = np.load(tmp_path / "perturbed" / "raw" / "case14perturbed1r1a_edge_features.npy")
    assert node.shape == (8, n, 6) and edge.shape == (8, e, 4) and np.isfinite(node).all()
    lists = edge[:, :, :2].astype(np.int64).transpose(0, 2, 1).copy()
    assert len({lists[s].tobytes() for s in range(8)}) > 1
    worst = max(_residual_ratio(_Grid(lists[s], edge[s:s + 1, :, 2:]), node[s:s + 1, :, 2:], tol=gen_tol) for s in range(8))
    q, ty = node[:, :, 5], node[:, :, 1].astype(np.int64)
    print(f"perturbed Q-limited set on the sparse route: worst |mismatch| / bound {worst:.3g}, {int((ty != bt).any(axis=1).sum())} sample(s) switched")
    assert worst <= 1.0 and (np.abs(q[ty == 1]) <= cap + gen_tol).all() and (np.abs(q[(ty == 2) & (bt == 1)]) == cap).all()
