"""The Q-limited, per-sample-types power-flow solve on the device: `pfn_powerflow_solve_qlim` (csrc/powerflow_qlim.hip) through
`solve_power_flow_qlim`, held to the float64 yardstick of tests/powerflow_qlim_ref.py with tol = 1e-10 and max_iter = 10 --
  decisions  the final bus types and the number of re-solves equal the yardstick's EXACTLY.  That is fair only where no decision is
             close: each test first asserts that the smallest |Q - limit| the yardstick met at a live PV bus, in any round, is
             >= 1e-4 -- a condition on the inputs: kernel and yardstick agree to about tol ||J^-1|| times the line scale before a
             decision, orders of magnitude below that;
  residual   the yardstick's mismatch of the WRITTEN table, at all buses, <= tol + 64 * 2^-52 * scale_i (tests/powerflow_checks.py);
  solution   Vm and Va (radians) within 2 tol ||J^-1||_inf of the yardstick's table, J at the FINAL type set;
  given      what the final types give comes back bit for bit, a switched bus's Q being its limit.
Fixture limits, per sample: (lo, hi) = median -+ half the inter-quartile range of the unconstrained solution's Q at the PV buses, the
same pair at every bus (`band_limits`); (5, 6) has one PV bus and gets hi = Q_free - 0.05.  Then: no limits against the dense
solver's yardstick, per-sample types, independence from the batch, failures that stay local, the edge blocks and the closed loop
through dataset_generator.py --enforce-q-lims.  DESIGN.md section 7q."""
import functools
import re
import types

import numpy as np
import pytest
import torch

from poweflownet_amd.synth import make_physical_inputs
from poweflownet_amd.utils.powerflow import solve_power_flow, solve_power_flow_qlim
from tests import powerflow_qlim_ref as Q
from tests import powerflow_ref as P
from tests.powerflow_checks import DEV, TOL, _dev, _distance, _imbalance_bound, _residual_ratio, _run
from tests.test_gpu_powerflow import _case, _check_ac

pytestmark = pytest.mark.gpu
MAX_ITER = 10
MIN_MARGIN = 1e-4


class _QCase:
    """One shape's inputs on the host with the fixture limits [S, n, 2] and the yardstick's Q-limited solutions, computed once."""

    def __init__(self, n, e, S, seed=1, load=0.2):
        ei, bt, rx, spec = make_physical_inputs(n, e, S, seed, load)
        self.n, self.e, self.S = n, e, S
        self.ei, self.bt, self.rx, self.spec = ei.numpy(), bt.numpy(), rx.numpy(), spec.numpy()
        self.free = np.stack([P.newton(self.bt, self.spec[s], self.ei, self.rx[s], tol=TOL, max_iter=MAX_ITER)[0] for s in range(S)])
        if int((self.bt == 1).sum()) == 1:                          # one PV bus: it switches in round 1 and leaves no PV bus
            pv = int(np.flatnonzero(self.bt == 1)[0])
            self.limits = np.stack([np.tile([-np.inf, self.free[s, pv, 3] - 0.05], (n, 1)) for s in range(S)])
        else:
            self.limits = np.stack([Q.band_limits(self.bt, self.free[s]) for s in range(S)])
        self.ref = [Q.solve(self.bt, self.spec[s], self.ei, self.rx[s], self.limits[s], tol=TOL, max_iter=MAX_ITER) for s in range(S)]

    def solve(self, rows=slice(None), bt=None, limits="fixture", **kw):
        kw = {"tol": TOL, "max_iter": MAX_ITER, **kw}
        bt = self.bt if bt is None else bt
        limits = self.limits[rows] if isinstance(limits, str) else limits
        return solve_power_flow_qlim(_dev(bt[rows] if bt.ndim == 2 else bt), _dev(self.spec[rows]), _dev(self.ei), _dev(self.rx[rows]),
                                     None if limits is None else _dev(limits), **kw)


@functools.lru_cache(maxsize=None)
def _qcase(n, e, S):
    return _QCase(n, e, S)


class _Grid:
    """what `_residual_ratio` reads of a case"""

    def __init__(self, ei, rx):
        self.ei, self.rx = ei, rx


def _check_against(refs, res, ei, rx, spec, what):
    """`res` against the yardstick's `refs` (one QLimRef per sample, all converged): decisions exact, the bounds of the docstring."""
    table, status = res.table.cpu().numpy(), res.status.cpu().numpy()
    types, rounds = res.bus_type.cpu().numpy(), res.rounds.cpu().numpy()
    S = len(refs)
    assert table.shape == (S,) + spec.shape[1:] and table.dtype == np.float64 and types.dtype == rounds.dtype == np.int32
    assert int(res.flags.item()) == 0 and torch.equal(res.iterations, res.status) and bool((res.residual < TOL).all())
    assert all(r.table is not None for r in refs)
    assert np.array_equal(types, np.stack([r.bus_type for r in refs])), what
    assert rounds.tolist() == [r.rounds for r in refs], (what, rounds.tolist(), [r.rounds for r in refs])
    assert ((status >= rounds + 1) & (status <= (rounds + 1) * MAX_ITER)).all(), (what, status, rounds)
    worst_f = _residual_ratio(_Grid(ei, rx), table)
    worst_x = 0.0
    for s, r in enumerate(refs):
        inv_norm = P.jacobian_inverse_norm(r.table, r.bus_type, ei, rx[s])
        worst_x = max(worst_x, float(_distance(table[s], r.table) / (2 * TOL * inv_norm)))
        ty = r.bus_type
        # given quantities under the FINAL types, bit for bit; r.spec's Q of a switched bus is the limit it was fixed at
        assert np.array_equal(table[s][ty != 2, 0], spec[s][ty != 2, 0]) and np.array_equal(table[s][ty != 0, 2], spec[s][ty != 0, 2])
        assert np.array_equal(table[s][ty == 2, 3], r.spec[ty == 2, 3]) and np.array_equal(table[s][ty == 0, 1], spec[s][ty == 0, 1])
    print(f"{what}: route {res.route}, rounds {rounds.min()}..{rounds.max()}, solves {status.min()}..{status.max()}, PQ buses at the end "
          f"{(types == 2).sum(axis=1).min()}..{(types == 2).sum(axis=1).max()}, worst |mismatch| / bound {worst_f:.3g}, "
          f"worst |x - yardstick| / (2 tol ||J^-1||) {worst_x:.3g}")
    assert worst_f <= 1.0 and worst_x <= 1.0, (what, worst_f, worst_x)


def _check_fixture(case, res, what):
    margin = min(r.margin for r in case.ref)
    assert margin >= MIN_MARGIN, (what, margin)                      # a condition on the inputs: no decision is close
    _check_against(case.ref, res, case.ei, case.rx, case.spec, f"{what} (smallest margin {margin:.3g})")
    table, types = res.table.cpu().numpy(), res.bus_type.cpu().numpy()
    moved = types != case.bt
    assert moved.any(axis=1).all() and (case.bt[np.nonzero(moved)[1]] == 1).all() and (types[moved] == 2).all()
    for s in range(case.S):                                          # a switched bus's Q is ITS limit, bit for bit
        q = table[s, moved[s], 3]
        assert (np.equal(q, case.limits[s, moved[s], 0]) | np.equal(q, case.limits[s, moved[s], 1])).all()


# ------------------------------------------------------------------------------------------- decisions and solution
@pytest.mark.parametrize("n,e,S", [(5, 6, 3), (14, 20, 16), (70, 100, 8), (118, 186, 4)])
def test_decisions_and_solution(n, e, S):
    case = _qcase(n, e, S)
    res = case.solve()
    assert res.route == ("lds" if n <= 70 else "global")
    _check_fixture(case, res, f"n {n} e {e} S {S}")
    if n == 5:
        assert not (res.bus_type == 1).any() and res.rounds.tolist() == [1] * S
    else:
        assert max(r.rounds for r in case.ref) >= 2
    if n <= 70:
        assert torch.equal(case.solve(route="lds").table, res.table)
    else:
        with pytest.raises(RuntimeError, match=r"code -1.*LDS"):
            case.solve(route="lds")


def test_the_global_route_meets_the_same_bounds():
    case = _qcase(14, 20, 16)
    res = case.solve(route="global")
    assert res.route == "global"
    _check_fixture(case, res, "global route, n 14 e 20 S 16")


# --------------------------------------------------------------------------------------------------------- no limits
@pytest.mark.parametrize("n,e,S", [(14, 20, 64), (118, 186, 8)])
def test_without_limits_it_is_the_dense_solve(n, e, S):
    case = _case(n, e, S)                                             # test_gpu_powerflow.py's case and its yardstick solutions
    res = solve_power_flow_qlim(_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), None, tol=TOL, max_iter=MAX_ITER)
    _check_ac(case, res, f"no limits, n {n} e {e} S {S}")
    assert res.rounds.tolist() == [0] * S and torch.equal(res.bus_type, _dev(case.bt.astype(np.int32)).expand(S, n))
    dense = case.solve()
    print(f"no limits, n {n}: table bit-equal to solve_power_flow's: {torch.equal(res.table, dense.table)}, "
          f"status equal: {torch.equal(res.status, dense.status)}, routes {res.route} / {dense.route}")
    # limits nobody reaches, and limits that are not there, change nothing
    wide = torch.tensor([[-1e9, 1e9]], dtype=torch.float64, device=DEV).expand(n, 2)
    open_ = torch.tensor([[float("nan"), float("inf")]], dtype=torch.float64, device=DEV).expand(n, 2)
    for lim in (wide, open_):
        again = solve_power_flow_qlim(_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), lim, tol=TOL, max_iter=MAX_ITER)
        assert torch.equal(again.table, res.table) and torch.equal(again.status, res.status) and again.rounds.tolist() == [0] * S


def _own_types(n, e, S, seed):
    """Every sample its own PV set -- sample s has the buses i with i % 3 == s % 3 (bus 0 stays the slack) -- and a specification
    drawn for THOSE types the way make_physical_inputs draws it."""
    ei, _, rx, _ = make_physical_inputs(n, e, S, seed)
    rng = np.random.default_rng(seed + 1000)
    types, spec = np.full((S, n), 2, dtype=np.int64), np.zeros((S, n, 4))
    for s in range(S):
        types[s, (s % 3)::3] = 1
        types[s, 0] = 0
        pv, pq = np.flatnonzero(types[s] == 1), np.flatnonzero(types[s] == 2)
        spec[s, types[s] != 2, 0] = rng.uniform(1.00, 1.05, n - pq.size)
        spec[s, pq, 2] = rng.normal(0.2, 0.02, pq.size)
        spec[s, pq, 3] = rng.normal(0.05, 0.005, pq.size)
        spec[s, pv, 2] = -spec[s, pq, 2].sum() / pv.size * rng.uniform(0.8, 1.2, pv.size)
    return ei.numpy(), types, rx.numpy(), spec


def test_per_sample_types_without_limits():
    n, e, S = 14, 20, 8
    ei, types, rx, spec = _own_types(n, e, S, seed=5)
    assert len({t.tobytes() for t in types}) == 3
    refs = [Q.solve(types[s], spec[s], ei, rx[s], None, tol=TOL, max_iter=MAX_ITER) for s in range(S)]
    for route in ("auto", "global"):
        res = solve_power_flow_qlim(_dev(types), _dev(spec), _dev(ei), _dev(rx), None, tol=TOL, max_iter=MAX_ITER, route=route)
        _check_against(refs, res, ei, rx, spec, f"per-sample types, route {route}")
        assert torch.equal(res.bus_type, _dev(types.astype(np.int32))) and res.rounds.tolist() == [0] * S
    # a sample with its own row against the same sample under that row shared
    for s in (0, 1, 2):
        one = solve_power_flow_qlim(_dev(types[s]), _dev(spec[s:s + 1]), _dev(ei), _dev(rx[s:s + 1]), None, tol=TOL, max_iter=MAX_ITER, route="global")
        assert torch.equal(one.table[0], res.table[s]) and int(one.status[0]) == int(res.status[s])


# ------------------------------------------------------------------------------------------------------ independence
def _same(a, b):
    return (torch.equal(a.table, b.table) and torch.equal(a.status, b.status) and torch.equal(a.rounds, b.rounds)
            and torch.equal(a.bus_type, b.bus_type) and torch.equal(a.residual, b.residual))


def _cat(parts):
    return types.SimpleNamespace(**{f: torch.cat([getattr(r, f) for r in parts]) for f in ("table", "status", "residual", "bus_type", "rounds")})


def test_a_sample_does_not_depend_on_its_batch():
    case = _qcase(14, 20, 16)
    whole = case.solve()
    assert bool((whole.status >= 1).all()) and len(set(whole.rounds.tolist())) > 1
    assert _same(_cat([case.solve(rows=slice(k, k + 1)) for k in range(case.S)]), whole)
    assert _same(_cat([case.solve(rows=slice(0, 5)), case.solve(rows=slice(5, 16))]), whole)
    assert _same(case.solve(), whole)
    # shared [n, 2] limits against the same limits repeated per sample; shared [n] types against the row repeated
    shared = case.solve(limits=case.limits[3])
    assert bool((shared.rounds >= 1).all()) and bool((shared.status >= 1).all())
    assert _same(case.solve(limits=np.stack([case.limits[3]] * case.S)), shared)
    assert _same(case.solve(bt=np.stack([case.bt] * case.S)), whole)
    assert _same(case.solve(route="global"), whole)                  # (the matrix's address is no input either)


# ---------------------------------------------------------------------------------------------------------- failures
@pytest.mark.parametrize("route", ["auto", "global"])
def test_failures_stay_local(route):
    case = _qcase(14, 20, 16)
    S, n = case.S, case.n
    rounds = [r.rounds for r in case.ref]
    two, one = [s for s in range(S) if rounds[s] == 2], [s for s in range(S) if rounds[s] == 1]
    assert len(two) >= 1 and len(one) >= 4 and len(two) + len(one) == S
    a, b = one[0], one[1]                                             # a: two slacks; b: a non-finite start
    types = np.stack([case.bt] * S)
    types[a, 1] = 0
    init = np.zeros((S, n, 2))
    init[:, :, 0] = 1.0                                               # the flat start, spelled out: Vm 1 at PQ buses, Va the slack's 0
    clean = case.solve(bt=np.stack([case.bt] * S), init=_dev(init), route=route)
    assert _same(clean, case.solve(route=route)) and int(clean.flags.item()) == 0
    init[b, int(np.flatnonzero(case.bt == 2)[0]), 0] = np.nan
    res = case.solve(bt=types, init=_dev(init), max_rounds=1, route=route)
    status = res.status.tolist()
    assert status[a] == -5 and status[b] == -3 and [status[s] for s in two] == [-7] * len(two)
    assert int(res.flags.item()) == 1                                 # bit 0: a type row was refused, as on the dense route
    failed = [a, b] + two
    assert torch.isnan(res.table[failed]).all() and torch.equal(res.bus_type[failed], _dev(types[failed].astype(np.int32)))
    assert res.rounds[[a, b]].tolist() == [0, 0] and res.rounds[two].tolist() == [1] * len(two)
    assert res.iterations.tolist() == [s if s >= 0 else -1 for s in status]
    assert torch.isnan(res.residual[[a, b]]).all() and bool((res.residual[two] < TOL).all())
    keep = one[2:]
    for f in ("table", "status", "rounds", "bus_type", "residual"):
        assert torch.equal(getattr(res, f)[keep], getattr(clean, f)[keep]), f


# ------------------------------------------------------------------------------------------------------- edge blocks
@pytest.mark.parametrize("route", ["auto", "global"])
def test_every_pv_bus_switches(route):
    case = _qcase(14, 20, 16)
    S, n = 8, case.n
    pv = case.bt == 1
    limits = np.stack([np.tile([-np.inf, case.free[s, pv, 3].min() - 0.05], (n, 1)) for s in range(S)])
    refs = [Q.solve(case.bt, case.spec[s], case.ei, case.rx[s], limits[s], tol=TOL, max_iter=MAX_ITER) for s in range(S)]
    assert min(r.margin for r in refs) >= MIN_MARGIN and all(r.rounds == 1 and not (r.bus_type == 1).any() for r in refs)
    res = case.solve(rows=slice(0, S), limits=limits, route=route)
    _check_against(refs, res, case.ei, case.rx[:S], case.spec[:S], f"every PV bus switches (m = m_max = {2 * (n - 1)}), route {route}")
    assert int((res.bus_type == 2).sum()) == S * (n - 1)


def test_limits_on_a_grid_without_a_pv_bus():
    case = _case(14, 20, 8, seed=2, types="no_pv")
    limits = torch.zeros(14, 2, dtype=torch.float64, device=DEV)     # (nobody reads them: the limits belong to PV buses)
    res = solve_power_flow_qlim(_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), limits, tol=TOL, max_iter=MAX_ITER)
    _check_ac(case, res, "no PV bus, limits given")
    assert res.rounds.tolist() == [0] * 8 and torch.equal(res.bus_type, _dev(case.bt.astype(np.int32)).expand(8, 14))


# ------------------------------------------------------------------------------------------------------- closed loop
def test_generator_with_enforced_q_limits(tmp_path):
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
    text = _run(dataset_generator.main, ["--case", "14", "--samples", str(S), "--root", root, "--enforce-q-lims", "--q-limit", repr(cap)])
    assert "Failed to converge and drawn again: 0" in text
    node = np.load(tmp_path / "qlim" / "raw" / "case14_node_features.npy")
    edge = np.load(tmp_path / "qlim" / "raw" / "case14_edge_features.npy")
    assert node.shape == (S, n, 6) and edge.shape == (S, e, 4) and np.isfinite(node).all()
    direct = solve_power_flow_qlim(_dev(bt), _dev(spec), _dev(ei), _dev(rx), _dev(limits), tol=gen_tol)
    types = node[:, :, 1].astype(np.int64)
    assert np.array_equal(types, direct.bus_type.cpu().numpy()) and np.array_equal(node[:, :, 2:], direct.table.cpu().numpy())
    assert np.array_equal(types, want) and len({t.tobytes() for t in types}) > 1
    said = re.search(r"(\d+) sample\(s\) had a bus switched to a load bus, at most (\d+) re-solve", text)
    assert said and int(said.group(1)) == int((types != bt).any(axis=1).sum()) and int(said.group(2)) == int(direct.rounds.max())
    q = node[:, :, 5]
    assert (np.abs(q[types == 1]) <= cap + gen_tol).all() and (np.abs(q[(types == 2) & (bt == 1)]) == cap).all()

    seen = []
    for task in ("train", "val", "test"):
        ds = PowerFlowData(root=root, case="14", split=split, task=task, device=DEV)
        seen += [ds[k].bus_type.cpu().numpy() for k in range(len(ds))]
    assert np.array_equal(np.stack(seen), types)
    ds = PowerFlowData(root=root, case="14", split=split, task="test", device=DEV)
    torch.manual_seed(7)
    model = MaskEmbdMultiMPN(4, 2, 4, 32, 3, 2, 0.0).to(DEV).eval()
    stats = [t.cpu() for t in ds.get_data_means_stds()]
    report = evaluate_report(model, DataLoader(ds, batch_size=4, shuffle=False), DEV, xystd=ds.xystd, power_imbalance=PowerImbalance(*stats))
    got = report["PowerImbalance(ref)"]
    bound = _imbalance_bound(node[24:, :, 2:].astype(np.float32), edge[0, :, :2].T.astype(np.int64), edge[24:, :, 2:].astype(np.float32).astype(np.float64))
    print(f"--enforce-q-lims --q-limit {cap:.6g}: {said.group(0)}; PowerImbalance(ref) {got:.3e} (bound {bound:.3e})")
    assert got < bound

    # without the flag nothing changed: two runs write the same bytes, one type row for all samples, the dense solver's tables
    plain = []
    for name in ("plain_a", "plain_b"):
        text = _run(dataset_generator.main, ["--case", "14", "--samples", str(S), "--root", str(tmp_path / name)])
        assert "switched" not in text
        plain.append([(tmp_path / name / "raw" / f"case14_{kind}_features.npy").read_bytes() for kind in ("node", "edge")])
    assert plain[0] == plain[1]
    node0 = np.load(tmp_path / "plain_a" / "raw" / "case14_node_features.npy")
    assert np.array_equal(node0[:, :, 1], np.broadcast_to(bt, (S, n)))
    dense = solve_power_flow(_dev(bt), _dev(spec), _dev(ei), _dev(rx))
    assert np.array_equal(node0[:, :, 2:], dense.table.cpu().numpy())
