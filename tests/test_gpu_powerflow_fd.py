"""The warm start and the fast-decoupled modes of the batched power-flow solver: `pfn_powerflow_solve_init` (csrc/powerflow.hip)
through `solve_power_flow(mode="fdxb" | "fdbx", init=...)`, held to the float64 yardsticks of tests/powerflow_ref.py and
tests/powerflow_fd_ref.py with tol = 1e-10.  The bounds are the ones tests/test_gpu_powerflow.py holds Newton to, unchanged, because
the state, the mismatch and the convergence test are the same fp64 code --
  residual   the yardstick's mismatch of the WRITTEN table, at all buses, <= tol + 64 * 2^-52 * scale_i;
  solution   Vm and Va (radians) within 2 tol ||J^-1||_inf of the yardstick's NEWTON solution, J at that solution;
-- with max_iter = twice the yardstick's own worst half-iteration count of the case (computed here; counts are not compared: an
fp32 inverse may move them by one).  Then the warm start of modes 0, 2 and 3, independence of a sample from its batch, failures
that stay local, capture, and speedup_evaluator.py end to end.

Worst ratios measured on an MI355X (bound 1; each test prints its own): residual 0.985 (fdxb) / 0.982 (fdbx) -- a linearly converging
iteration stops just under tol --, distance to the Newton yardstick's solution 0.066 / 0.058; half-iterations 14-35 (fdxb) and 13-23
(fdbx) at the shapes with PQ buses, every range equal to the float64 yardstick's.  DESIGN.md section 7j has the table."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.synth import make_topology
from poweflownet_amd.utils.powerflow import solve_power_flow
from tests import powerflow_fd_ref as FD
from tests import powerflow_ref as P
from tests.powerflow_checks import DEV, TOL, _dev, _run
from tests.test_gpu_powerflow import _case

pytestmark = pytest.mark.gpu
MODES = {"ac": 0, "fdxb": 2, "fdbx": 3}
FD_MODES = ("fdxb", "fdbx")
YARDSTICK_CAP = 200                                            # the yardstick's own limit while its worst count is measured


@functools.lru_cache(maxsize=None)
def _max_iter(key, mode):
    """Twice the yardstick's worst half-iteration count over the samples of the case (Newton: the suite's 10)."""
    if mode == "ac":
        return 10
    case = _case(*key)
    counts = [FD.fast_decoupled(case.bt, case.spec[s], case.ei, case.rx[s], mode[2:], tol=TOL, max_iter=YARDSTICK_CAP)[1] for s in range(case.S)]
    assert min(counts) >= 1, counts
    return 2 * max(counts)


def _solve(key, mode, **kw):
    return _case(*key).solve(mode=mode, max_iter=_max_iter(key, mode), **kw)


def _check(key, res, mode, what, lowest=1):
    case, max_iter = _case(*key), _max_iter(key, mode)
    table, status = res.table.cpu().numpy(), res.status.cpu().numpy()
    assert table.shape == (case.S, case.n, 4) and table.dtype == np.float64 and int(res.flags.item()) == 0
    assert ((status >= lowest) & (status <= max_iter)).all(), (what, status, max_iter)
    assert torch.equal(res.iterations, res.status) and bool((res.residual < TOL).all())
    worst_f = worst_x = 0.0
    for s in range(case.S):
        dp, dq = P.mismatch(table[s], case.ei, case.rx[s])
        bound = TOL + 64 * P.EPS64 * P.scale(table[s], case.ei, case.rx[s])
        worst_f = max(worst_f, float((np.maximum(np.abs(dp), np.abs(dq)) / bound).max()))
        dx = max(np.abs(table[s, :, 0] - case.ref[s, :, 0]).max(), np.abs(table[s, :, 1] - case.ref[s, :, 1]).max() * P.RAD)
        worst_x = max(worst_x, float(dx / (2 * TOL * case.inv_norm[s])))
        assert np.array_equal(table[s][case.bt != 2, 0], case.spec[s][case.bt != 2, 0]) and np.array_equal(table[s][case.bt != 0, 2], case.spec[s][case.bt != 0, 2])
        assert np.array_equal(table[s][case.bt == 2, 3], case.spec[s][case.bt == 2, 3]) and np.array_equal(table[s][case.bt == 0, 1], case.spec[s][case.bt == 0, 1])
    print(f"{what} [{mode}]: route {res.route}, iterations {status.min()}..{status.max()} (mean {status.mean():.2f}, max_iter {max_iter}), "
          f"worst |mismatch| / bound {worst_f:.3g}, worst |x - Newton yardstick| / (2 tol ||J^-1||) {worst_x:.3g}")
    assert worst_f <= 1.0 and worst_x <= 1.0, (what, worst_f, worst_x)


def _workspace(case, mode, route=0):
    n_pq = int((case.bt == 2).sum())
    return int(L.load().pfn_powerflow_workspace_bytes_mode(case.S, case.n, case.e, n_pq, MODES[mode], route))


# ----------------------------------------------------------------------------------------- accuracy, routes, edges
LDS_SHAPES = [(5, 6, 3), (14, 20, 16), (70, 100, 8), (118, 186, 4)]


@pytest.mark.parametrize("mode", FD_MODES)
@pytest.mark.parametrize("key", LDS_SHAPES)
def test_residual_and_solution_on_the_lds_route(key, mode):
    case = _case(*key)
    assert _workspace(case, mode) == 0
    res = _solve(key, mode)
    assert res.route == "lds"
    _check(key, res, mode, f"n {key[0]} e {key[1]} S {key[2]}")
    assert torch.equal(_solve(key, mode, route="lds").table, res.table)


@pytest.mark.parametrize("mode", FD_MODES)
@pytest.mark.parametrize("key", [(14, 20, 16), (70, 100, 8)])
def test_the_global_route_meets_the_same_bounds(key, mode):
    case = _case(*key)
    n_pq = int((case.bt == 2).sum())
    mats = sum(((m * (m | 1) + 3) & ~3) for m in (case.n - 1, n_pq))
    assert _workspace(case, mode, route=2) == case.S * mats * 4
    res = _solve(key, mode, route="global")
    assert res.route == "global"
    _check(key, res, mode, f"global route, n {key[0]} e {key[1]} S {key[2]}")


@pytest.mark.parametrize("mode", FD_MODES)
def test_the_shape_newton_cannot_hold_in_lds(mode):
    """(130, 200): m = 215 sends Newton to the global route; the two fast-decoupled matrices (129^2 + 86 * 87 floats) still fit."""
    key = (130, 200, 4)
    case = _case(*key)
    lib = L.load()
    n_pq = int((case.bt == 2).sum())
    assert lib.pfn_powerflow_workspace_bytes(case.S, case.n, case.e, n_pq, 0) > 0        # the old function answers as before
    assert lib.pfn_powerflow_workspace_bytes_mode(case.S, case.n, case.e, n_pq, 0, 0) == lib.pfn_powerflow_workspace_bytes(case.S, case.n, case.e, n_pq, 0)
    assert lib.pfn_powerflow_workspace_bytes_mode(case.S, case.n, case.e, n_pq, 1, 0) == lib.pfn_powerflow_workspace_bytes(case.S, case.n, case.e, 0, 0)
    res = _solve(key, mode)
    assert res.route == ("lds" if _workspace(case, mode) == 0 else "global")
    _check(key, res, mode, "n 130 e 200 S 4")


@pytest.mark.parametrize("mode", FD_MODES)
@pytest.mark.parametrize("types", ["no_pv", "no_pq"])
def test_block_edge_cases(types, mode):
    key = (14, 20, 8, 2, 0.2, types)
    _check(key, _solve(key, mode), mode, types)
    _check(key, _solve(key, mode, route="global"), mode, types + ", global route")


# ------------------------------------------------------------------------------------------------------ warm start
def _flat_init(case):
    """The flat start written out: [S, n, 2] = (1 at PQ buses else the given Vm, the slack's Va in degrees)."""
    slack = int(np.flatnonzero(case.bt == 0)[0])
    init = np.empty((case.S, case.n, 2))
    init[:, :, 0] = np.where(case.bt == 2, 1.0, case.spec[:, :, 0])
    init[:, :, 1] = case.spec[:, slack, 1][:, None]
    return init


def _same(a, b):
    return torch.equal(a.table, b.table) and torch.equal(a.status, b.status) and torch.equal(a.residual, b.residual)


def _old_entry(case, mode=0, max_iter=10):
    """`pfn_powerflow_solve`, the entry point without `init`, called directly."""
    bt, spec, ei, rx = _dev(case.bt.astype(np.int32)), _dev(case.spec), _dev(case.ei), _dev(case.rx)
    table = torch.empty(case.S, case.n, 4, dtype=torch.float64, device=DEV)
    status = torch.empty(case.S, dtype=torch.int32, device=DEV)
    residual = torch.empty(case.S, dtype=torch.float64, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = L.load().pfn_powerflow_solve(ei.data_ptr(), 0, case.e, rx.data_ptr(), bt.data_ptr(), spec.data_ptr(), case.S, case.n,
                                      int((case.bt == 1).sum()), int((case.bt == 2).sum()), mode, C.c_double(TOL), max_iter, 0,
                                      table.data_ptr(), status.data_ptr(), residual.data_ptr(), flags.data_ptr(), None, 0, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, table, status, residual


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("key", [(14, 20, 16), (118, 186, 4)])
def test_the_flat_start_written_out_is_the_flat_start(key, mode):
    case = _case(*key)
    cold = _solve(key, mode)
    assert bool((cold.status >= 1).all())
    assert _same(_solve(key, mode, init=_dev(_flat_init(case))), cold)
    if mode == "ac":
        rc, table, status, residual = _old_entry(case)
        assert rc == 0 and torch.equal(table, cold.table) and torch.equal(status, cold.status) and torch.equal(residual, cold.residual)
        assert L.load().pfn_powerflow_solve(None, 0, 0, None, None, None, 0, 5, 1, 3, 2, C.c_double(TOL), 10, 0, None, None, None, None, None, 0,
                                            None) == -1                                   # the old entry still knows modes 0 and 1 only


@pytest.mark.parametrize("mode", sorted(MODES))
def test_warm_starts(mode):
    key = (14, 20, 16)
    case = _case(*key)
    cold = _solve(key, "ac")
    # ---- a converged table: nothing is solved
    done = _solve(key, mode, init=cold.table)
    assert done.status.tolist() == [0] * case.S and bool((done.residual < TOL).all()) and int(done.flags.item()) == 0
    _check(key, done, mode, "start = Newton's table", lowest=0)
    assert torch.equal(done.table[:, :, 0], cold.table[:, :, 0])
    # ---- the solution plus N(0, 1e-3) in Vm and in radians
    rng = np.random.default_rng(5)
    near = cold.table.cpu().numpy()[:, :, :2] + rng.normal(size=(case.S, case.n, 2)) * np.array([1e-3, 1e-3 / P.RAD])
    warm = _solve(key, mode, init=_dev(near))
    _check(key, warm, mode, "start = solution + N(0, 1e-3)")
    flat = _solve(key, mode)
    print(f"[{mode}] iterations from the flat start {flat.status.tolist()}, from solution + noise {warm.status.tolist()}")
    if mode == "ac":
        assert bool((warm.status <= flat.status).all())
        for s in range(case.S):                                                            # ... and the yardstick agrees on the count's bound
            assert FD.newton_from(case.bt, case.spec[s], case.ei, case.rx[s], init=near[s], tol=TOL)[1] <= int(flat.status[s])
    # ---- what is never read may hold anything: the slack's row and the PV buses' Vm
    junk = near.copy()
    junk[:, case.bt == 0] = np.nan
    junk[:, case.bt == 1, 0] = np.array([np.inf, -7.0, np.nan, 1e300])[np.arange((case.bt == 1).sum()) % 4]
    assert _same(_solve(key, mode, init=_dev(junk)), warm)
    # ---- any float table [S, n, >= 2] on the device: cast there
    wide = torch.cat([_dev(near), torch.full((case.S, case.n, 2), float("nan"), dtype=torch.float64, device=DEV)], dim=2).float()
    assert wide.dtype == torch.float32 and tuple(wide.shape) == (case.S, case.n, 4)
    assert _same(_solve(key, mode, init=wide), _solve(key, mode, init=wide[:, :, :2].double()))
    _check(key, _solve(key, mode, init=wide), mode, "start = a float32 [S, n, 4] table")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _solve(key, mode, init=torch.from_numpy(near))
    with pytest.raises(RuntimeError, match="init must be"):
        _solve(key, mode, init=_dev(near[:, :-1]))


# ---------------------------------------------------------------------------------------------------- independence
@pytest.mark.parametrize("mode", FD_MODES)
def test_a_sample_does_not_depend_on_its_batch(mode):
    key = (14, 20, 8, 3)
    case = _case(*key)
    kw = {"mode": mode, "max_iter": _max_iter(key, mode)}
    init = _flat_init(case) + np.random.default_rng(2).normal(size=(case.S, case.n, 2)) * np.array([1e-2, 1.0])
    lists = np.stack([make_topology(14, 20, seed=k).numpy() for k in range(4)])
    batch = case.solve(rows=slice(0, 4), ei=lists, init=_dev(init[:4]), **kw)
    assert bool((batch.status >= 1).all())
    for k in range(4):                                         # [S, 2, e] against four single-sample calls in [2, e] form
        one = case.solve(rows=slice(k, k + 1), ei=lists[k], init=_dev(init[k:k + 1]), **kw)
        assert torch.equal(one.table[0], batch.table[k]) and int(one.status[0]) == int(batch.status[k])
        assert torch.equal(one.residual[0], batch.residual[k])
    for start in (None, init):
        part = (lambda r: None) if start is None else (lambda r: _dev(start[r]))
        whole = case.solve(init=part(slice(None)), **kw)
        a, b = case.solve(rows=slice(0, 3), init=part(slice(0, 3)), **kw), case.solve(rows=slice(3, 8), init=part(slice(3, 8)), **kw)
        assert bool((whole.status >= 1).all())
        assert torch.equal(torch.cat([a.table, b.table]), whole.table) and torch.equal(torch.cat([a.status, b.status]), whole.status)
        assert torch.equal(torch.cat([a.residual, b.residual]), whole.residual)
        assert _same(case.solve(init=part(slice(None)), **kw), whole)


# -------------------------------------------------------------------------------------------------------- failures
@pytest.mark.parametrize("mode", sorted(MODES))
def test_failures_stay_local(mode):
    n, e = 14, 20
    key = (n, e, 8, 4)
    good, heavy = _case(*key), _case(n, e, 8, 4, 2.0)
    kw = {"mode": mode, "tol": TOL, "max_iter": _max_iter(key, mode)}
    lists = np.stack([good.ei] * 8)
    spec, rx, init = good.spec.copy(), good.rx.copy(), _flat_init(good)
    clean = solve_power_flow(_dev(good.bt), _dev(spec), _dev(lists), _dev(rx), init=_dev(init), **kw)
    pq = int(np.flatnonzero(good.bt == 2)[0])
    init[1, pq, 0] = np.nan                                    # sample 1: a NaN where the start is read
    lists[2] = np.where(lists[2] == 13, 1, lists[2])           # sample 2: bus 13 has no line
    spec[5], rx[5] = heavy.spec[5], heavy.rx[5]                # sample 5: ten times the load
    lists[6, 1, 7] = n                                         # sample 6: a line to bus id n
    for route in ("auto", "global"):
        res = solve_power_flow(_dev(good.bt), _dev(spec), _dev(lists), _dev(rx), init=_dev(init), route=route, **kw)
        status = res.status.tolist()
        print(f"[{mode}, {route}] statuses {status}")
        assert [status[k] for k in (1, 2, 6)] == [-3, -2, -4] and int(res.flags.item()) == 0
        assert status[5] == -1 if mode == "ac" else status[5] in (-1, -3)      # (a diverging fast-decoupled run may overflow first)
        assert res.iterations.tolist() == [s if s >= 0 else -1 for s in status]
        assert torch.isnan(res.table[[1, 2, 5, 6]]).all() and torch.isnan(res.residual[1])
        if route == "auto":
            keep = [0, 3, 4, 7]
            assert bool((clean.status >= 1).all())
            assert torch.equal(res.table[keep], clean.table[keep]) and torch.equal(res.status[keep], clean.status[keep])
            assert torch.equal(res.residual[keep], clean.residual[keep])


def _inputs(case):
    return _dev(case.bt.astype(np.int32)), _dev(case.spec), _dev(case.ei), _dev(case.rx)


def _raw_call(case, inputs, mode, n_pv, n_pq, max_iter, table, status, residual, flags, init=None):
    """`pfn_powerflow_solve_init` itself, on device tensors the caller made (and keeps alive): nothing but the launch."""
    bt, spec, ei, rx = inputs
    return L.load().pfn_powerflow_solve_init(ei.data_ptr(), 0, case.e, rx.data_ptr(), bt.data_ptr(), spec.data_ptr(), L.ptr(init), case.S,
                                             case.n, n_pv, n_pq, mode, C.c_double(TOL), max_iter, 0, table.data_ptr(), status.data_ptr(),
                                             residual.data_ptr(), flags.data_ptr(), None, 0, L.stream_ptr())


@pytest.mark.parametrize("mode", FD_MODES)
def test_counts_that_contradict_bus_type_raise_the_flag(mode):
    case = _case(14, 20, 8, 4)
    n_pv, n_pq = int((case.bt == 1).sum()), int((case.bt == 2).sum())
    guard = -7.5
    table = torch.full((case.S + 1, case.n, 4), guard, dtype=torch.float64, device=DEV)
    status = torch.full((case.S,), 99, dtype=torch.int32, device=DEV)
    residual = torch.zeros(case.S, dtype=torch.float64, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    # one PQ bus fewer, one PV bus more than the device array holds: the launch is sized for a smaller B'' and must not obey it
    rc = _raw_call(case, _inputs(case), MODES[mode], n_pv + 1, n_pq - 1, 40, table, status, residual, flags)
    torch.cuda.synchronize()
    assert rc == 0
    assert int(flags.item()) & 1 and status.tolist() == [-5] * case.S
    assert torch.isnan(table[:case.S]).all() and bool((table[case.S] == guard).all())


def test_an_unknown_mode_is_refused():
    case = _case(14, 20, 8, 4)
    n_pv, n_pq = int((case.bt == 1).sum()), int((case.bt == 2).sum())
    table = torch.zeros(case.S, case.n, 4, dtype=torch.float64, device=DEV)
    status = torch.zeros(case.S, dtype=torch.int32, device=DEV)
    residual = torch.zeros(case.S, dtype=torch.float64, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    for bad in (4, -1):
        rc = _raw_call(case, _inputs(case), bad, n_pv, n_pq, 10, table, status, residual, flags)
        assert rc == -1 and b"mode" in L.load().pfn_last_error()
    assert L.load().pfn_powerflow_workspace_bytes_mode(case.S, case.n, case.e, n_pq, 4, 2) == 0
    torch.cuda.synchronize()
    assert not table.any() and not status.any()
    with pytest.raises(ValueError, match="mode"):
        case.solve(mode="gs")


# --------------------------------------------------------------------------------------------------------- capture
@pytest.mark.parametrize("mode,warm", [("fdxb", False), ("fdbx", False), ("fdxb", True), ("ac", True)])
def test_a_solve_is_capturable(mode, warm):
    """No sync, no allocation inside the launch: a hipGraph holding it replays the same solve into the same tensors, bit for bit."""
    key = (14, 20, 16)
    case = _case(*key)
    n_pv, n_pq = int((case.bt == 1).sum()), int((case.bt == 2).sum())
    init = _dev(_flat_init(case) + np.random.default_rng(3).normal(size=(case.S, case.n, 2)) * np.array([1e-3, 0.1])) if warm else None
    want = _solve(key, mode, init=init)                        # eager (and the LDS limit of the kernel is raised before the capture)
    assert bool((want.status >= 1).all())
    table = torch.zeros(case.S, case.n, 4, dtype=torch.float64, device=DEV)
    status = torch.zeros(case.S, dtype=torch.int32, device=DEV)
    residual = torch.zeros(case.S, dtype=torch.float64, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    inputs, max_iter = _inputs(case), _max_iter(key, mode)
    torch.cuda.synchronize()
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            rc = _raw_call(case, inputs, MODES[mode], n_pv, n_pq, max_iter, table, status, residual, flags, init=init)
    assert rc == 0
    for _ in range(2):
        table.fill_(-7.0)
        status.fill_(99)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(table, want.table) and torch.equal(status, want.status) and torch.equal(residual, want.residual)
    assert int(flags.item()) == 0


# ------------------------------------------------------------------------------------------------------ end to end
def test_speedup_evaluator(tmp_path):
    import re
    import dataset_generator
    import dc_error
    import speedup_evaluator
    root = str(tmp_path / "solved")
    _run(dataset_generator.main, ["--case", "14", "--samples", "32", "--root", root])
    torch.manual_seed(0)
    text = _run(speedup_evaluator.main, ["--case", "14", "--data-dir", root, "--split", "0.5", "0.25", "0.25", "--hidden_dim", "32",
                                        "--n_gnn_layers", "3", "--K", "2"])
    print(text)
    assert "RANDOM" in text and "Number of samples: 8" in text             # 32 samples: the last quarter is the test split
    assert all(h in text for h in ("Results with auto_init:", "Results with results init:", "Results DC:"))
    value = {}
    for name in ("nr", "fdxb", "fdbx", "nr_result_init", "fdxb_result_init", "fdbx_result_init", "dc"):
        sec = re.search(rf"^{name}: (\S+)$", text, flags=re.M)
        row = re.search(rf"^{name} solves: mean (\S+) max (\S+) failures (\d+)$", text, flags=re.M)
        assert sec and row, name
        value[name] = (float(sec.group(1)), float(row.group(1)), int(row.group(2)), int(row.group(3)))
    for name in ("nr", "fdxb", "fdbx", "dc"):                               # flat starts on a solved set: finite, no failure
        sec, mean, most, failed = value[name]
        assert 0 < sec < 1 and np.isfinite(mean) and 1 <= mean <= most and failed == 0, (name, value[name])
    for name in ("nr_result_init", "fdxb_result_init", "fdbx_result_init"):  # a random model's start: finite figures, failures counted
        sec, mean, most, failed = value[name]
        assert 0 < sec < 1 and np.isfinite(mean) and 0 <= mean <= most and 0 <= failed < 8, (name, value[name])
    gnn = float(re.search(r"^GNNs:  (\S+)$", text, flags=re.M).group(1))
    loss_dc = float(re.search(r"^Loss DC: (\S+)$", text, flags=re.M).group(1))
    loss_init = float(re.search(r"^Loss result_init: (\S+)$", text, flags=re.M).group(1))
    assert 0 < gnn < 1 and np.isfinite(loss_dc)
    assert loss_dc == float(dc_error.dc_losses(root, "14", split=(.5, .25, .25)).mean())
    assert np.isfinite(loss_init) and loss_init >= 0
