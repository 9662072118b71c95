"""The AC N-1 screen on the sparse route: `pfn_contingency_ac_sparse` (csrc/contingency_ac_sparse.hip) through
`contingency_screen_ac(route="sparse", plan=sparse_plan(..., mode="fd"))`, held to the float64 yardstick of tests/contingency_ac_ref.py
exactly as tests/test_gpu_contingency_ac.py holds the dense route (the same inputs, `make_physical_inputs(n, e, S, seed=1)`; every
shape's grid has a bridge, and outages with one end and with both ends outside the PQ set):

  base        `base_table`, `status`, `residual` are `torch.equal` to `solve_power_flow(mode="fd" + variant, route="sparse", plan=plan)`;
  state       the kept state of every non-islanding outage k against the yardstick's compensated form STARTED AT THE DEVICE'S base state,
              theta (radians) and Vm separately:
                  |dev - f64| <= C_BOUND * u_k + the fp32 rounding of the table,   u_k = 2^-24 max_i |state_i - base_i| / min(|den'_k|, |den''_k|)
  currents    within `branch_flows`' bound (C = 32) of `branch_ref.flows` evaluated at the DEVICE's kept state;
  mismatch    the yardstick's up to what the state's deviation is worth in a bus's line sums (the dense test's bound);
  figures     severity, worst line, overloads, vm_min, vm_min_bus, v_violations are bit-exact functions of the kernel's own tables in numpy
              fp32; the worst line is the yardstick's wherever its top two loadings differ by more than twice the bounds;
  the rest    tile edges, the shape beyond the dense cap, both sides of the LDS threshold, bit-for-bit independence of the batch, of
              `groups`, `threads` and the placement; `halves` 0, odd, 40 (against `verify_contingencies(route="sparse")`); the dense
              screen; failures that stay local; graph capture; the script.

Worst state ratios (|dev - f64| - rounding) / u measured on an MI355X (each test prints its own; WORST below): 0 at
(3, 3) (the fp32 table's rounding covers it), 3.43 at (5, 6), 5.1 at (14, 20), 6.0 at (70, 100), 5.25 at (118, 186), 3.52 / 7.21 / 3.64 at the
tile edges (40, 63 / 64 / 65), 3.81 at (80, 120, the last in LDS), 3.83 at (81, 121), 20.4 at (1100, 1530); "bx" 7.14, one half 5.1, three
halves 0.35, four halves 0.27 at (14, 20).  The same on both placements, as it must be.  They are a few units on every grid the dense
screen takes -- a substitution through the fp32 factor carries the factor's rounding once, where the dense route's Gauss-Jordan inverses
carry cond(B) units (32.9 at (118, 186) there) -- and grow with the depth of the elimination.  C_BOUND = 128 is the smallest power of two
>= 4 x the worst (4 x 20.4 = 82), DESIGN 7t's rule.  Currents: at most 0.043 of `branch_flows`' bound.  40 halves: mismatch 2.9e-14 at
(14, 20), 1.5e-11 at (118, 186)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.loss import branch_flows
from poweflownet_amd.utils.contingency import contingency_screen_ac, verify_contingencies
from poweflownet_amd.utils.powerflow import solve_power_flow, sparse_plan
from tests import branch_ref as B
from tests import contingency_ac_ref as A
from tests import contingency_ac_checks as K
from tests import powerflow_ref as P
from tests.contingency_ac_checks import EPS, MAX_ITER, _all_failed, _base_currents, _base_of, _bits, _same, _yard
from tests.powerflow_checks import DEV, TOL, _dev, _run
from tests.test_gpu_contingency_ac import C_BOUND as DENSE_C_BOUND          # (the dense route's measured bound: test_against_the_dense_screen)
from tests.test_gpu_powerflow import _case

pytestmark = pytest.mark.gpu
# (n, e, S): the issue's five, the three tile edges, and the shape beyond the dense cap
SHAPES = [(3, 3, 2), (5, 6, 3), (14, 20, 8), (70, 100, 2), (118, 186, 2)]
TILES = [(40, 63, 2), (40, 64, 2), (40, 65, 2)]
BEYOND = (1100, 1530, 1)
# worst (|dev - f64| - rounding) / u measured on an MI355X per (n, e), two halves, "xb": the figures C_BOUND was set from
WORST = {(3, 3): 0.0, (5, 6): 3.43, (14, 20): 5.1, (70, 100): 6.0, (118, 186): 5.25, (40, 63): 3.52, (40, 64): 7.21, (40, 65): 3.64, (80, 120): 3.81,
         (81, 121): 3.83, (1100, 1530): 20.4}
C_BOUND = 128.0
assert C_BOUND == 2.0 ** np.ceil(np.log2(4 * max(WORST.values())))


@functools.lru_cache(maxsize=None)
def _plan(case):
    return sparse_plan(_dev(case.bt), _dev(case.ei), mode="fd")


def _fits_lds(plan):
    """does the forced LDS placement take this plan's block?  (the library says: 0 bytes where it refuses)"""
    return int(L.load().pfn_contingency_ac_sparse_workspace_bytes(1, plan.e, C.addressof(plan.header), 1, 0)) != 0


def _placements(case):
    return ("lds", "global") if _fits_lds(_plan(case)) else ("global",)


def _screen(case, rows=slice(None), ratings=None, ei=None, spec=None, rx=None, plan=None, **kw):
    kw = {"tol": TOL, "max_iter": MAX_ITER, **kw}
    return contingency_screen_ac(_dev(case.bt), _dev((case.spec if spec is None else spec)[rows]), _dev(case.ei if ei is None else ei),
                                 _dev((case.rx if rx is None else rx)[rows]), None if ratings is None else _dev(ratings), route="sparse",
                                 plan=_plan(case) if plan is None else plan, **kw)


def _check_base(case, res, variant, **kw):
    direct = solve_power_flow(_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), mode="fd" + variant, tol=TOL, max_iter=MAX_ITER,
                              route="sparse", plan=_plan(case), **kw)
    assert torch.equal(_bits(res.base_table), _bits(direct.table)) and torch.equal(res.status, direct.status)
    assert torch.equal(_bits(res.residual), _bits(direct.residual))
    return direct


def _check(case, res, variant, halves, what, ratings=None, **kw):
    """contingency_ac_checks' `_check` under this route's C_BOUND, and what this route reports of its placement"""
    assert res.route == "sparse" and res.group == 0 and res.block in ("lds", "global")
    return K._check(case, res, variant, halves, what, C_BOUND, ratings, **kw)


def _full(case, what, variant="xb", halves=2):
    """item 1's check on every placement the shape takes; the placements agree bit for bit"""
    plain = _screen(case)                                                   # (no ratings: 1.0 everywhere; also the one host read)
    ratings = 1.2 * _base_currents(case, plain).max(axis=0)                 # [e]
    got = {}
    for block in _placements(case):
        res = _screen(case, ratings=ratings, keep_table=True, keep_state=True, block=block, variant=variant, halves=halves)
        assert res.block == block
        _check_base(case, res, variant)
        _check(case, res, variant, halves, f"{what} block {block}", ratings)
        got[block] = res
    first = next(iter(got.values()))
    assert all(_same(first, other) for other in got.values())
    auto = _screen(case, ratings=ratings, keep_table=True, keep_state=True, variant=variant, halves=halves)
    assert auto.block == _placements(case)[0] and _same(auto, first)
    if variant == "xb" and halves == 2:
        for k in ("vm_min", "vm_min_bus", "v_violations", "mismatch", "base_table", "status", "residual"):
            assert torch.equal(_bits(getattr(plain, k)), _bits(getattr(first, k))), k   # (the ratings change the loading figures only)
    return first


# -------------------------------------------------------------------------------------------------- the screen itself
@pytest.mark.parametrize("n,e,S", SHAPES)
def test_states_currents_and_figures_against_the_yardstick(n, e, S):
    _full(_case(n, e, S), f"n {n} e {e} S {S}")


@pytest.mark.parametrize("n,e,S", TILES)
def test_tile_edges(n, e, S):
    """a partial tile, exactly one tile, a full tile plus a one-lane tile"""
    case = _case(n, e, S)
    assert _placements(case) == ("lds", "global")
    _full(case, f"tile edge n {n} e {e}")


def test_beyond_the_dense_cap():
    n, e, S = BEYOND
    case = _case(n, e, S)
    assert n - 1 > int(L.load().pfn_powerflow_max_unknowns())
    with pytest.raises(ValueError, match="max_unknowns"):
        contingency_screen_ac(_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx))
    res = _full(case, f"beyond the cap n {n} e {e}")
    assert res.block == "global" and bool((res.islands > 0).any())


def test_both_sides_of_the_lds_threshold():
    """the largest n whose block fits LDS and one more, found through the library's own sizes"""
    lib = L.load()
    n = 40
    while _fits_lds(_plan(_case(n + 1, n + 1 + (n + 1) // 2, 1))):
        n += 1
        assert n < 400
    last, first = _case(n, n + n // 2, 1), _case(n + 1, n + 1 + (n + 1) // 2, 1)
    budget = int(lib.pfn_contingency_ac_sparse_block_bytes(C.addressof(_plan(last).header)))
    over = int(lib.pfn_contingency_ac_sparse_block_bytes(C.addressof(_plan(first).header)))
    print(f"the LDS threshold: {n} buses ({budget} bytes) fit, {n + 1} ({over} bytes) do not")
    assert budget <= 159 * 1024 < over
    inside = _full(last, f"last in LDS n {n}")
    assert inside.block == "lds"
    auto = _screen(first, keep_table=True, keep_state=True)
    assert auto.block == "global"
    _check(first, auto, "xb", 2, f"first on the workspace n {n + 1}")
    with pytest.raises(RuntimeError, match="does not fit LDS"):
        _screen(first, block="lds")


@pytest.mark.parametrize("variant,halves", [("bx", 2), ("xb", 3), ("bx", 4), ("xb", 1)])
def test_both_variants_and_odd_halves(variant, halves):
    _full(_case(14, 20, 8), f"variant {variant} halves {halves}", variant, halves)


def test_a_grid_without_a_pq_bus():
    case = _case(14, 20, 2, types="no_pq")
    res = _screen(case, halves=3, keep_table=True, keep_state=True)         # every half is a P half
    _check_base(case, res, "xb")
    _check(case, res, "xb", 3, "no PQ bus")
    ok = (res.islands == 0).cpu().numpy()
    assert torch.isnan(res.vm_min).all() and bool((res.vm_min_bus == -1).all())
    assert bool((res.v_violations[:, torch.from_numpy(ok)] == 0).all())


def test_ratings_per_scenario_and_unmonitored_lines():
    case = _case(14, 20, 8)
    plain = _screen(case)
    base = _base_currents(case, plain)
    ratings = 0.9 * base + 0.05                                             # [S, e]: some lines overloaded before any outage
    ratings[:, 3] = 0.0
    ratings[:, 7] = -1.0
    ratings[2, 11] = np.nan
    res = _screen(case, ratings=ratings, keep_table=True, keep_state=True, v_limits=(0.97, 1.02))
    _check(case, res, "xb", 2, "ratings [S, e]", ratings, limits=(0.97, 1.02))
    w = res.worst_line.cpu().numpy()
    assert not np.isin(w, [3, 7]).any() and not (w[2] == 11).any() and bool((res.overloads[:, (res.islands == 0)] > 0).any())
    assert bool((res.v_violations[:, (res.islands == 0)] > 0).any())
    one = _screen(case, ratings=ratings[0], keep_table=True, keep_state=True)                             # [e]
    _check(case, one, "xb", 2, "ratings [e]", ratings[0])
    none = _screen(case, ratings=np.zeros(case.e), keep_table=True, keep_state=True)
    ok = res.islands == 0
    assert bool((none.severity[:, ok] == 0).all()) and bool((none.worst_line[:, ok] == -1).all()) and bool((none.overloads[:, ok] == 0).all())
    assert torch.equal(_bits(none.post_current), _bits(res.post_current)) and torch.equal(_bits(none.post_state), _bits(res.post_state))


# ------------------------------------------------------------------------------------------------------ independence
def test_no_bit_depends_on_groups_threads_or_the_placement():
    case = _case(70, 100, 4)
    ratings = 1.2 * _base_currents(case, _screen(case))                     # [S, e]
    kw = dict(ratings=ratings, keep_table=True, keep_state=True)
    whole = _screen(case, **kw)
    assert bool((whole.status >= 0).all()) and whole.block == "lds"
    for block in ("lds", "global"):
        for groups in (1, 3, None):
            for threads in (64, 256):
                got = _screen(case, block=block, groups=groups, threads=threads, **kw)
                assert got.block == block and _same(got, whole), (block, groups, threads)


def test_a_scenario_does_not_depend_on_its_batch():
    case = _case(14, 20, 8)
    ratings = 1.2 * _base_currents(case, _screen(case))                     # [S, e]
    whole = _screen(case, ratings=ratings, keep_table=True, keep_state=True)
    a = _screen(case, slice(0, 4), ratings[:4], keep_table=True, keep_state=True)
    b = _screen(case, slice(4, 8), ratings[4:], keep_table=True, keep_state=True)
    assert _same(a, whole, rows_b=slice(0, 4)) and _same(b, whole, rows_b=slice(4, 8))
    one = _screen(case, slice(5, 6), ratings[5:6], keep_table=True, keep_state=True)
    assert _same(one, whole, rows_b=slice(5, 6))


# -------------------------------------------------------------------------------------------------------------- base
def test_the_base_is_the_sparse_fast_decoupled_solve_with_and_without_a_start():
    case = _case(14, 20, 8)
    cold = _screen(case, keep_table=True, keep_state=True)
    _check_base(case, cold, "xb")
    # a start that is converged already: no half runs (status 0) and the factors are there all the same
    start = cold.base_table[:, :, :2].contiguous()
    warm = _screen(case, init=start, keep_table=True, keep_state=True)
    direct = _check_base(case, warm, "xb", init=start)
    assert direct.status.tolist() == [0] * 8
    _check(case, warm, "xb", 2, "a converged start", tag="warm")
    # a start a little off: a few halves
    off = start.clone()
    off[:, :, 0] += 1e-3
    off[:, :, 1] += 0.05
    near = _screen(case, init=off, variant="bx", keep_table=True, keep_state=True)
    _check_base(case, near, "bx", init=off)
    assert bool((near.status > 0).all()) and bool((near.status < cold.status.max()).all())
    _check(case, near, "bx", 2, "a near start", tag="near")


# ------------------------------------------------------------------------------------------------------------ halves
def test_no_half_gives_the_base_loadings_with_the_line_unmonitored():
    case = _case(14, 20, 8)
    res = _screen(case, halves=0, keep_table=True, keep_state=True)
    flows = branch_flows(res.base_table.float(), _dev(case.ei), _dev(case.rx).float())[0][:, :, 0]      # [S, e]: the base currents
    ok = (res.islands == 0).cpu().numpy()
    cur = res.post_current
    for k in np.flatnonzero(ok):
        keep = torch.arange(case.e, device=DEV) != int(k)
        assert torch.equal(_bits(cur[:, k][:, keep]), _bits(flows[:, keep])) and torch.isnan(cur[:, k, k]).all()
        assert torch.equal(_bits(res.post_state[:, k]), _bits(res.base_table[:, :, :2].float()))
        want = flows.clone()
        want[:, k] = -1.0
        assert torch.equal(res.severity[:, k], want.max(dim=1).values) and bool((res.worst_line[:, k] != k).all())
    assert bool((res.mismatch[:, torch.from_numpy(ok)] >= 0).all())


@pytest.mark.parametrize("n,e,S", [(14, 20, 2), (118, 186, 1)])
def test_forty_halves_agree_with_the_ac_verification(n, e, S):
    """With 40 halves the estimate is converged: mismatch < 1e-6 -- no constant of this file is involved --, and the loadings are
    `verify_contingencies(route="sparse")`'s AC loadings within the dense test's two bounds."""
    case = _case(n, e, S)
    plain = _screen(case)
    ratings = 1.2 * _base_currents(case, plain).max(axis=0)
    res = _screen(case, ratings=ratings, halves=40, keep_table=True, keep_state=True)
    isl, _, _, den = _yard(case, plain, "xb", 2)
    ok = np.flatnonzero(isl == 0)
    worst_mis = float(res.mismatch[:, torch.from_numpy(ok)].max())
    print(f"40 halves at ({n}, {e}): largest mismatch {worst_mis:.3g}")
    assert worst_mis < 1e-6
    pairs = [(s, int(k)) for s in range(S) for k in ok]
    ver = verify_contingencies(res, _dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), _dev(ratings), pairs=pairs, tol=TOL, max_iter=10,
                               route="sparse")
    assert ver.pairs.tolist() == [list(p) for p in pairs] and bool((ver.status >= 1).all())
    assert torch.equal(_bits(ver.dc_severity), _bits(res.severity[ver.pairs[:, 0], ver.pairs[:, 1]]))
    load, table, state = ver.loading.cpu().numpy(), ver.table.cpu().numpy(), res.post_state.cpu().numpy()
    cur = res.post_current.cpu().numpy()
    r32 = ratings.astype(np.float32).astype(np.float64)
    worst = 0.0
    for t, (s, k) in enumerate(pairs):
        keep = np.arange(e) != k
        vm0, th0 = _base_of(res, s)
        _, scale = A.currents(state[s, k], case.ei, case.rx[s], k)
        full = table[t]
        d_state = EPS * (np.abs(full[:, 0] - vm0).max() + np.abs(full[:, 1] * P.RAD - th0).max()) / den[s, k]
        bound = (2 * B.C_BOUND * B.EPS * scale + scale * (C_BOUND * d_state + 4 * EPS)) / r32 + 2 * EPS * np.abs(load[t])
        mine = cur[s, k] / ratings.astype(np.float32)
        worst = max(worst, float((np.abs(mine[keep].astype(np.float64) - load[t, keep]) / bound[keep]).max()))
        assert int(ver.worst_line[t]) == int(res.worst_line[s, k]) or abs(float(ver.severity[t]) - float(res.severity[s, k])) <= bound[keep].max()
    print(f"40 halves at ({n}, {e}): worst |loading - verified| / bound {worst:.3g}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------ the dense screen
@pytest.mark.parametrize("n,e,S", [(14, 20, 8), (118, 186, 2)])
@pytest.mark.parametrize("variant", ["xb", "bx"])
def test_against_the_dense_screen(n, e, S, variant):
    """the two routes' kept states agree within the sum of their bounds (each is within its own of the yardstick started at its own
    base state, and the two base states are TOL apart); what the line list alone decides agrees exactly"""
    case = _case(n, e, S)
    bt, spec, ei, rx = _dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx)
    dense = contingency_screen_ac(bt, spec, ei, rx, variant=variant, tol=TOL, max_iter=MAX_ITER, keep_table=True, keep_state=True)
    sparse = _screen(case, variant=variant, keep_table=True, keep_state=True)
    assert torch.equal(dense.islands, sparse.islands) and bool((dense.status >= 0).all()) and bool((sparse.status >= 0).all())
    isl, want, _, den = _yard(case, sparse, variant, 2)
    bridge = torch.from_numpy(isl > 0).to(DEV)
    for k in ("severity", "worst_line", "overloads", "vm_min", "vm_min_bus", "v_violations", "mismatch", "post_current", "post_state"):
        assert torch.equal(_bits(getattr(dense, k)[:, bridge]), _bits(getattr(sparse, k)[:, bridge])), k
    a, b = dense.post_state.cpu().numpy().astype(np.float64), sparse.post_state.cpu().numpy().astype(np.float64)
    slack = case.bt == 0
    worst = 0.0
    for s in range(S):
        vm0, th0 = _base_of(sparse, s)
        for k in np.flatnonzero(isl == 0):
            for col, base, unit in ((0, vm0, 1.0), (1, th0, P.RAD)):
                f64 = want[s, k, :, col]
                u = EPS * np.abs(f64 - base).max() / den[s, k]
                bound = (C_BOUND + DENSE_C_BOUND) * u + 4 * EPS * np.abs(f64) + 1e-8      # (two fp32 tables; two base states, each within TOL-sized steps)
                worst = max(worst, float((np.abs(a[s, k, :, col] - b[s, k, :, col])[~slack] * unit / bound[~slack]).max()))
    print(f"({n}, {e}) {variant}: worst |dense - sparse| / (the two bounds) {worst:.3g}")
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------- failures
def _raw(case, n_pv, n_pq, S, bt=None):
    return K._raw(case, n_pv, n_pq, S, plan=_plan(case), bt=bt)


def test_failures_stay_local():
    n, e = 14, 20
    case = _case(n, e, 6)
    clean = _screen(case, keep_table=True, keep_state=True)
    spec, rx = case.spec.copy(), case.rx.copy()
    spec[1, 5, 2] = np.nan                                                  # scenario 1: a NaN in P
    assert 0 not in case.ei[:, 10] and case.bt[0] == 0
    rx[4, 10, 1] = 0.0                                                      # scenario 4: x = 0 on a line between two angle buses
    res = _screen(case, spec=spec, rx=rx, keep_table=True, keep_state=True)
    direct = solve_power_flow(_dev(case.bt), _dev(spec), _dev(case.ei), _dev(rx), mode="fdxb", tol=TOL, max_iter=MAX_ITER, route="sparse",
                              plan=_plan(case))
    status = res.status.tolist()
    # the base is the solver's kernel and carries its statuses: a NaN in P is -3, x = 0 whatever the sparse solver reports for it
    assert torch.equal(res.status, direct.status) and status[1] == -3 and status[4] < 0 and int(res.flags.item()) == 0
    assert _all_failed(res, 1) and _all_failed(res, 4)                      # float outputs NaN, integer outputs -1: bridges too
    keep = [0, 2, 3, 5]
    assert _same(res, clean, rows_a=keep, rows_b=keep) and bool((clean.status >= 0).all())
    # one half-iteration is not enough for the base solve: -1, and all of the scenarios' outputs say so
    res = _screen(case, max_iter=1, keep_table=True, keep_state=True)
    assert res.status.tolist() == [-1] * 6 and all(_all_failed(res, s) for s in range(6)) and bool(torch.isfinite(res.residual).all())
    # a plan built for another line list: -6 everywhere
    other = case.ei.copy()
    other[:, [2, 9]] = other[:, [9, 2]]
    assert not np.array_equal(other, case.ei)
    stale = sparse_plan(_dev(case.bt), _dev(other), mode="fd")
    res = _screen(case, plan=stale, keep_table=True, keep_state=True)
    assert res.status.tolist() == [-6] * 6 and all(_all_failed(res, s) for s in range(6))
    # counts that contradict bus_type: -5 and the flag, nothing beyond the scenarios' rows is written
    n_pv, n_pq = int((case.bt == 1).sum()), int((case.bt == 2).sum())
    raw = _raw(case, n_pv + 1, n_pq - 1, 6)
    assert raw.rc == 0 and int(raw.flags.item()) & 1 and raw.status[:6].tolist() == [-5] * 6
    for t in (raw.severity, raw.vm_min, raw.mismatch, raw.table, raw.residual):
        assert torch.isnan(t[:6]).all() and bool((t[6] == raw.guard).all())
    for t in (raw.worst_line, raw.overloads, raw.vm_min_bus, raw.v_violations):
        assert bool((t[:6] == -1).all()) and bool((t[6] == 77).all())
    assert int(raw.status[6]) == 77
    # bus types on the device that are not the plan's (a PV bus turned PQ under the plan's counts): the solver's own -5
    bt = case.bt.copy()
    bt[int(np.flatnonzero(bt == 1)[0])] = 2
    raw = _raw(case, n_pv, n_pq, 6, bt=bt)
    assert raw.rc == 0 and int(raw.flags.item()) & 1 and raw.status[:6].tolist() == [-5] * 6 and torch.isnan(raw.severity[:6]).all()
    good = _raw(case, n_pv, n_pq, 6)                                        # (the same call with the right counts runs)
    assert good.rc == 0 and int(good.flags.item()) == 0 and bool((good.status[:6] >= 0).all())
    assert bool((good.severity[6] == good.guard).all()) and int(good.status[6]) == 77


# ----------------------------------------------------------------------------------------------------------- capture
def test_the_screen_is_capturable():
    case = _case(14, 20, 8)
    bt, spec, ei, rx = _dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx)
    kw = dict(tol=TOL, max_iter=MAX_ITER, keep_table=True, keep_state=True, route="sparse", plan=_plan(case))
    eager = contingency_screen_ac(bt, spec, ei, rx, **kw)                   # (also: the one host read)
    torch.cuda.synchronize()
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            res = contingency_screen_ac(bt, spec, ei, rx, **kw)
    for _ in range(2):
        for t in (res.severity, res.vm_min, res.mismatch, res.base_table, res.residual, res.post_current, res.post_state):
            t.fill_(-7.0)
        for t in (res.worst_line, res.overloads, res.vm_min_bus, res.v_violations, res.status, res.islands):
            t.fill_(99)
        g.replay()
        torch.cuda.synchronize()
        assert _same(res, eager) and bool((res.status >= 0).all())


# ------------------------------------------------------------------------------------------------------------ script
def test_the_script_runs_end_to_end_on_the_sparse_route(tmp_path, monkeypatch):
    import contingency
    monkeypatch.chdir(tmp_path)
    text = _run(contingency.main, ["--case", "14", "--samples", "8", "--verify-top", "2", "--ac", "--route", "sparse"])
    assert "AC screen: 2 half-iterations" in text and "1P1Q" in text and "worst line equals AC's" in text and "lowest Vm" in text
    assert "sparse" in text
    shapes = {"severity": np.float32, "worst_line": np.int32, "overloads": np.int32, "vm_min": np.float32, "vm_min_bus": np.int32,
              "v_violations": np.int32, "mismatch": np.float64}
    for name, dtype in shapes.items():
        a = np.load(tmp_path / "results" / f"case14_contingency_ac_{name}.npy")
        assert a.shape == (8, 20) and a.dtype == dtype, name
    sev, dc = np.load(tmp_path / "results" / "case14_contingency_ac_severity.npy"), np.load(tmp_path / "results" / "case14_contingency_severity.npy")
    assert np.array_equal(np.isinf(sev), np.isinf(dc)) and np.isfinite(sev[~np.isinf(sev)]).all()
