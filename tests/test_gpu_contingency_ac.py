"""The AC N-1 screen on the device: `pfn_contingency_ac` (csrc/contingency_ac.hip) through `contingency_screen_ac`, held to the float64
yardstick of tests/contingency_ac_ref.py (tests/test_contingency_ac_host.py pins its compensated form to literally deleting the line).
Inputs are `make_physical_inputs(n, e, S, seed=1)`; every shape's grid has a bridge, and outages with one end and with both ends
outside the PQ set.

  base        `base_table`, `status`, `residual` are `torch.equal` to `solve_power_flow(mode="fd" + variant)`'s: the same code;
  state       the kept state of every non-islanding outage k against the yardstick STARTED AT THE DEVICE'S base state (the base solve's
              own error is `solve_power_flow`'s tests'), theta (radians) and Vm separately:
                  |dev - f64| <= C_BOUND * u_k + the fp32 rounding of the table,   u_k = 2^-24 max_i |state_i - base_i| / min(|den'_k|, |den''_k|)
              -- the update is formed with fp32 inverses, so it is worth a few units of fp32 rounding of the largest change of the
              state, amplified by the outage's 1 / den; den = 1 - c_k a^T X a, the yardstick's (`dens`);
  currents    within `branch_flows`' bound (C = 32) of `branch_ref.flows` evaluated at the DEVICE's kept state: the solver's error and
              the current arithmetic are judged separately;
  figures     severity, worst line, overloads, vm_min, vm_min_bus, v_violations are bit-exact functions of the kernel's own tables
              and the fp32 ratings and limits, recomputed in numpy fp32; the worst line is the yardstick's wherever its top two
              loadings differ by more than twice the bounds;
  the rest    bit-for-bit independence of the batch, of `group` and of the placement; `halves` 0, odd, 40 (against
              `verify_contingencies`); failures that stay local; graph capture; the script.

Worst state ratios (|dev - f64| - rounding) / u measured on an MI355X (each test prints its own; WORST below): 0 at
(3, 3) (the fp32 table's rounding covers it), 5.8 at (5, 6), 5.5 at (14, 20), 14.1 at (70, 100), 32.9 at (118, 186), 56.3 at (152, 228, the
largest with the inverses in LDS under "auto"), 39.4 at (153, 229, the first on the slab), 43.2 at (200, 300); "bx" 6.0, one half 5.5,
three halves 0.99, four halves 0.82 at (14, 20).  They grow with the grid because the fp32 Gauss-Jordan inverses carry cond(B) units
of rounding, not one.  C_BOUND = 256 is the smallest power of two >= 4 x the worst (4 x 56.3 = 225), the margin the DC screen's
C = 64 keeps.  Currents: at most 0.042 of `branch_flows`' bound.  40 halves: mismatch 2.8e-14."""
import numpy as np
import pytest
import torch

from poweflownet_amd.loss import branch_flows
from poweflownet_amd.utils.contingency import contingency_screen_ac, verify_contingencies
from poweflownet_amd.utils.powerflow import solve_power_flow
from tests import branch_ref as B
from tests import contingency_ac_ref as A
from tests import contingency_ac_checks as K
from tests import powerflow_ref as P
from tests.contingency_ac_checks import EPS, MAX_ITER, _all_failed, _base_currents, _base_of, _bits, _same, _yard
from tests.powerflow_checks import DEV, TOL, _dev, _run
from tests.test_gpu_powerflow import _case

pytestmark = pytest.mark.gpu
# (n, e, S): the issue's five, both sides of the largest shape whose inverses sit in LDS (152 buses: four waves beside them; 153: the
# slab), and the slab with 16 waves
SHAPES = [(3, 3, 2), (5, 6, 3), (14, 20, 8), (70, 100, 2), (118, 186, 2), (152, 228, 1), (153, 229, 1), (200, 300, 1)]
PLACED = {3: ("lds", 16), 5: ("lds", 16), 14: ("lds", 16), 70: ("lds", 16), 118: ("lds", 8), 152: ("lds", 4), 153: ("global", 16), 200: ("global", 16)}
# worst (|dev - f64| - rounding) / u measured on an MI355X per (n, e), two halves, "xb": the figures C_BOUND was set from
WORST = {(3, 3): 0.0, (5, 6): 5.8, (14, 20): 5.5, (70, 100): 14.1, (118, 186): 32.9, (152, 228): 56.3, (153, 229): 39.4, (200, 300): 43.2}
C_BOUND = 256.0
assert C_BOUND == 2.0 ** np.ceil(np.log2(4 * max(WORST.values())))


def _screen(case, rows=slice(None), ratings=None, ei=None, spec=None, rx=None, **kw):
    kw = {"tol": TOL, "max_iter": MAX_ITER, **kw}
    return contingency_screen_ac(_dev(case.bt), _dev((case.spec if spec is None else spec)[rows]), _dev(case.ei if ei is None else ei),
                                 _dev((case.rx if rx is None else rx)[rows]), None if ratings is None else _dev(ratings), **kw)


def _check_base(case, res, variant, **kw):
    direct = solve_power_flow(_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), mode="fd" + variant, tol=TOL, max_iter=MAX_ITER, **kw)
    assert torch.equal(_bits(res.base_table), _bits(direct.table)) and torch.equal(res.status, direct.status)
    assert torch.equal(_bits(res.residual), _bits(direct.residual))
    return direct


def _check(case, res, variant, halves, what, ratings=None, **kw):
    """contingency_ac_checks' `_check` under this route's C_BOUND"""
    return K._check(case, res, variant, halves, what, C_BOUND, ratings, **kw)


# -------------------------------------------------------------------------------------------------- the screen itself
@pytest.mark.parametrize("n,e,S", SHAPES)
def test_states_currents_and_figures_against_the_yardstick(n, e, S):
    case = _case(n, e, S)
    plain = _screen(case)                                                   # (no ratings: 1.0 everywhere; also the one host read)
    ratings = 1.2 * _base_currents(case, plain).max(axis=0)                 # [e]
    res = _screen(case, ratings=ratings, keep_table=True, keep_state=True)
    assert (res.route, res.group) == PLACED[n]
    _check_base(case, res, "xb")
    _check(case, res, "xb", 2, f"n {n} e {e} S {S}", ratings)
    for k in ("vm_min", "vm_min_bus", "v_violations", "mismatch", "base_table", "status", "residual"):
        assert torch.equal(_bits(getattr(plain, k)), _bits(getattr(res, k))), k       # (the ratings change the loading figures only)


@pytest.mark.parametrize("variant,halves", [("bx", 2), ("xb", 3), ("bx", 4), ("xb", 1)])
def test_both_variants_and_odd_halves(variant, halves):
    case = _case(14, 20, 8)
    res = _screen(case, variant=variant, halves=halves, keep_table=True, keep_state=True)
    _check_base(case, res, variant)
    _check(case, res, variant, halves, f"variant {variant} halves {halves}")


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
    none = _screen(case, ratings=np.zeros(case.e), keep_table=True, keep_state=True)
    ok = res.islands == 0
    assert bool((none.severity[:, ok] == 0).all()) and bool((none.worst_line[:, ok] == -1).all()) and bool((none.overloads[:, ok] == 0).all())
    assert torch.equal(_bits(none.post_current), _bits(res.post_current)) and torch.equal(_bits(none.post_state), _bits(res.post_state))


# ------------------------------------------------------------------------------------------------------ independence
def test_a_scenario_does_not_depend_on_batch_group_or_placement():
    case = _case(14, 20, 8)
    ratings = 1.2 * _base_currents(case, _screen(case))                     # [S, e]
    whole = _screen(case, ratings=ratings, keep_table=True, keep_state=True)
    assert bool((whole.status >= 0).all()) and (whole.route, whole.group) == ("lds", 16)
    a = _screen(case, slice(0, 4), ratings[:4], keep_table=True, keep_state=True)
    b = _screen(case, slice(4, 8), ratings[4:], keep_table=True, keep_state=True)
    assert _same(a, whole, rows_b=slice(0, 4)) and _same(b, whole, rows_b=slice(4, 8))
    one = _screen(case, slice(5, 6), ratings[5:6], keep_table=True, keep_state=True)
    assert _same(one, whole, rows_b=slice(5, 6))
    for route in ("lds", "global"):
        for group in range(1, 17):
            got = _screen(case, ratings=ratings, keep_table=True, keep_state=True, route=route, group=group)
            assert (got.route, got.group) == (route, group) and _same(got, whole), (route, group)
    big = _case(118, 186, 2)                                                # eight waves in LDS against sixteen on the slab
    both, last = _screen(big), _screen(big, slice(1, 2), route="global")
    assert (both.group, last.group, last.route) == (8, 16, "global") and _same(last, both, rows_b=slice(1, 2), tables=False)


def test_the_lds_placement_is_refused_where_it_does_not_fit():
    """route="lds" takes fewer waves before it gives up: 164 buses are the last whose inverses fit beside ONE wave's vectors"""
    last = _case(164, 246, 1)
    auto, forced = _screen(last, keep_table=True, keep_state=True), _screen(last, keep_table=True, keep_state=True, route="lds")
    assert (auto.route, auto.group, forced.route, forced.group) == ("global", 16, "lds", 1) and _same(auto, forced)
    for n, e in ((165, 247), (200, 300)):
        case = _case(n, e, 1)
        assert _screen(case).route == "global"
        with pytest.raises(RuntimeError, match="do not fit LDS"):
            _screen(case, route="lds")
    with pytest.raises(RuntimeError, match="do not fit LDS"):
        _screen(_case(152, 228, 1), route="lds", group=5)                   # four waves fit beside the inverses, five do not
    assert _screen(_case(152, 228, 1), route="lds", group=2).route == "lds"


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


def test_forty_halves_agree_with_the_ac_verification():
    """With 40 halves the estimate is converged: mismatch < 1e-6, and the loadings are `verify_contingencies`' AC loadings within the
    two bounds -- each side's currents within `branch_flows`' bound of the yardstick at its own fp32 state (C = 32, one more
    rounding for the division by the rating), and the two fp32 states within the state bound of one another, carried to a current by
    the scale of `branch_flows`' bound (an upper bound of a current's sensitivity to a relative change of its two ends)."""
    case = _case(14, 20, 2)
    S, e = 2, 20
    plain = _screen(case)
    ratings = 1.2 * _base_currents(case, plain).max(axis=0)
    res = _screen(case, ratings=ratings, halves=40, keep_table=True, keep_state=True)
    isl, _, _, den = _yard(case, plain, "xb", 2)
    ok = np.flatnonzero(isl == 0)
    assert bool((res.mismatch[:, torch.from_numpy(ok)] < 1e-6).all())
    pairs = [(s, int(k)) for s in range(S) for k in ok]
    ver = verify_contingencies(res, _dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), _dev(ratings), pairs=pairs, tol=TOL, max_iter=10)
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
    print(f"40 halves: largest mismatch {float(res.mismatch[:, torch.from_numpy(ok)].max()):.3g}, worst |loading - verified| / bound {worst:.3g}")
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------- failures
def test_failures_stay_local():
    n, e = 14, 20
    case = _case(n, e, 6)
    clean = _screen(case, keep_table=True, keep_state=True)
    spec, rx = case.spec.copy(), case.rx.copy()
    spec[1, 5, 2] = np.nan                                                  # scenario 1: a NaN in P
    assert 0 not in case.ei[:, 10] and case.bt[0] == 0
    rx[4, 10, 1] = 0.0                                                      # scenario 4: x = 0 on a line between two angle buses
    rx[2, 10] = 0.0                                                         # scenario 2: r = x = 0 on it
    res = _screen(case, spec=spec, rx=rx, keep_table=True, keep_state=True)
    direct = solve_power_flow(_dev(case.bt), _dev(spec), _dev(case.ei), _dev(rx), mode="fdxb", tol=TOL, max_iter=MAX_ITER)
    status = res.status.tolist()
    # The base is the solver's fast-decoupled code and carries its statuses: a NaN in P and a line without impedance are -3.  x = 0
    # alone leaves the AC mismatch finite (g = 1 / r) and reaches the solver through 1 / x in B': a NaN pivot, -2, exactly as
    # solve_power_flow(mode="fdxb") reports it (at a line of the slack bus it is a -1: the infinite diagonal inverts to a zero row).
    # The DC screen's -3 for x = 0 comes from its flow (theta_a - theta_b) / x, which this screen does not form.
    assert torch.equal(res.status, direct.status) and [status[1], status[2], status[4]] == [-3, -3, -2] and int(res.flags.item()) == 0
    assert _all_failed(res, 1) and _all_failed(res, 2) and _all_failed(res, 4)      # float outputs NaN, integer outputs -1: bridges too
    keep = [0, 3, 5]
    assert _same(res, clean, rows_a=keep, rows_b=keep) and bool((clean.status >= 0).all())
    # one half-iteration is not enough for the base solve: -1, and all of the scenarios' outputs say so
    res = _screen(case, max_iter=1, keep_table=True, keep_state=True)
    assert res.status.tolist() == [-1] * 6 and all(_all_failed(res, s) for s in range(6)) and bool(torch.isfinite(res.residual).all())
    # a bus without a line in the base grid: singular, everywhere
    lonely = np.where(case.ei == 13, 1, case.ei)
    res = _screen(case, ei=lonely, keep_table=True, keep_state=True)
    assert res.status.tolist() == [-2] * 6 and bool((res.islands >= 1).all()) and all(_all_failed(res, s) for s in range(6))
    # a line to bus id n: -4 everywhere, islands included
    far = case.ei.copy()
    far[1, 7] = n
    res = _screen(case, ei=far, keep_table=True, keep_state=True)
    assert res.status.tolist() == [-4] * 6 and res.islands.tolist() == [-4] * e and all(_all_failed(res, s) for s in range(6))
    # counts that contradict bus_type: -5 and the flag, nothing beyond the scenarios' rows is written
    n_pv, n_pq = int((case.bt == 1).sum()), int((case.bt == 2).sum())
    raw = K._raw(case, n_pv + 1, n_pq - 1, 6)
    assert raw.rc == 0 and int(raw.flags.item()) & 1 and raw.status[:6].tolist() == [-5] * 6
    for t in (raw.severity, raw.vm_min, raw.mismatch, raw.table, raw.residual):
        assert torch.isnan(t[:6]).all() and bool((t[6] == raw.guard).all())
    for t in (raw.worst_line, raw.overloads, raw.vm_min_bus, raw.v_violations):
        assert bool((t[:6] == -1).all()) and bool((t[6] == 77).all())
    assert int(raw.status[6]) == 77
    good = K._raw(case, n_pv, n_pq, 6)                                     # (the same call with the right counts runs)
    assert good.rc == 0 and int(good.flags.item()) == 0 and bool((good.status[:6] >= 0).all())


# ----------------------------------------------------------------------------------------------------------- capture
def test_the_screen_is_capturable():
    case = _case(14, 20, 8)
    bt, spec, ei, rx = _dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx)
    kw = dict(tol=TOL, max_iter=MAX_ITER, keep_table=True, keep_state=True)
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
def test_the_script_runs_end_to_end(tmp_path, monkeypatch):
    import contingency
    monkeypatch.chdir(tmp_path)
    text = _run(contingency.main, ["--case", "14", "--samples", "8", "--verify-top", "2", "--ac", "--halves", "2"])
    assert "AC screen: 2 half-iterations" in text and "1P1Q" in text and "worst line equals AC's" in text and "lowest Vm" in text
    shapes = {"severity": np.float32, "worst_line": np.int32, "overloads": np.int32, "vm_min": np.float32, "vm_min_bus": np.int32,
              "v_violations": np.int32, "mismatch": np.float64}
    for name, dtype in shapes.items():
        a = np.load(tmp_path / "results" / f"case14_contingency_ac_{name}.npy")
        assert a.shape == (8, 20) and a.dtype == dtype, name
    sev, dc = np.load(tmp_path / "results" / "case14_contingency_ac_severity.npy"), np.load(tmp_path / "results" / "case14_contingency_severity.npy")
    assert np.array_equal(np.isinf(sev), np.isinf(dc)) and np.isfinite(sev[~np.isinf(sev)]).all()
