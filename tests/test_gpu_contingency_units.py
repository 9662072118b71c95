"""The generator-outage screen on the device: `pfn_contingency_units` (csrc/contingency_units.hip) through `contingency_screen_units`,
and `verify_unit_contingencies`, held to the float64 yardstick of tests/contingency_units_ref.py, which LITERALLY edits `spec` (and
deletes line k) and solves the DC model again.  Inputs are `make_physical_inputs(n, e, S, seed=1)`; the units are the PV buses, the
last PQ bus, the slack and the first PV bus once more, with graded participation unless a test says otherwise; the bounds, the
measured ratios and C_BOUND are in tests/contingency_units_checks.py.

Measured on an MI355X: see WORST in tests/contingency_units_checks.py and DESIGN.md section 7zc."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.loss import branch_flows  # noqa: F401  (the import fails loudly where the library is missing)
from poweflownet_amd.utils.contingency import contingency_screen, contingency_screen_units, verify_unit_contingencies
from poweflownet_amd.utils.powerflow import solve_power_flow
from tests import branch_ref as B
from tests import contingency_ref as R
from tests import contingency_units_ref as U
from tests import powerflow_ref as P
from tests.contingency_units_checks import (LINE_FIELDS, MAX_ITER, bits, check_flows, recompute, same, screen, yard)
from tests.powerflow_checks import DEV, TOL, _dev, _distance, _residual_ratio, _run
from tests.test_gpu_powerflow import _case

pytestmark = pytest.mark.gpu


# -------------------------------------------------------------------------------------------------------- flows
@pytest.mark.parametrize("n,e,S", [(5, 6, 3), (14, 20, 8), (70, 100, 2), (118, 186, 2)])
def test_flows_against_editing_spec_and_solving_again(n, e, S):
    case, y = _case(n, e, S), yard(n, e, S)
    res = screen(case, y, keep_table=True)
    assert res.route == "lds"
    check_flows(case, y, res, f"n {n} e {e} S {S}")
    recompute(res, None, S, y.isl)
    bare = screen(case, y)                                                  # without the tables: the same bits, no table
    assert bare.post_flow is None and bare.line_post_flow is None and same(bare, res, table=False)
    alone = screen(case, y, lines=None, keep_table=True)                    # without lines: the same unit figures, nothing of the lines
    assert alone.lines is None and alone.islands is None and alone.line_severity is None and same(alone, res, lines=False)
    every = screen(case, y, lines="all")                                    # "all" is every line
    assert same(every, res, table=False)
    line = screen(case, y, lines=[int(y.lines[-1])], keep_table=True)       # a candidate list of one line
    assert same(line, res, lines=False)
    for k in LINE_FIELDS + ("line_post_flow",):
        assert torch.equal(bits(getattr(line, k)[:, :, 0]), bits(getattr(res, k)[:, :, -1])), k
    # base_flow and status are contingency_screen's bits
    n1 = contingency_screen(_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), tol=TOL, max_iter=MAX_ITER)
    assert torch.equal(bits(n1.base_flow), bits(res.base_flow)) and torch.equal(n1.status, res.status)


def test_slack_pickup_and_the_defaults():
    n, e, S = 14, 20, 8
    case = _case(n, e, S)
    for name in ("slack pickup", "participation on one unit only", "zero participation"):
        y = yard(n, e, S, name)
        res = screen(case, y, keep_table=True)
        check_flows(case, y, res, f"n {n}: {name}")
    y = yard(n, e, S, "slack pickup")
    res = screen(case, y, keep_table=True)
    zero = screen(case, yard(n, e, S, "zero participation"), keep_table=True)
    one = screen(case, yard(n, e, S, "participation on one unit only"), keep_table=True)
    assert same(zero, res)                                                  # a = 0 everywhere IS the slack's pickup
    assert torch.equal(bits(one.post_flow[:, 0]), bits(res.post_flow[:, 0])) and not torch.equal(one.post_flow[:, 2], res.post_flow[:, 2])
    slack = int(np.flatnonzero(case.bt == 0)[0])
    g_slack = int(np.flatnonzero(y.units == slack)[0])
    base32 = res.base_flow.float()
    assert torch.equal(res.post_flow[:, g_slack], base32)                   # a unit at the slack under slack pickup: exactly the base flows
    assert torch.equal(res.post_flow[:, 1], base32) and y.p[1] == 0         # p = 0: the base flows
    assert y.units[0] == y.units[-1] and not torch.equal(res.post_flow[:, 0], res.post_flow[:, -1])      # duplicate buses: ordinary items
    # [S, G] inputs are [G] inputs repeated: the same bits
    wide = screen(case, y, p=np.broadcast_to(y.p, (S, len(y.p))).copy(), a=np.zeros((S, len(y.p))), keep_table=True)
    assert same(wide, res)
    # units=None: the PV buses, ascending; unit_p=None: max(-P, 0) of the scenario
    args = (_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx))
    auto = contingency_screen_units(*args, tol=TOL, max_iter=MAX_ITER, keep_table=True)
    pv = np.flatnonzero(case.bt == 1)
    want_p = np.stack([U.default_unit_p(case.spec[s], pv) for s in range(S)])
    assert auto.units.tolist() == pv.tolist() and np.array_equal(auto.unit_p.cpu().numpy(), want_p) and (want_p > 0).any()
    named = contingency_screen_units(*args, units=pv.tolist(), unit_p=_dev(want_p), tol=TOL, max_iter=MAX_ITER, keep_table=True)
    assert same(auto, named, lines=False)


# --------------------------------------------------------------------------------------------------- reductions
def test_figures_are_exact_functions_of_the_tables_and_the_ratings():
    n, e, S = 14, 20, 8
    case, y = _case(n, e, S), yard(n, e, S)
    per_line = 1.05 * np.abs(y.f).max(axis=0)                               # some outages overload some lines
    per_line[[2, 9, 11]] = [0.0, -1.0, np.nan]                              # unmonitored: zero, negative, NaN
    res = screen(case, y, ratings=per_line, keep_table=True)
    check_flows(case, y, res, "ratings [e]", ratings=np.where(per_line > 0, per_line, 0.0))
    recompute(res, per_line, S, y.isl)
    over = res.line_overloads.cpu().numpy()[:, :, y.isl == 0]
    assert (over > 0).any() and ((over == 0).any() or bool((res.overloads == 0).any()))
    assert not np.isin(res.worst_line.cpu().numpy(), [2, 9, 11]).any() and not np.isin(res.line_worst_line.cpu().numpy(), [2, 9, 11]).any()
    rng = np.random.default_rng(0)
    per_sample = np.abs(y.f) * rng.uniform(0.5, 2.0, y.f.shape)
    per_sample[rng.random(y.f.shape) < 0.2] = 0.0
    per_sample[3, 4] = 1e-60                                               # not > 0 once it is fp32: unmonitored
    per_sample[5, 6] = 1e-42                                               # an fp32 denormal: its loading overflows -> NaN severity
    res2 = screen(case, y, ratings=per_sample, keep_table=True)
    assert torch.equal(bits(res2.post_flow), bits(res.post_flow)) and torch.equal(bits(res2.line_post_flow), bits(res.line_post_flow))
    recompute(res2, per_sample, S, y.isl)
    assert torch.isnan(res2.severity[5]).all() and bool((res2.worst_line[5] == 6).all()) and not torch.isnan(res2.severity[[0, 1, 2, 3, 4, 6, 7]]).any()
    none = screen(case, y, ratings=np.zeros(e), keep_table=True)           # nothing monitored: 0, -1, 0 (bridges keep their marks)
    recompute(none, np.zeros(e), S, y.isl)
    ok = torch.from_numpy(y.isl == 0).to(DEV)
    assert bool((none.worst_line == -1).all()) and bool((none.severity == 0).all()) and bool((none.overloads == 0).all())
    assert bool((none.line_worst_line == -1).all()) and bool((none.line_severity[:, :, ok] == 0).all()) and bool((none.line_overloads[:, :, ok] == 0).all())


# ------------------------------------------------------------------------------------------- routes, thresholds
def _lds_fit():
    lib = L.load()
    return max(n for n in range(100, 220) if lib.pfn_contingency_units_workspace_bytes(1, n, n + n // 2, n // 3, 0) == 0)


def _threshold_case(n):
    """a case of n buses and 1.5 n lines with n / 3 units -- the PV buses first, then the lowest PQ buses -- graded participation and
    every ninth line behind them"""
    case = _case(n, n + n // 2, 1)
    G = n // 3
    units = np.concatenate([np.flatnonzero(case.bt == 1), np.flatnonzero(case.bt == 2)])[:G]
    return case, types.SimpleNamespace(units=units, p=0.05 + 0.01 * np.arange(G), a=1.0 + (np.arange(G) % 7), lines=np.arange(0, case.e, 9))


def _yard_of(case, y):
    """the yardstick of a hand-made unit list (one scenario)"""
    y.isl = R.islands(case.bt, case.ei)
    y.f = R.base_flow(case.bt, case.spec[0], case.ei, case.rx[0])[None]
    y.inv = np.array([P.dc_solve(case.bt, case.spec[0], case.ei, case.rx[0])[1]])
    y.post = U.resolve_units(case.bt, case.spec[0], case.ei, case.rx[0], y.units, y.p, y.a)[None]
    closed, d = U.closed_form(case.bt, case.spec[0], case.ei, case.rx[0], y.units, y.p, y.a)
    y.d = d[None]
    y.post2 = U.closed_form_lines(case.bt, case.ei, case.rx[0], y.post[0], y.lines)[0][None]
    y.den = U.closed_form_lines(case.bt, case.ei, case.rx[0], closed, y.lines)[1][None]
    ok = y.isl[y.lines] == 0
    assert ok.any() and np.abs(y.den[:, ok]).min() >= 0.05
    y.post2[:, :, ~ok] = np.nan
    # (the distribution factors over the LITERAL post-unit flows stand for deleting the line here: a third of n units times a ninth
    # of the lines are thousands of solves; tests/test_contingency_units_host.py and the four flow shapes hold the two together)
    j = int(np.flatnonzero(ok)[0])
    few = (y.units[:3], y.p[:3], y.a[:3])                                   # three units sharing by their graded factors
    literal = U.resolve_unit_lines(case.bt, case.spec[0], case.ei, case.rx[0], *few, [int(y.lines[j])], y.isl)
    factors = U.closed_form_lines(case.bt, case.ei, case.rx[0], U.resolve_units(case.bt, case.spec[0], case.ei, case.rx[0], *few), [int(y.lines[j])])[0]
    assert len(set(y.a[:3])) == 3 and np.abs(literal - factors).max() <= 1e-9 * max(1.0, np.abs(y.f).max()) / abs(y.den[0, j])
    return y


@pytest.mark.parametrize("which", ["m = PF_BIG_M", "m = PF_BIG_M + 1", "largest in LDS", "one more", "global"])
def test_both_sides_of_the_dispatch_thresholds(which):
    fit = _lds_fit()
    assert 150 < fit < 187
    n = {"m = PF_BIG_M": 91, "m = PF_BIG_M + 1": 92, "largest in LDS": fit, "one more": fit + 1, "global": 200}[which]
    case, y = _threshold_case(n)
    y = _yard_of(case, y)
    res = screen(case, y, keep_table=True)
    assert res.route == ("global" if which in ("one more", "global") else "lds")
    check_flows(case, y, res, f"{which}: n {n} e {case.e} G {len(y.units)}")
    recompute(res, None, 1, y.isl)
    if res.route == "global":
        with pytest.raises(RuntimeError, match=r"code -1.*LDS"):
            screen(case, y, route="lds")


def test_the_global_route_gives_the_lds_routes_bits():
    case, y = _case(14, 20, 8), yard(14, 20, 8)
    glob, lds = screen(case, y, keep_table=True, route="global"), screen(case, y, keep_table=True, route="lds")
    assert (glob.route, lds.route) == ("global", "lds") and same(glob, lds)


# ---------------------------------------------------------------------------------------------------- independence
def test_a_scenario_does_not_depend_on_its_batch():
    case, y = _case(14, 20, 8), yard(14, 20, 8)
    ratings = 1.05 * np.abs(y.f)                                            # [S, e]
    G = len(y.units)
    p = y.p[None, :] * (1.0 + 0.1 * np.arange(8))[:, None]                  # [S, G] inputs, every scenario its own
    a = y.a[None, :] + np.arange(8)[:, None]
    whole = screen(case, y, ratings=ratings, p=p, a=a, keep_table=True)
    assert bool((whole.status >= 0).all()) and p.shape == (8, G)
    first = screen(case, y, slice(0, 4), ratings[:4], p=p[:4], a=a[:4], keep_table=True)
    second = screen(case, y, slice(4, 8), ratings[4:], p=p[4:], a=a[4:], keep_table=True)
    assert same(first, whole, rows_b=slice(0, 4)) and same(second, whole, rows_b=slice(4, 8))
    one = screen(case, y, slice(5, 6), ratings[5:6], p=p[5:6], a=a[5:6], keep_table=True)
    assert same(one, whole, rows_b=slice(5, 6))
    big, yb = _case(118, 186, 2), yard(118, 186, 2)                         # ... nor on the workgroup's other waves: 1024 threads
    both, last = screen(big, yb), screen(big, yb, slice(1, 2))
    assert same(last, both, rows_b=slice(1, 2), table=False)


# -------------------------------------------------------------------------------------------------------- failures
def test_failures_stay_local():
    n, e, S = 14, 20, 8
    case, y = _case(n, e, S), yard(n, e, S)
    G = len(y.units)
    clean = screen(case, y, keep_table=True)
    spec, rx = case.spec.copy(), case.rx.copy()
    p, a = np.broadcast_to(y.p, (S, G)).copy(), np.broadcast_to(y.a, (S, G)).copy()
    spec[1, 5, 2] = np.nan                                                  # scenario 1: a NaN in P
    rx[4, 8, 1] = 0.0                                                       # scenario 4: x = 0 on a line
    p[2, 3] = np.nan                                                        # scenario 2: a NaN unit_p
    a[6, 0] = -1.0                                                          # scenario 6: a negative participation factor
    a[7, G - 1] = np.inf                                                    # scenario 7: an infinite one
    res = screen(case, y, spec=spec, rx=rx, p=p, a=a, keep_table=True)
    assert res.status.tolist()[1:3] == [-3, -3] and [res.status.tolist()[s] for s in (4, 6, 7)] == [-3, -3, -3] and int(res.flags.item()) == 0
    for s in (1, 2, 4, 6, 7):                                               # float outputs NaN, integer outputs -1: bridges too
        for k in ("severity", "base_flow", "post_flow", "line_severity", "line_post_flow"):
            assert torch.isnan(getattr(res, k)[s]).all(), (s, k)
        for k in ("worst_line", "overloads", "line_worst_line", "line_overloads"):
            assert bool((getattr(res, k)[s] == -1).all()), (s, k)
    keep = [0, 3, 5]
    assert same(res, clean, rows_a=keep, rows_b=keep) and bool((clean.status >= 0).all())
    p_inf = p.copy()
    p_inf[:] = y.p
    p_inf[0, 0] = -np.inf                                                   # an infinite unit_p, whatever its sign
    res = screen(case, y, p=p_inf, keep_table=True)
    assert res.status.tolist()[0] == -3 and same(res, clean, rows_a=slice(1, 8), rows_b=slice(1, 8))
    # a line to bus id n: -4 everywhere, the candidates' islands included
    far = case.ei.copy()
    far[1, 7] = n
    res = screen(case, y, ei=far)
    assert res.status.tolist() == [-4] * S and res.islands.tolist() == [-4] * e and torch.isnan(res.severity).all() and bool((res.line_worst_line == -1).all())


def _raw(case, y, units, n_pv, n_pq, S, lines=True):
    """the C entry itself, with guard rows behind every output"""
    e, n, G, c = case.e, case.n, len(units), len(y.lines) if lines else 0
    bt, spec, ei, rx = _dev(case.bt.astype(np.int32)), _dev(case.spec), _dev(case.ei), _dev(case.rx)
    isl = torch.zeros(e, dtype=torch.int32, device=DEV)
    un, p, ln = _dev(np.asarray(units, dtype=np.int32)), _dev(y.p[:G].copy()), _dev(y.lines.astype(np.int32))
    guard = -7.5
    full = lambda v, dtype, *shape: torch.full(shape, v, dtype=dtype, device=DEV)     # noqa: E731
    out = types.SimpleNamespace(severity=full(guard, torch.float32, S + 1, G), worst_line=full(77, torch.int32, S + 1, G),
                                overloads=full(77, torch.int32, S + 1, G), base_flow=full(guard, torch.float64, S + 1, e),
                                status=full(99, torch.int32, S + 1), line_severity=full(guard, torch.float32, S + 1, G, max(c, 1)),
                                line_worst_line=full(77, torch.int32, S + 1, G, max(c, 1)), line_overloads=full(77, torch.int32, S + 1, G, max(c, 1)),
                                flags=torch.zeros(1, dtype=torch.int32, device=DEV), guard=guard)
    out.rc = L.load().pfn_contingency_units(ei.data_ptr(), e, rx.data_ptr(), bt.data_ptr(), spec.data_ptr(), None, 0, un.data_ptr(), G, p.data_ptr(), 0,
                                            None, 0, ln.data_ptr() if c else None, c, isl.data_ptr() if c else None, S, n, n_pv, n_pq, C.c_double(TOL),
                                            MAX_ITER, 0, out.severity.data_ptr(), out.worst_line.data_ptr(), out.overloads.data_ptr(),
                                            out.base_flow.data_ptr(), out.status.data_ptr(), None, out.line_severity.data_ptr() if c else None,
                                            out.line_worst_line.data_ptr() if c else None, out.line_overloads.data_ptr() if c else None, None,
                                            out.flags.data_ptr(), None, 0, L.stream_ptr())
    torch.cuda.synchronize()
    return out


def test_bad_unit_ids_and_wrong_counts_through_the_c_entry():
    n, e, S = 14, 20, 6
    case, y = _case(n, e, S), yard(n, e, 8)
    n_pv, n_pq = int((case.bt == 1).sum()), int((case.bt == 2).sum())
    G = len(y.units)

    def all_failed(raw, code):
        assert raw.rc == 0 and raw.status[:S].tolist() == [code] * S and int(raw.status[S]) == 99
        assert torch.isnan(raw.severity[:S]).all() and torch.isnan(raw.base_flow[:S]).all() and torch.isnan(raw.line_severity[:S]).all()
        assert bool((raw.worst_line[:S] == -1).all()) and bool((raw.overloads[:S] == -1).all()) and bool((raw.line_worst_line[:S] == -1).all())
        assert bool((raw.line_overloads[:S] == -1).all())
        assert bool((raw.severity[S] == raw.guard).all()) and bool((raw.base_flow[S] == raw.guard).all()) and bool((raw.line_severity[S] == raw.guard).all())
        assert bool((raw.worst_line[S] == 77).all()) and bool((raw.line_overloads[S] == 77).all())
    for bad in (n, -1, 2 ** 31 - 1):                                        # a unit id outside [0, n): -4 everywhere, nothing followed
        units = y.units.copy()
        units[2] = bad
        raw = _raw(case, y, units, n_pv, n_pq, S)
        all_failed(raw, -4)
        assert int(raw.flags.item()) == 0
    raw = _raw(case, y, y.units, n_pv + 1, n_pq - 1, S)                     # counts that contradict bus_type: -5 and the flag
    all_failed(raw, -5)
    assert int(raw.flags.item()) & 1
    good = _raw(case, y, y.units, n_pv, n_pq, S)                            # (the same call with good ids and counts runs)
    assert good.rc == 0 and int(good.flags.item()) == 0 and bool((good.status[:S] >= 0).all()) and bool((good.worst_line[:S] >= 0).all())
    assert bool((good.severity[S] == good.guard).all()) and good.severity.shape == (S + 1, G)
    alone = _raw(case, y, y.units, n_pv, n_pq, S, lines=False)              # without candidates every line pointer may be null
    assert alone.rc == 0 and torch.equal(bits(alone.severity), bits(good.severity)) and bool((alone.line_severity == alone.guard).all())


# ------------------------------------------------------------------------------------------------------------ ties
def test_ties_go_to_the_lowest_line():
    """tests/test_gpu_contingency_ties.py's grid: 75 parallel copies of one line carry the same flow bit for bit, five of them -- in
    different lanes and trips of a wave's stride over the lines -- with one small rating, taken out of monitoring one by one"""
    from tests.test_gpu_contingency_ties import RATED, SPOTS, E, S, _grid
    g = _grid()
    bt, spec, ei, rx = g.dev
    units = [int(b) for b in np.flatnonzero(g.bt == 1)[::6]]
    G = len(units)
    p = _dev(0.05 + 0.01 * np.arange(G))
    a = _dev(1.0 + np.arange(G, dtype=np.float64))
    assert all(g.checked[k] for k in g.lines) and G >= 3                   # no candidate is a copy or a bridge
    first = None
    for step, spot in enumerate(SPOTS):
        res = contingency_screen_units(bt, spec, ei, rx, g.ratings(step), units=units, unit_p=p, participation=a, lines=g.lines, tol=TOL,
                                       max_iter=MAX_ITER, keep_table=True)
        assert bool((res.status >= 0).all()) and bool((res.islands == 0).all())
        r = g.ratings(step).float()
        for post, worst, sev, over in ((res.post_flow, res.worst_line, res.severity, res.overloads),
                                       (res.line_post_flow, res.line_worst_line, res.line_severity, res.line_overloads)):
            copies = post[..., torch.from_numpy(np.flatnonzero(g.copy)).to(DEV)]
            assert torch.equal(bits(copies), bits(copies[..., :1].expand_as(copies)))           # the copies carry one flow, bit for bit
            load = torch.where(r > 0, post.abs() / r, torch.full_like(post, -1.0))
            assert torch.equal(load.max(dim=-1).values, load[..., spot]) and bool((load[..., spot] > 0).all())      # ... and the rated ones the largest loading
            assert bool((worst == spot).all()), (step, spot)
            assert torch.equal(over, (load > 1).sum(dim=-1).to(torch.int32))
            assert torch.equal(sev, load[..., spot])
        if first is None:
            first = res
        assert torch.equal(bits(res.severity), bits(first.severity)) and torch.equal(bits(res.line_severity), bits(first.line_severity))
    assert E == int(ei.shape[1]) and S == int(spec.shape[0]) and RATED < 1


# ---------------------------------------------------------------------------------------------------------- verify
@pytest.mark.parametrize("n,e", [(5, 6), (14, 20)])
def test_verify_solves_the_shifted_grids_with_the_ac_solver(n, e):
    S = 2
    case, y = _case(n, e, S), yard(n, e, S)
    ratings = 1.2 * np.abs(y.f).max(axis=0)
    ok = np.flatnonzero(y.isl == 0)
    lines = sorted({0, e - 1, int(ok[0]), int(ok[-1]), int(ok[len(ok) // 2])})          # the first and the last line among them, bridge or not
    res = screen(case, y, ratings=ratings, lines=lines)
    args = (_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), _dev(ratings))
    ver = verify_unit_contingencies(res, *args, top=2, tol=TOL, max_iter=MAX_ITER)
    rank = res.ranking(2)[0].cpu().tolist()
    pairs = res.line_ranking(len(y.units) * len(lines))[0].cpu().tolist()
    want = [(s, g, -1) for s in range(S) for g in rank[s]] + [(s, g, k) for s in range(S) for g, k in [gk for gk in pairs[s] if y.isl[gk[1]] == 0][:2]]
    assert [tuple(r) for r in ver.items.tolist()] == want and len(want) == 8
    _check_verified(case, y, res, ver, ratings, lines)
    G = len(y.units)
    items = [(0, 0), (1, G - 1, lines[0]), (0, 1, lines[-1]), (1, 2, int(ok[0])), (0, G - 2)]      # k = 0 and k = e - 1: original numbering
    chosen = verify_unit_contingencies(res, *args, items=items, tol=TOL, max_iter=MAX_ITER)
    kept = [it if len(it) == 3 else it + (-1,) for it in items if len(it) == 2 or y.isl[it[2]] == 0]
    assert sorted(tuple(r) for r in chosen.items.tolist()) == sorted(kept) and len(kept) >= 3
    _check_verified(case, y, res, chosen, ratings, lines)
    with pytest.raises(ValueError, match="no \\(scenario, unit"):
        verify_unit_contingencies(res, *args, items=[(0, 0, [k for k in range(e) if k not in lines][0])])


def _check_verified(case, y, res, ver, ratings, lines):
    n, e = case.n, case.e
    status, table, loading = ver.status.tolist(), ver.table.cpu().numpy(), ver.loading.cpu().numpy()
    assert loading.dtype == np.float32 and loading.shape == (len(status), e)
    worst_f = worst_x = worst_i = 0.0
    for t, (s, g, k) in enumerate(ver.items.tolist()):
        keep = np.arange(e) != k                                            # (k = -1: every line stays)
        ei, rx = np.ascontiguousarray(case.ei[:, keep]), np.ascontiguousarray(case.rx[s][keep])
        spec = U.shifted_spec(case.spec[s], y.units, y.p, y.a, g)
        # the table is solve_power_flow's on inputs built in numpy, bit for bit; Newton converged
        direct = solve_power_flow(_dev(case.bt), _dev(spec[None]), _dev(ei), _dev(rx[None]), tol=TOL, max_iter=MAX_ITER)
        assert 1 <= status[t] <= MAX_ITER and int(direct.status[0]) == status[t] and torch.equal(direct.table[0], ver.table[t]), (t, s, g, k)
        want, st, _ = P.newton(case.bt, spec, ei, rx, tol=TOL, max_iter=MAX_ITER)
        assert 1 <= st <= MAX_ITER
        reduced = types.SimpleNamespace(ei=ei, rx=rx[None], bt=case.bt, spec=spec[None])
        worst_f = max(worst_f, _residual_ratio(reduced, table[t:t + 1]))
        worst_x = max(worst_x, float(_distance(table[t], want) / (2 * TOL * P.jacobian_inverse_norm(want, case.bt, ei, rx))))
        # the loadings: branch_flows' bound on the current, divided by the fp32 rating (one more rounding), in ORIGINAL numbering
        flows, scales = B.flows(table[t:t + 1].astype(np.float32), ei, rx.astype(np.float32).astype(np.float64))
        r32 = ratings.astype(np.float32).astype(np.float64)
        ref = np.full(e, np.nan)
        ref[keep] = flows[0, :, 0] / r32[keep]
        bound = (B.C_BOUND * B.EPS * scales[0, :, 0]) / r32[keep] + B.EPS * np.abs(ref[keep])
        assert (k < 0 or np.isnan(loading[t, k])) and np.isfinite(loading[t, keep]).all()
        worst_i = max(worst_i, float((np.abs(loading[t, keep] - ref[keep]) / bound).max()))
        # severity, worst line and count by the screen's rules from the loadings themselves; the worst line in original numbering
        row = np.where(np.isnan(loading[t]), 0.0, loading[t])
        if k < 0:
            sev, worst, over = (v[0] for v in U.summarise_units(row[None], None, dtype=np.float32))
        else:
            sev, worst, over = (v[0] for v in U.summarise_unit_lines(row[None], None, np.zeros(e, dtype=np.int32), [k], dtype=np.float32))
        assert float(ver.severity[t]) == float(sev) and int(ver.worst_line[t]) == int(worst) != k and int(ver.overloads[t]) == int(over)
        dc = res.severity[s, g] if k < 0 else res.line_severity[s, g, lines.index(k)]
        assert float(ver.dc_severity[t]) == float(dc)
    print(f"verify n {n}: {len(status)} items, worst |mismatch| / bound {worst_f:.3g}, worst |x - yardstick| / (2 tol ||J^-1||) {worst_x:.3g}, "
          f"worst |loading - f64| / bound {worst_i:.3g}")
    assert worst_f <= 1.0 and worst_x <= 1.0 and worst_i <= 1.0


# --------------------------------------------------------------------------------------------------------- capture
def test_the_screen_is_capturable():
    case, y = _case(14, 20, 8), yard(14, 20, 8)
    ratings = _dev(1.05 * np.abs(y.f).max(axis=0))
    bt, spec, ei, rx = _dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx)
    kw = dict(units=[int(b) for b in y.units], unit_p=_dev(y.p), participation=_dev(y.a), lines=[int(k) for k in y.lines], tol=TOL,
              max_iter=MAX_ITER, keep_table=True)
    eager = contingency_screen_units(bt, spec, ei, rx, ratings, **kw)       # (also: the one host read and the two uploads)
    auto = contingency_screen_units(bt, spec, ei, rx, ratings, tol=TOL, max_iter=MAX_ITER)
    torch.cuda.synchronize()
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            res = contingency_screen_units(bt, spec, ei, rx, ratings, **kw)
            res2 = contingency_screen_units(bt, spec, ei, rx, ratings, tol=TOL, max_iter=MAX_ITER)       # units and unit_p formed on the device
    for _ in range(2):
        for t in (res.severity, res.base_flow, res.post_flow, res.line_severity, res.line_post_flow, res2.severity, res2.base_flow):
            t.fill_(-7.0)
        for t in (res.worst_line, res.overloads, res.status, res.line_worst_line, res.line_overloads, res2.worst_line, res2.status):
            t.fill_(99)
        g.replay()
        torch.cuda.synchronize()
        assert same(res, eager) and bool((res.status >= 0).all()) and same(res2, auto, table=False, lines=False)


# ---------------------------------------------------------------------------------------------------------- script
def test_the_script_runs_end_to_end(tmp_path, monkeypatch):
    import contingency
    monkeypatch.chdir(tmp_path)
    text = _run(contingency.main, ["--case", "14", "--samples", "8", "--verify-top", "2", "--units", "--unit-lines", "3", "--participation", "output"])
    assert "units:" in text and "unit x line:" in text and "the DC unit screen called secure" in text
    units = np.load(tmp_path / "results" / "case14_contingency_units_units.npy")
    lines = np.load(tmp_path / "results" / "case14_contingency_units_lines.npy")
    G, c = len(units), len(lines)
    assert G >= 1 and 3 <= c <= 24 and units.dtype == np.int64
    shapes = {"unit_p": ((8, G), np.float64), "severity": ((8, G), np.float32), "worst_line": ((8, G), np.int32), "overloads": ((8, G), np.int32),
              "islands": ((c,), np.int32), "line_severity": ((8, G, c), np.float32), "line_worst_line": ((8, G, c), np.int32),
              "line_overloads": ((8, G, c), np.int32)}
    for name, (shape, dtype) in shapes.items():
        arr = np.load(tmp_path / "results" / f"case14_contingency_units_{name}.npy")
        assert arr.shape == shape and arr.dtype == dtype, name
    assert np.isfinite(np.load(tmp_path / "results" / "case14_contingency_units_severity.npy")).all()
