"""The N-1 line-outage screen on the device: `pfn_contingency_islands` and `pfn_contingency_dc` (csrc/contingency.hip) through
`contingency_screen`, and `verify_contingencies`, held to the float64 yardstick of tests/contingency_ref.py, which LITERALLY removes
line k and solves the DC model again.  Inputs are `make_physical_inputs(n, e, S, seed=1)`; every test asserts on the yardstick that
its grid has a bridge and that no non-bridge outage is near-singular (min |den| >= 0.05), so nothing needs excluding.

  islands     equal to the yardstick's, exactly; -4 everywhere for a bad id;
  base flow   within the DC bound of DESIGN 7h (theta within 2 tol ||B'^-1||_inf of the float64 solve) carried to a line:
              |f - f64| <= 4 tol ||B'^-1||_inf / |x_l| + 64 * 2^-52 |f64|;
  flows       for every non-bridge outage k and every line l:  |dev - f64| <= C_BOUND * u_k,  u_k = 2^-24 max_l |f_l| / |den_k|, den_k the
              yardstick's: the kernel's per-line arithmetic and its fp32 inverse of B' are worth a few units of fp32 rounding of the
              largest flow, amplified by the outage's 1 / den;
  reductions  severity, worst line and overload count are bit-exact functions of the kernel's own table and the fp32 ratings;
  the rest    bridge rows, both sides of every dispatch threshold, bit-for-bit independence of the batch, failures that stay local,
              the AC verification against `solve_power_flow`, `powerflow_ref.newton` and `branch_ref.flows`, graph capture, the script.

Worst flow ratios |dev - f64| / u measured on an MI355X (each test prints its own; WORST below): 0.52 at (3, 3),
3.8 at (5, 6), 3.7 at (14, 20), 7.1 at (70, 100), 10.8 at (118, 186); at the thresholds 4.4 (m = 90), 8.4 (m = 91), 7.0 (m = 186, the
largest in LDS), 13 (m = 187, the first on the global route), 9.7 at (200, 300).  C_BOUND = 64 is the smallest power of two >= 4 x the
worst of them (4 x 13 = 52; 4 x 10.8 = 43 over the five flow shapes alone gives the same), the margin branch_flows' C = 32 keeps
over its measured 1.6-8.  Base flows: at most 2.9e-4 of their bound.  AC verification: mismatch 0.69, distance 3.9e-3, loadings 0.029
of their bounds."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.loss import branch_flows  # noqa: F401  (the import fails loudly where the library is missing)
from poweflownet_amd.utils.contingency import contingency_screen, verify_contingencies
from poweflownet_amd.utils.powerflow import solve_power_flow
from tests import branch_ref as B
from tests import contingency_ref as R
from tests import powerflow_ref as P
from tests.powerflow_checks import DEV, TOL, _dev, _distance, _residual_ratio, _run
from tests.test_gpu_powerflow import _case

pytestmark = pytest.mark.gpu
MAX_ITER = 10
EPS = 2.0 ** -24
# worst |dev - f64| / u measured on an MI355X per shape (n, e): the figures C_BOUND was set from
WORST = {(3, 3): 0.52, (5, 6): 3.8, (14, 20): 3.7, (70, 100): 7.1, (118, 186): 10.8, (91, 136): 4.4, (92, 138): 8.4, (187, 280): 7.0,
         (188, 282): 13.0, (200, 300): 9.7}
C_BOUND = 64.0
assert C_BOUND == 2.0 ** np.ceil(np.log2(4 * max(WORST.values())))


@functools.lru_cache(maxsize=None)
def _yard(n, e, S):
    """(islands [e], literal post-outage flows [S, e, e], den [S, e], base flows [S, e], ||B'^-1||_inf [S]) of the yardstick, once"""
    case = _case(n, e, S)
    isl = R.islands(case.bt, case.ei)
    lit = np.stack([R.resolve(case.bt, case.spec[s], case.ei, case.rx[s], isl) for s in range(S)])
    den = np.stack([R.lodf(case.bt, case.spec[s], case.ei, case.rx[s])[1] for s in range(S)])
    f = np.stack([R.base_flow(case.bt, case.spec[s], case.ei, case.rx[s]) for s in range(S)])
    inv = np.array([P.dc_solve(case.bt, case.spec[s], case.ei, case.rx[s])[1] for s in range(S)])
    assert (isl > 0).any() and (isl == 0).any() and np.abs(den[:, isl == 0]).min() >= 0.05, (n, e)
    return isl, lit, den, f, inv


def _screen(case, rows=slice(None), ratings=None, ei=None, **kw):
    kw = {"tol": TOL, "max_iter": MAX_ITER, **kw}
    return contingency_screen(_dev(case.bt), _dev(case.spec[rows]), _dev(case.ei if ei is None else ei), _dev(case.rx[rows]),
                              None if ratings is None else _dev(ratings), **kw)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b, rows_a=slice(None), rows_b=slice(None), table=True):
    """two results agree bit for bit on the given scenario rows (NaN bits included)"""
    names = ["severity", "worst_line", "overloads", "base_flow", "status"] + (["post_flow"] if table else [])
    return all(torch.equal(_bits(getattr(a, k)[rows_a]), _bits(getattr(b, k)[rows_b])) for k in names) and torch.equal(a.islands, b.islands)


def _check_flows(case, res, what, ratings=None):
    """status, base flows, the flow bound, the bridge rows and the worst line of a result with its table against the yardstick"""
    S, e = case.S, case.e
    isl, lit, den, f, inv = _yard(case.n, case.e, case.S)
    status, base, post = res.status.cpu().numpy(), res.base_flow.cpu().numpy(), res.post_flow.cpu().numpy()
    sev, worst, over = res.severity.cpu().numpy(), res.worst_line.cpu().numpy(), res.overloads.cpu().numpy()
    assert ((status >= 0) & (status <= MAX_ITER)).all() and int(res.flags.item()) == 0, (what, status)
    assert np.array_equal(res.islands.cpu().numpy(), isl)
    assert post.shape == (S, e, e) and post.dtype == np.float32 and sev.dtype == np.float32 and base.dtype == np.float64
    bridge, ok = isl > 0, isl == 0
    worst_base = worst_ratio = 0.0
    for s in range(S):
        bound = 4 * TOL * inv[s] / np.abs(case.rx[s, :, 1]) + 64 * P.EPS64 * np.abs(f[s])
        worst_base = max(worst_base, float((np.abs(base[s] - f[s]) / bound).max()))
        with np.errstate(divide="ignore"):
            u = EPS * np.abs(f[s]).max() / np.abs(den[s])                  # [e], per outage (a bridge's is not used)
        ratio = np.abs(post[s][ok].astype(np.float64) - lit[s][ok]) / u[ok][:, None]
        worst_ratio = max(worst_ratio, float(ratio.max()))
        assert (post[s][np.arange(e), np.arange(e)][ok] == 0).all()
        # an islanding outage: +inf, -1, -1 and a NaN row
        assert np.isnan(post[s][bridge]).all() and (sev[s][bridge] == np.inf).all() and (worst[s][bridge] == -1).all() and (over[s][bridge] == -1).all()
        # the worst line is the yardstick's wherever the yardstick's top two loadings differ by more than 2 C u
        want_sev, want_worst, _ = R.summarise(lit[s], ratings, isl)
        r = np.ones(e) if ratings is None else np.asarray(ratings, dtype=np.float64)
        for k in np.flatnonzero(ok):
            if want_worst[k] >= 0 and R.top_two_gap(lit[s], ratings, k) > 2 * C_BOUND * u[k] / r[want_worst[k]]:
                assert worst[s, k] == want_worst[k], (what, s, k)
            if want_worst[k] >= 0:
                assert abs(sev[s, k] - want_sev[k]) <= C_BOUND * u[k] / r[r > 0].min() + EPS * want_sev[k], (what, s, k)
    print(f"{what}: route {res.route}, solves {status.min()}..{status.max()}, worst |base flow - f64| / bound {worst_base:.3g}, "
          f"worst |post flow - f64| / u {worst_ratio:.3g} (C = {C_BOUND:g})")
    assert worst_base <= 1.0 and worst_ratio <= C_BOUND, (what, worst_base, worst_ratio)
    return worst_ratio


def _recompute(res, ratings, S):
    """severity, worst line and overload count again from the kernel's own table in numpy fp32: bit for bit"""
    isl, post = res.islands.cpu().numpy(), res.post_flow.cpu().numpy()
    for s in range(S):
        r = None if ratings is None else (ratings if ratings.ndim == 1 else ratings[s])
        sev, worst, over = R.summarise(post[s], r, isl, dtype=np.float32)
        got = res.severity[s].cpu().numpy()
        fin = ~np.isnan(sev)
        assert sev.dtype == np.float32 and np.array_equal(np.isnan(got), ~fin), s
        assert np.array_equal(got[fin].view(np.uint32), sev[fin].view(np.uint32)), s
        assert np.array_equal(res.worst_line[s].cpu().numpy(), worst) and np.array_equal(res.overloads[s].cpu().numpy(), over), s
    return isl


# ------------------------------------------------------------------------------------------------------ islands
def _islands(ei, n, root=0):
    ei = _dev(np.ascontiguousarray(ei, dtype=np.int64))
    out = torch.full((ei.shape[1],), 77, dtype=torch.int32, device=DEV)
    L.check(L.load().pfn_contingency_islands(ei.data_ptr(), int(ei.shape[1]), n, root, out.data_ptr(), L.stream_ptr()), "pfn_contingency_islands")
    return out.tolist()


@pytest.mark.parametrize("n,e", [(3, 3), (5, 6), (14, 20), (70, 100), (118, 186), (200, 300)])
def test_islands_equal_the_yardstick(n, e):
    case = _case(n, e, 1)
    want = R.islands(case.bt, case.ei)
    assert (want > 0).sum() == {3: 1, 5: 1, 14: 3, 70: 14, 118: 16, 200: 39}[n]
    assert _islands(case.ei, n) == want.tolist()


def test_islands_of_grids_made_by_hand_and_bad_ids():
    assert _islands([[0, 1, 2, 3, 4], [1, 2, 3, 4, 5]], 6) == [5, 4, 3, 2, 1]             # a path: every line is a bridge
    assert _islands([[0, 1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 0]], 6) == [0] * 6                # a ring: none
    pendant = [[0, 1, 2, 3, 2], [1, 2, 3, 0, 4]]
    assert _islands(pendant, 5) == [0, 0, 0, 0, 1] and _islands(pendant, 5, root=4) == [0, 0, 0, 0, 4]
    assert _islands([[0, 1, 1, 2], [1, 2, 2, 0]], 3) == [0] * 4                            # a doubled line: neither copy is a bridge
    assert _islands([[0, 1, 1], [1, 2, 2]], 3) == [2, 0, 0]
    assert _islands([[0, 1, 70], [1, 2, 3]], 71) == [70, 69, 68]                           # more buses than lines, an id of n - 1, a base grid in pieces
    for bad in (-1, 14):
        ei = _case(14, 20, 1).ei.copy()
        ei[1, 7] = bad
        assert _islands(ei, 14) == [-4] * 20


# -------------------------------------------------------------------------------------------------------- flows
@pytest.mark.parametrize("n,e,S", [(3, 3, 2), (5, 6, 3), (14, 20, 8), (70, 100, 2), (118, 186, 2)])
def test_flows_against_removing_the_line(n, e, S):
    case = _case(n, e, S)
    res = _screen(case, keep_table=True, route="lds" if n == 118 else "auto")
    assert res.route == "lds"
    _check_flows(case, res, f"n {n} e {e} S {S}")
    _recompute(res, None, S)
    bare = _screen(case)                                                    # without the table: the same bits, no table
    assert bare.post_flow is None and _same(bare, res, table=False)


# --------------------------------------------------------------------------------------------------- reductions
def test_reductions_are_exact_functions_of_the_table_and_the_ratings():
    n, e, S = 14, 20, 8
    case = _case(n, e, S)
    isl, lit, den, f, inv = _yard(n, e, S)
    per_line = 1.2 * np.abs(f).max(axis=0)                                  # some outages overload some lines
    per_line[[2, 9, 11]] = [0.0, -1.0, np.nan]                              # unmonitored: zero, negative, NaN
    res = _screen(case, ratings=per_line, keep_table=True)
    _check_flows(case, res, "ratings [e]", ratings=np.where(per_line > 0, per_line, 0.0))
    _recompute(res, per_line, S)
    over = res.overloads.cpu().numpy()[:, isl == 0]
    assert (over > 0).any() and (over == 0).any()
    assert not np.isin(res.worst_line.cpu().numpy(), [2, 9, 11]).any()
    rng = np.random.default_rng(0)
    per_sample = np.abs(f) * rng.uniform(0.5, 2.0, f.shape)
    per_sample[rng.random(f.shape) < 0.2] = 0.0
    per_sample[3, 4] = 1e-60                                               # not > 0 once it is fp32: unmonitored
    per_sample[5, 6] = 1e-42                                               # an fp32 denormal: its loading overflows -> NaN severity
    res2 = _screen(case, ratings=per_sample, keep_table=True)
    assert torch.equal(_bits(res2.post_flow), _bits(res.post_flow)) and torch.equal(res2.base_flow, res.base_flow)
    _recompute(res2, per_sample, S)
    sev5, worst5 = res2.severity[5].cpu().numpy(), res2.worst_line[5].cpu().numpy()
    assert np.isnan(sev5).any() and not np.isnan(sev5[6]) and (worst5[np.isnan(sev5)] == 6).all()
    assert not np.isnan(res2.severity[[0, 1, 2, 3, 4, 6, 7]].cpu().numpy()).any()
    none = _screen(case, ratings=np.zeros(e), keep_table=True)             # nothing monitored: 0, -1, 0 (bridges keep their marks)
    _recompute(none, np.zeros(e), S)
    ok = torch.from_numpy(isl == 0).to(DEV)
    assert bool((none.worst_line == -1).all()) and bool((none.severity[:, ok] == 0).all()) and bool((none.overloads[:, ok] == 0).all())


# ------------------------------------------------------------------------------------------- routes, thresholds
def _lds_fit():
    lib = L.load()
    return max(n for n in range(100, 220) if lib.pfn_contingency_workspace_bytes(1, n, n + n // 2, 0) == 0)


@pytest.mark.parametrize("which", ["m = PF_BIG_M", "m = PF_BIG_M + 1", "largest in LDS", "one more"])
def test_both_sides_of_the_dispatch_thresholds(which):
    fit = _lds_fit()
    assert fit == 187
    n = {"m = PF_BIG_M": 91, "m = PF_BIG_M + 1": 92, "largest in LDS": fit, "one more": fit + 1}[which]     # 256 | 1024 threads; LDS | global
    case = _case(n, n + n // 2, 1)
    res = _screen(case, keep_table=True)
    assert res.route == ("global" if which == "one more" else "lds")
    _check_flows(case, res, f"{which}: n {n} e {case.e}")
    _recompute(res, None, 1)
    if which == "one more":
        with pytest.raises(RuntimeError, match=r"code -1.*LDS"):
            _screen(case, route="lds")


def test_the_global_route():
    case = _case(200, 300, 1)
    res = _screen(case, keep_table=True)
    assert res.route == "global"
    _check_flows(case, res, "n 200 e 300 S 1")
    with pytest.raises(RuntimeError, match=r"code -1.*LDS"):
        _screen(case, route="lds")
    small = _case(14, 20, 8)
    glob, lds = _screen(small, keep_table=True, route="global"), _screen(small, keep_table=True, route="lds")
    assert (glob.route, lds.route) == ("global", "lds")
    _check_flows(small, glob, "n 14 e 20 S 8, global route")
    assert _same(glob, lds)                                                 # the same code: the same bits


# ---------------------------------------------------------------------------------------------------- independence
def test_a_scenario_does_not_depend_on_its_batch():
    case = _case(14, 20, 8)
    ratings = 1.2 * np.abs(_yard(14, 20, 8)[3])                             # [S, e]
    whole = _screen(case, ratings=ratings, keep_table=True)
    assert bool((whole.status >= 0).all())
    a, b = _screen(case, slice(0, 4), ratings[:4], keep_table=True), _screen(case, slice(4, 8), ratings[4:], keep_table=True)
    assert _same(a, whole, rows_b=slice(0, 4)) and _same(b, whole, rows_b=slice(4, 8))
    one = _screen(case, slice(5, 6), ratings[5:6], keep_table=True)
    assert _same(one, whole, rows_b=slice(5, 6))
    big = _case(118, 186, 2)                                                # ... nor on the workgroup's other waves: 1024 threads
    both, last = _screen(big), _screen(big, slice(1, 2))
    assert _same(last, both, rows_b=slice(1, 2), table=False)


# -------------------------------------------------------------------------------------------------------- failures
def _raw_dc(case, n_pv, n_pq, S):
    e, n = case.e, case.n
    bt, spec, ei, rx = _dev(case.bt.astype(np.int32)), _dev(case.spec), _dev(case.ei), _dev(case.rx)
    isl = torch.zeros(e, dtype=torch.int32, device=DEV)
    guard = -7.5
    out = types.SimpleNamespace(severity=torch.full((S + 1, e), guard, dtype=torch.float32, device=DEV),
                                worst_line=torch.full((S, e), 77, dtype=torch.int32, device=DEV), overloads=torch.full((S, e), 77, dtype=torch.int32, device=DEV),
                                base_flow=torch.full((S + 1, e), guard, dtype=torch.float64, device=DEV), status=torch.full((S,), 99, dtype=torch.int32, device=DEV),
                                flags=torch.zeros(1, dtype=torch.int32, device=DEV), guard=guard)
    out.rc = L.load().pfn_contingency_dc(ei.data_ptr(), e, rx.data_ptr(), bt.data_ptr(), spec.data_ptr(), None, 0, isl.data_ptr(), S, n, n_pv, n_pq,
                                         C.c_double(TOL), MAX_ITER, 0, out.severity.data_ptr(), out.worst_line.data_ptr(), out.overloads.data_ptr(),
                                         out.base_flow.data_ptr(), out.status.data_ptr(), None, out.flags.data_ptr(), None, 0, L.stream_ptr())
    return out


def test_failures_stay_local():
    n, e = 14, 20
    case = _case(n, e, 6)
    isl = _yard(n, e, 6)[0]
    clean = _screen(case, keep_table=True)
    spec, rx = case.spec.copy(), case.rx.copy()
    spec[1, 5, 2] = np.nan                                                  # scenario 1: a NaN in P
    rx[4, 8, 1] = 0.0                                                       # scenario 4: x = 0 on a line
    res = contingency_screen(_dev(case.bt), _dev(spec), _dev(case.ei), _dev(rx), tol=TOL, max_iter=MAX_ITER, keep_table=True)
    status = res.status.tolist()
    assert [status[1], status[4]] == [-3, -3] and int(res.flags.item()) == 0
    for s in (1, 4):                                                        # float outputs NaN, integer outputs -1: bridges too
        assert torch.isnan(res.severity[s]).all() and torch.isnan(res.base_flow[s]).all() and torch.isnan(res.post_flow[s]).all()
        assert bool((res.worst_line[s] == -1).all()) and bool((res.overloads[s] == -1).all())
    keep = [0, 2, 3, 5]
    assert _same(res, clean, rows_a=keep, rows_b=keep) and bool((clean.status >= 0).all())
    # a bus without a line in the base grid: singular, everywhere; the islands count it under every outage
    lonely = np.where(case.ei == 13, 1, case.ei)
    res = _screen(case, ei=lonely, keep_table=True)
    assert res.status.tolist() == [-2] * 6 and bool((res.islands >= 1).all())
    assert torch.isnan(res.severity).all() and torch.isnan(res.base_flow).all() and torch.isnan(res.post_flow).all() and bool((res.overloads == -1).all())
    # a line to bus id n: -4 everywhere, islands included
    far = case.ei.copy()
    far[1, 7] = n
    res = _screen(case, ei=far)
    assert res.status.tolist() == [-4] * 6 and res.islands.tolist() == [-4] * e and torch.isnan(res.severity).all() and bool((res.worst_line == -1).all())
    # counts that contradict bus_type: -5 and the flag, nothing beyond the scenarios' rows is written
    n_pv, n_pq = int((case.bt == 1).sum()), int((case.bt == 2).sum())
    raw = _raw_dc(case, n_pv + 1, n_pq - 1, 6)
    assert raw.rc == 0 and int(raw.flags.item()) & 1 and raw.status.tolist() == [-5] * 6
    assert torch.isnan(raw.severity[:6]).all() and torch.isnan(raw.base_flow[:6]).all() and bool((raw.worst_line == -1).all())
    assert bool((raw.severity[6] == raw.guard).all()) and bool((raw.base_flow[6] == raw.guard).all())
    good = _raw_dc(case, n_pv, n_pq, 6)                                     # (the same call with the right counts runs)
    assert good.rc == 0 and int(good.flags.item()) == 0 and bool((good.status >= 0).all()) and isl.size == e


# ---------------------------------------------------------------------------------------------------------- verify
@pytest.mark.parametrize("n,e", [(5, 6), (14, 20)])
def test_verify_solves_the_reduced_grids_with_the_ac_solver(n, e):
    S = 2
    case = _case(n, e, S)
    isl, lit, den, f, inv = _yard(n, e, S)
    ratings = 1.2 * np.abs(f).max(axis=0)
    res = _screen(case, ratings=ratings)
    args = (_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), _dev(ratings))
    ver = verify_contingencies(res, *args, top=3, tol=TOL, max_iter=MAX_ITER)
    rank = res.ranking(e)[0].cpu().numpy()
    want_pairs = [(s, int(k)) for s in range(S) for k in [k for k in rank[s] if isl[k] == 0][:3]]
    assert ver.pairs.tolist() == [list(p) for p in want_pairs] and len(want_pairs) == 6
    assert (isl[rank[:, 0]] > 0).all()                                      # (the islanding outages rank first and are skipped)
    if n == 14:                                                             # the first, a middle and the last line; a bridge is skipped
        assert isl[[0, 10, 19]].tolist() == [0, 0, 0] and isl[1] > 0
        chosen = verify_contingencies(res, *args, pairs=[(0, 0), (0, 1), (0, 10), (1, 19)], tol=TOL, max_iter=MAX_ITER)
        assert chosen.pairs.tolist() == [[0, 0], [0, 10], [1, 19]]
        _check_verified(case, res, chosen, ratings)
    _check_verified(case, res, ver, ratings)


def _check_verified(case, res, ver, ratings):
    n, e = case.n, case.e
    status, table, loading = ver.status.tolist(), ver.table.cpu().numpy(), ver.loading.cpu().numpy()
    assert loading.dtype == np.float32 and loading.shape == (len(status), e)
    worst_f = worst_x = worst_i = 0.0
    for t, (s, k) in enumerate(ver.pairs.tolist()):
        keep = np.arange(e) != k
        ei, rx = np.ascontiguousarray(case.ei[:, keep]), np.ascontiguousarray(case.rx[s][keep])
        # the table is solve_power_flow's on lists built in numpy, bit for bit; Newton converged (the yardstick's does: a -1 is a failure)
        direct = solve_power_flow(_dev(case.bt), _dev(case.spec[s:s + 1]), _dev(ei), _dev(rx[None]), tol=TOL, max_iter=MAX_ITER)
        assert 1 <= status[t] <= MAX_ITER and int(direct.status[0]) == status[t] and torch.equal(direct.table[0], ver.table[t])
        want, st, _ = P.newton(case.bt, case.spec[s], ei, rx, tol=TOL, max_iter=MAX_ITER)
        assert 1 <= st <= MAX_ITER
        reduced = types.SimpleNamespace(ei=ei, rx=rx[None], bt=case.bt, spec=case.spec[s:s + 1])
        worst_f = max(worst_f, _residual_ratio(reduced, table[t:t + 1]))
        worst_x = max(worst_x, float(_distance(table[t], want) / (2 * TOL * P.jacobian_inverse_norm(want, case.bt, ei, rx))))
        # the loadings: branch_flows' bound on the current, divided by the fp32 rating (one more rounding), in ORIGINAL numbering
        flows, scales = B.flows(table[t:t + 1].astype(np.float32), ei, rx.astype(np.float32).astype(np.float64))
        r32 = ratings.astype(np.float32).astype(np.float64)
        ref = np.full(e, np.nan)
        ref[keep] = flows[0, :, 0] / r32[keep]
        bound = (B.C_BOUND * B.EPS * scales[0, :, 0]) / r32[keep] + B.EPS * np.abs(ref[keep])
        assert np.isnan(loading[t, k]) and np.isfinite(loading[t, keep]).all()
        worst_i = max(worst_i, float((np.abs(loading[t, keep] - ref[keep]) / bound).max()))
        # severity, worst line and count by the screen's rules from the loadings themselves; the worst line in original numbering
        row = np.where(np.isnan(loading[t]), 0.0, loading[t])[None].repeat(e, axis=0)
        sev, worst, over = R.summarise(row, None, np.zeros(e, dtype=np.int32), dtype=np.float32)     # (they ARE loadings: rating 1)
        assert float(ver.severity[t]) == float(sev[k]) and int(ver.worst_line[t]) == int(worst[k]) != k and int(ver.overloads[t]) == int(over[k])
        assert float(ver.dc_severity[t]) == float(res.severity[s, k])
    print(f"verify n {n}: {len(status)} pairs, worst |mismatch| / bound {worst_f:.3g}, worst |x - yardstick| / (2 tol ||J^-1||) {worst_x:.3g}, "
          f"worst |loading - f64| / bound {worst_i:.3g}")
    assert worst_f <= 1.0 and worst_x <= 1.0 and worst_i <= 1.0


# --------------------------------------------------------------------------------------------------------- capture
def test_the_screen_is_capturable():
    case = _case(14, 20, 8)
    ratings = _dev(1.2 * np.abs(_yard(14, 20, 8)[3]).max(axis=0))
    bt, spec, ei, rx = _dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx)
    eager = contingency_screen(bt, spec, ei, rx, ratings, tol=TOL, max_iter=MAX_ITER, keep_table=True)      # (also: the one host read)
    torch.cuda.synchronize()
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            res = contingency_screen(bt, spec, ei, rx, ratings, tol=TOL, max_iter=MAX_ITER, keep_table=True)
    for _ in range(2):
        for t in (res.severity, res.base_flow, res.post_flow):
            t.fill_(-7.0)
        for t in (res.worst_line, res.overloads, res.status, res.islands):
            t.fill_(99)
        g.replay()
        torch.cuda.synchronize()
        assert _same(res, eager) and bool((res.status >= 0).all())


# ---------------------------------------------------------------------------------------------------------- script
def test_the_script_runs_end_to_end(tmp_path, monkeypatch):
    import contingency
    monkeypatch.chdir(tmp_path)
    text = _run(contingency.main, ["--case", "14", "--samples", "8", "--verify-top", "2"])
    assert "islanding outages" in text and "called secure" in text
    shapes = {"severity": ((8, 20), np.float32), "worst_line": ((8, 20), np.int32), "overloads": ((8, 20), np.int32), "islands": ((20,), np.int32),
              "base_flow": ((8, 20), np.float64)}
    for name, (shape, dtype) in shapes.items():
        a = np.load(tmp_path / "results" / f"case14_contingency_{name}.npy")
        assert a.shape == shape and a.dtype == dtype, name
    assert np.isfinite(np.load(tmp_path / "results" / "case14_contingency_base_flow.npy")).all()
