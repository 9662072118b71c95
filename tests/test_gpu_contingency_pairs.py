"""The N-2 line-pair outage screen on the device: `pfn_contingency_pair_islands` and `pfn_contingency_pairs`
(csrc/contingency_pairs.hip) through `contingency_screen_pairs`, and `verify_pair_contingencies`, held to the float64 yardstick of
tests/contingency_pairs_ref.py, which LITERALLY removes both lines and solves the DC model again.  Inputs are
`make_physical_inputs(n, e, S, seed=1)`; every test asserts on the yardstick that its pair set has an islanding pair, (from (5, 6)
up) an islanding pair of two non-bridges, and max ||M^-1||_inf <= 32 over its non-islanding pairs, so nothing needs excluding.

  islands     equal to the yardstick's, exactly; -4 everywhere for a bad id;
  base        base flows and statuses carry `contingency_screen`'s bits for the same inputs;
  flows       for every non-islanding pair p and every line l:  |dev - f64| <= C2 * u_p,  u_p = 2^-24 max_l |f_l| ||M_p^-1||_inf, M the
              yardstick's: the kernel's per-line arithmetic and its fp32 inverse of B' are worth a few units of fp32 rounding of the
              largest flow, amplified by the pair's 2 x 2 solve;
  reductions  severity, worst line and overload count are bit-exact functions of the kernel's own table and the fp32 ratings;
  the rest    islanding rows, both sides of the LDS / global threshold, bit-for-bit independence of the batch, of the candidate list and
              of the route, failures that stay local, the ranking, the AC verification, graph capture, the script.

Candidate subsets are chosen by a fixed rule (`_candidates`): every ceil(e / (c - 2))-th line, the two lines of the first non-slack
bus of degree two whose lines are both non-bridges (removing both cuts the bus off: a known non-bridge islanding pair), filled up
with the lowest unused ids.

Worst flow ratios |dev - f64| / u measured on an MI355X on 2026-10-21 (each test prints its own; WORST below):
0 at (3, 3) (every pair islands), 6.25 at (5, 6), 5.73 at (14, 20), all pairs each; 8.76 at (70, 100) with 30 candidates, 5.42 at
(118, 186) with 24, 6.21 at (200, 300) with 16 (the global route); at the threshold, 8 candidates each, 4.37 at (190, 285), the largest
in LDS, and 3.54 at (191, 286), the first on the global route.  C2 = 64 is the smallest power of two >= 4 x the worst of them
(4 x 8.76 = 35), the rule by which the N-1 test arrived at its C_BOUND.  AC verification: mismatch 1.7e-4, distance 8.8e-6, loadings
0.029 of their bounds."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.loss import branch_flows  # noqa: F401  (the import fails loudly where the library is missing)
from poweflownet_amd.utils.contingency import contingency_screen, contingency_screen_pairs, pair_lines, verify_pair_contingencies
from poweflownet_amd.utils.powerflow import solve_power_flow
from tests import branch_ref as B
from tests import contingency_pairs_ref as R2
from tests import contingency_ref as R
from tests import powerflow_ref as P
from tests.powerflow_checks import DEV, TOL, _dev, _distance, _residual_ratio, _run
from tests.test_gpu_powerflow import _case

pytestmark = pytest.mark.gpu
MAX_ITER = 10
EPS = 2.0 ** -24
NORM_CAP = 32.0
# worst |dev - f64| / u measured on an MI355X per shape (n, e): the figures C2 was set from
WORST = {(3, 3): 0.0, (5, 6): 6.25, (14, 20): 5.73, (70, 100): 8.76, (118, 186): 5.42, (200, 300): 6.21, (190, 285): 4.37, (191, 286): 3.54}
C2 = 64.0
assert C2 == 2.0 ** np.ceil(np.log2(4 * max(WORST.values())))


def _candidates(case, c):
    """the fixed rule of the module docstring; None for all lines"""
    if c is None:
        return None
    e = case.e
    single = R.islands(case.bt, case.ei)
    slack = int(np.flatnonzero(case.bt == 0)[0])
    known = next(inc for b in range(case.n) if b != slack
                 for inc in [np.flatnonzero((case.ei[0] == b) | (case.ei[1] == b))] if len(inc) == 2 and (single[inc] == 0).all())
    lines = set(np.arange(0, e, -(-e // (c - 2)))[:c - 2].tolist()) | set(known.tolist())
    lines |= set([k for k in range(e) if k not in lines][:c - len(lines)])
    assert len(lines) == c
    return tuple(sorted(lines))


@functools.lru_cache(maxsize=None)
def _yard(n, e, S, lines=None):
    """(pairs [P, 2], islands [P], literal post-pair flows [S, P, e], ||M^-1||_inf [S, P], base flows [S, e]) of the yardstick, once"""
    case = _case(n, e, S)
    pairs = R2.pair_list(e if lines is None else lines)
    isl = R2.islands(case.bt, case.ei, pairs)
    single = R.islands(case.bt, case.ei)
    lit = np.stack([R2.resolve_pairs(case.bt, case.spec[s], case.ei, case.rx[s], pairs, isl) for s in range(S)])
    norm = np.stack([R2.inverse_norm(R2.lodf_pairs(case.bt, case.spec[s], case.ei, case.rx[s], pairs)[1])[0] for s in range(S)])
    f = np.stack([R.base_flow(case.bt, case.spec[s], case.ei, case.rx[s]) for s in range(S)])
    assert (isl > 0).any(), (n, e)
    if n >= 5:
        assert ((isl > 0) & (single[pairs[:, 0]] == 0) & (single[pairs[:, 1]] == 0)).any() and (isl == 0).any(), (n, e)
        assert norm[:, isl == 0].max() <= NORM_CAP, (n, e, norm[:, isl == 0].max())
    return pairs, isl, lit, norm, f


def _screen(case, rows=slice(None), ratings=None, ei=None, spec=None, rx=None, **kw):
    kw = {"tol": TOL, "max_iter": MAX_ITER, **kw}
    spec, rx = case.spec if spec is None else spec, case.rx if rx is None else rx
    return contingency_screen_pairs(_dev(case.bt), _dev(spec[rows]), _dev(case.ei if ei is None else ei), _dev(rx[rows]),
                                    None if ratings is None else _dev(ratings), **kw)


def _single(case, rows=slice(None), ei=None, spec=None, rx=None):
    spec, rx = case.spec if spec is None else spec, case.rx if rx is None else rx
    return contingency_screen(_dev(case.bt), _dev(spec[rows]), _dev(case.ei if ei is None else ei), _dev(rx[rows]), tol=TOL, max_iter=MAX_ITER)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b, rows_a=slice(None), rows_b=slice(None), cols_a=slice(None), cols_b=slice(None), table=True):
    """two results agree bit for bit on the given scenario rows and pair columns (NaN bits included)"""
    names = ["severity", "worst_line", "overloads"] + (["post_flow"] if table else [])
    return (all(torch.equal(_bits(getattr(a, k)[rows_a][:, cols_a]), _bits(getattr(b, k)[rows_b][:, cols_b])) for k in names)
            and all(torch.equal(_bits(getattr(a, k)[rows_a]), _bits(getattr(b, k)[rows_b])) for k in ("base_flow", "status"))
            and torch.equal(a.islands[cols_a], b.islands[cols_b]) and torch.equal(a.pairs[cols_a], b.pairs[cols_b]))


def _base_is_the_single_screens(res, single):
    assert torch.equal(_bits(res.base_flow), _bits(single.base_flow)) and torch.equal(res.status, single.status)


def _check_flows(case, res, yard, what, ratings=None):
    """status, the flow bound, the islanding rows, the worst line and the severity of a result with its table against the yardstick"""
    S, e = case.S, case.e
    pairs, isl, lit, norm, f = yard
    n_pairs = len(pairs)
    status, post = res.status.cpu().numpy(), res.post_flow.cpu().numpy()
    sev, worst, over = res.severity.cpu().numpy(), res.worst_line.cpu().numpy(), res.overloads.cpu().numpy()
    assert ((status >= 0) & (status <= MAX_ITER)).all() and int(res.flags.item()) == 0, (what, status)
    assert np.array_equal(res.islands.cpu().numpy(), isl) and np.array_equal(res.pairs.cpu().numpy(), pairs) and res.pairs.dtype == torch.int64
    assert post.shape == (S, n_pairs, e) and post.dtype == np.float32 and sev.dtype == np.float32 and sev.shape == (S, n_pairs)
    cut, ok = isl > 0, isl == 0
    worst_ratio = 0.0
    r = np.ones(e) if ratings is None else np.asarray(ratings, dtype=np.float64)
    for s in range(S):
        # an islanding pair: +inf, -1, -1 and a NaN row
        assert np.isnan(post[s][cut]).all() and (sev[s][cut] == np.inf).all() and (worst[s][cut] == -1).all() and (over[s][cut] == -1).all()
        if not ok.any():
            continue
        u = EPS * np.abs(f[s]).max() * norm[s]                              # [P], per pair (an islanding pair's is not used)
        ratio = np.abs(post[s][ok].astype(np.float64) - lit[s][ok]) / u[ok][:, None]
        worst_ratio = max(worst_ratio, float(ratio.max()))
        assert (post[s][ok, pairs[ok, 0]] == 0).all() and (post[s][ok, pairs[ok, 1]] == 0).all()
        # the worst line is the yardstick's wherever the yardstick's top two loadings differ by more than 2 C2 u / rating
        want_sev, want_worst, _ = R2.summarise_pairs(lit[s], ratings, isl, pairs)
        for p in np.flatnonzero(ok):
            if want_worst[p] < 0:
                continue
            if R2.top_two_gap(lit[s][p], ratings, *pairs[p]) > 2 * C2 * u[p] / r[want_worst[p]]:
                assert worst[s, p] == want_worst[p], (what, s, p)
            assert abs(sev[s, p] - want_sev[p]) <= C2 * u[p] / r[r > 0].min() + EPS * want_sev[p], (what, s, p)
    print(f"{what}: route {res.route}, {n_pairs} pairs ({int(cut.sum())} islanding), solves {status.min()}..{status.max()}, "
          f"worst |post flow - f64| / u {worst_ratio:.3g} (C2 = {C2:g})")
    assert worst_ratio <= C2, (what, worst_ratio)
    return worst_ratio


def _recompute(res, ratings, S):
    """severity, worst line and overload count again from the kernel's own table in numpy fp32: bit for bit"""
    isl, pairs, post = res.islands.cpu().numpy(), res.pairs.cpu().numpy(), res.post_flow.cpu().numpy()
    for s in range(S):
        r = None if ratings is None else (ratings if ratings.ndim == 1 else ratings[s])
        sev, worst, over = R2.summarise_pairs(post[s], r, isl, pairs, dtype=np.float32)
        got = res.severity[s].cpu().numpy()
        fin = ~np.isnan(sev)
        assert sev.dtype == np.float32 and np.array_equal(np.isnan(got), ~fin), s
        assert np.array_equal(got[fin].view(np.uint32), sev[fin].view(np.uint32)), s
        assert np.array_equal(res.worst_line[s].cpu().numpy(), worst) and np.array_equal(res.overloads[s].cpu().numpy(), over), s
    return isl


# ------------------------------------------------------------------------------------------------------ islands
@pytest.mark.parametrize("n,e,c", [(3, 3, None), (5, 6, None), (14, 20, None), (70, 100, 30), (118, 186, 24), (200, 300, 16)])
def test_pair_islands_equal_the_yardstick(n, e, c):
    case = _case(n, e, 1)
    lines = _candidates(case, c)
    pairs = R2.pair_list(e if lines is None else lines)
    want = R2.islands(case.bt, case.ei, pairs)
    ld = _dev(np.asarray(range(e) if lines is None else lines, dtype=np.int32))
    out = torch.full((len(pairs) + 1,), 77, dtype=torch.int32, device=DEV)
    slack = int(np.flatnonzero(case.bt == 0)[0])
    L.check(L.load().pfn_contingency_pair_islands(_dev(case.ei).data_ptr(), e, n, slack, ld.data_ptr(), int(ld.shape[0]), out.data_ptr(),
                                                  L.stream_ptr()), "pfn_contingency_pair_islands")
    assert out[:-1].tolist() == want.tolist() and int(out[-1]) == 77       # (nothing beyond the P words is written)
    assert pair_lines(e if lines is None else list(lines)).tolist() == pairs.tolist()


def test_a_bad_id_is_minus_four_everywhere_and_the_statuses_are_the_single_screens():
    case = _case(14, 20, 3)
    for bad in (-1, 14):
        ei = case.ei.copy()
        ei[1, 7] = bad
        res, single = _screen(case, ei=ei, keep_table=True), _single(case, ei=ei)
        assert res.islands.tolist() == [-4] * 190 and res.status.tolist() == [-4] * 3 == single.status.tolist()
        assert torch.isnan(res.severity).all() and torch.isnan(res.post_flow).all() and torch.isnan(res.base_flow).all()
        assert bool((res.worst_line == -1).all()) and bool((res.overloads == -1).all())


# -------------------------------------------------------------------------------------------------------- flows
@pytest.mark.parametrize("n,e,S,c", [(3, 3, 2, None), (5, 6, 3, None), (14, 20, 4, None), (70, 100, 2, 30), (118, 186, 2, 24), (200, 300, 1, 16)])
def test_flows_against_removing_both_lines(n, e, S, c):
    case = _case(n, e, S)
    lines = _candidates(case, c)
    yard = _yard(n, e, S, lines)
    res = _screen(case, lines=lines, keep_table=True)
    assert res.route == ("global" if n == 200 else "lds")
    _check_flows(case, res, yard, f"n {n} e {e} S {S} candidates {c or e}")
    _recompute(res, None, S)
    _base_is_the_single_screens(res, _single(case))
    bare = _screen(case, lines=lines)                                       # without the table: the same bits, no table
    assert bare.post_flow is None and _same(bare, res, table=False)
    if lines is not None:                                                   # a CPU int64 tensor is the same list
        assert _same(_screen(case, lines=torch.tensor(lines), keep_table=True), res)


# --------------------------------------------------------------------------------------------------- reductions
def test_reductions_are_exact_functions_of_the_table_and_the_ratings():
    n, e, S = 14, 20, 4
    case = _case(n, e, S)
    yard = _yard(n, e, S)
    pairs, isl, lit, norm, f = yard
    per_line = 1.2 * np.abs(f).max(axis=0)                                  # some pairs overload some lines
    per_line[[2, 9, 11]] = [0.0, -1.0, np.nan]                              # unmonitored: zero, negative, NaN
    res = _screen(case, ratings=per_line, keep_table=True)
    _check_flows(case, res, yard, "ratings [e]", ratings=np.where(per_line > 0, per_line, 0.0))
    _recompute(res, per_line, S)
    over = res.overloads.cpu().numpy()[:, isl == 0]
    assert (over > 0).any() and (over == 0).any()
    assert not np.isin(res.worst_line.cpu().numpy(), [2, 9, 11]).any()
    rng = np.random.default_rng(0)
    per_sample = np.abs(f) * rng.uniform(0.5, 2.0, f.shape)
    per_sample[rng.random(f.shape) < 0.2] = 0.0
    per_sample[3, 4] = 1e-60                                               # not > 0 once it is fp32: unmonitored
    per_sample[1, 6] = 1e-42                                               # an fp32 denormal: its loading overflows -> NaN severity
    res2 = _screen(case, ratings=per_sample, keep_table=True)
    assert torch.equal(_bits(res2.post_flow), _bits(res.post_flow)) and torch.equal(res2.base_flow, res.base_flow)
    _recompute(res2, per_sample, S)
    sev1, worst1 = res2.severity[1].cpu().numpy(), res2.worst_line[1].cpu().numpy()
    with_six = (pairs == 6).any(axis=1)
    assert np.isnan(sev1).any() and not np.isnan(sev1[with_six]).any() and (worst1[np.isnan(sev1)] == 6).all()
    assert not np.isnan(res2.severity[[0, 2, 3]].cpu().numpy()).any()
    none = _screen(case, ratings=np.zeros(e), keep_table=True)             # nothing monitored: 0, -1, 0 (islanding pairs keep their marks)
    _recompute(none, np.zeros(e), S)
    ok = torch.from_numpy(isl == 0).to(DEV)
    assert bool((none.worst_line == -1).all()) and bool((none.severity[:, ok] == 0).all()) and bool((none.overloads[:, ok] == 0).all())
    plain = _screen(case, keep_table=True)                                 # ratings None: 1.0 everywhere
    _recompute(plain, None, S)
    assert _same(plain, _screen(case, ratings=np.ones(e), keep_table=True))


# ------------------------------------------------------------------------------------------- routes, thresholds
def _lds_fit():
    lib = L.load()
    return max(n for n in range(100, 260) if lib.pfn_contingency_pairs_workspace_bytes(1, n, n + n // 2, 8, 1) != 0)


@pytest.mark.parametrize("which", ["largest in LDS", "one more"])
def test_both_sides_of_the_lds_threshold(which):
    fit = _lds_fit()
    assert 100 < fit < 259 and L.load().pfn_contingency_pairs_workspace_bytes(1, fit + 1, fit + 1 + (fit + 1) // 2, 8, 1) == 0
    n = fit + (which == "one more")
    case = _case(n, n + n // 2, 1)
    lines = _candidates(case, 8)
    yard = _yard(n, case.e, 1, lines)
    res = _screen(case, lines=lines, keep_table=True)
    assert res.route == ("global" if which == "one more" else "lds")
    _check_flows(case, res, yard, f"{which}: n {n} e {case.e}")
    _recompute(res, None, 1)
    _base_is_the_single_screens(res, _single(case))
    if which == "one more":
        with pytest.raises(RuntimeError, match=r"code -1.*LDS"):
            _screen(case, lines=lines, route="lds")
    else:
        assert _same(_screen(case, lines=lines, keep_table=True, route="global"), res)


def test_the_forced_global_route_has_the_same_bits():
    case = _case(14, 20, 4)
    glob, lds = _screen(case, keep_table=True, route="global"), _screen(case, keep_table=True, route="lds")
    assert (glob.route, lds.route) == ("global", "lds")
    _check_flows(case, glob, _yard(14, 20, 4), "n 14 e 20 S 4, global route")
    assert _same(glob, lds)


def test_beyond_the_dense_cap_it_raises_and_names_the_limit():
    n = int(L.load().pfn_powerflow_max_unknowns()) + 2
    ei = torch.stack([torch.arange(n - 1), torch.arange(1, n)]).to(DEV)
    bt = torch.tensor([0] + [2] * (n - 1), device=DEV)
    spec, rx = torch.zeros(1, n, 4, dtype=torch.float64, device=DEV), torch.ones(1, n - 1, 2, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match=rf"{n - 2}.*max_unknowns"):
        contingency_screen_pairs(bt, spec, ei, rx, lines=[0, 1, 2])


# ---------------------------------------------------------------------------------------------------- independence
def test_a_pair_depends_neither_on_its_batch_nor_on_the_candidate_list():
    case = _case(14, 20, 4)
    ratings = 1.2 * np.abs(_yard(14, 20, 4)[4])                             # [S, e]
    whole = _screen(case, ratings=ratings, keep_table=True)
    assert bool((whole.status >= 0).all())
    for rows in (slice(0, 2), slice(2, 4), slice(3, 4)):                    # halves and an S = 1 run
        part = _screen(case, rows, ratings[rows], keep_table=True)
        assert _same(part, whole, rows_b=rows)
    lines = _candidates(case, 7)
    sub = _screen(case, ratings=ratings, lines=lines, keep_table=True)
    where = {tuple(p): k for k, p in enumerate(whole.pairs.tolist())}
    cols = torch.tensor([where[tuple(p)] for p in sub.pairs.tolist()], device=DEV)
    assert len(cols) == 21 and _same(sub, whole, cols_b=cols)
    big = _case(118, 186, 2)                                                # ... nor on the workgroup's other waves: 1024 threads
    lines = _candidates(big, 24)
    both, last = _screen(big, lines=lines), _screen(big, slice(1, 2), lines=lines)
    assert _same(last, both, rows_b=slice(1, 2), table=False)


# -------------------------------------------------------------------------------------------------------- failures
def _raw_pairs(case, n_pv, n_pq, S, c=5):
    e, n = case.e, case.n
    bt, spec, ei, rx = _dev(case.bt.astype(np.int32)), _dev(case.spec), _dev(case.ei), _dev(case.rx)
    lib = L.load()
    P_ = c * (c - 1) // 2
    lines = torch.arange(c, dtype=torch.int32, device=DEV)
    isl = torch.zeros(P_, dtype=torch.int32, device=DEV)
    guard = -7.5
    need = int(lib.pfn_contingency_pairs_workspace_bytes(S, n, e, c, 0))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = types.SimpleNamespace(severity=torch.full((S + 1, P_), guard, dtype=torch.float32, device=DEV),
                                worst_line=torch.full((S, P_), 77, dtype=torch.int32, device=DEV), overloads=torch.full((S, P_), 77, dtype=torch.int32, device=DEV),
                                base_flow=torch.full((S + 1, e), guard, dtype=torch.float64, device=DEV), status=torch.full((S,), 99, dtype=torch.int32, device=DEV),
                                flags=torch.zeros(1, dtype=torch.int32, device=DEV), guard=guard)
    out.rc = lib.pfn_contingency_pairs(ei.data_ptr(), e, rx.data_ptr(), bt.data_ptr(), spec.data_ptr(), None, 0, lines.data_ptr(), c, isl.data_ptr(), S, n,
                                       n_pv, n_pq, C.c_double(TOL), MAX_ITER, 0, out.severity.data_ptr(), out.worst_line.data_ptr(),
                                       out.overloads.data_ptr(), out.base_flow.data_ptr(), out.status.data_ptr(), None, out.flags.data_ptr(),
                                       ws.data_ptr(), need, L.stream_ptr())
    return out


def test_failures_stay_local():
    n, e = 14, 20
    case = _case(n, e, 4)
    clean = _screen(case, keep_table=True)
    spec, rx = case.spec.copy(), case.rx.copy()
    spec[1, 5, 2] = np.nan                                                  # scenario 1: a NaN in P
    rx[2, 8, 1] = 0.0                                                       # scenario 2: x = 0 on a line
    res = _screen(case, spec=spec, rx=rx, keep_table=True)
    assert res.status.tolist()[1:3] == [-3, -3] and int(res.flags.item()) == 0
    _base_is_the_single_screens(res, _single(case, spec=spec, rx=rx))
    for s in (1, 2):                                                        # float outputs NaN, integer outputs -1: islanding pairs too
        assert torch.isnan(res.severity[s]).all() and torch.isnan(res.base_flow[s]).all() and torch.isnan(res.post_flow[s]).all()
        assert bool((res.worst_line[s] == -1).all()) and bool((res.overloads[s] == -1).all())
    assert _same(res, clean, rows_a=[0, 3], rows_b=[0, 3]) and bool((clean.status >= 0).all())
    # a bus without a line in the base grid: singular, everywhere; the islands count it under every pair
    lonely = np.where(case.ei == 13, 1, case.ei)
    res = _screen(case, ei=lonely, keep_table=True)
    assert res.status.tolist() == [-2] * 4 and bool((res.islands >= 1).all())
    assert torch.isnan(res.severity).all() and torch.isnan(res.base_flow).all() and torch.isnan(res.post_flow).all() and bool((res.overloads == -1).all())
    # counts that contradict bus_type: -5 and the flag, nothing beyond the scenarios' rows is written
    n_pv, n_pq = int((case.bt == 1).sum()), int((case.bt == 2).sum())
    raw = _raw_pairs(case, n_pv + 1, n_pq - 1, 4)
    assert raw.rc == 0 and int(raw.flags.item()) & 1 and raw.status.tolist() == [-5] * 4
    assert torch.isnan(raw.severity[:4]).all() and torch.isnan(raw.base_flow[:4]).all() and bool((raw.worst_line == -1).all())
    assert bool((raw.severity[4] == raw.guard).all()) and bool((raw.base_flow[4] == raw.guard).all())
    good = _raw_pairs(case, n_pv, n_pq, 4)                                  # (the same call with the right counts runs)
    assert good.rc == 0 and int(good.flags.item()) == 0 and bool((good.status >= 0).all()) and bool((good.severity[:4] != good.guard).all())


# --------------------------------------------------------------------------------------------------------- ranking
def test_ranking_against_a_plain_sort_on_the_host():
    case = _case(14, 20, 4)
    spec = case.spec.copy()
    spec[2, 5, 2] = np.nan                                                  # a failed scenario: all NaN, in index order
    res = _screen(case, spec=spec, ratings=1.2 * np.abs(_yard(14, 20, 4)[4]).max(axis=0))
    sev = res.severity.cpu().numpy()
    ids, vals = res.ranking(190)
    for s in range(4):
        key = [(0 if np.isnan(v) else 1 if v == np.inf else 2, 0.0 if not np.isfinite(v) else -float(v), p) for p, v in enumerate(sev[s])]
        assert ids[s].tolist() == [k[2] for k in sorted(key)], s
    assert torch.equal(_bits(vals), _bits(res.severity.gather(1, ids))) and res.ranking(5)[0].tolist() == ids[:, :5].tolist()
    assert ids[2].tolist() == list(range(190)) and bool((res.islands[ids[0, 0]] > 0))


# ---------------------------------------------------------------------------------------------------------- verify
@pytest.mark.parametrize("n,e", [(5, 6), (14, 20)])
def test_verify_solves_the_reduced_grids_with_the_ac_solver(n, e):
    S = 2
    case = _case(n, e, S)
    pairs, isl, lit, norm, f = _yard(n, e, S)
    ratings = 1.2 * np.abs(f).max(axis=0)
    res = _screen(case, ratings=ratings)
    args = (_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), _dev(ratings))
    ver = verify_pair_contingencies(res, *args, top=3, tol=TOL, max_iter=MAX_ITER)
    rank = res.ranking(len(pairs))[0].cpu().numpy()
    want = [(s, int(p)) for s in range(S) for p in [p for p in rank[s] if isl[p] == 0][:3]]
    assert ver.triples.tolist() == [[s, *pairs[p].tolist()] for s, p in want] and ver.pair_index.tolist() == [p for _, p in want] and len(want) == 6
    assert (isl[rank[:, 0]] > 0).all()                                      # (the islanding pairs rank first and are skipped)
    _check_verified(case, res, ver, ratings)
    if n == 14:                                                             # chosen triples, either order of the lines; an islanding pair is skipped
        cut = pairs[np.flatnonzero(isl > 0)[0]]
        fine = pairs[np.flatnonzero(isl == 0)[[0, 40, -1]]]
        chosen = verify_pair_contingencies(res, *args, triples=[(0, *fine[0]), (0, *cut), (1, fine[1][1], fine[1][0]), (1, *fine[2])],
                                           tol=TOL, max_iter=MAX_ITER)
        assert chosen.triples.tolist() == [[0, *fine[0].tolist()], [1, *fine[1].tolist()], [1, *fine[2].tolist()]]
        _check_verified(case, res, chosen, ratings)
        with pytest.raises(ValueError, match="no \\(scenario, pair\\)"):
            verify_pair_contingencies(res, *args, triples=[(0, 3, 3)])


def _check_verified(case, res, ver, ratings):
    n, e = case.n, case.e
    status, table, loading = ver.status.tolist(), ver.table.cpu().numpy(), ver.loading.cpu().numpy()
    assert loading.dtype == np.float32 and loading.shape == (len(status), e)
    worst_f = worst_x = worst_i = 0.0
    for t, (s, a, b) in enumerate(ver.triples.tolist()):
        keep = (np.arange(e) != a) & (np.arange(e) != b)
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
        assert np.isnan(loading[t, a]) and np.isnan(loading[t, b]) and np.isfinite(loading[t, keep]).all()
        worst_i = max(worst_i, float((np.abs(loading[t, keep] - ref[keep]) / bound).max()))
        # severity, worst line and count by the screen's rules from the loadings themselves; the worst line in original numbering
        row = np.where(np.isnan(loading[t]), 0.0, loading[t])[None]
        sev, worst, over = R2.summarise_pairs(row, None, np.zeros(1, dtype=np.int32), np.array([[a, b]]), dtype=np.float32)   # (they ARE loadings: rating 1)
        assert float(ver.severity[t]) == float(sev[0]) and int(ver.worst_line[t]) == int(worst[0]) not in (a, b) and int(ver.overloads[t]) == int(over[0])
        assert float(ver.dc_severity[t]) == float(res.severity[s, int(ver.pair_index[t])])
    print(f"verify pairs n {n}: {len(status)} rows, worst |mismatch| / bound {worst_f:.3g}, worst |x - yardstick| / (2 tol ||J^-1||) {worst_x:.3g}, "
          f"worst |loading - f64| / bound {worst_i:.3g}")
    assert worst_f <= 1.0 and worst_x <= 1.0 and worst_i <= 1.0


# --------------------------------------------------------------------------------------------------------- capture
def test_the_pair_screen_is_capturable():
    case = _case(14, 20, 4)
    ratings = _dev(1.2 * np.abs(_yard(14, 20, 4)[4]).max(axis=0))
    bt, spec, ei, rx = _dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx)
    lines = list(_candidates(case, 7))
    kw = dict(lines=lines, tol=TOL, max_iter=MAX_ITER, keep_table=True)
    eager = contingency_screen_pairs(bt, spec, ei, rx, ratings, **kw)       # (also: the one host read, the one upload of the candidates)
    torch.cuda.synchronize()
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            res = contingency_screen_pairs(bt, spec, ei, rx, ratings, **kw)
    for _ in range(2):
        for t in (res.severity, res.base_flow, res.post_flow):
            t.fill_(-7.0)
        for t in (res.worst_line, res.overloads, res.status, res.islands):
            t.fill_(99)
        g.replay()
        torch.cuda.synchronize()
        assert _same(res, eager) and bool((res.status >= 0).all())


# ---------------------------------------------------------------------------------------------------------- script
def test_the_script_screens_pairs_end_to_end(tmp_path, monkeypatch):
    import contingency
    monkeypatch.chdir(tmp_path)
    text = _run(contingency.main, ["--case", "14", "--samples", "4", "--verify-top", "2", "--pairs", "--candidates", "4"])
    assert "islanding outages" in text and "N-2:" in text and "the DC pair screen called secure" in text
    pairs = np.load(tmp_path / "results" / "case14_contingency_pairs_pairs.npy")
    n_pairs = len(pairs)
    assert pairs.dtype == np.int64 and pairs.shape == (n_pairs, 2) and 6 <= n_pairs <= 120 and (pairs[:, 0] < pairs[:, 1]).all()
    shapes = {"severity": ((4, n_pairs), np.float32), "worst_line": ((4, n_pairs), np.int32), "overloads": ((4, n_pairs), np.int32),
              "islands": ((n_pairs,), np.int32)}
    for name, (shape, dtype) in shapes.items():
        a = np.load(tmp_path / "results" / f"case14_contingency_pairs_{name}.npy")
        assert a.shape == shape and a.dtype == dtype, name
    assert (tmp_path / "results" / "case14_contingency_severity.npy").exists()
