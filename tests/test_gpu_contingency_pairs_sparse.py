"""The sparse route of the N-2 line-pair outage screen on the device: `pfn_contingency_pairs_sparse`
(csrc/contingency_pairs_sparse.hip) through `contingency_screen_pairs(route="sparse", plan=sparse_plan(..., mode="dc"))`, held to the
float64 yardstick of tests/contingency_pairs_ref.py -- the literal re-solve without both lines up to (118, 186), its float64 rank-2
form `lodf_pairs` beyond (tests/test_contingency_pairs_host.py holds the two together).  Inputs are `_case(n, e, S)` with seed 1, the
candidates tests/test_gpu_contingency_pairs.py's fixed `_candidates` rule; every pair set asserts on the yardstick that it holds an
islanding pair, (from (5, 6) up) an islanding pair of two non-bridges, and max ||M^-1||_inf <= 32 over its non-islanding pairs, so
nothing needs excluding.

  islands     equal to the yardstick's, exactly;
  base        base flows and statuses carry `contingency_screen(route="sparse")`'s bits for the same inputs;
  flows       for every non-islanding pair p and every line l:  |dev - f64| <= C3 * u_p,  u_p = 2^-24 max_l |f_l| ||M_p^-1||_inf, M the
              yardstick's (the dense pair screen's bound, its own constant);
  reductions  severity, worst line and overload count are bit-exact functions of the kernel's own table and the fp32 ratings;
  the rest    candidate tile edges, beyond the dense cap, both sides of both placement thresholds, bit-for-bit independence of the
              batch, the candidate list, `groups`, `threads`, `waves` and both placements, the dense pair screen, failures that stay
              local, graph capture, the AC verification on the sparse solver, the script.

Worst flow ratios |dev - f64| / u measured on an MI355X on 2026-10-21 (each test prints its own; WORST below),
the same on both placements, which give the same bits: 0 at (3, 3) (every pair islands), 3.00 at (5, 6), 2.52 at (14, 20), all pairs
each; 1.91 at (70, 100) with 30 candidates, 1.38 at (118, 186) with 24; 2.08 at (70, 100) with 63, 64 and 65; 1.19 at (1100, 1530)
with 16; with 8 candidates 1.35 / 0.898 at (636, 954) / (637, 955), the two sides of the block threshold, and 0.962 / 1.94 at
(2394, 3591) / (2395, 3592), the two sides of the columns threshold with 16 waves.  C3 = 16 is the smallest power of two >= 4 x the
worst of them (4 x 3.00 = 12), DESIGN 7t's rule and margin; the dense pair screen's C2 is 64 (worst 8.76)."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.utils.contingency import contingency_screen, contingency_screen_pairs, verify_pair_contingencies
from poweflownet_amd.utils.powerflow import sparse_plan
from tests import contingency_pairs_ref as R2
from tests import contingency_ref as R
from tests import powerflow_ref as P
from tests.powerflow_checks import DEV, TOL, _dev, _distance, _residual_ratio, _run
from tests.test_gpu_contingency_pairs import C2, NORM_CAP, _bits, _candidates, _recompute, _same
from tests.test_gpu_contingency_sparse import _plan
from tests.test_gpu_powerflow import _case

pytestmark = pytest.mark.gpu
MAX_ITER = 10
EPS = 2.0 ** -24
# worst |dev - f64| / u measured on an MI355X per shape (n, e) or (n, e, candidates): the figures C3 was set from
WORST = {(3, 3): 0.0, (5, 6): 3.0, (14, 20): 2.52, (70, 100): 1.91, (118, 186): 1.38, (70, 100, 63): 2.08, (70, 100, 64): 2.08, (70, 100, 65): 2.08,
         (636, 954): 1.35, (637, 955): 0.898, (1100, 1530): 1.19, (2394, 3591): 0.962, (2395, 3592): 1.94}
C3 = 16.0
assert C3 == 2.0 ** np.ceil(np.log2(4 * max(WORST.values())))
LITERAL_UP_TO = 118                                                         # buses: the literal re-solve up to here, `lodf_pairs` beyond
PLACEMENTS = [("lds", "lds"), ("global", "global")]                         # (block, columns)


@functools.lru_cache(maxsize=None)
def _yard(n, e, S, lines=None):
    """(pairs [P, 2], islands [P], float64 post-pair flows [S, P, e], ||M^-1||_inf [S, P], base flows [S, e]) of the yardstick, once"""
    case = _case(n, e, S)
    pairs = R2.pair_list(e if lines is None else lines)
    isl = R2.islands(case.bt, case.ei, pairs)
    single = R.islands(case.bt, case.ei)
    both = [R2.lodf_pairs(case.bt, case.spec[s], case.ei, case.rx[s], pairs) for s in range(S)]
    norm = np.stack([R2.inverse_norm(M)[0] for _, M in both])
    if n <= LITERAL_UP_TO:
        want = np.stack([R2.resolve_pairs(case.bt, case.spec[s], case.ei, case.rx[s], pairs, isl) for s in range(S)])
    else:
        want = np.stack([p for p, _ in both])
        want[:, isl > 0] = np.nan
    f = np.stack([R.base_flow(case.bt, case.spec[s], case.ei, case.rx[s]) for s in range(S)])
    assert (isl > 0).any(), (n, e)
    if n >= 5:
        assert ((isl > 0) & (single[pairs[:, 0]] == 0) & (single[pairs[:, 1]] == 0)).any() and (isl == 0).any(), (n, e)
        assert norm[:, isl == 0].max() <= NORM_CAP, (n, e, norm[:, isl == 0].max())
    return pairs, isl, want, norm, f


def _screen(case, rows=slice(None), ratings=None, ei=None, spec=None, rx=None, plan=None, **kw):
    kw = {"tol": TOL, "max_iter": MAX_ITER, "route": "sparse", "plan": _plan(case.n, case.e, case.S) if plan is None else plan, **kw}
    spec, rx = case.spec if spec is None else spec, case.rx if rx is None else rx
    return contingency_screen_pairs(_dev(case.bt), _dev(spec[rows]), _dev(case.ei if ei is None else ei), _dev(rx[rows]),
                                    None if ratings is None else _dev(ratings), **kw)


def _single(case, rows=slice(None), ei=None, spec=None, rx=None, plan=None):
    spec, rx = case.spec if spec is None else spec, case.rx if rx is None else rx
    return contingency_screen(_dev(case.bt), _dev(spec[rows]), _dev(case.ei if ei is None else ei), _dev(rx[rows]), tol=TOL, max_iter=MAX_ITER,
                              route="sparse", plan=_plan(case.n, case.e, case.S) if plan is None else plan)


def _base_is_the_single_screens(res, single):
    assert torch.equal(_bits(res.base_flow), _bits(single.base_flow)) and torch.equal(res.status, single.status)


def _check_flows(case, res, yard, what, ratings=None):
    """status, the flow bound, the islanding rows, the worst line and the severity of a result with its table against the yardstick"""
    S, e = case.S, case.e
    pairs, isl, want, norm, f = yard
    n_pairs = len(pairs)
    status, post = res.status.cpu().numpy(), res.post_flow.cpu().numpy()
    sev, worst, over = res.severity.cpu().numpy(), res.worst_line.cpu().numpy(), res.overloads.cpu().numpy()
    assert res.route == "sparse" and ((status >= 0) & (status <= MAX_ITER)).all() and int(res.flags.item()) == 0, (what, status)
    assert np.array_equal(res.islands.cpu().numpy(), isl) and np.array_equal(res.pairs.cpu().numpy(), pairs) and res.pairs.dtype == torch.int64
    assert post.shape == (S, n_pairs, e) and post.dtype == np.float32 and sev.dtype == np.float32 and sev.shape == (S, n_pairs)
    assert worst.dtype == np.int32 and over.dtype == np.int32 and res.base_flow.dtype == torch.float64
    cut, ok = isl > 0, isl == 0
    worst_ratio = 0.0
    r = np.ones(e) if ratings is None else np.asarray(ratings, dtype=np.float64)
    for s in range(S):
        # an islanding pair: +inf, -1, -1 and a NaN row
        assert np.isnan(post[s][cut]).all() and (sev[s][cut] == np.inf).all() and (worst[s][cut] == -1).all() and (over[s][cut] == -1).all()
        if not ok.any():
            continue
        u = EPS * np.abs(f[s]).max() * norm[s]                              # [P], per pair (an islanding pair's is not used)
        ratio = np.abs(post[s][ok].astype(np.float64) - want[s][ok]) / u[ok][:, None]
        worst_ratio = max(worst_ratio, float(ratio.max()))
        assert (post[s][ok, pairs[ok, 0]] == 0).all() and (post[s][ok, pairs[ok, 1]] == 0).all()
        # the worst line is the yardstick's wherever the yardstick's top two loadings differ by more than 2 C3 u / rating
        want_sev, want_worst, _ = R2.summarise_pairs(want[s], ratings, isl, pairs)
        for p in np.flatnonzero(ok):
            if want_worst[p] < 0:
                continue
            if R2.top_two_gap(want[s][p], ratings, *pairs[p]) > 2 * C3 * u[p] / r[want_worst[p]]:
                assert worst[s, p] == want_worst[p], (what, s, p)
            assert abs(sev[s, p] - want_sev[p]) <= C3 * u[p] / r[r > 0].min() + EPS * want_sev[p], (what, s, p)
    print(f"{what}: block {res.block}, columns {res.columns}, {n_pairs} pairs ({int(cut.sum())} islanding), solves {status.min()}..{status.max()}, "
          f"worst |post flow - f64| / u {worst_ratio:.3g} (C3 = {C3:g})")
    assert worst_ratio <= C3, (what, worst_ratio)
    return worst_ratio


# -------------------------------------------------------------------------------------------------------- flows
@pytest.mark.parametrize("block,columns", PLACEMENTS)
@pytest.mark.parametrize("n,e,S,c", [(3, 3, 2, None), (5, 6, 3, None), (14, 20, 8, None), (70, 100, 2, 30), (118, 186, 2, 24)])
def test_flows_against_removing_both_lines(n, e, S, c, block, columns):
    case = _case(n, e, S)
    lines = _candidates(case, c)
    res = _screen(case, lines=lines, keep_table=True, block=block, columns=columns)
    assert (res.block, res.columns) == (block, columns)
    _check_flows(case, res, _yard(n, e, S, lines), f"n {n} e {e} S {S} candidates {c or e}")
    _recompute(res, None, S)
    _base_is_the_single_screens(res, _single(case))
    bare = _screen(case, lines=lines, block=block, columns=columns)         # without the table: the same bits, no table
    assert bare.post_flow is None and _same(bare, res, table=False)


@pytest.mark.parametrize("c", [63, 64, 65])
def test_candidate_tile_edges(c):
    """a partial tile, exactly one tile, a full tile plus a one-lane tile"""
    case = _case(70, 100, 2)
    lines = _candidates(case, c)
    res = _screen(case, lines=lines, keep_table=True)
    assert (res.block, res.columns) == ("lds", "lds")
    _check_flows(case, res, _yard(70, 100, 2, lines), f"n 70 e 100 S 2 candidates {c}")
    _recompute(res, None, 2)
    assert _same(_screen(case, lines=lines, keep_table=True, block="global", columns="global"), res)


# ------------------------------------------------------------------------------------------ beyond the dense cap
def test_beyond_the_dense_cap():
    case = _case(1100, 1530, 1)
    lines = _candidates(case, 16)
    with pytest.raises(ValueError, match=r"1099.*max_unknowns.*route='sparse'"):
        contingency_screen_pairs(_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), lines=lines, tol=TOL, max_iter=MAX_ITER)
    res = _screen(case, lines=lines, keep_table=True)
    assert (res.block, res.columns) == ("global", "lds")
    _check_flows(case, res, _yard(1100, 1530, 1, lines), "n 1100 e 1530 S 1 candidates 16")
    _recompute(res, None, 1)
    _base_is_the_single_screens(res, _single(case))


# --------------------------------------------------------------------------------------------------- thresholds
def _fits(n, block_route, column_route, waves):
    """does the workspace-bytes entry grant the forced placement at n buses, e = n + n // 2, 8 candidates?"""
    e = n + n // 2
    return int(L.load().pfn_contingency_pairs_sparse_workspace_bytes(1, e, 8, C.addressof(_plan(n, e).header), block_route, 0, column_route, waves)) != 0


@pytest.mark.parametrize("which", ["largest in LDS", "one more"])
def test_both_sides_of_the_lds_block_threshold(which):
    assert _fits(636, 1, 2, 0) and not _fits(637, 1, 2, 0) and _fits(637, 0, 2, 0)
    n = {"largest in LDS": 636, "one more": 637}[which]
    case = _case(n, n + n // 2, 1)
    lines = _candidates(case, 8)
    res = _screen(case, lines=lines, keep_table=True)
    assert res.block == ("lds" if which == "largest in LDS" else "global") and res.columns == "lds"
    _check_flows(case, res, _yard(n, case.e, 1, lines), f"block, {which}: n {n} e {case.e}")
    _recompute(res, None, 1)
    if which == "one more":
        with pytest.raises(RuntimeError, match=r"code -1.*LDS"):
            _screen(case, lines=lines, block="lds")
    else:
        assert _same(_screen(case, lines=lines, keep_table=True, block="global"), res)


@functools.lru_cache(maxsize=None)
def _columns_fit():
    """the largest bus count whose 1 + 16 columns fit LDS, by the workspace-bytes entry"""
    fit = max(n for n in range(2390, 2401) if _fits(n, 2, 1, 16))
    assert 2390 < fit < 2400 and not _fits(fit + 1, 2, 1, 16) and _fits(fit + 1, 2, 0, 16)
    return fit


@pytest.mark.parametrize("which", ["largest in LDS", "one more"])
def test_both_sides_of_the_lds_columns_threshold(which):
    n = _columns_fit() + (which == "one more")
    case = _case(n, n + n // 2, 1)
    lines = _candidates(case, 8)
    res = _screen(case, lines=lines, keep_table=True, waves=16)
    assert res.columns == ("lds" if which == "largest in LDS" else "global") and res.block == "global"
    _check_flows(case, res, _yard(n, case.e, 1, lines), f"columns, {which}: n {n} e {case.e}")
    _recompute(res, None, 1)
    if which == "one more":
        with pytest.raises(RuntimeError, match=r"code -1.*LDS"):
            _screen(case, lines=lines, columns="lds", waves=16)
    else:
        assert _same(_screen(case, lines=lines, keep_table=True, columns="global", waves=16), res)


# ---------------------------------------------------------------------------------------------------------- bits
def test_bits_do_not_depend_on_groups_threads_waves_or_placement():
    case = _case(70, 100, 4)
    lines = _candidates(case, 30)
    ref = _screen(case, lines=lines, keep_table=True)
    assert (ref.block, ref.columns) == ("lds", "lds") and bool((ref.status >= 0).all())
    for kw in ({"groups": 1}, {"groups": 2}, {"groups": 3}, {"threads": 64}, {"threads": 256}, {"waves": 1}, {"waves": 4}, {"waves": 16},
               {"block": "global"}, {"columns": "global"}, {"block": "global", "columns": "global", "groups": 3, "threads": 256, "waves": 16},
               {"block": "global", "groups": 1, "waves": 1}):
        assert _same(_screen(case, lines=lines, keep_table=True, **kw), ref), kw
    bare = _screen(case, lines=lines)                                       # without the table: the same bits, no table
    assert bare.post_flow is None and _same(bare, ref, table=False)
    assert _same(_screen(case, lines=lines, groups=2, block="global", columns="global", waves=16), ref, table=False)


def test_a_pair_depends_neither_on_its_batch_nor_on_the_candidate_list():
    case = _case(14, 20, 8)
    ratings = 1.2 * np.abs(_yard(14, 20, 8)[4])                             # [S, e]
    whole = _screen(case, ratings=ratings, keep_table=True)
    assert bool((whole.status >= 0).all())
    for rows in (slice(0, 4), slice(4, 8), slice(5, 6)):                    # halves and an S = 1 run
        part = _screen(case, rows, ratings[rows], keep_table=True)
        assert _same(part, whole, rows_b=rows)
    lines = _candidates(case, 7)
    sub = _screen(case, ratings=ratings, lines=lines, keep_table=True)
    where = {tuple(p): k for k, p in enumerate(whole.pairs.tolist())}
    cols = torch.tensor([where[tuple(p)] for p in sub.pairs.tolist()], device=DEV)
    assert len(cols) == 21 and _same(sub, whole, cols_b=cols) and bool(torch.isnan(sub.post_flow).any())   # (NaN bits included)
    _base_is_the_single_screens(whole, _single(case))


# --------------------------------------------------------------------------------------------------- reductions
def test_reductions_are_exact_functions_of_the_table_and_the_ratings():
    n, e, S = 14, 20, 4
    case = _case(n, e, S)
    yard = _yard(n, e, S)
    pairs, isl, want, norm, f = yard
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


# ---------------------------------------------------------------------------------------- the dense pair screen
def test_against_the_dense_pair_screen():
    n, e, S = 118, 186, 2
    case = _case(n, e, S)
    lines = _candidates(case, 24)
    pairs, isl, want, norm, f = _yard(n, e, S, lines)
    sparse = _screen(case, lines=lines)
    dense = contingency_screen_pairs(_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), lines=lines, tol=TOL, max_iter=MAX_ITER)
    assert torch.equal(sparse.islands, dense.islands) and torch.equal(sparse.pairs, dense.pairs)
    assert bool((sparse.status >= 0).all()) and bool((dense.status >= 0).all())
    sa, sb = sparse.severity.cpu().numpy(), dense.severity.cpu().numpy()
    ok = isl == 0
    worst = 0.0
    for s in range(S):
        u = EPS * np.abs(f[s]).max() * norm[s][ok]
        assert np.array_equal(sa[s][~ok], sb[s][~ok])
        worst = max(worst, float((np.abs(sa[s][ok].astype(np.float64) - sb[s][ok]) / ((C2 + C3) * u + EPS * np.abs(sb[s][ok]))).max()))
    print(f"sparse against dense pairs at (118, 186): worst |severity difference| / ((C2 + C3) u) {worst:.3g}")
    assert worst <= 1.0


# -------------------------------------------------------------------------------------------------------- failures
def _raw_pairs(case, plan, n_pv, n_pq, S, c=5):
    e, n = case.e, case.n
    bt, spec, ei, rx = _dev(case.bt.astype(np.int32)), _dev(case.spec), _dev(case.ei), _dev(case.rx)
    lib, header = L.load(), C.addressof(plan.header)
    n_pairs = c * (c - 1) // 2
    lines = torch.arange(c, dtype=torch.int32, device=DEV)
    isl = torch.zeros(n_pairs, dtype=torch.int32, device=DEV)
    guard = -7.5
    need = int(lib.pfn_contingency_pairs_sparse_workspace_bytes(S, e, c, header, 0, 0, 0, 0))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = types.SimpleNamespace(severity=torch.full((S + 1, n_pairs), guard, dtype=torch.float32, device=DEV),
                                worst_line=torch.full((S + 1, n_pairs), 77, dtype=torch.int32, device=DEV),
                                overloads=torch.full((S + 1, n_pairs), 77, dtype=torch.int32, device=DEV),
                                base_flow=torch.full((S + 1, e), guard, dtype=torch.float64, device=DEV),
                                status=torch.full((S + 1,), 99, dtype=torch.int32, device=DEV), flags=torch.zeros(1, dtype=torch.int32, device=DEV),
                                guard=guard)
    out.rc = lib.pfn_contingency_pairs_sparse(ei.data_ptr(), e, rx.data_ptr(), bt.data_ptr(), spec.data_ptr(), None, 0, lines.data_ptr(), c,
                                              isl.data_ptr(), S, n, n_pv, n_pq, C.c_double(TOL), MAX_ITER, out.severity.data_ptr(),
                                              out.worst_line.data_ptr(), out.overloads.data_ptr(), out.base_flow.data_ptr(), out.status.data_ptr(), None,
                                              out.flags.data_ptr(), ws.data_ptr(), need, header, plan.blob.data_ptr(), 0, 0, 0, 0, 0, L.stream_ptr())
    torch.cuda.synchronize()
    return out


def test_failures_stay_local():
    n, e = 14, 20
    case = _case(n, e, 6)
    clean = _screen(case, keep_table=True)
    spec, rx = case.spec.copy(), case.rx.copy()
    spec[1, 5, 2] = np.nan                                                  # scenario 1: a NaN in P
    rx[4, 8, 1] = 0.0                                                       # scenario 4: x = 0 on a line
    res = _screen(case, spec=spec, rx=rx, keep_table=True)
    status = res.status.tolist()
    assert [status[1], status[4]] == [-3, -3] and int(res.flags.item()) == 0
    _base_is_the_single_screens(res, _single(case, spec=spec, rx=rx))
    for s in (1, 4):                                                        # float outputs NaN, integer outputs -1: islanding pairs too
        assert torch.isnan(res.severity[s]).all() and torch.isnan(res.base_flow[s]).all() and torch.isnan(res.post_flow[s]).all()
        assert bool((res.worst_line[s] == -1).all()) and bool((res.overloads[s] == -1).all())
    keep = [0, 2, 3, 5]
    assert _same(res, clean, rows_a=keep, rows_b=keep) and bool((clean.status >= 0).all())
    # a bus without a line in the base grid (the plan is that grid's): singular, everywhere; the islands count it under every pair
    lonely = np.where(case.ei == 13, 1, case.ei)
    lonely_plan = sparse_plan(torch.from_numpy(case.bt), torch.from_numpy(lonely), mode="dc", device=DEV)
    res = _screen(case, ei=lonely, plan=lonely_plan, keep_table=True)
    assert res.status.tolist() == [-2] * 6 and bool((res.islands >= 1).all())
    assert torch.isnan(res.severity).all() and torch.isnan(res.base_flow).all() and torch.isnan(res.post_flow).all() and bool((res.overloads == -1).all())
    # a plan built from another line list of the same size: stale, everywhere
    other = case.ei.copy()
    other[1, 7] = next(b for b in range(n) if b not in (other[0, 7], other[1, 7]))
    res = _screen(case, plan=sparse_plan(torch.from_numpy(case.bt), torch.from_numpy(other), mode="dc", device=DEV))
    assert res.status.tolist() == [-6] * 6 and int(res.flags.item()) == 0 and torch.isnan(res.severity).all() and bool((res.worst_line == -1).all())
    # a line to bus id n: -4 on every pair and every scenario
    far = case.ei.copy()
    far[1, 7] = n
    res = _screen(case, ei=far)
    assert res.status.tolist() == [-4] * 6 and res.islands.tolist() == [-4] * 190 and torch.isnan(res.severity).all() and bool((res.worst_line == -1).all())
    # counts that contradict bus_type: -5 and the flag, nothing beyond the scenarios' rows is written
    n_pv, n_pq = int((case.bt == 1).sum()), int((case.bt == 2).sum())
    raw = _raw_pairs(case, _plan(n, e, 6), n_pv + 1, n_pq - 1, 6)
    assert raw.rc == 0 and int(raw.flags.item()) & 1 and raw.status[:6].tolist() == [-5] * 6
    assert torch.isnan(raw.severity[:6]).all() and torch.isnan(raw.base_flow[:6]).all() and bool((raw.worst_line[:6] == -1).all())
    assert bool((raw.severity[6] == raw.guard).all()) and bool((raw.base_flow[6] == raw.guard).all())
    assert bool((raw.worst_line[6] == 77).all()) and bool((raw.overloads[6] == 77).all()) and int(raw.status[6]) == 99
    good = _raw_pairs(case, _plan(n, e, 6), n_pv, n_pq, 6)                  # (the same call with the right counts runs)
    assert good.rc == 0 and int(good.flags.item()) == 0 and bool((good.status[:6] >= 0).all()) and int(good.status[6]) == 99
    assert bool((good.severity[:6] != good.guard).all()) and bool((good.severity[6] == good.guard).all()) and bool((good.worst_line[6] == 77).all())


# --------------------------------------------------------------------------------------------------------- capture
def test_the_four_launches_are_capturable():
    case = _case(14, 20, 4)
    ratings = _dev(1.2 * np.abs(_yard(14, 20, 4)[4]).max(axis=0))
    bt, spec, ei, rx = _dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx)
    lines = list(_candidates(case, 7))
    kw = dict(lines=lines, tol=TOL, max_iter=MAX_ITER, keep_table=True, route="sparse", plan=_plan(14, 20, 4))
    for block, columns in PLACEMENTS:
        eager = contingency_screen_pairs(bt, spec, ei, rx, ratings, block=block, columns=columns, **kw)   # (also: the host read, the upload)
        torch.cuda.synchronize()
        g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                res = contingency_screen_pairs(bt, spec, ei, rx, ratings, block=block, columns=columns, **kw)
        for _ in range(2):
            for t in (res.severity, res.base_flow, res.post_flow):
                t.fill_(-7.0)
            for t in (res.worst_line, res.overloads, res.status, res.islands):
                t.fill_(99)
            g.replay()
            torch.cuda.synchronize()
            assert _same(res, eager) and bool((res.status >= 0).all())


# ---------------------------------------------------------------------------------------------------------- verify
def test_verify_on_the_sparse_solver_agrees_with_the_dense_route():
    n, e, S = 14, 20, 2
    case = _case(n, e, S)
    pairs, isl, want, norm, f = _yard(n, e, S)
    ratings = 1.2 * np.abs(f).max(axis=0)
    res = _screen(case, ratings=ratings)
    args = (_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), _dev(ratings))
    dense = verify_pair_contingencies(res, *args, top=3, tol=TOL, max_iter=MAX_ITER)
    sparse = verify_pair_contingencies(res, *args, top=3, tol=TOL, max_iter=MAX_ITER, route="sparse")     # builds ONE cover plan itself
    assert sparse.triples.tolist() == dense.triples.tolist() and len(dense.triples) == 6 and sparse.status.tolist() == dense.status.tolist()
    assert all(1 <= st <= MAX_ITER for st in sparse.status.tolist()) and (isl[sparse.pair_index.cpu().numpy()] == 0).all()
    assert torch.equal(_bits(sparse.dc_severity), _bits(dense.dc_severity)) and sparse.worst_line.tolist() == dense.worst_line.tolist()
    worst_f = worst_x = 0.0
    for t, (s, a, b) in enumerate(sparse.triples.tolist()):
        keep = (np.arange(e) != a) & (np.arange(e) != b)
        ei, rx = np.ascontiguousarray(case.ei[:, keep]), np.ascontiguousarray(case.rx[s][keep])
        ref, st, _ = P.newton(case.bt, case.spec[s], ei, rx, tol=TOL, max_iter=MAX_ITER)
        assert 1 <= st <= MAX_ITER
        reduced = types.SimpleNamespace(ei=ei, rx=rx[None], bt=case.bt, spec=case.spec[s:s + 1])
        for ver in (sparse, dense):                                         # DESIGN 7h's Newton bounds, both routes
            table = ver.table[t].cpu().numpy()
            worst_f = max(worst_f, _residual_ratio(reduced, table[None]))
            worst_x = max(worst_x, float(_distance(table, ref) / (2 * TOL * P.jacobian_inverse_norm(ref, case.bt, ei, rx))))
        assert np.isnan(sparse.loading[t, [a, b]].cpu().numpy()).all() and bool(torch.isfinite(sparse.loading[t, torch.from_numpy(keep).to(DEV)]).all())
    print(f"verify pairs on the sparse route: worst |mismatch| / bound {worst_f:.3g}, worst |x - yardstick| / (2 tol ||J^-1||) {worst_x:.3g}")
    assert worst_f <= 1.0 and worst_x <= 1.0


# ---------------------------------------------------------------------------------------------------------- script
def test_the_script_screens_pairs_on_the_sparse_route(tmp_path, monkeypatch):
    import contingency
    monkeypatch.chdir(tmp_path)
    text = _run(contingency.main, ["--case", "118", "--route", "sparse", "--pairs", "--samples", "4"])
    assert "on the sparse route" in text and "N-2:" in text and text.count("on the sparse route") == 2 and "the DC pair screen called secure" in text
    pairs = np.load(tmp_path / "results" / "case118_contingency_pairs_pairs.npy")
    n_pairs = len(pairs)
    assert pairs.dtype == np.int64 and pairs.shape == (n_pairs, 2) and n_pairs >= 45 and (pairs[:, 0] < pairs[:, 1]).all()
    shapes = {"severity": ((4, n_pairs), np.float32), "worst_line": ((4, n_pairs), np.int32), "overloads": ((4, n_pairs), np.int32),
              "islands": ((n_pairs,), np.int32)}
    for name, (shape, dtype) in shapes.items():
        a = np.load(tmp_path / "results" / f"case118_contingency_pairs_{name}.npy")
        assert a.shape == shape and a.dtype == dtype, name
