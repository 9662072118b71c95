"""The sparse route of the N-1 line-outage screen on the device: `pfn_contingency_sparse` (csrc/contingency_sparse.hip) through
`contingency_screen(route="sparse", plan=sparse_plan(..., mode="dc"))`, held to the float64 yardstick of tests/contingency_ref.py --
the literal re-solve up to (118, 186), its float64 `lodf` form beyond (tests/test_contingency_host.py holds the two together).  Inputs
are `_case(n, e, S)` with seed 1; every test asserts on the yardstick that its grid has a bridge and that no non-bridge outage is
near-singular (min |den| >= 0.05), so nothing needs excluding.

  islands     equal to the yardstick's, exactly;
  base flow   DESIGN 7t's bound: |f - f64| <= 4 tol ||B'^-1||_inf / |x_l| + 64 * 2^-52 |f64|;
  flows       for every non-bridge outage k and every line l:  |dev - f64| <= C_BOUND * u_k,  u_k = 2^-24 max_l |f_l| / |den_k|, den_k the
              yardstick's;
  worst line  the yardstick's wherever its top two loadings differ by more than 2 C u;
  reductions  severity, worst line and overload count are bit-exact functions of the kernel's own table and the fp32 ratings;
  the rest    tile edges, both block placements, both sides of the LDS-block threshold, bit-for-bit independence of the batch, the
              grid size, the base threads and the placement, failures that stay local, graph capture, the AC verification on the
              sparse solver, the script.

Worst flow ratios |dev - f64| / u measured on an MI355X (each test prints its own; WORST below, DESIGN.md section 7v, beside the dense
screen's at the same shapes): 0.19 at (3, 3), 2.85 at (5, 6), 1.13 at (14, 20), 1.63 at (70, 100), 2.09 at (118, 186); at the tile edges
1.76, 1.58, 2.15; 2.69 at (636, 954), the largest block in LDS, 2.77 at (637, 955), 2.49 at (1100, 1530) -- the same on both block
placements, which give the same bits.  C_BOUND = 16 is the smallest power of two >= 4 x the worst of them (4 x 2.85 = 11.4), DESIGN
7t's rule and margin.  Base flows: at most 6.2e-5 of their bound."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.utils.contingency import contingency_screen, verify_contingencies
from poweflownet_amd.utils.powerflow import cover_plan, sparse_plan
from tests import contingency_ref as R
from tests import powerflow_ref as P
from tests.powerflow_checks import DEV, TOL, _dev, _distance, _residual_ratio, _run
from tests.test_gpu_contingency import C_BOUND as C_DENSE
from tests.test_gpu_contingency import _bits, _recompute, _same
from tests.test_gpu_powerflow import _case

pytestmark = pytest.mark.gpu
MAX_ITER = 10
EPS = 2.0 ** -24
# worst |dev - f64| / u measured on an MI355X per shape (n, e): the figures C_BOUND was set from (the dense screen's at the five flow
# shapes, tests/test_gpu_contingency.py: 0.52, 3.8, 3.7, 7.1, 10.8)
WORST = {(3, 3): 0.19, (5, 6): 2.85, (14, 20): 1.13, (70, 100): 1.63, (118, 186): 2.09, (40, 63): 1.76, (40, 64): 1.58, (40, 65): 2.15,
         (636, 954): 2.69, (637, 955): 2.77, (1100, 1530): 2.49}
C_BOUND = 16.0
assert C_BOUND == 2.0 ** np.ceil(np.log2(4 * max(WORST.values())))
LITERAL_UP_TO = 118                                                         # buses: the literal re-solve up to here, `lodf` beyond


@functools.lru_cache(maxsize=None)
def _yard(n, e, S):
    """(islands [e], float64 post-outage flows [S, e, e], den [S, e], base flows [S, e], ||B'^-1||_inf [S]) of the yardstick, once"""
    case = _case(n, e, S)
    isl = R.islands(case.bt, case.ei)
    both = [R.lodf(case.bt, case.spec[s], case.ei, case.rx[s]) for s in range(S)]
    den = np.stack([d for _, d in both])
    if n <= LITERAL_UP_TO:
        want = np.stack([R.resolve(case.bt, case.spec[s], case.ei, case.rx[s], isl) for s in range(S)])
    else:
        want = np.stack([p for p, _ in both])
        want[:, isl > 0] = np.nan
    f = np.stack([R.base_flow(case.bt, case.spec[s], case.ei, case.rx[s]) for s in range(S)])
    inv = np.array([P.dc_solve(case.bt, case.spec[s], case.ei, case.rx[s])[1] for s in range(S)])
    assert (isl > 0).any() and (isl == 0).any() and np.abs(den[:, isl == 0]).min() >= 0.05, (n, e)
    return isl, want, den, f, inv


@functools.lru_cache(maxsize=None)
def _plan(n, e, S=1):
    case = _case(n, e, S)
    return sparse_plan(torch.from_numpy(case.bt), torch.from_numpy(case.ei), mode="dc", device=DEV)


def _screen(case, rows=slice(None), ratings=None, ei=None, plan=None, **kw):
    kw = {"tol": TOL, "max_iter": MAX_ITER, "route": "sparse", "plan": _plan(case.n, case.e, case.S) if plan is None else plan, **kw}
    return contingency_screen(_dev(case.bt), _dev(case.spec[rows]), _dev(case.ei if ei is None else ei), _dev(case.rx[rows]),
                              None if ratings is None else _dev(ratings), **kw)


def _check_flows(case, res, what, ratings=None):
    """status, islands, base flows, the flow bound, the bridge rows and the worst line of a result with its table against the yardstick"""
    S, e = case.S, case.e
    isl, want, den, f, inv = _yard(case.n, case.e, case.S)
    status, base, post = res.status.cpu().numpy(), res.base_flow.cpu().numpy(), res.post_flow.cpu().numpy()
    sev, worst, over = res.severity.cpu().numpy(), res.worst_line.cpu().numpy(), res.overloads.cpu().numpy()
    assert res.route == "sparse" and ((status >= 0) & (status <= MAX_ITER)).all() and int(res.flags.item()) == 0, (what, status)
    assert np.array_equal(res.islands.cpu().numpy(), isl)
    assert post.shape == (S, e, e) and post.dtype == np.float32 and sev.dtype == np.float32 and base.dtype == np.float64
    bridge, ok = isl > 0, isl == 0
    worst_base = worst_ratio = 0.0
    for s in range(S):
        bound = 4 * TOL * inv[s] / np.abs(case.rx[s, :, 1]) + 64 * P.EPS64 * np.abs(f[s])
        worst_base = max(worst_base, float((np.abs(base[s] - f[s]) / bound).max()))
        with np.errstate(divide="ignore"):
            u = EPS * np.abs(f[s]).max() / np.abs(den[s])                  # [e], per outage (a bridge's is not used)
        ratio = np.abs(post[s][ok].astype(np.float64) - want[s][ok]) / u[ok][:, None]
        worst_ratio = max(worst_ratio, float(ratio.max()))
        assert (post[s][np.arange(e), np.arange(e)][ok] == 0).all()
        # an islanding outage: +inf, -1, -1 and a NaN row
        assert np.isnan(post[s][bridge]).all() and (sev[s][bridge] == np.inf).all() and (worst[s][bridge] == -1).all() and (over[s][bridge] == -1).all()
        # the worst line is the yardstick's wherever the yardstick's top two loadings differ by more than 2 C u
        want_sev, want_worst, _ = R.summarise(want[s], ratings, isl)
        r = np.ones(e) if ratings is None else np.asarray(ratings, dtype=np.float64)
        for k in np.flatnonzero(ok):
            if want_worst[k] >= 0 and R.top_two_gap(want[s], ratings, k) > 2 * C_BOUND * u[k] / r[want_worst[k]]:
                assert worst[s, k] == want_worst[k], (what, s, k)
            if want_worst[k] >= 0:
                assert abs(sev[s, k] - want_sev[k]) <= C_BOUND * u[k] / r[r > 0].min() + EPS * want_sev[k], (what, s, k)
    print(f"{what}: block {res.block}, solves {status.min()}..{status.max()}, worst |base flow - f64| / bound {worst_base:.3g}, "
          f"worst |post flow - f64| / u {worst_ratio:.3g} (C = {C_BOUND:g})")
    assert worst_base <= 1.0 and worst_ratio <= C_BOUND, (what, worst_base, worst_ratio)
    return worst_ratio


# -------------------------------------------------------------------------------------------------------- flows
@pytest.mark.parametrize("block", ["lds", "global"])
@pytest.mark.parametrize("n,e,S", [(3, 3, 2), (5, 6, 3), (14, 20, 8), (70, 100, 2), (118, 186, 2)])
def test_flows_against_removing_the_line(n, e, S, block):
    case = _case(n, e, S)
    res = _screen(case, keep_table=True, block=block)
    assert res.block == block
    _check_flows(case, res, f"n {n} e {e} S {S}")
    _recompute(res, None, S)


@pytest.mark.parametrize("block", ["lds", "global"])
@pytest.mark.parametrize("e", [63, 64, 65])
def test_tile_edges(e, block):
    """a partial tile, exactly one tile, a full tile plus a one-lane tile"""
    case = _case(40, e, 2)
    res = _screen(case, keep_table=True, block=block)
    _check_flows(case, res, f"n 40 e {e} S 2")
    _recompute(res, None, 2)


# ------------------------------------------------------------------------------------------ beyond the dense cap
def test_beyond_the_dense_cap():
    case = _case(1100, 1530, 1)
    with pytest.raises(RuntimeError, match="dense"):
        contingency_screen(_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), tol=TOL, max_iter=MAX_ITER)
    res = _screen(case, keep_table=True)
    assert res.block == "global"
    _check_flows(case, res, "n 1100 e 1530 S 1")
    _recompute(res, None, 1)


@pytest.mark.parametrize("which", ["largest in LDS", "one more"])
def test_both_sides_of_the_lds_block_threshold(which):
    n = {"largest in LDS": 636, "one more": 637}[which]
    case = _case(n, n + n // 2, 1)
    plan, lib = _plan(n, case.e), L.load()
    size = [int(lib.pfn_contingency_sparse_workspace_bytes(1, case.e, C.addressof(plan.header), route, 0)) for route in (0, 1, 2)]
    assert size[1] < size[2] and size[0] == (size[1] if which == "largest in LDS" else size[2])       # what "auto" takes, by its bytes
    res = _screen(case, keep_table=True)
    assert res.block == ("lds" if which == "largest in LDS" else "global")
    _check_flows(case, res, f"{which}: n {n} e {case.e}")
    _recompute(res, None, 1)
    if which == "one more":
        with pytest.raises(RuntimeError, match=r"code -1.*LDS"):
            _screen(case, block="lds")
    else:
        assert _same(_screen(case, keep_table=True, block="global"), res)


# ---------------------------------------------------------------------------------------------------------- bits
def test_bits_do_not_depend_on_groups_threads_or_placement():
    case = _case(70, 100, 4)
    ref = _screen(case, keep_table=True)
    assert ref.block == "lds" and bool((ref.status >= 0).all())
    for kw in ({"groups": 1}, {"groups": 2}, {"groups": 3}, {"threads": 64}, {"threads": 256}, {"block": "global"},
               {"block": "global", "groups": 3, "threads": 256}):
        assert _same(_screen(case, keep_table=True, **kw), ref), kw
    bare = _screen(case)                                                    # without the table: the same bits, no table
    assert bare.post_flow is None and _same(bare, ref, table=False)
    assert _same(_screen(case, groups=2, block="global"), ref, table=False)


def test_a_scenario_does_not_depend_on_its_batch():
    case = _case(14, 20, 8)
    ratings = 1.2 * np.abs(_yard(14, 20, 8)[3])                             # [S, e]
    whole = _screen(case, ratings=ratings, keep_table=True)
    assert bool((whole.status >= 0).all())
    a, b = _screen(case, slice(0, 4), ratings[:4], keep_table=True), _screen(case, slice(4, 8), ratings[4:], keep_table=True)
    assert _same(a, whole, rows_b=slice(0, 4)) and _same(b, whole, rows_b=slice(4, 8))
    one = _screen(case, slice(5, 6), ratings[5:6], keep_table=True)
    assert _same(one, whole, rows_b=slice(5, 6))


def test_reductions_are_exact_functions_of_the_table_and_the_ratings():
    n, e, S = 14, 20, 8
    case = _case(n, e, S)
    isl, want, den, f, inv = _yard(n, e, S)
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


# --------------------------------------------------------------------------------------------- the dense screen
def test_against_the_dense_screen():
    n, e, S = 118, 186, 2
    case = _case(n, e, S)
    isl, want, den, f, inv = _yard(n, e, S)
    sparse = _screen(case)
    dense = contingency_screen(_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), tol=TOL, max_iter=MAX_ITER)
    assert torch.equal(sparse.islands, dense.islands) and bool((sparse.status >= 0).all()) and bool((dense.status >= 0).all())
    a, b, sa, sb = (t.cpu().numpy() for t in (sparse.base_flow, dense.base_flow, sparse.severity, dense.severity))
    worst = 0.0
    for s in range(S):
        bound = 4 * TOL * inv[s] / np.abs(case.rx[s, :, 1]) + 64 * P.EPS64 * np.abs(f[s])
        assert (np.abs(a[s] - b[s]) <= 2 * bound).all()                    # each within its bound of the float64 solve
        ok = isl == 0
        u = EPS * np.abs(f[s]).max() / np.abs(den[s][ok])
        assert np.array_equal(sa[s][~ok], sb[s][~ok])
        worst = max(worst, float((np.abs(sa[s][ok].astype(np.float64) - sb[s][ok]) / ((C_DENSE + C_BOUND) * u + EPS * np.abs(sb[s][ok]))).max()))
    print(f"sparse against dense at (118, 186): worst |severity difference| / ((C_dense + C_sparse) u) {worst:.3g}")
    assert worst <= 1.0


# -------------------------------------------------------------------------------------------------------- failures
def _raw_sparse(case, plan, n_pv, n_pq, S):
    e, n = case.e, case.n
    bt, spec, ei, rx = _dev(case.bt.astype(np.int32)), _dev(case.spec), _dev(case.ei), _dev(case.rx)
    isl = torch.zeros(e, dtype=torch.int32, device=DEV)
    guard, lib, header = -7.5, L.load(), C.addressof(plan.header)
    need = int(lib.pfn_contingency_sparse_workspace_bytes(S, e, header, 0, 0))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = types.SimpleNamespace(severity=torch.full((S + 1, e), guard, dtype=torch.float32, device=DEV),
                                worst_line=torch.full((S + 1, e), 77, dtype=torch.int32, device=DEV), overloads=torch.full((S + 1, e), 77, dtype=torch.int32, device=DEV),
                                base_flow=torch.full((S + 1, e), guard, dtype=torch.float64, device=DEV), status=torch.full((S + 1,), 99, dtype=torch.int32, device=DEV),
                                flags=torch.zeros(1, dtype=torch.int32, device=DEV), guard=guard)
    out.rc = lib.pfn_contingency_sparse(ei.data_ptr(), e, rx.data_ptr(), bt.data_ptr(), spec.data_ptr(), None, 0, isl.data_ptr(), S, n, n_pv, n_pq,
                                        C.c_double(TOL), MAX_ITER, out.severity.data_ptr(), out.worst_line.data_ptr(), out.overloads.data_ptr(),
                                        out.base_flow.data_ptr(), out.status.data_ptr(), None, out.flags.data_ptr(), ws.data_ptr(), need, header,
                                        plan.blob.data_ptr(), 0, 0, 0, L.stream_ptr())
    torch.cuda.synchronize()
    return out


def test_failures_stay_local():
    n, e = 14, 20
    case = _case(n, e, 6)
    clean = _screen(case, keep_table=True)
    spec, rx = case.spec.copy(), case.rx.copy()
    spec[1, 5, 2] = np.nan                                                  # scenario 1: a NaN in P
    rx[4, 8, 1] = 0.0                                                       # scenario 4: x = 0 on a line
    res = contingency_screen(_dev(case.bt), _dev(spec), _dev(case.ei), _dev(rx), tol=TOL, max_iter=MAX_ITER, keep_table=True, route="sparse",
                             plan=_plan(n, e, 6))
    status = res.status.tolist()
    assert [status[1], status[4]] == [-3, -3] and int(res.flags.item()) == 0
    for s in (1, 4):                                                        # float outputs NaN, integer outputs -1: bridges too
        assert torch.isnan(res.severity[s]).all() and torch.isnan(res.base_flow[s]).all() and torch.isnan(res.post_flow[s]).all()
        assert bool((res.worst_line[s] == -1).all()) and bool((res.overloads[s] == -1).all())
    keep = [0, 2, 3, 5]
    assert _same(res, clean, rows_a=keep, rows_b=keep) and bool((clean.status >= 0).all())
    # a bus without a line in the base grid (the plan is that grid's): singular, everywhere; the islands count it under every outage
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
    # a line to bus id n: -4 everywhere, islands included
    far = case.ei.copy()
    far[1, 7] = n
    res = _screen(case, ei=far)
    assert res.status.tolist() == [-4] * 6 and res.islands.tolist() == [-4] * e and torch.isnan(res.severity).all() and bool((res.worst_line == -1).all())
    # counts that contradict bus_type: -5 and the flag, nothing beyond the scenarios' rows is written
    n_pv, n_pq = int((case.bt == 1).sum()), int((case.bt == 2).sum())
    raw = _raw_sparse(case, _plan(n, e, 6), n_pv + 1, n_pq - 1, 6)
    assert raw.rc == 0 and int(raw.flags.item()) & 1 and raw.status[:6].tolist() == [-5] * 6
    assert torch.isnan(raw.severity[:6]).all() and torch.isnan(raw.base_flow[:6]).all() and bool((raw.worst_line[:6] == -1).all())
    assert bool((raw.severity[6] == raw.guard).all()) and bool((raw.base_flow[6] == raw.guard).all())
    assert bool((raw.worst_line[6] == 77).all()) and bool((raw.overloads[6] == 77).all()) and int(raw.status[6]) == 99
    good = _raw_sparse(case, _plan(n, e, 6), n_pv, n_pq, 6)                 # (the same call with the right counts runs)
    assert good.rc == 0 and int(good.flags.item()) == 0 and bool((good.status[:6] >= 0).all()) and int(good.status[6]) == 99
    assert bool((good.severity[6] == good.guard).all()) and bool((good.worst_line[6] == 77).all())


# --------------------------------------------------------------------------------------------------------- capture
def test_the_three_launches_are_capturable():
    case = _case(14, 20, 8)
    ratings = _dev(1.2 * np.abs(_yard(14, 20, 8)[3]).max(axis=0))
    bt, spec, ei, rx = _dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx)
    kw = {"tol": TOL, "max_iter": MAX_ITER, "keep_table": True, "route": "sparse", "plan": _plan(14, 20, 8)}
    for block in ("lds", "global"):
        eager = contingency_screen(bt, spec, ei, rx, ratings, block=block, **kw)                            # (also: the one host read)
        torch.cuda.synchronize()
        g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                res = contingency_screen(bt, spec, ei, rx, ratings, block=block, **kw)
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
    isl, want, den, f, inv = _yard(n, e, S)
    ratings = 1.2 * np.abs(f).max(axis=0)
    res = _screen(case, ratings=ratings)
    args = (_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), _dev(ratings))
    dense = verify_contingencies(res, *args, top=3, tol=TOL, max_iter=MAX_ITER)
    sparse = verify_contingencies(res, *args, top=3, tol=TOL, max_iter=MAX_ITER, route="sparse")           # builds ONE cover plan itself
    given = cover_plan(_dev(case.bt), _dev(case.ei)[None], mode="ac", base=_dev(case.ei))
    again = verify_contingencies(res, *args, top=3, tol=TOL, max_iter=MAX_ITER, route="sparse", plan=given)  # ... or reuses the caller's
    assert given.e_cover == e and given.extras == 0
    assert sparse.pairs.tolist() == dense.pairs.tolist() and len(dense.pairs) == 6 and sparse.status.tolist() == dense.status.tolist()
    assert all(1 <= st <= MAX_ITER for st in sparse.status.tolist())
    assert torch.equal(again.table, sparse.table) and torch.equal(_bits(again.loading), _bits(sparse.loading))     # (NaN at the outaged line)
    worst_f = worst_x = 0.0
    for t, (s, k) in enumerate(sparse.pairs.tolist()):
        keep = np.arange(e) != k
        ei, rx = np.ascontiguousarray(case.ei[:, keep]), np.ascontiguousarray(case.rx[s][keep])
        ref, st, _ = P.newton(case.bt, case.spec[s], ei, rx, tol=TOL, max_iter=MAX_ITER)
        assert 1 <= st <= MAX_ITER
        reduced = types.SimpleNamespace(ei=ei, rx=rx[None], bt=case.bt, spec=case.spec[s:s + 1])
        for ver in (sparse, dense):                                         # DESIGN 7h's Newton bounds, both routes
            table = ver.table[t].cpu().numpy()
            worst_f = max(worst_f, _residual_ratio(reduced, table[None]))
            worst_x = max(worst_x, float(_distance(table, ref) / (2 * TOL * P.jacobian_inverse_norm(ref, case.bt, ei, rx))))
    print(f"verify on the sparse route: worst |mismatch| / bound {worst_f:.3g}, worst |x - yardstick| / (2 tol ||J^-1||) {worst_x:.3g}")
    assert worst_f <= 1.0 and worst_x <= 1.0


# ---------------------------------------------------------------------------------------------------------- script
def test_the_script_runs_end_to_end_on_the_sparse_route(tmp_path, monkeypatch):
    import contingency
    monkeypatch.chdir(tmp_path)
    text = _run(contingency.main, ["--case", "118", "--route", "sparse", "--samples", "4"])
    assert "on the sparse route" in text and "islanding outages" in text and "called secure" in text
    shapes = {"severity": ((4, 186), np.float32), "worst_line": ((4, 186), np.int32), "overloads": ((4, 186), np.int32), "islands": ((186,), np.int32),
              "base_flow": ((4, 186), np.float64)}
    for name, (shape, dtype) in shapes.items():
        a = np.load(tmp_path / "results" / f"case118_contingency_{name}.npy")
        assert a.shape == shape and a.dtype == dtype, name
    assert np.isfinite(np.load(tmp_path / "results" / "case118_contingency_base_flow.npy")).all()
