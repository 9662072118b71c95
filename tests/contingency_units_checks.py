"""What the GPU tests of the generator-outage screen (test_gpu_contingency_units.py) share: the yardstick of a case, computed once
(tests/contingency_units_ref.py: `spec` literally edited -- and the line deleted -- and the DC model solved again in float64), the
call, and the bounds.

  base flow   the N-1 screen's bound (DESIGN 7h carried to a line): |f - f64| <= 4 tol ||B'^-1||_inf / |x_l| + 64 * 2^-52 |f64|;
  units       for every unit g and every line l:  |dev - f64| <= C_BOUND * u_g,
              u_g = 2^-24 max(max_l |f_l|, max_l (|d_g[a]| + |d_g[b]|) / |x_l|): the kernel adds (d_g[a] - d_g[b]) / x_l to the base flow
              in fp32, d_g from its fp32 inverse of B' -- a few roundings of the larger of the two terms;
  unit x line for every unit g, every non-bridge candidate k and every line l:  |dev - f64| <= C_BOUND * u_{g,k},
              u_{g,k} = 2^-24 max(max_l |f_l^(g)|, the same d term) / |den_k|: the N-1 screen's amplification on the post-unit flows;
              f, f^(g), d_g and den_k are the yardstick's;
  figures     severity, worst line and overload count are bit-exact functions of the kernel's own table and the fp32 ratings; the
              worst line is the yardstick's wherever its top two loadings differ by more than 2 C u.

Worst ratios |dev - f64| / u measured on an MI355X (each test prints its own): WORST below, (units, unit x line) per shape (n, e) --
the four flow shapes, both sides of the 256 | 1024-thread threshold (m = 90 | 91), both sides of the LDS boundary and (200, 300) on
the global route.  C_BOUND is the smallest power of two >= 4 x the worst of them, the N-1 screen's rule and margin."""
import functools
import types

import numpy as np
import torch

from poweflownet_amd.utils.contingency import contingency_screen_units
from tests import contingency_ref as R
from tests import contingency_units_ref as U
from tests import powerflow_ref as P
from tests.powerflow_checks import TOL, _dev
from tests.test_gpu_powerflow import _case

MAX_ITER = 10
EPS = 2.0 ** -24
WORST = {(5, 6): (1.89, 3.76), (14, 20): (4.69, 6.96), (70, 100): (4.99, 7.16), (118, 186): (9.22, 10.8), (91, 136): (2.71, 2.56),
         (92, 138): (2.99, 3.62), (184, 276): (9.28, 13.1), (185, 277): (12.6, 15.1), (200, 300): (8.75, 6.84)}    # (n, e): (units, unit x line)
C_BOUND = 64.0
assert C_BOUND == 2.0 ** np.ceil(np.log2(4 * max(max(v) for v in WORST.values())))


def units_of(case, name="graded participation"):
    """(units, p, a) of a case: tests/contingency_units_ref.unit_cases; from 70 buses on every fifth PV bus only (the yardstick solves
    the DC model once per (unit, line))"""
    units, p, a = U.unit_cases(case.bt)[name]
    if case.n >= 70:
        n_pv = int((case.bt == 1).sum())
        keep = np.concatenate([np.arange(0, n_pv, 5), np.arange(n_pv, len(units))])
        units, p, a = units[keep], p[keep], None if a is None else a[keep]
    return units, p, a


def lines_of(case, lines):
    """the candidate lines of a test: "all", or every `lines`-th line"""
    return list(range(case.e)) if lines == "all" else list(range(0, case.e, lines))


@functools.lru_cache(maxsize=None)
def yard(n, e, S, name="graded participation", lines="all"):
    """the yardstick of a case, once: islands [e], base flows [S, e], ||B'^-1||_inf [S], the literal post-unit flows [S, G, e], the
    closed form's d [S, G, n], the literal unit x line flows [S, G, c, e] and den [S, c]"""
    case = _case(n, e, S)
    units, p, a = units_of(case, name)
    cand = lines_of(case, lines)
    y = types.SimpleNamespace(units=units, p=p, a=a, lines=np.array(cand))
    y.isl = R.islands(case.bt, case.ei)
    y.f = np.stack([R.base_flow(case.bt, case.spec[s], case.ei, case.rx[s]) for s in range(S)])
    y.inv = np.array([P.dc_solve(case.bt, case.spec[s], case.ei, case.rx[s])[1] for s in range(S)])
    y.post = np.stack([U.resolve_units(case.bt, case.spec[s], case.ei, case.rx[s], units, p, a) for s in range(S)])
    closed = [U.closed_form(case.bt, case.spec[s], case.ei, case.rx[s], units, p, a) for s in range(S)]
    y.d = np.stack([d for _, d in closed])
    y.post2 = np.stack([U.resolve_unit_lines(case.bt, case.spec[s], case.ei, case.rx[s], units, p, a, cand, y.isl) for s in range(S)])
    y.den = np.stack([U.closed_form_lines(case.bt, case.ei, case.rx[s], closed[s][0], cand)[1] for s in range(S)])
    ok = y.isl[y.lines] == 0
    assert ok.any() and np.abs(y.den[:, ok]).min() >= 0.05, (n, e)           # no near-singular outage: nothing needs excluding
    assert (~ok).any(), (n, e)                                               # ... and a bridge among the candidates: its rows are checked
    return y


def screen(case, y, rows=slice(None), ratings=None, lines="yard", p=None, a="yard", units=None, spec=None, rx=None, ei=None, **kw):
    """`contingency_screen_units` on the case with the yardstick's units, outputs, factors and lines unless the call names its own"""
    kw = {"tol": TOL, "max_iter": MAX_ITER, **kw}
    a = y.a if isinstance(a, str) else a
    return contingency_screen_units(_dev(case.bt), _dev((case.spec if spec is None else spec)[rows]), _dev(case.ei if ei is None else ei),
                                    _dev((case.rx if rx is None else rx)[rows]), None if ratings is None else _dev(ratings),
                                    units=[int(b) for b in (y.units if units is None else units)], unit_p=_dev(y.p if p is None else p),
                                    participation=None if a is None else _dev(a), lines=[int(k) for k in y.lines] if lines == "yard" else lines,
                                    **kw)


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


UNIT_FIELDS = ("severity", "worst_line", "overloads", "base_flow", "status")
LINE_FIELDS = ("line_severity", "line_worst_line", "line_overloads")


def same(a, b, rows_a=slice(None), rows_b=slice(None), table=True, lines=True):
    """two results agree bit for bit on the given scenario rows (NaN bits included)"""
    names = list(UNIT_FIELDS) + (["post_flow"] if table else [])
    if lines:
        names += list(LINE_FIELDS) + (["line_post_flow"] if table else [])
    return all(torch.equal(bits(getattr(a, k)[rows_a]), bits(getattr(b, k)[rows_b])) for k in names)


def check_flows(case, y, res, what, ratings=None):
    """status, base flows, both flow bounds, the bridge rows and the worst lines of a result with its tables against the yardstick;
    returns the two worst ratios"""
    S, e, G, c = case.S, case.e, len(y.units), len(y.lines)
    status, base = res.status.cpu().numpy(), res.base_flow.cpu().numpy()
    post, post2 = res.post_flow.cpu().numpy(), res.line_post_flow.cpu().numpy()
    sev, worst, over = res.severity.cpu().numpy(), res.worst_line.cpu().numpy(), res.overloads.cpu().numpy()
    sev2, worst2, over2 = res.line_severity.cpu().numpy(), res.line_worst_line.cpu().numpy(), res.line_overloads.cpu().numpy()
    assert ((status >= 0) & (status <= MAX_ITER)).all() and int(res.flags.item()) == 0, (what, status)
    assert post.shape == (S, G, e) and post2.shape == (S, G, c, e) and post.dtype == post2.dtype == sev.dtype == sev2.dtype == np.float32
    assert res.units.tolist() == y.units.tolist() and res.lines.tolist() == y.lines.tolist()
    assert np.array_equal(res.islands.cpu().numpy(), y.isl[y.lines]) and np.array_equal(res.unit_p.cpu().numpy(), np.broadcast_to(y.p, (S, G)))
    isl_c = y.isl[y.lines]
    bridge, ok = isl_c > 0, isl_c == 0
    r = np.ones(e) if ratings is None else np.asarray(ratings, dtype=np.float64)
    rmin = r[r > 0].min() if (r > 0).any() else 1.0
    worst_base = ratio_units = ratio_lines = 0.0
    for s in range(S):
        x = np.abs(case.rx[s, :, 1])
        bound = 4 * TOL * y.inv[s] / x + 64 * P.EPS64 * np.abs(y.f[s])
        worst_base = max(worst_base, float((np.abs(base[s] - y.f[s]) / bound).max()))
        dterm = ((np.abs(y.d[s][:, case.ei[0]]) + np.abs(y.d[s][:, case.ei[1]])) / x[None, :]).max(axis=1)      # [G]
        u = EPS * np.maximum(np.abs(y.f[s]).max(), dterm)                   # [G]
        assert np.array_equal(u, EPS * U.unit_scale(y.f[s], y.d[s], case.ei, case.rx[s]))
        ratio_units = max(ratio_units, float((np.abs(post[s].astype(np.float64) - y.post[s]) / u[:, None]).max()))
        with np.errstate(divide="ignore"):
            u2 = EPS * np.maximum(np.abs(y.post[s]).max(axis=1), dterm)[:, None] / np.abs(y.den[s])[None, :]    # [G, c]
        ratio_lines = max(ratio_lines, float((np.abs(post2[s][:, ok].astype(np.float64) - y.post2[s][:, ok]) / u2[:, ok][:, :, None]).max()))
        assert (post2[s][:, np.arange(c), y.lines][:, ok] == 0).all()
        # an islanding line: +inf, -1, -1 and a NaN row under every unit
        assert np.isnan(post2[s][:, bridge]).all() and (sev2[s][:, bridge] == np.inf).all() and (worst2[s][:, bridge] == -1).all()
        assert (over2[s][:, bridge] == -1).all()
        # the worst line is the yardstick's wherever the yardstick's top two loadings differ by more than 2 C u
        want_sev, want_worst, _ = U.summarise_units(y.post[s], ratings)
        for g in range(G):
            if want_worst[g] >= 0:
                if U.top_two_gap(y.post[s][g], ratings) > 2 * C_BOUND * u[g] / r[want_worst[g]]:
                    assert worst[s, g] == want_worst[g], (what, s, g)
                assert abs(sev[s, g] - want_sev[g]) <= C_BOUND * u[g] / rmin + EPS * want_sev[g], (what, s, g)
            want_sev2, want_worst2, _ = U.summarise_unit_lines(y.post2[s][g], ratings, y.isl, y.lines)
            for j in np.flatnonzero(ok):
                if want_worst2[j] >= 0:
                    if U.top_two_gap(y.post2[s][g, j], ratings, skip=y.lines[j]) > 2 * C_BOUND * u2[g, j] / r[want_worst2[j]]:
                        assert worst2[s, g, j] == want_worst2[j], (what, s, g, j)
                    assert abs(sev2[s, g, j] - want_sev2[j]) <= C_BOUND * u2[g, j] / rmin + EPS * want_sev2[j], (what, s, g, j)
    print(f"{what}: route {res.route}, {G} units, {c} lines, solves {status.min()}..{status.max()}, worst |base flow - f64| / bound {worst_base:.3g}, "
          f"worst |post flow - f64| / u {ratio_units:.3g} (units) {ratio_lines:.3g} (unit x line) (C = {C_BOUND:g})")
    assert worst_base <= 1.0 and ratio_units <= C_BOUND and ratio_lines <= C_BOUND, (what, worst_base, ratio_units, ratio_lines)
    return ratio_units, ratio_lines


def _equal_bits(got, want):
    fin = ~np.isnan(want)
    return want.dtype == np.float32 and np.array_equal(np.isnan(got), ~fin) and np.array_equal(got[fin].view(np.uint32), want[fin].view(np.uint32))


def recompute(res, ratings, S, isl):
    """severity, worst line and overload count again from the kernel's own tables in numpy fp32: bit for bit"""
    post, post2 = res.post_flow.cpu().numpy(), None if res.line_post_flow is None else res.line_post_flow.cpu().numpy()
    lines = None if res.lines is None else res.lines.cpu().numpy()
    for s in range(S):
        r = None if ratings is None else (ratings if ratings.ndim == 1 else ratings[s])
        sev, worst, over = U.summarise_units(post[s], r, dtype=np.float32)
        assert _equal_bits(res.severity[s].cpu().numpy(), sev), s
        assert np.array_equal(res.worst_line[s].cpu().numpy(), worst) and np.array_equal(res.overloads[s].cpu().numpy(), over), s
        for g in range(post.shape[1] if post2 is not None else 0):
            sev, worst, over = U.summarise_unit_lines(post2[s, g], r, isl, lines, dtype=np.float32)
            assert _equal_bits(res.line_severity[s, g].cpu().numpy(), sev), (s, g)
            assert np.array_equal(res.line_worst_line[s, g].cpu().numpy(), worst) and np.array_equal(res.line_overloads[s, g].cpu().numpy(), over), (s, g)
