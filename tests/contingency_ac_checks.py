"""What the GPU tests of the AC N-1 screen (test_gpu_contingency_ac.py, the dense route; test_gpu_contingency_ac_sparse.py, the sparse
route) share: bit comparisons of two results, the float64 yardstick of tests/contingency_ac_ref.py started at the device's base state,
the check of a result with both tables against it, and the raw C entry with guarded outputs.  Both routes are held to the same
definitions, so the checks are one text; what a route measured itself -- `WORST`, the `C_BOUND` set from it, the placement it must
report -- stays with its test file, which passes `c_bound` in.  A `case` is test_gpu_powerflow's `_case(n, e, S)`."""
import ctypes as C
import types

import numpy as np
import torch

from poweflownet_amd import _lib as L
from tests import branch_ref as B
from tests import contingency_ac_ref as A
from tests import powerflow_ref as P
from tests.powerflow_checks import DEV, TOL, _dev

MAX_ITER = 60
EPS = 2.0 ** -24
_FIELDS = ("severity", "worst_line", "overloads", "vm_min", "vm_min_bus", "v_violations", "mismatch", "base_table", "status", "residual")


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b, rows_a=slice(None), rows_b=slice(None), tables=True):
    """two results agree bit for bit on the given scenario rows (NaN bits included)"""
    names = _FIELDS + (("post_current", "post_state") if tables else ())
    return all(torch.equal(_bits(getattr(a, k)[rows_a]), _bits(getattr(b, k)[rows_b])) for k in names) and torch.equal(a.islands, b.islands)


def _base_of(res, s):
    """(vm, theta) of scenario s of the device's base table"""
    t = res.base_table[s].cpu().numpy()
    return t[:, 0].copy(), t[:, 1] * P.RAD


def _base_currents(case, res):
    """[S, e] float64 currents of the device's base tables (the yardstick's arithmetic)"""
    t = res.base_table.cpu().numpy()
    return np.stack([A.currents(t[s, :, :2].astype(np.float32), case.ei, case.rx[s])[0] for s in range(case.S)])


def _all_failed(res, s):
    floats = (res.severity[s], res.vm_min[s], res.mismatch[s], res.base_table[s], res.post_current[s], res.post_state[s])
    ints = (res.worst_line[s], res.overloads[s], res.vm_min_bus[s], res.v_violations[s])
    return all(bool(torch.isnan(t).all()) for t in floats) and all(bool((t == -1).all()) for t in ints)


_YARD = {}


def _yard(case, res, variant, halves, tag=""):
    """(islands [e], states [S, e, n, 2] = (vm, theta) float64, mismatch [S, e], den [S, e] = min(|den'|, |den''|)) of the yardstick's
    compensated form started at the device's base state.  A pure function of the inputs and of that base state: computed once per
    shape and per ROUTE (the two routes' base solves differ in their last bits); `tag` tells apart runs of one route whose base
    differs, such as another start."""
    key = (case.n, case.e, case.S, variant, halves, case.m, res.route == "sparse", tag)
    if key not in _YARD:
        isl = A.islands(case.bt, case.ei)
        st = np.full((case.S, case.e, case.n, 2), np.nan)
        mis, den = np.full((case.S, case.e), np.nan), np.full((case.S, case.e), np.nan)
        for s in range(case.S):
            vm0, th0 = _base_of(res, s)
            inv = A.inverses(case.bt, case.ei, case.rx[s], variant)
            dp, dq = A.dens(case.bt, case.ei, case.rx[s], variant)
            den[s] = np.minimum(np.abs(dp), np.abs(dq))
            for k in np.flatnonzero(isl == 0):
                vm, th, mis[s, k] = A.outage_state(case.bt, case.spec[s], case.ei, case.rx[s], vm0, th0, k, halves, variant, "compensated", inv)
                st[s, k, :, 0], st[s, k, :, 1] = vm, th
        assert (isl == 0).any() and np.nanmin(den[:, isl == 0]) >= 0.05, (key, np.nanmin(den[:, isl == 0]))
        _YARD[key] = (isl, st, mis, den)
    return _YARD[key]


def _check(case, res, variant, halves, what, c_bound, ratings=None, limits=(0.9, 1.1), tag=""):
    """states, currents, mismatch, figures, bridges and the worst line of a result with both tables against the yardstick, the state
    under the route's `c_bound`; returns the worst state ratio"""
    S, n, e = case.S, case.n, case.e
    isl, want, want_mis, den = _yard(case, res, variant, halves, tag)
    status = res.status.cpu().numpy()
    assert ((status >= 0) & (status <= MAX_ITER)).all() and int(res.flags.item()) == 0, (what, status)
    assert np.array_equal(res.islands.cpu().numpy(), isl)
    state, cur = res.post_state.cpu().numpy(), res.post_current.cpu().numpy()
    assert state.shape == (S, e, n, 2) and state.dtype == np.float32 and cur.shape == (S, e, e) and cur.dtype == np.float32
    sev, worst, over = res.severity.cpu().numpy(), res.worst_line.cpu().numpy(), res.overloads.cpu().numpy()
    vmin, vbus, vviol, mis = (getattr(res, k).cpu().numpy() for k in ("vm_min", "vm_min_bus", "v_violations", "mismatch"))
    bridge, ok = isl > 0, isl == 0
    worst_ratio = worst_cur = worst_mis = 0.0
    y = 1.0 / np.hypot(case.rx[:, :, 0], case.rx[:, :, 1])                  # [S, e]: |y| of a line; a bus's line sums move by at most
    jscale = np.zeros(S)                                                    # 4 V^2 sum |y| per unit of (relative Vm, angle) deviation
    for s in range(S):
        per_bus = np.zeros(n)
        np.add.at(per_bus, case.ei[0], y[s])
        np.add.at(per_bus, case.ei[1], y[s])
        jscale[s] = 4 * 1.2 ** 2 * per_bus.max()
    slack = case.bt == 0
    for s in range(S):
        vm0, th0 = _base_of(res, s)
        r = None if ratings is None else (ratings if ratings.ndim == 1 else ratings[s])
        r64 = np.ones(e) if r is None else r.astype(np.float32).astype(np.float64)
        # an islanding outage: +inf, -1, -1, NaN voltage figures and mismatch, NaN rows
        assert np.isnan(cur[s][bridge]).all() and np.isnan(state[s][bridge]).all() and (sev[s][bridge] == np.inf).all()
        assert (worst[s][bridge] == -1).all() and (over[s][bridge] == -1).all() and np.isnan(vmin[s][bridge]).all() and np.isnan(mis[s][bridge]).all()
        assert (vbus[s][bridge] == -1).all() and (vviol[s][bridge] == -1).all()
        lit = np.full((e, e), np.nan)
        bound_rows = np.zeros((e, e))
        for k in np.flatnonzero(ok):
            dev_vm, dev_th = state[s, k, :, 0].astype(np.float64), state[s, k, :, 1].astype(np.float64) * P.RAD
            for dev_x, f64, base in ((dev_vm, want[s, k, :, 0], vm0), (dev_th, want[s, k, :, 1], th0)):
                u = EPS * np.abs(f64 - base).max() / den[s, k]
                excess = np.abs(dev_x - f64) - 2 * EPS * np.abs(f64)         # (the table's fp32 rounding; the angle's twice: degrees and back)
                if u > 0:
                    worst_ratio = max(worst_ratio, float(np.maximum(excess[~slack], 0).max() / u))
                else:
                    assert (excess <= 0).all(), (what, s, k)
            # the currents at the device's own state
            ref, scale = A.currents(state[s, k], case.ei, case.rx[s], k)
            keep = np.arange(e) != k
            assert np.isnan(cur[s, k, k]) and np.isfinite(cur[s, k, keep]).all()
            worst_cur = max(worst_cur, float((np.abs(cur[s, k, keep] - ref[keep]) / (B.C_BOUND * B.EPS * scale[keep])).max()))
            # the mismatch: the yardstick's up to what the state's deviation is worth in a bus's line sums
            dev_max = max(float(np.abs(dev_vm - want[s, k, :, 0]).max()), float(np.abs(dev_th - want[s, k, :, 1])[~slack].max()))
            worst_mis = max(worst_mis, abs(mis[s, k] - want_mis[s, k]) / (jscale[s] * dev_max + 1e-13))
            # the yardstick's loadings and what the two bounds are worth in loading
            st64 = A.state32(want[s, k, :, 0], want[s, k, :, 1], case.bt, case.spec[s])
            lit[k], sc = A.currents(st64, case.ei, case.rx[s], k)
            u_all = EPS * (np.abs(want[s, k, :, 0] - vm0).max() + np.abs(want[s, k, :, 1] - th0).max()) / den[s, k]
            bound_rows[k] = (B.C_BOUND * B.EPS * sc + sc * (c_bound * u_all + 4 * EPS)) / np.where(r64 > 0, r64, 1.0)
        # the figures again from the kernel's own tables in numpy fp32: bit for bit
        want_sev, want_worst, want_over = A.summarise(cur[s], r, isl, dtype=np.float32)
        fin = ~np.isnan(want_sev)
        assert np.array_equal(np.isnan(sev[s]), ~fin) and np.array_equal(sev[s][fin].view(np.uint32), want_sev[fin].view(np.uint32)), (what, s)
        assert np.array_equal(worst[s], want_worst) and np.array_equal(over[s], want_over), (what, s)
        for k in np.flatnonzero(ok):
            low, bus, count = A.voltage_figures(state[s, k, :, 0], case.bt, *limits)
            assert (np.isnan(low) and np.isnan(vmin[s, k])) or np.float32(low).view(np.uint32) == vmin[s, k].view(np.uint32), (what, s, k)
            assert bus == vbus[s, k] and count == vviol[s, k], (what, s, k)
        # the worst line is the yardstick's wherever the yardstick's top two loadings differ by more than twice the bound
        ysev, yworst, _ = A.summarise(lit, r, isl, dtype=np.float64)
        for k in np.flatnonzero(ok):
            mon = (r64 > 0) & (np.arange(e) != k)
            if yworst[k] < 0:
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                load = np.sort((lit[k] / r64)[mon])
            gap = load[-1] - load[-2] if load.size >= 2 else np.inf
            if gap > 2 * bound_rows[k][mon].max():
                assert worst[s, k] == yworst[k], (what, s, k)
            assert abs(sev[s, k] - ysev[k]) <= bound_rows[k][mon].max() + EPS * ysev[k], (what, s, k, sev[s, k], ysev[k])
    placed = f"block {res.block}" if res.route == "sparse" else f"placement {res.route}, {res.group} waves"
    print(f"{what}: {placed}, base halves {status.min()}..{status.max()}, min den {np.nanmin(den[:, ok]):.3g}, worst (|state - f64| - rounding) / u "
          f"{worst_ratio:.3g} (C = {c_bound:g}), worst |current - f64| / bound {worst_cur:.3g}, worst |mismatch - f64| / bound {worst_mis:.3g}")
    assert worst_cur <= 1.0 and worst_ratio <= c_bound and worst_mis <= 1.0, (what, worst_ratio, worst_cur, worst_mis)
    return worst_ratio


def _raw(case, n_pv, n_pq, S, plan=None, bt=None):
    """either C entry (`plan`: the sparse one, under that plan) with guarded outputs of S + 1 rows, two halves, "xb", every route
    option at its default"""
    e, n = case.e, case.n
    bt, spec, ei, rx = _dev((case.bt if bt is None else bt).astype(np.int32)), _dev(case.spec), _dev(case.ei), _dev(case.rx)
    isl = torch.zeros(e, dtype=torch.int32, device=DEV)
    guard = -7.5
    f32 = lambda *shape: torch.full(shape, guard, dtype=torch.float32, device=DEV)       # noqa: E731
    i32 = lambda *shape: torch.full(shape, 77, dtype=torch.int32, device=DEV)            # noqa: E731
    out = types.SimpleNamespace(severity=f32(S + 1, e), worst_line=i32(S + 1, e), overloads=i32(S + 1, e), vm_min=f32(S + 1, e), vm_min_bus=i32(S + 1, e),
                                v_violations=i32(S + 1, e), mismatch=torch.full((S + 1, e), guard, dtype=torch.float64, device=DEV),
                                table=torch.full((S + 1, n, 4), guard, dtype=torch.float64, device=DEV), status=i32(S + 1),
                                residual=torch.full((S + 1,), guard, dtype=torch.float64, device=DEV), flags=torch.zeros(1, dtype=torch.int32, device=DEV),
                                guard=guard)
    lib = L.load()
    if plan is None:
        entry, middle, need = lib.pfn_contingency_ac, (0, 0), int(lib.pfn_contingency_ac_workspace_bytes(S, n, e, n_pq))
    else:
        header = C.addressof(plan.header)
        entry, middle = lib.pfn_contingency_ac_sparse, (header, plan.blob.data_ptr(), 0, 0, 0)
        need = int(lib.pfn_contingency_ac_sparse_workspace_bytes(S, e, header, 0, 0))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out.rc = entry(ei.data_ptr(), e, rx.data_ptr(), bt.data_ptr(), spec.data_ptr(), None, None, 0, isl.data_ptr(), S, n, n_pv, n_pq, 0, 2, 0.9, 1.1,
                   C.c_double(TOL), MAX_ITER, *middle, out.severity.data_ptr(), out.worst_line.data_ptr(), out.overloads.data_ptr(),
                   out.vm_min.data_ptr(), out.vm_min_bus.data_ptr(), out.v_violations.data_ptr(), out.mismatch.data_ptr(), out.table.data_ptr(),
                   out.status.data_ptr(), out.residual.data_ptr(), None, None, out.flags.data_ptr(), ws.data_ptr(), need, L.stream_ptr())
    torch.cuda.synchronize()
    return out
