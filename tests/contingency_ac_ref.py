"""float64 numpy yardstick of the AC N-1 screen (csrc/contingency_ac.hip, `contingency_screen_ac`), written for the tests on top of
tests/powerflow_ref.py, tests/powerflow_fd_ref.py (`fd_matrices`, `_mismatch`, `start`, `newton_from`), tests/contingency_ref.py
(`islands`, `summarise`) and tests/branch_ref.py (`flows`).  One scenario at a time: bus_type [n], spec [n, 4], lines [2, e], rx
[e, 2].  The state after `halves` half-iterations of outage k comes in two forms that tests/test_contingency_ac_host.py holds
together without a GPU:

  literal      line k is deleted, B' and B'' are rebuilt over the reduced list and solved with (`np.linalg.solve`);
  compensated  the inverses X', X'' of the FULL list's matrices and the rank-1 correction the kernel applies,
               X_k g = X g + w (w . g) / (1 / c_k - a^T w),  a = e_i - e_j restricted to the matrix's buses, w = X a.

Half h forms the mismatch of the grid without line k at the current state; an even h (every h where there is no PQ bus) updates
theta over the angle buses from dP / Vm, an odd h updates Vm over the PQ buses from dQ / Vm.  `dens` gives the dimensionless
denominators den_k = 1 - c_k a^T X a of both matrices (0 up to rounding for a bridge): the outage's amplification of rounding in
the tests' bound.  The currents and the summary follow the kernel's definitions in fp32: the state rounded to fp32 (Vm, Va in
degrees), `branch_ref.flows` on it, loading I / rating, `contingency_ref.summarise`, and `voltage_figures` over the PQ buses.
It imports nothing of the library."""
import numpy as np

from tests import branch_ref as B
from tests import contingency_ref as R
from tests import powerflow_fd_ref as FD
from tests import powerflow_ref as P

islands = R.islands


def base_state(bus_type, spec, edge_index, rx, variant="xb", init=None, tol=1e-10, max_iter=60):
    """(vm, theta in radians, status) of the fast-decoupled base solve of the full grid; (None, None, status) where it fails."""
    table, status, _ = FD.fast_decoupled(bus_type, spec, edge_index, rx, variant=variant, init=init, tol=tol, max_iter=max_iter)
    if table is None:
        return None, None, status
    return table[:, 0].copy(), table[:, 1] * P.RAD, status


def weights(rx, variant):
    """(c' [e], c'' [e]): a line's weight in B' and in B''."""
    rx = np.asarray(rx, dtype=np.float64)
    r, x = rx[:, 0], rx[:, 1]
    w_x, w_b = 1.0 / x, x / (r * r + x * x)
    return (w_x, w_b) if variant == "xb" else (w_b, w_x)


def _incidence(buses, i, j):
    """a = e_i - e_j restricted to `buses` (one entry where one end is outside, none where both are)"""
    a = np.zeros(len(buses))
    a[buses == i] += 1.0
    a[buses == j] -= 1.0
    return a


def dens(bus_type, edge_index, rx, variant="xb"):
    """(den' [e], den'' [e]) = 1 - c_k a^T X a of the two matrices of the full list; 1 where both ends are outside the matrix."""
    ei = np.asarray(edge_index)
    ang, mag = P.unknowns(bus_type)
    Bp, Bq = FD.fd_matrices(bus_type, ei, rx, variant)
    cp, cq = weights(rx, variant)
    out = np.ones((2, ei.shape[1]))
    for which, (M, buses, c) in enumerate(((Bp, np.asarray(ang), cp), (Bq, np.asarray(mag), cq))):
        if not len(buses):
            continue
        X = np.linalg.inv(M)
        for k in range(ei.shape[1]):
            a = _incidence(buses, ei[0, k], ei[1, k])
            out[which, k] = 1.0 - c[k] * float(a @ X @ a)
    return out[0], out[1]


def inverses(bus_type, edge_index, rx, variant="xb"):
    """(X', X''): the inverses of the full list's two matrices, for `outage_state(..., inv=)` over many outages of one scenario."""
    Bp, Bq = FD.fd_matrices(bus_type, np.asarray(edge_index), rx, variant)
    return np.linalg.inv(Bp), (np.linalg.inv(Bq) if Bq.size else Bq)


def outage_state(bus_type, spec, edge_index, rx, vm0, th0, k, halves, variant="xb", form="literal", inv=None):
    """(vm, theta, mismatch): the state after `halves` half-iterations of the outage of line k from (vm0, th0), and max |F| of the
    reduced grid there.  form: "literal" or "compensated" (inv: `inverses` of the scenario, formed here where None)."""
    assert form in ("literal", "compensated")
    ei, rx, sp = np.asarray(edge_index), np.asarray(rx, dtype=np.float64), np.asarray(spec, dtype=np.float64)
    keep = np.arange(ei.shape[1]) != k
    ei_k, rx_k = ei[:, keep], rx[keep]
    ang, mag = (np.asarray(u) for u in P.unknowns(bus_type))
    vm, th = np.array(vm0, dtype=np.float64), np.array(th0, dtype=np.float64)
    if form == "literal":
        Bp, Bq = FD.fd_matrices(bus_type, ei_k, rx_k, variant)
        apply_p = lambda g: np.linalg.solve(Bp, g)                            # noqa: E731
        apply_q = lambda g: np.linalg.solve(Bq, g)                            # noqa: E731
    else:
        Xp, Xq = inverses(bus_type, ei, rx, variant) if inv is None else inv
        cp, cq = weights(rx, variant)

        def compensated(X, buses, c):
            a = _incidence(buses, ei[0, k], ei[1, k])
            w = X @ a
            den = 1.0 / c - float(a @ w)
            return lambda g: X @ g + w * (float(w @ g) / den)
        apply_p = compensated(Xp, ang, cp[k])
        apply_q = compensated(Xq, mag, cq[k]) if len(mag) else None
    for h in range(halves):
        dp, dq, _ = FD._mismatch(vm, th, bus_type, sp, ei_k, rx_k)
        if len(mag) and h % 2:
            vm[mag] -= apply_q(dq[mag] / vm[mag])
        else:
            th[ang] -= apply_p(dp[ang] / vm[ang])
    _, _, F = FD._mismatch(vm, th, bus_type, sp, ei_k, rx_k)
    return vm, th, (float(np.abs(F).max()) if F.size else 0.0)


def newton_outage(bus_type, spec, edge_index, rx, vm0, th0, k, tol=1e-10, max_iter=20):
    """(vm, theta) of `newton_from` on the grid without line k, started at (vm0, th0): the AC truth; None where it fails."""
    ei, rx = np.asarray(edge_index), np.asarray(rx, dtype=np.float64)
    keep = np.arange(ei.shape[1]) != k
    init = np.stack([vm0, np.asarray(th0) / P.RAD], axis=1)
    table, status, _ = FD.newton_from(bus_type, spec, ei[:, keep], rx[keep], init=init, tol=tol, max_iter=max_iter)
    return None if table is None else (table[:, 0].copy(), table[:, 1] * P.RAD)


def state32(vm, th, bus_type, spec):
    """fp32 [n, 2] = (Vm, Va in degrees) as the kernel rounds a state: the slack's angle is the specification's."""
    va = np.where(np.asarray(bus_type) == 0, np.asarray(spec, dtype=np.float64)[:, 1], np.asarray(th) * (1.0 / P.RAD))
    return np.stack([vm, va], axis=1).astype(np.float32)


def currents(st32, edge_index, rx, k=None):
    """(I [e] float64 with NaN at line k, the scale of branch_flows' bound [e]) of an fp32 state [n, 2]."""
    table = np.zeros((1, st32.shape[0], 4), dtype=np.float32)
    table[0, :, :2] = st32
    fl, scales = B.flows(table, edge_index, np.asarray(rx, dtype=np.float32).astype(np.float64))
    cur, sc = fl[0, :, 0].copy(), scales[0, :, 0]
    if k is not None:
        cur[k] = np.nan
    return cur, sc


def summarise(cur_table, ratings, isl, dtype=np.float32):
    """`contingency_ref.summarise` of a current table [e, e] (row = outage; the entry at (k, k) is not looked at)."""
    post = np.array(cur_table, dtype=dtype)
    post[np.arange(post.shape[0]), np.arange(post.shape[0])] = 0
    return R.summarise(post, ratings, isl, dtype=dtype)


def voltage_figures(vm32, bus_type, v_lo, v_hi):
    """(vm_min float32, vm_min_bus, v_violations) over the PQ buses of an fp32 Vm [n]: the lowest with ties to the lowest bus; a
    non-finite Vm counts as a violation, is the lowest, and makes vm_min NaN; without a PQ bus (NaN, -1, 0)."""
    vm32 = np.asarray(vm32, dtype=np.float32)
    pq = np.flatnonzero(np.asarray(bus_type) == 2)
    if not len(pq):
        return np.float32(np.nan), -1, 0
    v = vm32[pq]
    wild = ~np.isfinite(v)
    key = np.where(wild, -np.inf, v)
    at = int(np.argmin(key))                                                 # (numpy's argmin: the first of equals)
    lo, hi = np.float32(v_lo), np.float32(v_hi)
    with np.errstate(invalid="ignore"):
        count = int((wild | (v < lo) | (v > hi)).sum())
    return (np.float32(np.nan) if wild.any() else v[at]), int(pq[at]), count
