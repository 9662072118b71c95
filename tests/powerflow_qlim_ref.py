"""float64 numpy yardstick of the Q-limited power-flow solve (csrc/powerflow_qlim.hip, utils/powerflow.py solve_power_flow_qlim),
built on tests/powerflow_ref.py: Newton-Raphson from a GIVEN state under a given type row and Q specification, then the round loop of
the kernel -- after a converged inner loop every PV bus whose Q line sum exceeds hi + q_tol becomes PQ at hi, below lo - q_tol PQ at
lo; all violators of a round switch together, none switches back; Newton goes on from the current state.  Limits are (lo, hi) [n, 2]
on the table's Q column (demand-positive per-unit), NaN or +-inf meaning no limit on that side.  One sample at a time.
tests/test_powerflow_qlim_host.py pins it without a GPU; tests/test_gpu_powerflow_qlim.py holds the kernel to it."""
from dataclasses import dataclass

import numpy as np

from tests import powerflow_ref as P

PF_QLIM_ROUNDS = -7


def newton_from(vm, th, bus_type, spec, edge_index, rx, tol=1e-10, max_iter=10, solve=np.linalg.solve):
    """`P.newton`'s loop from the state (vm, th in radians; both updated in place) under `bus_type` and `spec` (its Q column: the
    effective specification).  Returns (status, residual): status = the Jacobian solves used, -1, -2 or -3 as there."""
    sp = np.asarray(spec, dtype=np.float64)
    ang, mag = P.unknowns(bus_type)
    for it in range(max_iter + 1):
        cur = np.stack([vm, th / P.RAD, sp[:, 2], sp[:, 3]], axis=1)
        dp, dq = P.mismatch(cur, edge_index, rx)
        F = np.concatenate([dp[ang], dq[mag]])
        if not np.isfinite(F).all():
            return -3, np.nan
        res = float(np.abs(F).max()) if F.size else 0.0
        if res < tol:
            return it, res
        if it == max_iter:
            return -1, res
        A = P.flow_jacobian(vm, th, bus_type, edge_index, rx)
        if (np.abs(A).sum(axis=1) == 0).any():
            return -2, res
        try:
            dx = solve(A, F)
        except np.linalg.LinAlgError:
            return -2, res
        th[ang] += dx[:len(ang)]
        vm[mag] += dx[len(ang):]
    raise AssertionError


@dataclass
class QLimRef:
    """`table` [n, 4] or None where the solve failed; `status` the total of Jacobian solves or the failure code (-7: limits still
    violated after max_rounds re-solves); `bus_type` the final types (the input's on failure); `rounds` the re-solves; `history`
    one (solves, over, under) per inner loop -- the buses found above hi and below lo after it --; `margin` the smallest
    |Q - limit| over the live PV buses and their finite limits seen after any inner loop (inf where there was none); `spec` the
    specification the final solve ran under (Q of a switched bus = its limit)."""
    table: object
    status: int
    residual: float
    bus_type: np.ndarray
    rounds: int
    history: list
    margin: float
    spec: np.ndarray


def solve(bus_type, spec, edge_index, rx, q_limits=None, tol=1e-10, max_iter=10, max_rounds=8, q_tol=None, init=None):
    """The kernel's algorithm in float64 numpy.  `init` [n, >= 2] = (Vm, Va in degrees) or None for the flat start: Va is read at
    the non-slack buses and Vm at the buses that are PQ on entry."""
    bt0 = np.asarray(bus_type).astype(np.int64)
    bt, sp = bt0.copy(), np.array(spec, dtype=np.float64)
    q_tol = tol if q_tol is None else q_tol
    vm, th, _ = P.flat_start(bt, sp)
    if init is not None:
        init = np.asarray(init, dtype=np.float64)
        vm[bt == 2] = init[bt == 2, 0]
        th[bt != 0] = init[bt != 0, 1] * P.RAD
        if not (np.isfinite(vm).all() and np.isfinite(th).all()):
            return QLimRef(None, -3, np.nan, bt0, 0, [], np.inf, sp)
    lim = None if q_limits is None else np.asarray(q_limits, dtype=np.float64)
    total, rounds, history, margin = 0, 0, [], np.inf
    while True:
        status, res = newton_from(vm, th, bt, sp, edge_index, rx, tol, max_iter)
        if status < 0:
            return QLimRef(None, status, res, bt0, rounds, history, margin, sp)
        total += status
        over = under = np.zeros(len(bt), dtype=bool)
        if lim is not None:
            _, sq = P.line_sums(np.stack([vm, th / P.RAD, sp[:, 2], sp[:, 3]], axis=1), edge_index, rx)
            pv = bt == 1
            lo, hi = lim[:, 0], lim[:, 1]
            with np.errstate(invalid="ignore"):
                over = pv & np.isfinite(hi) & (sq > hi + q_tol)
                under = pv & ~over & np.isfinite(lo) & (sq < lo - q_tol)
            gaps = np.concatenate([np.abs(sq - hi)[pv & np.isfinite(hi)], np.abs(sq - lo)[pv & np.isfinite(lo)]])
            if gaps.size:
                margin = min(margin, float(gaps.min()))
        history.append((status, int(over.sum()), int(under.sum())))
        if not (over.any() or under.any()):
            return QLimRef(P.finish_table(vm, th, bt, sp, edge_index, rx), total, res, bt, rounds, history, margin, sp)
        if rounds >= max_rounds:
            return QLimRef(None, PF_QLIM_ROUNDS, res, bt0, rounds, history, margin, sp)
        sp[over, 3], sp[under, 3] = lim[over, 1], lim[under, 0]
        bt[over | under] = 2
        rounds += 1


def band_limits(bus_type, free_table):
    """The fixture limits of the GPU tests for one sample: (lo, hi) = median -+ half the inter-quartile range of the UNCONSTRAINED
    solution's Q at the PV buses, the same pair at every bus.  Returns [n, 2]."""
    q = np.asarray(free_table)[np.asarray(bus_type) == 1, 3]
    w = 0.5 * (np.percentile(q, 75) - np.percentile(q, 25))
    return np.tile(np.array([np.median(q) - w, np.median(q) + w]), (len(bus_type), 1))
