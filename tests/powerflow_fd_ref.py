"""float64 numpy yardstick of the solver's warm start and fast-decoupled modes (`pfn_powerflow_solve_init`, csrc/powerflow.hip),
written for the tests on top of tests/powerflow_ref.py (mismatch, scale, Jacobian, `finish_table`): the start a caller's table
gives, a Newton-Raphson loop from it, and the XB / BX fast-decoupled iterations as the kernel runs them --

  B'   order n - 1 (the angle buses), B'' order n_pq (the PQ buses): Laplacians over the stored lines, parallel lines adding;
       XB: B' from 1 / x, B'' from -b = x / (r^2 + x^2); BX the other way round; constant, so factored once;
  half-iterations alternate, the P half first:  theta += sign B'^-1 (dP / Vm)  over the angle buses,
                                                Vm    += sign B''^-1 (dQ / Vm) over the PQ buses,
       sign = -1 for the project's demand-positive mismatch (dP = P - sum_j Pji); +1 diverges (tests/test_powerflow_fd_host.py);
  the mismatch is re-formed and max |F| tested against tol after every half-iteration; the count is of half-iterations; with no PQ
  bus only the P half runs.

One sample at a time, the conventions of tests/powerflow_ref.py."""
import numpy as np

from tests import powerflow_ref as P

F32 = lambda A, b: np.linalg.solve(A.astype(np.float32), b.astype(np.float32)).astype(np.float64)      # noqa: E731


def start(bus_type, spec, init=None):
    """(vm, theta in radians): the flat start, or Va at the non-slack buses and Vm at the PQ buses taken from `init` [n, >= 2] =
    (Vm, Va in degrees); the slack's Vm / Va and the PV buses' Vm come from `spec` whatever `init` holds there."""
    vm, th, _ = P.flat_start(bus_type, spec)
    if init is not None:
        init = np.asarray(init, dtype=np.float64)
        ang, mag = P.unknowns(bus_type)
        th[ang] = init[ang, 1] * P.RAD
        vm[mag] = init[mag, 0]
    return vm, th


def _mismatch(vm, th, bus_type, sp, edge_index, rx):
    ang, mag = P.unknowns(bus_type)
    dp, dq = P.mismatch(np.stack([vm, th / P.RAD, sp[:, 2], sp[:, 3]], axis=1), edge_index, rx)
    return dp, dq, np.concatenate([dp[ang], dq[mag]])


def newton_from(bus_type, spec, edge_index, rx, init=None, tol=1e-10, max_iter=10, solve=np.linalg.solve):
    """`powerflow_ref.newton` from `start(init)`: (table or None, status, residual); status 0 where the start is under tol already."""
    sp = np.asarray(spec, dtype=np.float64)
    ang, mag = P.unknowns(bus_type)
    vm, th = start(bus_type, sp, init)
    for it in range(max_iter + 1):
        _, _, F = _mismatch(vm, th, bus_type, sp, edge_index, rx)
        if not np.isfinite(F).all():
            return None, -3, np.nan
        res = float(np.abs(F).max()) if F.size else 0.0
        if res < tol:
            return P.finish_table(vm, th, bus_type, sp, edge_index, rx), it, res
        if it == max_iter:
            return None, -1, res
        A = P.flow_jacobian(vm, th, bus_type, edge_index, rx)
        try:
            dx = solve(A, F)
        except np.linalg.LinAlgError:
            return None, -2, res
        th[ang] += dx[:len(ang)]
        vm[mag] += dx[len(ang):]
    raise AssertionError


def laplacian(n, edge_index, w):
    ei = np.asarray(edge_index)
    B = np.zeros((n, n))
    np.add.at(B, (ei[0], ei[0]), w)
    np.add.at(B, (ei[1], ei[1]), w)
    np.add.at(B, (ei[0], ei[1]), -w)
    np.add.at(B, (ei[1], ei[0]), -w)
    return B


def fd_matrices(bus_type, edge_index, rx, variant):
    """(B' [n - 1, n - 1], B'' [n_pq, n_pq]) of variant "xb" or "bx"."""
    assert variant in ("xb", "bx")
    rx = np.asarray(rx, dtype=np.float64)
    r, x = rx[:, 0], rx[:, 1]
    w_x, w_b = 1.0 / x, x / (r * r + x * x)
    ang, mag = P.unknowns(bus_type)
    n = len(bus_type)
    wp, wq = (w_x, w_b) if variant == "xb" else (w_b, w_x)
    return laplacian(n, edge_index, wp)[np.ix_(ang, ang)], laplacian(n, edge_index, wq)[np.ix_(mag, mag)]


def fast_decoupled(bus_type, spec, edge_index, rx, variant="xb", init=None, tol=1e-10, max_iter=60, solve=np.linalg.solve, sign=-1.0):
    """(table or None, status, residual): status = the number of HALF-iterations used, -1 not converged in max_iter, -2 singular,
    -3 non-finite."""
    sp = np.asarray(spec, dtype=np.float64)
    ang, mag = P.unknowns(bus_type)
    vm, th = start(bus_type, sp, init)
    Bp, Bq = fd_matrices(bus_type, edge_index, rx, variant)
    half = 0
    for it in range(max_iter + 1):
        dp, dq, F = _mismatch(vm, th, bus_type, sp, edge_index, rx)
        if not np.isfinite(F).all():
            return None, -3, np.nan
        res = float(np.abs(F).max()) if F.size else 0.0
        if res < tol:
            return P.finish_table(vm, th, bus_type, sp, edge_index, rx), it, res
        if it == max_iter:
            return None, -1, res
        try:
            if half == 0:
                th[ang] += sign * solve(Bp, dp[ang] / vm[ang])
            else:
                vm[mag] += sign * solve(Bq, dq[mag] / vm[mag])
        except np.linalg.LinAlgError:
            return None, -2, res
        half = (1 - half) if len(mag) else 0
    raise AssertionError
