"""float64 numpy yardstick of the batched power-flow solver (csrc/powerflow.hip, utils/powerflow.py), written for the tests: the
mismatch of a bus table from the reference's message formulas (utils/custom_loss_functions.py:159-246, rectangular form), a
Newton-Raphson solve with np.linalg.solve, the DC solve, the error scale of the tests' residual bound and the Jacobian whose
inverse bounds the distance between two converged solutions.  One sample at a time: bus_type [n], spec / table [n, 4] =
(Vm, Va in degrees, P, Q) demand-positive per-unit, lines [2, e] (every stored line counts in both directions), rx [e, 2].
tests/test_powerflow_host.py pins it without a GPU; tests/test_gpu_powerflow.py holds the kernel to it."""
import numpy as np

RAD = np.pi / 180.0
EPS64 = 2.0 ** -52


def admittance(rx):
    rx = np.asarray(rx, dtype=np.float64)
    r, x = rx[:, 0], rx[:, 1]
    d = r * r + x * x
    return r / d, -x / d


def both_directions(edge_index, g, b):
    ei = np.asarray(edge_index)
    return np.concatenate([ei[0], ei[1]]), np.concatenate([ei[1], ei[0]]), np.concatenate([g, g]), np.concatenate([b, b])


def line_sums(table, edge_index, rx):
    """(sum_j Pji, sum_j Qji) [n] of PowerImbalance.message / aggregate: e = Vm cos, f = Vm sin."""
    t = np.asarray(table, dtype=np.float64)
    g, b = admittance(rx)
    i, j, g, b = both_directions(edge_index, g, b)
    ev, fv = t[:, 0] * np.cos(t[:, 1] * RAD), t[:, 0] * np.sin(t[:, 1] * RAD)
    ei_, fi_, ej_, fj_ = ev[i], fv[i], ev[j], fv[j]
    p = g * (ei_ * ej_ - ei_ ** 2 + fi_ * fj_ - fi_ ** 2) + b * (fi_ * ej_ - ei_ * fj_)
    q = g * (fi_ * ej_ - ei_ * fj_) + b * (-ei_ * ej_ + ei_ ** 2 - fi_ * fj_ + fi_ ** 2)
    sp, sq = np.zeros(t.shape[0]), np.zeros(t.shape[0])
    np.add.at(sp, i, p)
    np.add.at(sq, i, q)
    return sp, sq


def mismatch(table, edge_index, rx):
    """(dP, dQ) [n] = (P_i - sum Pji, Q_i - sum Qji): PowerImbalance.update."""
    t = np.asarray(table, dtype=np.float64)
    sp, sq = line_sums(t, edge_index, rx)
    return t[:, 2] - sp, t[:, 3] - sq


def scale(table, edge_index, rx):
    """scale_i = sum over the bus's lines of (|g| + |b|) (Vm_i + Vm_j) Vm_i (1 + |theta_i|), + |P_i| + |Q_i| (NaN P or Q count 0)."""
    t = np.asarray(table, dtype=np.float64)
    g, b = admittance(rx)
    i, j, g, b = both_directions(edge_index, g, b)
    vm, th = t[:, 0], np.abs(t[:, 1] * RAD)
    s = np.zeros(t.shape[0])
    np.add.at(s, i, (np.abs(g) + np.abs(b)) * (vm[i] + vm[j]) * vm[i] * (1 + th[i]))
    return s + np.nan_to_num(np.abs(t[:, 2])) + np.nan_to_num(np.abs(t[:, 3]))


def unknowns(bus_type):
    """(angle buses, magnitude buses): the unknown vector is [theta of the non-slack buses, Vm of the PQ buses], bus order."""
    bt = np.asarray(bus_type)
    assert (bt == 0).sum() == 1
    return np.flatnonzero(bt != 0), np.flatnonzero(bt == 2)


def flow_jacobian(vm, th, bus_type, edge_index, rx):
    """d(sum Pji at the non-slack buses, sum Qji at the PQ buses) / d(unknowns): minus the Jacobian of the mismatch."""
    ang, mag = unknowns(bus_type)
    n = len(vm)
    g, b = admittance(rx)
    i, j, g, b = both_directions(edge_index, g, b)
    c, s = np.cos(th[i] - th[j]), np.sin(th[i] - th[j])
    vv = vm[i] * vm[j]
    full = np.zeros((2 * n, 2 * n))                         # rows (P, Q) x columns (theta, Vm), all buses

    def add(r0, rows, c0, cols, vals):
        np.add.at(full, (r0 + rows, c0 + cols), vals)
    pti = vv * (-g * s + b * c)
    add(0, i, 0, i, pti)
    add(0, i, 0, j, -pti)
    add(0, i, n, i, g * (vm[j] * c - 2 * vm[i]) + b * vm[j] * s)
    add(0, i, n, j, vm[i] * (g * c + b * s))
    qti = vv * (g * c + b * s)
    add(n, i, 0, i, qti)
    add(n, i, 0, j, -qti)
    add(n, i, n, i, g * vm[j] * s - b * (vm[j] * c - 2 * vm[i]))
    add(n, i, n, j, vm[i] * (g * s - b * c))
    rows = np.concatenate([ang, n + mag])
    return full[np.ix_(rows, rows)]


def flat_start(bus_type, spec):
    bt, sp = np.asarray(bus_type), np.asarray(spec, dtype=np.float64)
    slack = int(np.flatnonzero(bt == 0)[0])
    return np.where(bt == 2, 1.0, sp[:, 0]), np.full(len(bt), sp[slack, 1] * RAD), slack


def finish_table(vm, th, bus_type, spec, edge_index, rx):
    """The table a solve writes: slack P, Q and PV Q are the aggregated line sums, everything else as given or solved."""
    bt, sp = np.asarray(bus_type), np.asarray(spec, dtype=np.float64)
    t = np.stack([vm, th / RAD, sp[:, 2], sp[:, 3]], axis=1)
    t[bt == 0, 1] = sp[bt == 0, 1]
    lp, lq = line_sums(t, edge_index, rx)
    t[bt == 0, 2] = lp[bt == 0]
    t[bt != 2, 3] = lq[bt != 2]
    return t


def newton(bus_type, spec, edge_index, rx, tol=1e-10, max_iter=10, solve=np.linalg.solve):
    """Newton-Raphson in polar form from a flat start.  Returns (table or None, status, residual): status = the number of Jacobian
    solves used, -1 not converged in max_iter, -2 singular, -3 non-finite."""
    sp = np.asarray(spec, dtype=np.float64)
    ang, mag = unknowns(bus_type)
    vm, th, _ = flat_start(bus_type, sp)
    for it in range(max_iter + 1):
        cur = np.stack([vm, th / RAD, sp[:, 2], sp[:, 3]], axis=1)
        dp, dq = mismatch(cur, edge_index, rx)
        F = np.concatenate([dp[ang], dq[mag]])
        if not np.isfinite(F).all():
            return None, -3, np.nan
        res = float(np.abs(F).max()) if F.size else 0.0
        if res < tol:
            return finish_table(vm, th, bus_type, sp, edge_index, rx), it, res
        if it == max_iter:
            return None, -1, res
        A = flow_jacobian(vm, th, bus_type, edge_index, rx)
        if (np.abs(A).sum(axis=1) == 0).any():
            return None, -2, res
        try:
            dx = solve(A, F)
        except np.linalg.LinAlgError:
            return None, -2, res
        th[ang] += dx[:len(ang)]
        vm[mag] += dx[len(ang):]
    raise AssertionError


def jacobian_inverse_norm(table, bus_type, edge_index, rx):
    """||J^-1||_inf at a solution (unknowns in radians and per-unit)."""
    t = np.asarray(table, dtype=np.float64)
    return float(np.abs(np.linalg.inv(flow_jacobian(t[:, 0].copy(), t[:, 1] * RAD, bus_type, edge_index, rx))).sum(axis=1).max())


# ------------------------------------------------------------------------------------------------------------ DC
def dc_matrix(bus_type, edge_index, rx):
    """B' [n, n]: the Laplacian of 1/x over the stored lines (parallel lines add)."""
    n = len(bus_type)
    ei = np.asarray(edge_index)
    w = 1.0 / np.asarray(rx, dtype=np.float64)[:, 1]
    B = np.zeros((n, n))
    np.add.at(B, (ei[0], ei[0]), w)
    np.add.at(B, (ei[1], ei[1]), w)
    np.add.at(B, (ei[0], ei[1]), -w)
    np.add.at(B, (ei[1], ei[0]), -w)
    return B


def dc_mismatch(table, edge_index, rx, bus_type):
    """F = B' theta + P at every bus, theta in radians from the table's degrees."""
    t = np.asarray(table, dtype=np.float64)
    return dc_matrix(bus_type, edge_index, rx) @ (t[:, 1] * RAD) + t[:, 2]


def dc_scale(table, edge_index, rx):
    t = np.asarray(table, dtype=np.float64)
    ei = np.asarray(edge_index)
    w = 1.0 / np.abs(np.asarray(rx, dtype=np.float64)[:, 1])
    th = np.abs(t[:, 1] * RAD)
    s = np.zeros(t.shape[0])
    np.add.at(s, ei[0], w * (th[ei[0]] + th[ei[1]]))
    np.add.at(s, ei[1], w * (th[ei[0]] + th[ei[1]]))
    return s + np.abs(t[:, 2])


def dc_solve(bus_type, spec, edge_index, rx, norm=True):
    """(table, ||B'^-1||_inf over the non-slack buses): theta from one float64 solve of B' theta = -P; Vm as given at the slack and
    PV buses and 1 at PQ buses, P as given with the slack's = -sum of the others, Q NaN.  norm=False: None instead of the norm."""
    bt, sp = np.asarray(bus_type), np.asarray(spec, dtype=np.float64)
    ang, _ = unknowns(bt)
    vm, th, slack = flat_start(bt, sp)
    B = dc_matrix(bt, edge_index, rx)
    Bn = B[np.ix_(ang, ang)]
    rhs = -sp[ang, 2] - B[np.ix_(ang, [slack])][:, 0] * th[slack]
    th[ang] = np.linalg.solve(Bn, rhs)
    p = sp[:, 2].copy()
    p[slack] = -sp[ang, 2].sum()
    return np.stack([vm, th / RAD, p, np.full(len(bt), np.nan)], axis=1), float(np.abs(np.linalg.inv(Bn)).sum(axis=1).max()) if norm else None
