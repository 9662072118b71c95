"""float64 numpy yardstick of the N-1 line-outage screen (csrc/contingency.hip, utils/contingency.py), written for the tests.  One
scenario at a time: bus_type [n], spec [n, 4], lines [2, e], rx [e, 2], ratings [e] or None.  The post-outage flows come from
LITERALLY deleting line k and solving the DC model again (`resolve`); the line outage distribution factors the kernel uses are
here too (`lodf`), so that tests/test_contingency_host.py can hold the two together without a GPU.  `islands` is
tests/topology_ref.unsupplied with the line left out.  It imports nothing of the library."""
import numpy as np

from tests import powerflow_ref as P
from tests import topology_ref as T


def islands(bus_type, edge_index):
    """int32 [e]: buses not reachable from the slack when line k is removed; -4 everywhere for an id outside [0, n)."""
    bt, ei = np.asarray(bus_type), np.asarray(edge_index, dtype=np.int64)
    n, e = len(bt), ei.shape[1]
    slack = int(np.flatnonzero(bt == 0)[0])
    return np.array([T.unsupplied(ei, n, slack, keep=np.arange(e) != k) for k in range(e)], dtype=np.int32)


def base_flow(bus_type, spec, edge_index, rx):
    """f_l = (theta_a - theta_b) / x_l [e] of the DC solution."""
    table, _ = P.dc_solve(bus_type, spec, edge_index, rx, norm=False)
    th, ei = table[:, 1] * P.RAD, np.asarray(edge_index)
    return (th[ei[0]] - th[ei[1]]) / np.asarray(rx, dtype=np.float64)[:, 1]


def resolve(bus_type, spec, edge_index, rx, isl=None):
    """[e, e] (row = outage, column = line, original numbering): the flows with line k literally removed and the DC model solved
    again; 0 at (k, k); NaN rows where the outage islands a bus."""
    ei, rx = np.asarray(edge_index), np.asarray(rx, dtype=np.float64)
    e = ei.shape[1]
    isl = islands(bus_type, ei) if isl is None else isl
    out = np.full((e, e), np.nan)
    for k in range(e):
        if isl[k] != 0:
            continue
        keep = np.arange(e) != k
        out[k, keep] = base_flow(bus_type, spec, ei[:, keep], rx[keep])
        out[k, k] = 0.0
    return out


def lodf(bus_type, spec, edge_index, rx):
    """(post [e, e], den [e]) by the formulas of include/pfn_hip.h: X = B'^-1 extended by zeros at the slack, w_k = X[:, i] - X[:, j],
    phi_{l,k} = (w_k[a] - w_k[b]) / x_l, den_k = 1 - phi_{k,k}, post[k, l] = f_l + phi_{l,k} / den_k f_k, post[k, k] = 0.  A bridge has
    den = 0 up to rounding: its row is whatever the division gives."""
    bt, ei, rx = np.asarray(bus_type), np.asarray(edge_index), np.asarray(rx, dtype=np.float64)
    n, e = len(bt), ei.shape[1]
    ang, _ = P.unknowns(bt)
    X = np.zeros((n, n))
    X[np.ix_(ang, ang)] = np.linalg.inv(P.dc_matrix(bt, ei, rx)[np.ix_(ang, ang)])
    f = base_flow(bt, spec, ei, rx)
    W = X[:, ei[0]] - X[:, ei[1]]                                            # [n, e]: column k is w_k
    phi = (W[ei[0], :] - W[ei[1], :]) / rx[:, 1][:, None]                    # [l, k]
    den = 1.0 - np.diagonal(phi)
    with np.errstate(divide="ignore", invalid="ignore"):
        post = (f[:, None] + phi / den[None, :] * f[None, :]).T              # [k, l]
    post[np.arange(e), np.arange(e)] = 0.0
    return post, den


def summarise(post, ratings, isl, dtype=np.float64):
    """(severity, worst_line, overloads) [e] of a post-outage table [e, e] by the rules of the screen, in `dtype` arithmetic: loading
    |f| / rating over the monitored lines l != k (a rating that is not > 0 is unmonitored), the maximum with ties to the lowest l, a
    non-finite loading counts as the largest and makes the severity NaN, no monitored line gives (0, -1, 0); an islanding outage
    gives (+inf, -1, -1)."""
    e = post.shape[0]
    r = np.ones(e, dtype=dtype) if ratings is None else np.asarray(ratings).astype(dtype)
    sev, worst, over = np.zeros(e, dtype=dtype), np.full(e, -1, dtype=np.int32), np.zeros(e, dtype=np.int32)
    for k in range(e):
        if isl[k] != 0:
            sev[k], worst[k], over[k] = np.inf, -1, -1
            continue
        mon = (r > 0) & (np.arange(e) != k)
        if not mon.any():
            continue
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            load = (np.abs(post[k].astype(dtype)) / r).astype(dtype)
        wild = mon & ~np.isfinite(load)
        key = np.where(mon, np.where(wild, np.inf, load), -1.0)
        worst[k] = int(np.argmax(key))                                       # (numpy's argmax: the first of equals)
        sev[k] = np.nan if wild.any() else key[worst[k]]
        over[k] = int((mon & (load > 1)).sum())
    return sev, worst, over


def top_two_gap(post, ratings, k):
    """The yardstick's largest loading of outage k minus its second largest (monitored lines l != k); inf with fewer than two."""
    e = post.shape[0]
    r = np.ones(e) if ratings is None else np.asarray(ratings, dtype=np.float64)
    mon = (r > 0) & (np.arange(e) != k)
    load = np.sort(np.abs(post[k][mon]) / r[mon])
    return float(load[-1] - load[-2]) if load.size >= 2 else np.inf
