"""float64 numpy yardstick of the N-2 line-pair outage screen (csrc/contingency_pairs.hip, utils/contingency.py), written for the
tests.  One scenario at a time: bus_type [n], spec [n, 4], lines [2, e], rx [e, 2], ratings [e] or None; `pairs` [P, 2] are line ids
a < b.  The post-pair flows come from LITERALLY deleting both lines and solving the DC model again (`resolve_pairs`); the rank-2
form the kernel uses is here too (`lodf_pairs`, which also returns M per pair), so that tests/test_contingency_pairs_host.py can hold
the two together without a GPU.  Pair islands are tests/topology_ref.unsupplied with two lines left out.  It builds on
tests/contingency_ref.py, powerflow_ref.py and topology_ref.py and imports nothing of the library."""
import numpy as np

from tests import contingency_ref as R
from tests import powerflow_ref as P
from tests import topology_ref as T


def pair_list(lines_or_e):
    """int64 [P, 2]: the pairs (lines[i], lines[j]), i < j, row-major in (i, j); an int e means all lines of range(e)."""
    lines = np.arange(lines_or_e) if np.isscalar(lines_or_e) else np.asarray(lines_or_e, dtype=np.int64)
    i, j = np.triu_indices(len(lines), 1)
    return np.stack([lines[i], lines[j]], axis=1).astype(np.int64).reshape(-1, 2)


def islands(bus_type, edge_index, pairs):
    """int32 [P]: buses not reachable from the slack when both lines of the pair are removed; -4 everywhere for an id outside [0, n)."""
    bt, ei = np.asarray(bus_type), np.asarray(edge_index, dtype=np.int64)
    n, e = len(bt), ei.shape[1]
    slack = int(np.flatnonzero(bt == 0)[0])
    ar = np.arange(e)
    return np.array([T.unsupplied(ei, n, slack, keep=(ar != a) & (ar != b)) for a, b in pairs], dtype=np.int32)


def resolve_pairs(bus_type, spec, edge_index, rx, pairs, isl=None):
    """[P, e] (row = pair, column = line, original numbering): the flows with both lines literally removed and the DC model solved
    again; 0 at the two outaged lines; NaN rows where the pair islands a bus."""
    ei, rx = np.asarray(edge_index), np.asarray(rx, dtype=np.float64)
    e = ei.shape[1]
    isl = islands(bus_type, ei, pairs) if isl is None else isl
    out = np.full((len(pairs), e), np.nan)
    ar = np.arange(e)
    for p, (a, b) in enumerate(pairs):
        if isl[p] != 0:
            continue
        keep = (ar != a) & (ar != b)
        out[p, keep] = R.base_flow(bus_type, spec, ei[:, keep], rx[keep])
        out[p, a] = out[p, b] = 0.0
    return out


def lodf_pairs(bus_type, spec, edge_index, rx, pairs):
    """(post [P, e], M [P, 2, 2]) by the formulas of include/pfn_hip.h: with X, w_k and phi_{l,k} as tests/contingency_ref.lodf,
    M = [[1 - phi_aa, -phi_ab], [-phi_ba, 1 - phi_bb]], t = M^-1 (f_a, f_b), post[p, l] = f_l + phi_la t_a + phi_lb t_b, 0 at a and b.
    An islanding pair has det M = 0 up to rounding: its row is whatever the division gives."""
    bt, ei, rx = np.asarray(bus_type), np.asarray(edge_index), np.asarray(rx, dtype=np.float64)
    n, e = len(bt), ei.shape[1]
    ang, _ = P.unknowns(bt)
    X = np.zeros((n, n))
    X[np.ix_(ang, ang)] = np.linalg.inv(P.dc_matrix(bt, ei, rx)[np.ix_(ang, ang)])
    f = R.base_flow(bt, spec, ei, rx)
    W = X[:, ei[0]] - X[:, ei[1]]                                            # [n, e]: column k is w_k
    phi = (W[ei[0], :] - W[ei[1], :]) / rx[:, 1][:, None]                    # [l, k]
    post, Ms = np.empty((len(pairs), e)), np.empty((len(pairs), 2, 2))
    for p, (a, b) in enumerate(pairs):
        M = np.array([[1.0 - phi[a, a], -phi[a, b]], [-phi[b, a], 1.0 - phi[b, b]]])
        det = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            ta = (M[1, 1] * f[a] - M[0, 1] * f[b]) / det
            tb = (-M[1, 0] * f[a] + M[0, 0] * f[b]) / det
            post[p] = f + phi[:, a] * ta + phi[:, b] * tb
        post[p, a] = post[p, b] = 0.0
        Ms[p] = M
    return post, Ms


def inverse_norm(M):
    """(||M^-1||_inf [P], |det M| [P]) of [P, 2, 2]; inf where det = 0"""
    det = M[:, 0, 0] * M[:, 1, 1] - M[:, 0, 1] * M[:, 1, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        rows = np.maximum(np.abs(M[:, 1, 1]) + np.abs(M[:, 0, 1]), np.abs(M[:, 1, 0]) + np.abs(M[:, 0, 0])) / np.abs(det)
    return np.where(det == 0, np.inf, rows), np.abs(det)


def summarise_pairs(post, ratings, isl, pairs, dtype=np.float64):
    """(severity, worst_line, overloads) [P] of a post-pair table [P, e] by the rules of the screen, in `dtype` arithmetic: loading
    |f| / rating over the monitored lines l != a, b (a rating that is not > 0 is unmonitored), the maximum with ties to the lowest l,
    a non-finite loading counts as the largest and makes the severity NaN, no monitored line gives (0, -1, 0); an islanding pair gives
    (+inf, -1, -1)."""
    n_pairs, e = post.shape
    r = np.ones(e, dtype=dtype) if ratings is None else np.asarray(ratings).astype(dtype)
    sev, worst, over = np.zeros(n_pairs, dtype=dtype), np.full(n_pairs, -1, dtype=np.int32), np.zeros(n_pairs, dtype=np.int32)
    ar = np.arange(e)
    for p, (a, b) in enumerate(pairs):
        if isl[p] != 0:
            sev[p], worst[p], over[p] = np.inf, -1, -1
            continue
        mon = (r > 0) & (ar != a) & (ar != b)
        if not mon.any():
            continue
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            load = (np.abs(post[p].astype(dtype)) / r).astype(dtype)
        wild = mon & ~np.isfinite(load)
        key = np.where(mon, np.where(wild, np.inf, load), -1.0)
        worst[p] = int(np.argmax(key))                                       # (numpy's argmax: the first of equals)
        sev[p] = np.nan if wild.any() else key[worst[p]]
        over[p] = int((mon & (load > 1)).sum())
    return sev, worst, over


def top_two_gap(row, ratings, a, b):
    """The yardstick's largest loading of a pair's row [e] minus its second largest (monitored lines l != a, b); inf with fewer than two."""
    e = row.shape[0]
    r = np.ones(e) if ratings is None else np.asarray(ratings, dtype=np.float64)
    mon = (r > 0) & (np.arange(e) != a) & (np.arange(e) != b)
    load = np.sort(np.abs(row[mon]) / r[mon])
    return float(load[-1] - load[-2]) if load.size >= 2 else np.inf
