"""float64 numpy yardstick of the generator-outage screen (csrc/contingency_units.hip, utils/contingency.py), written for the tests.
One scenario at a time: bus_type [n], spec [n, 4], lines [2, e], rx [e, 2]; units [G] bus ids, p [G] the outputs lost
(generation-positive), a [G] participation factors or None (all zero).  The post-outage flows come from LITERALLY editing `spec` and
solving the DC model again (`resolve_units`; `resolve_unit_lines` also deletes line k); the closed form the kernel uses stands beside
them (`closed_form`, `closed_form_lines`), so that tests/test_contingency_units_host.py can hold the two together without a GPU.
Summaries come from tests/contingency_ref.summarise.  It imports nothing of the library."""
import numpy as np

from tests import contingency_ref as R
from tests import powerflow_ref as P


def unit_cases(bt):
    """{name: (units, p, a)} for the tests: the PV buses, the last PQ bus, the slack and the first PV bus once more (two units on one
    bus), with every pickup rule; p[1] = 0"""
    pv, pq, slack = np.flatnonzero(bt == 1), np.flatnonzero(bt == 2), int(np.flatnonzero(bt == 0)[0])
    units = np.concatenate([pv, [pq[-1], slack, pv[0]]])
    G = len(units)
    p = 0.1 + 0.05 * np.arange(G)
    p[1] = 0.0                                                               # p = 0: an ordinary item, the base flows
    only = np.zeros(G)
    only[0] = 2.0                                                            # unit 0 alone participates: its own outage has rest = 0
    return {"slack pickup": (units, p, None), "graded participation": (units, p, 1.0 + np.arange(G)), "zero participation": (units, p, np.zeros(G)),
            "participation on one unit only": (units, p, only)}


def default_unit_p(spec, units):
    """max(-P, 0) at the units' buses: what `unit_p=None` means"""
    return np.maximum(-np.asarray(spec, dtype=np.float64)[np.asarray(units), 2], 0.0)


def shifted_spec(spec, units, p, a, g):
    """a copy of spec [n, 4] with the outage of unit g written into its demand-positive P column: +p_g at b_g and, where
    rest_g = A - a_g > 0, -p_g a_h / rest_g at b_h for every h != g -- the units in stored order, one addition each"""
    out = np.array(spec, dtype=np.float64)
    units = np.asarray(units)
    a = np.zeros(len(units)) if a is None else np.asarray(a, dtype=np.float64)
    rest = a.sum() - a[g]
    for h in range(len(units)):
        if h == g:
            out[units[h], 2] += p[g]
        elif rest > 0:
            out[units[h], 2] += -p[g] * a[h] / rest
    return out


def resolve_units(bus_type, spec, edge_index, rx, units, p, a=None):
    """[G, e]: the flows with the outage of unit g literally written into spec and the DC model solved again"""
    return np.stack([R.base_flow(bus_type, shifted_spec(spec, units, p, a, g), edge_index, rx) for g in range(len(units))])


def resolve_unit_lines(bus_type, spec, edge_index, rx, units, p, a, lines, isl):
    """[G, c, e] (original line numbering): spec edited for unit g AND line lines[j] deleted, the DC model solved again; 0 at the
    deleted line; NaN rows where its outage islands a bus (isl [e], contingency_ref.islands)"""
    ei, rx = np.asarray(edge_index), np.asarray(rx, dtype=np.float64)
    e = ei.shape[1]
    out = np.full((len(units), len(lines), e), np.nan)
    for g in range(len(units)):
        sp = shifted_spec(spec, units, p, a, g)
        for j, k in enumerate(lines):
            if isl[k] != 0:
                continue
            keep = np.arange(e) != k
            out[g, j, keep] = R.base_flow(bus_type, sp, ei[:, keep], rx[keep])
            out[g, j, k] = 0.0
    return out


def inverse(bus_type, edge_index, rx):
    """X [n, n]: B'^-1 extended by zeros at the slack"""
    bt = np.asarray(bus_type)
    ang, _ = P.unknowns(bt)
    X = np.zeros((len(bt), len(bt)))
    X[np.ix_(ang, ang)] = np.linalg.inv(P.dc_matrix(bt, edge_index, rx)[np.ix_(ang, ang)])
    return X


def closed_form(bus_type, spec, edge_index, rx, units, p, a=None):
    """(post [G, e], d [G, n]) by the formulas of include/pfn_hip.h: c_g = X[:, b_g], A = sum a, rest_g = A - a_g, u = sum_h a_h c_h,
    d_g = p_g ((u - a_g c_g) / rest_g - c_g) where rest_g > 0, else -p_g c_g; post[g, l] = f_l + (d_g[a] - d_g[b]) / x_l"""
    ei, rx = np.asarray(edge_index), np.asarray(rx, dtype=np.float64)
    units, p = np.asarray(units), np.asarray(p, dtype=np.float64)
    X = inverse(bus_type, ei, rx)
    f = R.base_flow(bus_type, spec, ei, rx)
    col = X[:, units]                                                        # [n, G]: column g is c_g
    a = np.zeros(len(units)) if a is None else np.asarray(a, dtype=np.float64)
    u = col @ a
    d = np.empty((len(units), X.shape[0]))
    for g in range(len(units)):
        rest = a.sum() - a[g]
        d[g] = p[g] * ((u - a[g] * col[:, g]) / rest - col[:, g]) if rest > 0 else -p[g] * col[:, g]
    return f[None, :] + (d[:, ei[0]] - d[:, ei[1]]) / rx[:, 1][None, :], d


def closed_form_lines(bus_type, edge_index, rx, post, lines):
    """(post2 [G, c, e], den [c]): line outage distribution factors applied to the post-unit flows post [G, e] --
    post2[g, j, l] = post[g, l] + phi_{l,k} / den_k post[g, k], 0 at k = lines[j].  A bridge has den = 0 up to rounding."""
    ei, rx = np.asarray(edge_index), np.asarray(rx, dtype=np.float64)
    lines = np.asarray(lines)
    X = inverse(bus_type, ei, rx)
    W = X[:, ei[0][lines]] - X[:, ei[1][lines]]                              # [n, c]: column j is w_k
    phi = (W[ei[0], :] - W[ei[1], :]) / rx[:, 1][:, None]                    # [l, j]
    den = 1.0 - phi[lines, np.arange(len(lines))]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = post[:, None, :] + (phi / den[None, :]).T[None, :, :] * post[:, lines][:, :, None]
    out[:, np.arange(len(lines)), lines] = 0.0
    return out, den


def unit_scale(f, d, edge_index, rx):
    """[G]: max(max_l |f_l|, max_l (|d_g[a]| + |d_g[b]|) / |x_l|) -- the size of what the kernel's fp32 expression for the post-unit
    flows rounds (times 2^-24: one unit of rounding)"""
    ei, x = np.asarray(edge_index), np.abs(np.asarray(rx, dtype=np.float64)[:, 1])
    return np.maximum(np.abs(f).max(), ((np.abs(d[:, ei[0]]) + np.abs(d[:, ei[1]])) / x[None, :]).max(axis=1))


def summarise_units(post, ratings, dtype=np.float64):
    """(severity, worst_line, overloads) [G] of post [G, e] with ALL lines monitored, by contingency_ref.summarise: row g sits in a
    table of e + G lines as the outage of a line e + g, and nobody monitors the G lines that were added"""
    G, e = post.shape
    r = np.ones(e) if ratings is None else np.asarray(ratings)
    table = np.zeros((e + G, e + G), dtype=post.dtype)
    table[e:, :e] = post
    sev, worst, over = R.summarise(table, np.concatenate([r.astype(np.float64), np.zeros(G)]), np.zeros(e + G, dtype=np.int32), dtype=dtype)
    return sev[e:], worst[e:], over[e:]


def summarise_unit_lines(post, ratings, isl, lines, dtype=np.float64):
    """(severity, worst_line, overloads) [c] of one unit's rows post [c, e]: row j is the outage of line lines[j] in
    contingency_ref.summarise's square table"""
    e = post.shape[1]
    lines = np.asarray(lines)
    table = np.zeros((e, e), dtype=post.dtype)
    table[lines] = post
    sev, worst, over = R.summarise(table, ratings, isl, dtype=dtype)
    return sev[lines], worst[lines], over[lines]


def top_two_gap(row, ratings, skip=-1):
    """the largest loading of a row [e] minus its second largest over the monitored lines l != skip; inf with fewer than two"""
    e = len(row)
    r = np.ones(e) if ratings is None else np.asarray(ratings, dtype=np.float64)
    mon = (r > 0) & (np.arange(e) != skip)
    load = np.sort(np.abs(row[mon]) / r[mon])
    return float(load[-1] - load[-2]) if load.size >= 2 else np.inf
