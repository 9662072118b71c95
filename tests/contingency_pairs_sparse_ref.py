"""numpy restatement of the sparse route of the N-2 pair screen (csrc/contingency_pairs_sparse.hip), written for the tests: one
column w_k per candidate line from the float32 factor of tests/contingency_sparse_ref.py (`dc_plan`, `factor`) by the kernel's
forward and backward column substitutions in float32, then one pair's arithmetic as csrc/contingency_line.hpp spells it -- the four
phi of M, t by Cramer's rule, two phi and the sum per line -- every operation rounded to float32 on its own.  numpy has no float32
fma, so the substitution rounds a product and its sum one after the other where the kernel rounds once: an expectation of the error
level, not a bit check.  One scenario at a time; no GPU."""
import numpy as np

from tests import contingency_pairs_ref as R2
from tests import contingency_ref as R
from tests import contingency_sparse_ref as CS

EPS = 2.0 ** -24


def ends(plan, edge_index):
    """(pa, pb) [e]: the plan-order unknown of either end of every line, m at the slack"""
    ei = np.asarray(edge_index)
    return np.where(plan.ua[ei[0]] >= 0, plan.ua[ei[0]], plan.m), np.where(plan.ua[ei[1]] >= 0, plan.ua[ei[1]], plan.m)


def columns(plan, slab, edge_index, lines):
    """W [m + 1, c] float32: column k is B'^-1 (e_i - e_j) of candidate lines[k] in plan order, row m (the slack) zero -- the
    kernel's column table, transposed"""
    m, c = plan.m, len(lines)
    pa, pb = ends(plan, edge_index)
    W = np.zeros((m + 1, c), dtype=np.float32)
    k = np.arange(c)
    np.add.at(W, (pa[lines], k), np.float32(1))
    np.add.at(W, (pb[lines], k), np.float32(-1))
    W[m] = 0
    cp, dg, rows = plan.colptr, plan.diag, plan.rowidx
    for j in range(m):
        lb, le = dg[j] + 1, cp[j + 1]
        if lb < le:
            W[rows[lb:le]] -= slab[lb:le, None] * W[j][None, :]
    for j in range(m - 1, -1, -1):
        ub, ue = cp[j], dg[j]
        W[j] = W[j] / slab[ue]
        if ub < ue:
            W[rows[ub:ue]] -= slab[ub:ue, None] * W[j][None, :]
    assert W.dtype == np.float32
    return W


def pair_flows(plan, W, edge_index, rx, base_flow, lines):
    """post [P, e] float32 in `pair_list(lines)`' order from the candidates' columns: ct_pair_phi, ct_pair_solve, ct_pair_post; 0 at
    the two outaged lines; an islanding pair's row is whatever the division gives (the kernel overwrites it from the islands)"""
    one = np.float32(1)
    f32 = np.asarray(base_flow, dtype=np.float64).astype(np.float32)
    x32 = np.asarray(rx, dtype=np.float64)[:, 1].astype(np.float32)
    pa, pb = ends(plan, edge_index)
    phi = (W[pa, :] - W[pb, :]) / x32[:, None]                               # [l, k] float32
    i, j = np.triu_indices(len(lines), 1)
    post = np.empty((len(i), len(f32)), dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for p, (ci, cj) in enumerate(zip(i, j)):
            a, b = lines[ci], lines[cj]
            paa, pab, pba, pbb = phi[a, ci], phi[a, cj], phi[b, ci], phi[b, cj]
            da, db = one - paa, one - pbb
            det = da * db - pab * pba
            ta = (db * f32[a] + pab * f32[b]) / det
            tb = (pba * f32[a] + da * f32[b]) / det
            post[p] = (f32 + phi[:, ci] * ta) + phi[:, cj] * tb
            post[p, a] = post[p, b] = 0
    assert post.dtype == np.float32 and phi.dtype == np.float32
    return post


def worst_ratio(bus_type, spec, edge_index, rx, lines, literal=True):
    """(max over the non-islanding pairs p and the lines l of |post - f64| / u_p, max ||M^-1||_inf over those pairs, the islands):
    u_p = 2^-24 max_l |f_l| ||M_p^-1||_inf with the yardstick's M; f64: the literal re-solve, or the yardstick's float64 rank-2 form
    where that is too slow"""
    lines = np.asarray(lines, dtype=np.int64)
    pairs = R2.pair_list(lines)
    isl = R2.islands(bus_type, edge_index, pairs)
    plan = CS.dc_plan(bus_type, edge_index)
    f = R.base_flow(bus_type, spec, edge_index, rx)
    W = columns(plan, CS.factor(plan, bus_type, spec, edge_index, rx), edge_index, lines)
    post = pair_flows(plan, W, edge_index, rx, f, lines)
    want, M = R2.lodf_pairs(bus_type, spec, edge_index, rx, pairs)
    if literal:
        want = R2.resolve_pairs(bus_type, spec, edge_index, rx, pairs, isl)
    ok = isl == 0
    norm = R2.inverse_norm(M)[0]
    u = EPS * np.abs(f).max() * norm[ok]
    return float((np.abs(post[ok].astype(np.float64) - want[ok]) / u[:, None]).max()), float(norm[ok].max()), isl
