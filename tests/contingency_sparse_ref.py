"""numpy restatement of the sparse route of the N-1 screen (csrc/contingency_sparse.hip), written for the tests: B' at the planned
positions of the mode-1 sparse plan in float32, tests/powerflow_sparse_ref.py's left-looking factorisation, then ONE LANE's arithmetic
for every outage at once -- the right-hand side e_i - e_j in plan order, the forward and backward column substitutions in float32,
den_k from two gathers, the per-line expression.  All e lanes run side by side as the columns of W [m + 1, e] (row m: the slack's
zeros), which is what the kernel's tiles of 64 do.  numpy has no float32 fma, so a product and its sum are rounded one after the
other where the kernel rounds once: the figures agree to rounding, not bit for bit.  One scenario at a time; no GPU."""
import numpy as np

from tests import contingency_ref as R
from tests import powerflow_ref as P
from tests import powerflow_sparse_ref as S

EPS = 2.0 ** -24


def dc_plan(bus_type, edge_index):
    rc, blob, err = S.build_plan(bus_type, edge_index, mode=1)
    assert rc == 0, err
    return S.Plan(blob)


def factor(plan, bus_type, spec, edge_index, rx):
    """The float32 factor of B' in the plan's slab: the solver's DC matrix at the planned positions is -B', entry for entry."""
    vm, th, _ = P.flat_start(np.asarray(bus_type), np.asarray(spec, dtype=np.float64))
    slab, _, _ = S.assemble(plan, vm, th, edge_index, rx, np.float32)
    slab = -slab
    assert S.factor(plan, slab)
    return slab


def lanes(plan, slab, edge_index, rx, base_flow):
    """(post [e, e] float32 with row = outage, den [e] float32) from the factor and the float64 base flows: what the kernel's lanes
    compute, bridges included (their rows are whatever the division gives: the kernel overwrites them from the islands)."""
    ei = np.asarray(edge_index)
    e, m = ei.shape[1], plan.m
    f32 = np.asarray(base_flow, dtype=np.float64).astype(np.float32)
    x32 = np.asarray(rx, dtype=np.float64)[:, 1].astype(np.float32)
    pa = np.where(plan.ua[ei[0]] >= 0, plan.ua[ei[0]], m)
    pb = np.where(plan.ua[ei[1]] >= 0, plan.ua[ei[1]], m)
    W = np.zeros((m + 1, e), dtype=np.float32)
    lane = np.arange(e)
    np.add.at(W, (pa, lane), np.float32(1))
    np.add.at(W, (pb, lane), np.float32(-1))
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
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        den = np.float32(1) - (W[pa, lane] - W[pb, lane]) / x32                   # [k]
        phi = (W[pa, :] - W[pb, :]) / x32[:, None]                               # [l, k]
        post = (f32[:, None] + (phi / den[None, :]) * f32[None, :]).T           # [k, l]
    post[lane, lane] = 0
    assert post.dtype == np.float32
    return post, den


def worst_ratio(bus_type, spec, edge_index, rx, isl, literal=True):
    """max over the non-bridge outages k and the lines l of |post - f64| / u_k, u_k = 2^-24 max_l |f_l| / |den_k| with the yardstick's
    den_k; f64: the literal re-solve, or the yardstick's float64 lodf form where that is too slow."""
    plan = dc_plan(bus_type, edge_index)
    f = R.base_flow(bus_type, spec, edge_index, rx)
    post, _ = lanes(plan, factor(plan, bus_type, spec, edge_index, rx), edge_index, rx, f)
    want, den = R.lodf(bus_type, spec, edge_index, rx)
    if literal:
        want = R.resolve(bus_type, spec, edge_index, rx, isl)
    ok = isl == 0
    u = EPS * np.abs(f).max() / np.abs(den[ok])
    return float((np.abs(post[ok].astype(np.float64) - want[ok]) / u[:, None]).max())
