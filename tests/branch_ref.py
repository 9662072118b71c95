"""float64 numpy yardstick of the per-line branch analysis (csrc/branch_flows.hip, utils/branch_analysis.py), written for the tests:
the four quantities (I, P, Q, loss) per (sample, stored line), the moments of their error, the scales of the tests' error bound and
the random inputs the tests share.  Everything is computed from the kernel's own fp32 inputs; the bus rows are de-normalised in
float32 first, product and sum rounded separately, as the kernel does.  tests/test_branch_host.py pins it without a GPU;
tests/test_gpu_branch.py holds the kernel to it."""
import warnings

import numpy as np

EPS = 2.0 ** -24
C_BOUND = 32.0


def denorm_rows(table, std=None, mean=None):
    """float32 rows * std + mean with two separately rounded operations (None: the rows as they are)."""
    t = np.asarray(table, dtype=np.float32)
    if std is None and mean is None:
        return t
    sd = np.ones(4, np.float32) if std is None else np.asarray(std, dtype=np.float32)
    mu = np.zeros(4, np.float32) if mean is None else np.asarray(mean, dtype=np.float32)
    p = t * sd
    out = p + mu
    assert p.dtype == np.float32 and out.dtype == np.float32
    return out


def physical_rx(edge_attr, edge_std=None, edge_mean=None):
    """float64 (r, x) from the fp32 attributes and fp32 statistics: attr * std + mean, exact products widened."""
    ea = np.asarray(edge_attr, dtype=np.float32).astype(np.float64)
    sd = np.ones(2) if edge_std is None else np.asarray(edge_std, dtype=np.float32).astype(np.float64)
    mu = np.zeros(2) if edge_mean is None else np.asarray(edge_mean, dtype=np.float32).astype(np.float64)
    return ea * sd + mu


def _gather(a, idx):
    """a [S, n] at idx [e] (one list) or [S, e] (per sample) -> [S, e]."""
    return a[:, idx] if idx.ndim == 1 else np.take_along_axis(a, idx, axis=1)


def flows(table, edge_index, rx):
    """(flows [S, e, 4] float64 = (I, P, Q, loss), scales [S, e, 4] of the tests' bound) from PHYSICAL fp32 bus rows [S, n, 4],
    int64 lines [2, e] or [S, 2, e] and float64 (r, x) [e, 2] or [S, e, 2]."""
    t = np.asarray(table, dtype=np.float32).astype(np.float64)
    vm, th = t[:, :, 0], t[:, :, 1] * (np.pi / 180.0)
    e_, f_ = vm * np.cos(th), vm * np.sin(th)
    ei = np.asarray(edge_index)
    i, j = (ei[0], ei[1]) if ei.ndim == 2 else (ei[:, 0], ei[:, 1])
    rx = np.asarray(rx, dtype=np.float64)
    r, x = rx[..., 0], rx[..., 1]                                            # [e] or [S, e]: broadcasts against [S, e]
    ei_, fi_, ej_, fj_ = _gather(e_, i), _gather(f_, i), _gather(e_, j), _gather(f_, j)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        d = r * r + x * x
        g, b = r / d, -x / d
        de, df = ei_ - ej_, fi_ - fj_
        cur = np.sqrt(de * de + df * df) / np.sqrt(d)
        p = g * (ei_ * ej_ - ei_ ** 2 + fi_ * fj_ - fi_ ** 2) + b * (fi_ * ej_ - ei_ * fj_)
        q = g * (fi_ * ej_ - ei_ * fj_) + b * (-ei_ * ej_ + ei_ ** 2 - fi_ * fj_ + fi_ ** 2)
        loss = g * (de * de + df * df)
        vmi, vmj, thi, thj = _gather(vm, i), _gather(vm, j), _gather(th, i), _gather(th, j)
        A = (1 + np.abs(thi)) * vmi + (1 + np.abs(thj)) * vmj
        spq = (np.abs(g) + np.abs(b)) * A * (vmi + vmj)
        scales = np.stack([A / np.sqrt(d), spq, spq, np.abs(g) * A * (vmi + vmj)], axis=-1)
    return np.stack([cur, p, q, loss], axis=-1), scales


def moments(err, valid=None):
    """(count, sum, sum_abs, sum_sq, min, max, abs_terms) -- each [e, 4]; abs_terms [e, 4, 3] = sum |term| of the three sums -- of an
    error table [S, e, 4], widened to float64; `valid` [S, e] (None: all) selects the (sample, line) pairs that count.  min / max
    ignore NaN, the sums propagate it."""
    ex = np.asarray(err).astype(np.float64)
    sel = np.ones(ex.shape[:2], dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    sel = np.broadcast_to(sel[..., None], ex.shape)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        count = sel.sum(axis=0).astype(np.float64)
        s = np.where(sel, ex, 0.0).sum(axis=0)
        sa = np.where(sel, np.abs(ex), 0.0).sum(axis=0)
        sq = np.where(sel, ex * ex, 0.0).sum(axis=0)
        fin = sel & ~np.isnan(ex)
        mn = np.where(fin, ex, np.inf).min(axis=0, initial=np.inf)
        mx = np.where(fin, ex, -np.inf).max(axis=0, initial=-np.inf)
        clean = np.where(sel, np.nan_to_num(ex, nan=0.0), 0.0)
        terms = np.stack([np.abs(clean).sum(axis=0)] * 2 + [(clean * clean).sum(axis=0)], axis=-1)
    return count, s, sa, sq, mn, mx, terms


def bus_sums(table, edge_index, rx):
    """mean_i (dP_i^2 + dQ_i^2) of ONE sample, formed from the yardstick's table of a stored-once list: the messages of the stored
    direction summed onto `from`, the reverse direction's -P - r I^2 / -Q - x I^2 summed onto `to`.  table: [n, 4] physical fp32."""
    t = np.asarray(table, dtype=np.float32)
    fl = flows(t[None], edge_index, rx)[0][0]
    r, x = np.asarray(rx)[:, 0], np.asarray(rx)[:, 1]
    i2 = fl[:, 0] ** 2
    sp, sq = np.zeros(t.shape[0]), np.zeros(t.shape[0])
    np.add.at(sp, edge_index[0], fl[:, 1])
    np.add.at(sp, edge_index[1], -fl[:, 1] - r * i2)
    np.add.at(sq, edge_index[0], fl[:, 2])
    np.add.at(sq, edge_index[1], -fl[:, 2] - x * i2)
    t64 = t.astype(np.float64)
    return float(np.mean((t64[:, 2] - sp) ** 2 + (t64[:, 3] - sq) ** 2))


# ------------------------------------------------------------------------------------------------ shared inputs
def topology(n, e, rng):
    """A random spanning tree plus extra lines, no self-loops: int64 [2, e], each line stored once in a random direction."""
    assert e >= n - 1
    src, dst = np.empty(e, dtype=np.int64), np.empty(e, dtype=np.int64)
    for k in range(1, n):
        src[k - 1], dst[k - 1] = rng.integers(0, k), k
    k = n - 1
    while k < e:
        a, b = int(rng.integers(0, n)), int(rng.integers(0, n))
        if a != b:
            src[k], dst[k] = a, b
            k += 1
    flip = rng.random(e) < 0.5
    return np.stack([np.where(flip, dst, src), np.where(flip, src, dst)])


STD4 = np.array([0.05, 20.0, 50.0, 20.0], dtype=np.float32)
MEAN4 = np.array([1.0, 0.0, 30.0, -10.0], dtype=np.float32)
EDGE_STD = np.array([0.03, 0.15], dtype=np.float32)          # |edge mean| <= edge std
EDGE_MEAN = np.array([0.03, 0.15], dtype=np.float32)


def bus_table(S, n, rng, normalised):
    """[S, n, 4] float32 with Vm in [0.9, 1.1] and Va in [-60, 60] degrees (after de-normalisation with STD4 / MEAN4 when
    `normalised`; a margin keeps the fp32 round trip inside)."""
    phys = np.stack([rng.uniform(0.901, 1.099, (S, n)), rng.uniform(-59.9, 59.9, (S, n)), rng.normal(30.0, 50.0, (S, n)),
                     rng.normal(-10.0, 20.0, (S, n))], axis=-1)
    if not normalised:
        return phys.astype(np.float32)
    return ((phys - MEAN4.astype(np.float64)) / STD4.astype(np.float64)).astype(np.float32)


def edge_attrs(shape, rng):
    """Normalised float32 attributes [..., 2] with r in [0.01, 0.1] and x in [0.05, 0.5] after de-normalisation with EDGE_STD /
    EDGE_MEAN (a margin keeps the fp32 values inside)."""
    r = rng.uniform(0.0101, 0.0999, shape)
    x = rng.uniform(0.0501, 0.4999, shape)
    phys = np.stack([r, x], axis=-1)
    return ((phys - EDGE_MEAN.astype(np.float64)) / EDGE_STD.astype(np.float64)).astype(np.float32)
