"""numpy yardsticks of the per-bus error analysis (csrc/bus_errors.hip, utils/error_analysis.py), written for the tests: the binning
rule of np.histogram with explicit edges, the accumulate call, the reference's range rule (error_per_feature.py:388-398) and its
report (:247-324).  tests/test_bus_errors_host.py pins them without a GPU; tests/test_gpu_bus_errors.py holds the kernels to them."""
import warnings

import numpy as np

FEATURES = ("Voltage Magnitude", "Voltage Angle", "Active Power", "Reactive Power")


def edge_rule(v, edges):
    """(hist [nbins], below, above, nan) of the values `v` (any float dtype) for increasing float64 `edges`, compared in float64:
    bin i holds edges[i] <= v < edges[i + 1], the last bin also v == edges[-1]."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    edges = np.asarray(edges, dtype=np.float64)
    nbins = edges.size - 1
    nan = np.isnan(v)
    w = v[~nan]
    below, above = w < edges[0], w > edges[-1]
    w = w[~below & ~above]
    i = np.searchsorted(edges, w, side="right") - 1             # edges[i] <= w < edges[i + 1]
    i[w == edges[-1]] = nbins - 1
    i = np.clip(i, 0, nbins - 1)                                # (equal edges: the last bin)
    return np.bincount(i, minlength=nbins).astype(np.int64), int(below.sum()), int(above.sum()), int(nan.sum())


def accumulate(o, y, mask, n_bus, idx, rows, std, mean):
    """The tables' rows and the moments one pfn_bus_errors_accumulate call adds, from float32 numpy arithmetic (every operation
    rounded on its own): {graph g: (row idx[g], err [n, 4], pred [n, 4])} for the graphs with an index inside [0, rows), and
    (count, sum, sum_abs, sum_sq, min, max, abs_terms) -- each [n, 4, 2]; abs_terms [n, 4, 2, 3] = sum |term| of the three sums."""
    o, y = np.asarray(o, dtype=np.float32), np.asarray(y, dtype=np.float32)
    std = np.ones(4, np.float32) if std is None else np.asarray(std, dtype=np.float32)
    mean = np.zeros(4, np.float32) if mean is None else np.asarray(mean, dtype=np.float32)
    G = o.shape[0] // n_bus
    e = ((o - y) * std).reshape(G, n_bus, 4)
    p = (o * std + mean).reshape(G, n_bus, 4)
    assert e.dtype == np.float32 and p.dtype == np.float32
    m = (np.asarray(mask).reshape(G, n_bus, 4) != 0)
    ok = np.asarray([0 <= int(i) < rows for i in idx], dtype=bool)
    written = {g: (int(idx[g]), e[g], p[g]) for g in range(G) if ok[g]}
    e64 = e[ok].astype(np.float64)
    sel = np.stack([m[ok], ~m[ok]], axis=-1)                                             # [G', n, 4, 2]
    ex = e64[..., None]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        count = sel.sum(axis=0).astype(np.float64)
        s = np.where(sel, ex, 0.0).sum(axis=0)
        sa = np.where(sel, np.abs(ex), 0.0).sum(axis=0)
        sq = np.where(sel, ex * ex, 0.0).sum(axis=0)
        fin = sel & ~np.isnan(ex)
        mn = np.where(fin, ex, np.inf).min(axis=0, initial=np.inf)
        mx = np.where(fin, ex, -np.inf).max(axis=0, initial=-np.inf)
        clean = np.nan_to_num(ex, nan=0.0)
        terms = np.stack([np.where(sel, np.abs(clean), 0.0).sum(axis=0)] * 2 + [np.where(sel, clean * clean, 0.0).sum(axis=0)], axis=-1)
    return written, (count, s, sa, sq, mn, mx, terms)


def sum_bound(n_terms, abs_terms):
    """Two double accumulations of `n_terms` terms in arbitrary orders differ by at most 2 * n_terms * 2^-53 * sum |terms|."""
    return 2.0 * n_terms * 2.0 ** -53 * abs_terms


def range_rule(scaled_errors, nbins=300, multiplier=(0.8, 0.8, 0.4, 0.4)):
    """Reference :388-398 on the SCALED float32 errors [S, n, 4]: min and max of a feature times its multiplier (in float64), made
    symmetric about 0 on the larger magnitude, np.linspace."""
    out = np.empty((4, nbins + 1), dtype=np.float64)
    for i in range(4):
        min_value = float(np.min(scaled_errors[:, :, i])) * multiplier[i]
        max_value = float(np.max(scaled_errors[:, :, i])) * multiplier[i]
        if abs(min_value) >= max_value:
            max_value = abs(min_value)
        elif abs(min_value) < max_value:
            min_value = -max_value
        out[i] = np.linspace(min_value, max_value, nbins + 1)
    return out


def report(errors, masks, types):
    """Reference :247-324 on errors [S, n, 4] float32, masks [S, n, 4] (0 / 1) and types [S, n], with float64 statistics of the
    float32 scaled errors; then the same figures over the load (type 2) and the generator (type 1) buses."""
    masks = np.array(masks, dtype=np.float32)
    out = {f"Number of {name}": int(np.sum(masks[0, :, f] == 1)) for f, name in enumerate(FEATURES)}
    masks[masks == 0] = 0.00001
    errors = (np.asarray(errors, dtype=np.float32) * masks).astype(np.float64)
    out["Number of Loads"] = int(np.sum(types[0, :] == 2))
    out["Number of Generators"] = int(np.sum(types[0, :] == 1))

    def figures(buses):
        fig = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            for f, name in enumerate(FEATURES):
                indexes = buses[masks[0, buses, f] == 1]
                sel = np.abs(errors[:, indexes, f].reshape(-1, 1))
                fig[f"Absolute Average of {name}"] = float(np.mean(sel)) if sel.size else float("nan")
                fig[f"Absolute Standard Deviation of {name}"] = float(np.std(sel)) if sel.size else float("nan")
            fig["Average of all errors"] = float(np.mean(errors[:, buses, :]))
            fig["Standard Deviation of all errors"] = float(np.std(errors[:, buses, :]))
        return fig
    out.update(figures(np.arange(errors.shape[1])))
    for title, code in (("Loads", 2), ("Generators", 1)):
        out.update({f"{title}: {k}": v for k, v in figures(np.where(types[0, :] == code)[0]).items()})
    return out
