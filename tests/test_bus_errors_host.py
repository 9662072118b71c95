"""Host side of the per-bus error analysis (utils/error_analysis.py): `histogram_edges` and `report_lines` from moments built in
numpy against direct numpy computations on random [S, n, 4] arrays, and the yardsticks the GPU tests use (tests/bus_errors_ref.py)
against np.histogram itself.  No GPU."""
import math

import numpy as np
import pytest
import torch

from poweflownet_amd.synth import _MASK_TABLE
from poweflownet_amd.utils.error_analysis import histogram_edges, mask_scale, report_lines
from tests import bus_errors_ref as R


def _split(S=23, n=14, seed=0, shift=(0.3, -0.5, 2.0, 0.1)):
    rng = np.random.default_rng(seed)
    types = np.full(n, 2, dtype=np.int64)
    types[::3] = 1
    types[0] = 0
    mask = _MASK_TABLE.numpy()[types]
    errors = (rng.normal(size=(S, n, 4)) * np.array([0.05, 3.0, 40.0, 15.0]) + np.array(shift)).astype(np.float32)
    return errors, mask, types


def _moments(errors, mask):
    """[n, 4, 2, 6] float64 from a table and ONE mask for every sample."""
    e = errors.astype(np.float64)
    S, n, _ = e.shape
    m = np.zeros((n, 4, 2, 6))
    m[..., 4], m[..., 5] = np.inf, -np.inf
    for g, sel in enumerate((mask != 0, mask == 0)):
        m[sel, g, 0] = S
        m[sel, g, 1] = e.sum(axis=0)[sel]
        m[sel, g, 2] = np.abs(e).sum(axis=0)[sel]
        m[sel, g, 3] = (e * e).sum(axis=0)[sel]
        m[sel, g, 4] = e.min(axis=0)[sel]
        m[sel, g, 5] = e.max(axis=0)[sel]
    return m


@pytest.mark.parametrize("shift", [(0.3, 9.0, 200.0, 60.0), (-0.3, -9.0, -200.0, -60.0)])     # second: the branch |min| >= max
@pytest.mark.parametrize("nbins", [300, 7])
def test_histogram_edges_follow_the_reference_range_rule(shift, nbins):
    errors, mask, _ = _split(shift=shift)
    scale = mask_scale(torch.from_numpy(mask))
    assert scale.dtype == torch.float32 and set(scale.unique().tolist()) == {float(np.float32(0.00001)), 1.0}
    scaled = errors * scale.numpy()[None]
    assert scaled.dtype == np.float32
    want = R.range_rule(scaled, nbins)
    lo, hi = scaled.reshape(-1, 4).min(axis=0), scaled.reshape(-1, 4).max(axis=0)
    assert ((np.abs(lo) >= hi) == (shift[0] < 0)).all()
    got = histogram_edges(_moments(errors, mask), scale, nbins=nbins)
    assert got.dtype == np.float64 and got.shape == (4, nbins + 1) and np.array_equal(got, want)
    assert np.array_equal(got[:, 0], -got[:, -1])
    # another multiplier and no scale
    want2 = R.range_rule(errors, nbins, multiplier=(0.3, 0.6, 0.4, 1.0))
    assert np.array_equal(histogram_edges(torch.from_numpy(_moments(errors, mask)), None, nbins=nbins, multiplier=(0.3, 0.6, 0.4, 1.0)), want2)


def test_report_lines_from_moments_match_the_direct_computation():
    errors, mask, types = _split(S=57, n=30, seed=4)
    S, n, _ = errors.shape
    want = R.report(errors, np.broadcast_to(mask, (S, n, 4)), np.broadcast_to(types, (S, n)))
    got = report_lines(_moments(errors, mask), torch.from_numpy(mask), torch.from_numpy(types))
    assert list(got) == list(want)
    assert list(got)[:6] == ["Number of Voltage Magnitude", "Number of Voltage Angle", "Number of Active Power", "Number of Reactive Power",
                             "Number of Loads", "Number of Generators"]
    assert got["Number of Loads"] == int((types == 2).sum()) and got["Number of Voltage Magnitude"] == int((types == 2).sum())
    checked = 0
    for k, w in want.items():
        g = got[k]
        if isinstance(w, int):
            assert g == w, k
        elif math.isnan(w):
            assert math.isnan(g), k                      # (a bus type that predicts none of a feature: the mean of nothing)
        else:
            assert abs(g - w) <= 1e-9 * abs(w), (k, g, w)
            checked += 1
    assert checked >= 20
    assert math.isnan(want["Loads: Absolute Average of Active Power"]) and not math.isnan(want["Generators: Absolute Average of Reactive Power"])


@pytest.mark.parametrize("nbins", [1, 7, 300, 2048])
def test_the_edge_rule_yardstick_is_np_histogram(nbins):
    rng = np.random.default_rng(nbins)
    edges = np.linspace(-0.7, 1.9, nbins + 1)
    v = rng.uniform(-1.0, 2.2, size=5000).astype(np.float32)
    planted = [np.float32(edges[0]), np.float32(edges[nbins // 2]), np.float32(edges[-1]), np.nextafter(np.float32(edges[0]), np.float32(-np.inf)),
               np.nextafter(np.float32(edges[-1]), np.float32(np.inf)), np.float32(np.inf), np.float32(-np.inf)]
    planted += [np.float32(x) for x in edges[:: max(1, nbins // 50)]]
    v[:len(planted)] = planted
    hist, below, above, nan = R.edge_rule(v, edges)
    want, _ = np.histogram(v.astype(np.float64), bins=edges)
    assert np.array_equal(hist, want)
    assert below == int((v.astype(np.float64) < edges[0]).sum()) and above == int((v.astype(np.float64) > edges[-1]).sum()) and nan == 0
    assert hist.sum() + below + above == v.size
    # exact float64 edges land where np.histogram puts them: edge i opens bin i, the last edge closes the last bin
    h2, b2, a2, _ = R.edge_rule(edges, edges)
    assert np.array_equal(h2, np.histogram(edges, bins=edges)[0]) and b2 == a2 == 0 and h2[-1] == 2
    # NaN is counted apart and enters no bin
    w = v.copy()
    w[100:110] = np.nan
    h3, b3, a3, n3 = R.edge_rule(w, edges)
    assert n3 == 10 and h3.sum() + b3 + a3 + n3 == w.size
    assert np.array_equal(h3, np.histogram(w[~np.isnan(w)].astype(np.float64), bins=edges)[0])


def test_the_accumulate_yardstick_on_a_hand_made_batch():
    o = np.array([[1, 2, 3, 4], [5, 6, 7, 8]], dtype=np.float32)              # one bus, two graphs
    y = np.zeros_like(o)
    mask = np.array([[1, 0, 1, 0], [1, 0, 0, 1]])
    written, (cnt, s, sa, sq, mn, mx, _) = R.accumulate(o, y, mask, 1, [1, 5], 3, [2, 2, 2, 2], [1, 1, 1, 1])
    assert list(written) == [0] and written[0][0] == 1                          # graph 1 names row 5 of 3: left out
    assert np.array_equal(written[0][1], [[2, 4, 6, 8]]) and np.array_equal(written[0][2], [[3, 5, 7, 9]])
    assert np.array_equal(cnt[0], [[1, 0], [0, 1], [1, 0], [0, 1]])
    assert np.array_equal(s[0], [[2, 0], [0, 4], [6, 0], [0, 8]]) and np.array_equal(sq[0], [[4, 0], [0, 16], [36, 0], [0, 64]])
    assert mn[0, 0, 0] == 2 and mn[0, 0, 1] == np.inf and mx[0, 1, 1] == 4 and mx[0, 1, 0] == -np.inf
