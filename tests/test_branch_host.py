"""The per-line branch analysis without a GPU: the float64 yardstick of tests/branch_ref.py against the CPU oracle's PowerImbalance,
its own identities and the reference's commented-out expression; `branch_report_lines` and the widened `histogram_edges` against
direct numpy; and `pfn_branch_flows`' argument checks, which answer before anything touches a device."""
import math

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from poweflownet_amd import _lib as L
from poweflownet_amd.utils.branch_analysis import QUANTITIES, branch_report_lines
from poweflownet_amd.utils.error_analysis import histogram_edges
from tests import branch_ref as R
from tests import bus_errors_ref as BR


def _grid(n, e, seed):
    rng = np.random.default_rng(seed)
    ei = R.topology(n, e, rng)
    table = R.bus_table(1, n, rng, normalised=False)[0]
    rx = R.physical_rx(R.edge_attrs((e,), rng), R.EDGE_STD, R.EDGE_MEAN)
    return ei, table, rx


@pytest.mark.parametrize("n,e", [(14, 20), (118, 186), (300, 411)])
def test_bus_sums_of_the_table_are_the_oracles_power_imbalance(n, e):
    for seed in range(20):
        ei, table, rx = _grid(n, e, 1000 * n + seed)
        if ref_cpu.is_directed(torch.from_numpy(ei)):
            break
    assert ref_cpu.is_directed(torch.from_numpy(ei))
    one4, zero4 = torch.ones(1, 4, dtype=torch.float64), torch.zeros(1, 4, dtype=torch.float64)
    one2, zero2 = torch.ones(1, 2, dtype=torch.float64), torch.zeros(1, 2, dtype=torch.float64)
    want = float(ref_cpu.power_imbalance(torch.from_numpy(table.astype(np.float64)), torch.from_numpy(ei), torch.from_numpy(rx), zero4,
                                         one4, zero2, one2))
    got = R.bus_sums(table, ei, rx)
    print(f"n {n}: {got!r} against {want!r}, relative difference {abs(got - want) / abs(want):.2e}")
    assert abs(got - want) <= 1e-12 * abs(want)


def test_loss_is_r_i_squared_and_the_scales_are_positive():
    ei, table, rx = _grid(118, 186, 5)
    fl, scales = R.flows(table[None], ei, rx)
    assert np.abs(fl[0, :, 3] - rx[:, 0] * fl[0, :, 0] ** 2).max() <= 1e-12 * np.abs(fl[0, :, 3]).max()
    assert (fl[0, :, 3] >= 0).all() and (fl[0, :, 0] >= 0).all() and (scales > 0).all()
    # a per-sample list and per-sample attributes give the same rows as the shared ones
    fl2, _ = R.flows(np.stack([table, table]), np.stack([ei, ei]), np.stack([rx, rx]))
    assert np.array_equal(fl2[0], fl[0]) and np.array_equal(fl2[1], fl[0])


def test_current_is_the_references_commented_expression():
    # a hand-made 3-bus case, the reference's error_per_feature.py:201-205 evaluated literally
    preds = np.array([[[1.05, 0.0, 0.0, 0.0], [1.0, -4.0, 0.0, 0.0], [0.97, -9.5, 0.0, 0.0]]], dtype=np.float32)
    lines = np.array([[0, 1, 2], [1, 2, 0]])
    r_t, x_t = np.array([0.02, 0.05, 0.01], dtype=np.float32), np.array([0.06, 0.19, 0.25], dtype=np.float32)
    fl, _ = R.flows(preds, lines, np.stack([r_t, x_t], axis=-1).astype(np.float64))
    mp = math.pi / 180
    for k in range(3):
        i, j = int(lines[0, k]), int(lines[1, k])
        r, x = float(r_t[k]), float(x_t[k])
        p = preds.astype(np.float64)
        i_pred = math.sqrt((p[0, i, 0] * math.cos(p[0, i, 1] * mp) - p[0, j, 0] * math.cos(p[0, j, 1] * mp)) ** 2 +
                           (p[0, i, 0] * math.sin(p[0, i, 1] * mp) - p[0, j, 0] * math.sin(p[0, j, 1] * mp)) ** 2) \
            / math.sqrt(r ** 2 + x ** 2)
        assert abs(fl[0, k, 0] - i_pred) <= 1e-14 * i_pred
    assert 0.5 < fl[0, 0, 0] < 2.0                                           # 0.05 pu and 4 degrees across |z| = 0.063


def test_denormalised_rows_are_two_rounded_operations():
    rng = np.random.default_rng(3)
    t = R.bus_table(4, 9, rng, normalised=True)
    back = R.denorm_rows(t, R.STD4, R.MEAN4)
    assert back.dtype == np.float32
    assert np.array_equal(back, (torch.from_numpy(t) * torch.from_numpy(R.STD4) + torch.from_numpy(R.MEAN4)).numpy())
    assert 0.9 <= back[..., 0].min() and back[..., 0].max() <= 1.1 and np.abs(back[..., 1]).max() <= 60.0
    rx = R.physical_rx(R.edge_attrs((50,), rng), R.EDGE_STD, R.EDGE_MEAN)
    assert 0.01 <= rx[:, 0].min() and rx[:, 0].max() <= 0.1 and 0.05 <= rx[:, 1].min() and rx[:, 1].max() <= 0.5
    assert (np.abs(R.EDGE_MEAN) <= R.EDGE_STD).all()


def _table(S, e, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(S, e, 4)) * np.array([0.1, 2.0, 3.0, 0.01])).astype(np.float32)


def _moments_of(err, valid=None):
    count, s, sa, sq, mn, mx, _ = R.moments(err, valid)
    return np.stack([count, s, sa, sq, mn, mx], axis=-1)


def test_report_lines_against_direct_numpy():
    err = _table(23, 11, 1)
    lines = branch_report_lines(_moments_of(err))
    e64 = err.astype(np.float64)
    want = {"i_error_table mean": np.mean(np.abs(e64[:, :, 0])), "i_error_table std": np.std(np.abs(e64[:, :, 0]))}
    for q, name in enumerate(QUANTITIES):
        want[f"Absolute Average of {name}"] = np.mean(np.abs(e64[:, :, q]))
        want[f"Absolute Standard Deviation of {name}"] = np.std(np.abs(e64[:, :, q]))
    for q, name in enumerate(QUANTITIES):
        s, k = np.unravel_index(np.argmax(np.abs(e64[:, :, q])), e64.shape[:2])
        want[f"Largest error of {name}: line"] = int(k)
        want[f"Largest error of {name}"] = float(e64[s, k, q])
    assert list(lines) == list(want)
    assert list(lines)[:4] == ["i_error_table mean", "i_error_table std", "Absolute Average of Line Current",
                               "Absolute Standard Deviation of Line Current"]
    for key, w in want.items():
        if key.endswith(": line"):
            assert lines[key] == w, key
        else:
            assert abs(lines[key] - w) <= 1e-9 * abs(w), (key, lines[key], w)
    assert lines["i_error_table mean"] == lines["Absolute Average of Line Current"]
    # a line no sample counted for (a bad id) changes nothing; torch moments are accepted; nothing at all gives NaN
    valid = np.ones((23, 11), dtype=bool)
    valid[:, 4] = False
    err2 = err.copy()
    err2[:, 4] = np.nan
    part = branch_report_lines(torch.from_numpy(_moments_of(err2, valid)))
    keep = np.delete(e64, 4, axis=1)
    assert abs(part["i_error_table mean"] - np.mean(np.abs(keep[:, :, 0]))) <= 1e-12
    assert part["Largest error of Active Flow: line"] != 4
    assert math.isnan(branch_report_lines(_moments_of(err[:0]))["i_error_table mean"])


def test_histogram_edges_accepts_one_group():
    err = _table(40, 7, 2)
    m3 = _moments_of(err)
    edges = histogram_edges(m3, nbins=50)
    assert np.array_equal(edges, BR.range_rule(err, nbins=50))
    # ... and the two-group form is what it was: the same table split over the groups
    m4 = np.zeros((7, 4, 2, 6))
    m4[..., 4], m4[..., 5] = np.inf, -np.inf
    m4[:, :, 0] = _moments_of(err[:25])
    m4[:, :, 1] = _moments_of(err[25:])
    assert np.array_equal(histogram_edges(m4, nbins=50), edges)
    scale = np.full((7, 4), 0.5, dtype=np.float32)
    assert np.array_equal(histogram_edges(m3, scale, nbins=50), BR.range_rule(err * scale[None], nbins=50))


def test_argument_errors_are_reported_not_fatal():
    lib = L.load()
    assert lib.pfn_branch_flows_lds_max_bus() == (160 * 1024 - 1024) // 16
    assert lib.pfn_branch_flows_workspace_bytes(3, 5, 0) == 0 and lib.pfn_branch_flows_workspace_bytes(3, 5, 1) == 3 * 5 * 16
    buf = (L.C.c_double * 64)()                                             # host memory: every call below fails before a launch
    a = L.C.addressof(buf)
    a += (-a) % 16
    call = lib.pfn_branch_flows
    cases = [
        ("null prediction table", (None, 0, a, 0, 1, 1, None, None, a, 0, 1, a, 0, None, None, a, None, None, None, a, None, 0, None)),
        ("need a truth table", (a, 0, None, 0, 1, 1, None, None, a, 0, 1, a, 0, None, None, a, None, None, a, a, None, 0, None)),
        ("need a truth table", (a, 0, None, 0, 1, 1, None, None, a, 0, 1, a, 0, None, None, a, None, a, None, a, None, 0, None)),
        ("bad sizes", (a, 0, a, 0, -1, 1, None, None, a, 0, 1, a, 0, None, None, a, None, None, None, a, None, 0, None)),
        ("bad sizes", (a, 0, a, 0, 1, -2, None, None, a, 0, 1, a, 0, None, None, a, None, None, None, a, None, 0, None)),
        ("bad sizes", (a, 0, a, 0, 1, 1, None, None, a, 0, -3, a, 0, None, None, a, None, None, None, a, None, 0, None)),
        ("bad sizes", (a, 0, a, 0, 1 << 20, 1 << 20, None, None, a, 0, 1, a, 0, None, None, a, None, None, None, a, None, 0, None)),
        ("null flags", (a, 0, a, 0, 1, 1, None, None, a, 0, 1, a, 0, None, None, a, None, None, None, None, None, 0, None)),
        ("null edge_index or edge_attr", (a, 0, a, 0, 1, 1, None, None, None, 0, 1, a, 0, None, None, a, None, None, None, a, None, 0, None)),
        ("16-byte aligned", (a + 4, 0, a, 0, 1, 1, None, None, a, 0, 1, a, 0, None, None, a, None, None, None, a, None, 0, None)),
    ]
    for want, args in cases:
        rc = call(*args)
        assert rc == -1 and want.encode() in lib.pfn_last_error(), (want, rc, lib.pfn_last_error())
    # moments without an error table need the workspace: its own code, and a message that says how much
    rc = call(a, 0, a, 0, 2, 1, None, None, a, 0, 3, a, 0, None, None, None, None, None, a, a, None, 0, None)
    assert rc == -2 and b"96 bytes" in lib.pfn_last_error(), (rc, lib.pfn_last_error())
    # nothing to do is not an error: no samples, or no lines
    assert call(None, 0, None, 0, 0, 5, None, None, None, 0, 4, None, 0, None, None, None, None, None, a, a, None, 0, None) == 0
    assert call(a, 0, a, 0, 3, 5, None, None, None, 0, 0, None, 0, None, None, None, None, None, a, a, None, 0, None) == 0
