"""The N-1 screen without a GPU: the yardstick's two forms of the post-outage flows (line outage distribution factors against
literally removing the line and solving again) agree, its islands are right on grids made by hand, `ContingencyResult.ranking` orders
NaN, then +inf, then descending, and the C ABI carries the three symbols and refuses what it must before anything is launched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.synth import make_physical_inputs
from poweflownet_amd.utils.contingency import ContingencyResult, summarise_loadings
from tests import contingency_ref as R


@pytest.mark.parametrize("n,e", [(3, 3), (5, 6), (14, 20)])
def test_lodf_form_equals_removing_the_line_and_solving_again(n, e):
    ei, bt, rx, spec = (t.numpy() for t in make_physical_inputs(n, e, 2, seed=1))
    isl = R.islands(bt, ei)
    assert (isl > 0).any() and (isl == 0).any()
    worst = 0.0
    for s in range(2):
        literal = R.resolve(bt, spec[s], ei, rx[s], isl)
        post, den = R.lodf(bt, spec[s], ei, rx[s])
        fmax = np.abs(R.base_flow(bt, spec[s], ei, rx[s])).max()
        for k in np.flatnonzero(isl == 0):
            assert abs(den[k]) >= 0.05
            bound = 1e-8 * max(1.0, fmax) / abs(den[k])
            worst = max(worst, float(np.abs(post[k] - literal[k]).max() / bound))
        assert np.isnan(literal[isl > 0]).all() and (np.abs(den[isl > 0]) < 1e-9).all()      # a bridge: den = 0 up to rounding
    print(f"n {n} e {e}: worst |lodf - literal| / bound {worst:.3g}")
    assert worst <= 1.0


def _types(n, slack=0):
    bt = np.full(n, 2)
    bt[slack] = 0
    return bt


def test_islands_of_grids_made_by_hand():
    n = 6
    path = np.array([[0, 1, 2, 3, 4], [1, 2, 3, 4, 5]])
    assert R.islands(_types(n), path).tolist() == [n - 1 - p for p in range(n - 1)]
    ring = np.array([[0, 1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 0]])
    assert R.islands(_types(n), ring).tolist() == [0] * 6
    pendant = np.array([[0, 1, 2, 3, 2], [1, 2, 3, 0, 4]])                  # a ring of four and bus 4 hanging off bus 2
    assert R.islands(_types(5), pendant).tolist() == [0, 0, 0, 0, 1]
    assert R.islands(_types(5, slack=4), pendant).tolist() == [0, 0, 0, 0, 4]  # seen from the pendant bus the ring is lost
    doubled = np.array([[0, 1, 1, 2], [1, 2, 2, 0]])                        # lines 1 and 2 are parallel
    assert R.islands(_types(3), doubled).tolist() == [0, 0, 0, 0]
    assert R.islands(_types(3), np.array([[0, 1, 1], [1, 2, 2]])).tolist() == [2, 0, 0]      # ... also where the rest is a path
    assert R.islands(_types(3), np.array([[0, 1], [1, 3]])).tolist() == [-4, -4]


def test_summaries_follow_the_rules():
    post = np.array([[0.0, 2.0, -2.0, 0.5], [1.0, 0.0, np.nan, 0.2], [0.1, 0.2, 0.0, 0.3], [np.nan] * 4])
    isl = np.array([0, 0, 0, 2])
    sev, worst, over = R.summarise(post, None, isl)
    assert worst.tolist() == [1, 2, 3, -1] and over.tolist() == [2, 0, 0, -1]            # a tie goes to the lowest line; NaN is the largest
    assert sev[0] == 2.0 and np.isnan(sev[1]) and sev[2] == 0.3 and sev[3] == np.inf
    sev, worst, over = R.summarise(post, np.array([1.0, 0.0, -1.0, np.nan]), isl)        # only line 0 is monitored
    assert worst.tolist() == [-1, 0, 0, -1] and over.tolist() == [0, 0, 0, -1] and sev.tolist()[:3] == [0.0, 1.0, 0.1]
    # the torch form verify_contingencies uses agrees with the yardstick on the same rows
    load = torch.tensor(np.abs(post[:3]), dtype=torch.float32)
    mon = torch.ones(3, 4, dtype=torch.bool) & ~torch.eye(4, dtype=torch.bool)[:3]
    s, w, o = summarise_loadings(load, mon)
    assert w.tolist() == [1, 2, 3] and o.tolist() == [2, 0, 0] and float(s[0]) == 2.0 and bool(torch.isnan(s[1]))
    s, w, o = summarise_loadings(load, torch.zeros(3, 4, dtype=torch.bool))
    assert s.tolist() == [0.0] * 3 and w.tolist() == [-1] * 3 and o.tolist() == [0] * 3


def test_ranking_puts_nan_first_then_inf_then_descending():
    nan, inf = float("nan"), float("inf")
    sev = torch.tensor([[0.5, inf, 2.0, nan, 2.0, 0.0, inf], [1.0, 1.0, 3.0, 0.25, 0.5, 0.75, 2.0]])
    z = torch.zeros(2, 7, dtype=torch.int32)
    res = ContingencyResult(severity=sev, worst_line=z, overloads=z, islands=z[0], base_flow=sev.double(), status=z[:, 0], post_flow=None, route="lds")
    ids, vals = res.ranking(7)
    assert ids.dtype == torch.int64 and ids.tolist() == [[3, 1, 6, 2, 4, 0, 5], [2, 6, 0, 1, 5, 4, 3]]
    assert bool(torch.isnan(vals[0, 0])) and vals[0, 1:].tolist() == [inf, inf, 2.0, 2.0, 0.5, 0.0]
    ids, vals = res.ranking(3)
    assert ids.tolist() == [[3, 1, 6], [2, 6, 0]] and vals[1].tolist() == [3.0, 2.0, 1.0]
    with pytest.raises(ValueError, match="top"):
        res.ranking(8)


def test_abi_surface_and_refusals():
    names = ("pfn_contingency_islands", "pfn_contingency_workspace_bytes", "pfn_contingency_dc")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pfn_hip.h")).read()
    lib = L.load()
    for name in names:
        assert name in L.SYMBOLS and name + "(" in header and hasattr(lib, name)
    assert lib.pfn_abi_version() == 8
    # the LDS route costs no workspace; the global route one slab of (n - 1) x ((n - 1) | 1) floats per scenario, rounded to 16 bytes
    assert lib.pfn_contingency_workspace_bytes(4096, 118, 186, 0) == 0 and lib.pfn_contingency_workspace_bytes(8, 14, 20, 1) == 0
    assert lib.pfn_contingency_workspace_bytes(8, 14, 20, 2) == 8 * 4 * ((13 * 13 + 3) // 4 * 4)
    assert lib.pfn_contingency_workspace_bytes(3, 200, 300, 0) == 3 * 4 * ((199 * 199 + 3) // 4 * 4)
    assert lib.pfn_contingency_workspace_bytes(1, int(lib.pfn_powerflow_max_unknowns()) + 2, 10, 2) == 0
    p = C.c_void_p(256)                                                      # (never followed: every call below is refused first)
    assert lib.pfn_contingency_islands(p, 20, 14, 14, p, None) == -1 and b"root 14" in lib.pfn_last_error()
    assert lib.pfn_contingency_islands(p, 60000, 6470, 0, p, None) == -1 and b"bytes of LDS" in lib.pfn_last_error()
    assert lib.pfn_contingency_islands(None, 0, 14, 0, None, None) == 0

    def dc(n_lines=20, n_bus=14, n_pv=4, n_pq=9, tol=1e-8, route=0, S=4, ws=None, ws_bytes=0):
        return lib.pfn_contingency_dc(p, n_lines, p, p, p, None, 0, p, S, n_bus, n_pv, n_pq, tol, 10, route, p, p, p, p, p, None, p, ws, ws_bytes, None)
    assert dc(n_pq=8) == -1 and b"exactly one slack" in lib.pfn_last_error()
    assert dc(route=3) == -1 and b"route" in lib.pfn_last_error()
    assert dc(tol=0.0) == -1 and b"tol" in lib.pfn_last_error()
    assert dc(n_bus=1, n_pv=0, n_pq=0) == -1 and b"bad sizes" in lib.pfn_last_error()
    assert dc(n_bus=1100, n_pv=0, n_pq=1099) == -1 and b"dense" in lib.pfn_last_error()
    assert dc(n_lines=300, n_bus=200, n_pv=0, n_pq=199, route=1) == -1 and b"bytes of LDS" in lib.pfn_last_error()
    assert dc(n_lines=300, n_bus=200, n_pv=0, n_pq=199) == -2 and b"workspace" in lib.pfn_last_error()
    assert dc(route=2) == -2 and b"workspace" in lib.pfn_last_error()
    assert dc(S=0) == 0
