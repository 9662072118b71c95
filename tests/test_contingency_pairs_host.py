"""The N-2 pair screen without a GPU: the yardstick's two forms of the post-pair flows (the rank-2 update of the inverse against
literally removing both lines and solving again) agree, pairs island buses although neither line is a bridge, the pair index
helpers round-trip, `lines` is validated on the host before any library call, `PairContingencyResult.ranking` has
`ContingencyResult.ranking`'s order, and the header, `_lib.py` and the wrapper name the same three symbols."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.synth import make_physical_inputs
from poweflownet_amd.utils import contingency as K
from poweflownet_amd.utils.contingency import PairContingencyResult, contingency_screen_pairs, pair_index, pair_lines, pair_positions
from tests import contingency_pairs_ref as R2
from tests import contingency_ref as R

NAMES = ("pfn_contingency_pair_islands", "pfn_contingency_pairs_workspace_bytes", "pfn_contingency_pairs")


@pytest.mark.parametrize("n,e,c", [(5, 6, None), (14, 20, None), (70, 100, 30)])
def test_rank_two_form_equals_removing_both_lines_and_solving_again(n, e, c):
    ei, bt, rx, spec = (t.numpy() for t in make_physical_inputs(n, e, 2, seed=1))
    pairs = R2.pair_list(e)
    if c is not None:                                                       # a 30-pair subset: every 165th pair of the 4950
        pairs = pairs[::len(pairs) // c][:c]
        assert len(pairs) == 30
    isl = R2.islands(bt, ei, pairs)
    single = R.islands(bt, ei)
    both_fine = (single[pairs[:, 0]] == 0) & (single[pairs[:, 1]] == 0)
    assert (isl > 0).any() and (isl == 0).any()
    if c is None:
        assert ((isl > 0) & both_fine).any()                                # islanding although neither line is a bridge
    worst = 0.0
    for s in range(2):
        literal = R2.resolve_pairs(bt, spec[s], ei, rx[s], pairs, isl)
        post, M = R2.lodf_pairs(bt, spec[s], ei, rx[s], pairs)
        norm, det = R2.inverse_norm(M)
        fmax = np.abs(R.base_flow(bt, spec[s], ei, rx[s])).max()
        ok = isl == 0
        assert norm[ok].max() <= 32 and det[ok].min() >= 0.01
        bound = 1e-8 * max(1.0, fmax) * norm[ok]
        worst = max(worst, float((np.abs(post[ok] - literal[ok]).max(axis=1) / bound).max()))
        assert np.isnan(literal[~ok]).all() and (det[~ok] < 1e-9).all()     # an islanding pair: det M = 0 up to rounding
        assert (literal[ok, pairs[ok, 0]] == 0).all() and (literal[ok, pairs[ok, 1]] == 0).all()
    print(f"n {n} e {e}: {len(pairs)} pairs, {int((isl > 0).sum())} islanding, worst |rank-2 - literal| / bound {worst:.3g}")
    assert worst <= 1.0


def test_the_pair_index_helpers_round_trip():
    for c in (2, 3, 7, 20):
        host = pair_lines(c)
        assert host.dtype == torch.int64 and host.tolist() == R2.pair_list(c).tolist() and len(host) == c * (c - 1) // 2
        for p, (i, j) in enumerate(host.tolist()):
            assert pair_index(i, j, c) == p and pair_positions(p, c) == (i, j)
        assert torch.equal(pair_index(host[:, 0], host[:, 1], c), torch.arange(len(host)))       # tensors too
    lines = [2, 5, 9, 11]
    assert pair_lines(lines).tolist() == [[2, 5], [2, 9], [2, 11], [5, 9], [5, 11], [9, 11]] == R2.pair_list(lines).tolist()
    assert pair_lines(torch.tensor(lines)).tolist() == pair_lines(lines).tolist() and pair_lines(np.array(lines)).tolist() == pair_lines(lines).tolist()
    assert pair_lines(1).shape == (0, 2) and pair_lines([]).shape == (0, 2)
    with pytest.raises(ValueError):
        pair_positions(6, 4)


def test_lines_are_validated_on_the_host_before_any_library_call(monkeypatch):
    def never(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", never)
    monkeypatch.setattr(L, "require_device", never)
    ei, bt, rx, spec = make_physical_inputs(14, 20, 2, seed=1)
    for bad, text in (([3, 1], "increasing"), ([1, 1, 4], "increasing"), ([0, 20], "within"), ([-1, 4], "within"), ([5], "two"), ([], "two"),
                      (torch.tensor([4, 2]), "increasing"), (torch.tensor([1, 2], dtype=torch.int32), "int64"), ([1.5, 2], "ints")):
        with pytest.raises(ValueError, match=text):
            contingency_screen_pairs(bt, spec, ei, rx, lines=bad)
    with pytest.raises(ValueError, match="route"):
        contingency_screen_pairs(bt, spec, ei, rx, route="sparse")


def test_ranking_has_the_single_outage_screens_order():
    nan, inf = float("nan"), float("inf")
    sev = torch.tensor([[0.5, inf, 2.0, nan, 2.0, 0.0], [1.0, 1.0, 3.0, 0.25, 0.5, 0.75]])
    z = torch.zeros(2, 6, dtype=torch.int32)
    res = PairContingencyResult(severity=sev, worst_line=z, overloads=z, islands=z[0], pairs=pair_lines(4), base_flow=sev.double(), status=z[:, 0],
                                post_flow=None, route="lds")
    ids, vals = res.ranking(6)
    assert ids.dtype == torch.int64 and ids.tolist() == [[3, 1, 2, 4, 0, 5], [2, 0, 1, 5, 4, 3]]
    assert bool(torch.isnan(vals[0, 0])) and vals[0, 1:].tolist() == [inf, 2.0, 2.0, 0.5, 0.0]
    assert res.ranking(2)[0].tolist() == [[3, 1], [2, 0]]
    with pytest.raises(ValueError, match="top"):
        res.ranking(7)


def test_header_bindings_and_wrapper_name_the_same_three_symbols():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pfn_hip.h")).read()
    wrapper = inspect.getsource(K)
    lib = L.load()
    for name in NAMES:
        assert name in L.SYMBOLS and name + "(" in header and hasattr(lib, name) and "lib." + name + "(" in wrapper, name
    assert lib.pfn_abi_version() == L.ABI_VERSION


def test_workspace_sizes_and_refusals():
    lib = L.load()
    ws = lib.pfn_contingency_pairs_workspace_bytes
    mat = lambda m: 4 * ((m * (m | 1) + 3) // 4 * 4)                         # noqa: E731
    slab = lambda n, e: (mat(n - 1) + 16 * e + 4 * n + 15) // 16 * 16        # noqa: E731
    # a slab per scenario on either route: X transposed and the staged vectors; the candidates do not enter
    assert ws(8, 14, 20, 20, 0) == ws(8, 14, 20, 5, 2) == ws(8, 14, 20, 20, 1) == 8 * slab(14, 20)
    assert ws(3, 200, 300, 16, 0) == ws(3, 200, 300, 16, 2) == 3 * slab(200, 300)
    # 0 for what the call would refuse: route 1 where X does not fit LDS, beyond the dense cap, more candidates than lines, a bad route
    assert ws(3, 200, 300, 16, 1) == 0 and ws(1, int(lib.pfn_powerflow_max_unknowns()) + 2, 10, 4, 2) == 0
    assert ws(1, 14, 20, 21, 0) == 0 and ws(1, 14, 20, 20, 3) == 0 and ws(0, 14, 20, 20, 0) == 0
    p = C.c_void_p(256)                                                      # (never followed: every call below is refused first)
    isl = lib.pfn_contingency_pair_islands
    assert isl(p, 20, 14, 14, p, 5, p, None) == -1 and b"root 14" in lib.pfn_last_error()
    assert isl(p, 20, 14, 0, p, 21, p, None) == -1 and b"candidates" in lib.pfn_last_error()
    assert isl(p, 60000, 6470, 0, p, 4, p, None) == -1 and b"bytes of LDS" in lib.pfn_last_error()
    assert isl(None, 20, 14, 0, None, 1, None, None) == 0                   # fewer than two candidates: no pair, nothing launched

    def run(n_lines=20, n_bus=14, n_pv=4, n_pq=9, tol=1e-8, route=0, S=4, c=6, ws_ptr=p, ws_bytes=1 << 30):
        return lib.pfn_contingency_pairs(p, n_lines, p, p, p, None, 0, p, c, p, S, n_bus, n_pv, n_pq, tol, 10, route, p, p, p, p, p, None, p,
                                         ws_ptr, ws_bytes, None)
    assert run(n_pq=8) == -1 and b"exactly one slack" in lib.pfn_last_error()
    assert run(route=3) == -1 and b"route" in lib.pfn_last_error()
    assert run(tol=0.0) == -1 and b"tol" in lib.pfn_last_error()
    assert run(c=21) == -1 and b"bad sizes" in lib.pfn_last_error()
    assert run(n_bus=1100, n_pv=0, n_pq=1099) == -1 and b"dense" in lib.pfn_last_error()
    assert run(n_lines=300, n_bus=200, n_pv=0, n_pq=199, route=1) == -1 and b"bytes of LDS" in lib.pfn_last_error()
    assert run(ws_bytes=64) == -2 and b"workspace" in lib.pfn_last_error()
    assert run(ws_ptr=None) == -1 and b"null" in lib.pfn_last_error()
    assert run(S=0) == 0
