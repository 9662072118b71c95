"""The generator-outage screen without a GPU: the yardstick's closed form of the post-outage flows (one column of the inverse per unit,
distribution factors on top for unit x line) agrees with literally editing `spec` -- and deleting the line -- and solving again, under
slack pickup, graded participation, a unit at the slack, two units on one bus, participation on the outaged unit only (rest = 0: the
slack picks up) and p = 0; `units` and `lines` are validated on the host before any library call; the two rankings have
`ContingencyResult.ranking`'s order; and the header, `_lib.py` and the wrapper name the same two symbols, whose refusals come before
anything is launched."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.synth import make_physical_inputs
from poweflownet_amd.utils import contingency as K
from poweflownet_amd.utils.contingency import UnitContingencyResult, contingency_screen_units, unit_outage_spec
from tests import contingency_ref as R
from tests import contingency_units_ref as U

NAMES = ("pfn_contingency_units_workspace_bytes", "pfn_contingency_units")


@pytest.mark.parametrize("n,e", [(5, 6), (14, 20), (70, 100)])
def test_closed_form_equals_editing_spec_and_solving_again(n, e):
    ei, bt, rx, spec = (t.numpy() for t in make_physical_inputs(n, e, 2, seed=1))
    isl = R.islands(bt, ei)
    lines = np.arange(e) if n < 70 else np.arange(0, e, 7)
    ok = isl[lines] == 0
    assert ok.any() and (isl > 0).any()
    slack = int(np.flatnonzero(bt == 0)[0])
    worst = worst2 = 0.0
    for name, (units, p, a) in U.unit_cases(bt).items():
        for s in range(2):
            f = R.base_flow(bt, spec[s], ei, rx[s])
            fmax = np.abs(f).max()
            literal = U.resolve_units(bt, spec[s], ei, rx[s], units, p, a)
            post, d = U.closed_form(bt, spec[s], ei, rx[s], units, p, a)
            worst = max(worst, float(np.abs(post - literal).max() / (1e-8 * max(1.0, fmax))))
            assert np.array_equal(post[1], f)                               # p = 0: exactly the base flows
            if name in ("slack pickup", "zero participation"):
                at_slack = int(np.flatnonzero(units == slack)[0])
                assert np.array_equal(post[at_slack], f) and not d[at_slack].any()      # a unit at the slack: the slack replaces itself
            if name == "participation on one unit only":                    # rest = 0: the slack picks unit 0's output up
                assert np.array_equal(post[0], U.closed_form(bt, spec[s], ei, rx[s], units, p, None)[0][0])
            if a is None:                                                   # two units on one bus: one column, scaled by their outputs
                assert np.allclose((post[-1] - f) * p[0], (post[0] - f) * p[-1], rtol=1e-12, atol=1e-15) and (post[0] != f).any()
            literal2 = U.resolve_unit_lines(bt, spec[s], ei, rx[s], units, p, a, lines, isl)
            post2, den = U.closed_form_lines(bt, ei, rx[s], post, lines)
            assert np.isnan(literal2[:, ~ok]).all() and (np.abs(den[~ok]) < 1e-9).all()
            if n < 70:
                assert np.abs(den[ok]).min() >= 0.05
            bound = 1e-8 * max(1.0, fmax) / np.abs(den[ok])
            worst2 = max(worst2, float((np.abs(post2[:, ok] - literal2[:, ok]).max(axis=2) / bound[None, :]).max()))
            assert (post2[:, np.arange(len(lines)), lines][:, ok] == 0).all()
    print(f"n {n} e {e}: worst |closed form - literal| / bound {worst:.3g} (units), {worst2:.3g} (unit x line)")
    assert worst <= 1.0 and worst2 <= 1.0


def test_the_wrappers_spec_shift_is_the_yardsticks():
    ei, bt, rx, spec = make_physical_inputs(14, 20, 2, seed=1)
    for name, (units, p, a) in U.unit_cases(bt.numpy()).items():
        G = len(units)
        g = torch.tensor([0, G - 1, 2, 1])
        sc = torch.tensor([0, 1, 1, 0])
        part = None if a is None else torch.tensor(a).expand(4, G)
        got = unit_outage_spec(spec[sc], torch.tensor(units), torch.tensor(p).expand(4, G), part, g).numpy()
        for t in range(4):
            want = U.shifted_spec(spec[int(sc[t])].numpy(), units, p, a, int(g[t]))
            assert np.array_equal(got[t], want), (name, t)                      # bit for bit: the units in stored order


def test_units_and_lines_are_validated_on_the_host_before_any_library_call(monkeypatch):
    def never(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", never)
    monkeypatch.setattr(L, "require_device", never)
    ei, bt, rx, spec = make_physical_inputs(14, 20, 2, seed=1)
    for bad, text in (([], "at least one"), ([0, 14], "within"), ([-1], "within"), ([1.5], "ints"), (3, "sequence of bus ids"), (-3, "sequence of bus ids"),
                      (True, "sequence of bus ids"), ([1, True], "units must be ints"), ([1.5], "units must be ints"),
                      (torch.tensor([1, 2], dtype=torch.int32), "units as a tensor must be a CPU int64")):
        with pytest.raises(ValueError, match=text):
            contingency_screen_units(bt, spec, ei, rx, units=bad)
    for bad, text in (([3, 1], "increasing"), ([1, 1], "increasing"), ([0, 20], "within"), ([-1, 4], "within"), ([], "at least one"),
                      ("some", "'all'"), ([1.5, 2], "ints")):
        with pytest.raises(ValueError, match=text):
            contingency_screen_units(bt, spec, ei, rx, units=[1, 2], lines=bad)
    with pytest.raises(ValueError, match="not built"):
        contingency_screen_units(bt, spec, ei, rx, route="sparse")
    with pytest.raises(ValueError, match="route"):
        contingency_screen_units(bt, spec, ei, rx, route="fast")


def test_rankings_have_the_single_outage_screens_order():
    nan, inf = float("nan"), float("inf")
    sev = torch.tensor([[0.5, 2.0, nan, 2.0], [1.0, 1.0, 3.0, 0.25]])
    line_sev = torch.tensor([[[0.5, inf], [2.0, inf], [nan, nan], [2.0, inf]], [[1.0, inf], [4.0, inf], [0.5, inf], [4.0, inf]]])
    z = torch.zeros(2, 4, dtype=torch.int32)
    res = UnitContingencyResult(units=torch.tensor([3, 5, 0, 3]), unit_p=sev.double(), severity=sev, worst_line=z, overloads=z, base_flow=sev.double(),
                                status=z[:, 0], post_flow=None, route="lds", lines=torch.tensor([4, 9]), islands=torch.tensor([0, 2], dtype=torch.int32),
                                line_severity=line_sev)
    ids, vals = res.ranking(4)
    assert ids.dtype == torch.int64 and ids.tolist() == [[2, 1, 3, 0], [2, 0, 1, 3]]
    assert bool(torch.isnan(vals[0, 0])) and vals[0, 1:].tolist() == [2.0, 2.0, 0.5]
    items, vals = res.line_ranking(8)
    assert items.dtype == torch.int64 and items.shape == (2, 8, 2)
    assert items[0].tolist() == [[2, 4], [2, 9], [0, 9], [1, 9], [3, 9], [1, 4], [3, 4], [0, 4]]
    assert items[1].tolist() == [[0, 9], [1, 9], [2, 9], [3, 9], [1, 4], [3, 4], [0, 4], [2, 4]]
    assert vals[1].tolist() == [inf] * 4 + [4.0, 4.0, 1.0, 0.5]
    assert res.line_ranking(2)[0][1].tolist() == [[0, 9], [1, 9]]
    with pytest.raises(ValueError, match="top"):
        res.ranking(5)
    with pytest.raises(ValueError, match="top"):
        res.line_ranking(9)
    res.line_severity = None
    with pytest.raises(ValueError, match="without lines"):
        res.line_ranking(1)


def test_header_bindings_and_wrapper_name_the_same_two_symbols():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pfn_hip.h")).read()
    wrapper = inspect.getsource(K)
    lib = L.load()
    for name in NAMES:
        assert name in L.SYMBOLS and name + "(" in header and hasattr(lib, name) and "lib." + name + "(" in wrapper, name
    assert lib.pfn_abi_version() == L.ABI_VERSION


def test_workspace_sizes_and_refusals():
    lib = L.load()
    ws = lib.pfn_contingency_units_workspace_bytes
    mat = lambda m: 4 * ((m * (m | 1) + 3) // 4 * 4)                         # noqa: E731
    # the LDS route costs no workspace; the global route one slab of (n - 1) x ((n - 1) | 1) floats per scenario
    assert ws(4096, 118, 186, 54, 0) == 0 and ws(8, 14, 20, 6, 1) == 0
    assert ws(8, 14, 20, 6, 2) == 8 * mat(13) and ws(3, 200, 300, 60, 0) == 3 * mat(199)
    # the unit screen's own vectors (24 G + 8 n + 4 e bytes) move the LDS boundary below the N-1 screen's 187 buses
    fit = max(n for n in range(100, 220) if ws(1, n, n + n // 2, n // 3, 0) == 0)
    assert 150 < fit < 187 and ws(1, fit + 1, fit + 1 + (fit + 1) // 2, (fit + 1) // 3, 0) == mat(fit)
    # 0 for sizes the call would refuse
    assert ws(1, int(lib.pfn_powerflow_max_unknowns()) + 2, 10, 4, 2) == 0 and ws(1, 14, 20, 0, 2) == 0 and ws(0, 14, 20, 4, 2) == 0
    p = C.c_void_p(256)                                                      # (never followed: every call below is refused first)

    def run(n_lines=20, n_bus=14, n_pv=4, n_pq=9, tol=1e-8, max_iter=10, route=0, S=4, G=5, c=0, units=p, unit_p=p, lines=None, islands=None,
            line_out=None, ws_ptr=None, ws_bytes=0, spec=p):
        return lib.pfn_contingency_units(p, n_lines, p, p, spec, None, 0, units, G, unit_p, 0, None, 0, lines, c, islands, S, n_bus, n_pv, n_pq, tol,
                                         max_iter, route, p, p, p, p, p, None, line_out, line_out, line_out, None, p, ws_ptr, ws_bytes, None)
    assert run(G=0) == -1 and b"bad sizes" in lib.pfn_last_error()
    assert run(c=21, lines=p, islands=p, line_out=p) == -1 and b"bad sizes" in lib.pfn_last_error()
    assert run(n_bus=1, n_pv=0, n_pq=0) == -1 and b"bad sizes" in lib.pfn_last_error()
    assert run(n_pq=8) == -1 and b"exactly one slack" in lib.pfn_last_error()
    assert run(route=3) == -1 and b"route" in lib.pfn_last_error()
    assert run(tol=0.0) == -1 and b"tol" in lib.pfn_last_error()
    assert run(max_iter=-1) == -1 and b"max_iter" in lib.pfn_last_error()
    assert run(n_bus=1100, n_pv=0, n_pq=1099) == -1 and b"the sparse route is not built" in lib.pfn_last_error()
    assert run(G=7000) == -1 and b"units need" in lib.pfn_last_error() and b"bytes of LDS" in lib.pfn_last_error()
    assert run(n_lines=300, n_bus=200, n_pv=0, n_pq=199, route=1) == -1 and b"route 1" in lib.pfn_last_error()
    assert run(units=None) == -1 and b"null" in lib.pfn_last_error()
    assert run(unit_p=None) == -1 and b"null" in lib.pfn_last_error()
    assert run(c=3, lines=p, islands=None, line_out=p) == -1 and b"null" in lib.pfn_last_error()
    assert run(c=3, lines=p, islands=p, line_out=None) == -1 and b"null" in lib.pfn_last_error()
    assert run(unit_p=C.c_void_p(260)) == -1 and b"aligned" in lib.pfn_last_error()
    assert run(spec=C.c_void_p(260)) == -1 and b"aligned" in lib.pfn_last_error()
    assert run(units=C.c_void_p(258)) == -1 and b"aligned" in lib.pfn_last_error()
    assert run(route=2) == -2 and b"workspace" in lib.pfn_last_error()
    assert run(n_lines=300, n_bus=200, n_pv=0, n_pq=199) == -2 and b"workspace" in lib.pfn_last_error()
    assert run(route=2, ws_ptr=p, ws_bytes=64) == -2 and b"workspace" in lib.pfn_last_error()
    assert run(S=0) == 0
