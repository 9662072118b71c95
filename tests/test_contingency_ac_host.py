"""The AC N-1 screen without a GPU: the yardstick's two forms of an outage's state (the rank-1-compensated inverses against
literally deleting the line and rebuilding both matrices) agree; the claim that justifies the screen -- two half-iterations are
an order of magnitude closer to the AC severity than the DC screen and name the AC worst line at least as often -- holds on the
yardstick alone; forty halves reach the Newton solution; the voltage figures follow their rules; the C ABI carries the symbols and
the C entry and `contingency_screen_ac` refuse what they must before anything is launched."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.synth import make_physical_inputs
from tests import contingency_ac_ref as A
from tests import contingency_ref as R


def _inputs(n, e, S, seed, no_pv=False):
    """`make_physical_inputs`: every third bus holds its voltage (bus_type[::3] = 1 behind the slack), so the grids have outages
    with one end and with both ends outside the PQ set.  no_pv: those buses become PQ buses (their P stays, their Q is the table's)."""
    ei, bt, rx, spec = (t.numpy().copy() for t in make_physical_inputs(n, e, S, seed=seed))
    if no_pv:
        bt[bt == 1] = 2
    return ei, bt, rx, spec


@pytest.mark.parametrize("n,e", [(3, 3), (5, 6), (14, 20), (30, 41)])
@pytest.mark.parametrize("no_pv", [False, True])
def test_compensated_inverses_equal_rebuilding_both_matrices(n, e, no_pv):
    ei, bt, rx, spec = _inputs(n, e, 2, 1, no_pv)
    isl = R.islands(bt, ei)
    assert (isl == 0).any()
    pq = bt == 2
    ends_pq = pq[ei[0]].astype(int) + pq[ei[1]].astype(int)
    if not no_pv and n >= 14:
        assert (ends_pq[isl == 0] == 1).any() and (ends_pq[isl == 0] == 0).any(), "the grid must hold both kinds of outage"
    worst = 0.0
    for s in range(2):
        for variant in ("xb", "bx"):
            vm0, th0, status = A.base_state(bt, spec[s], ei, rx[s], variant)
            assert status >= 0
            for k in np.flatnonzero(isl == 0):
                for halves in (2, 4):
                    lit = A.outage_state(bt, spec[s], ei, rx[s], vm0, th0, k, halves, variant, "literal")
                    com = A.outage_state(bt, spec[s], ei, rx[s], vm0, th0, k, halves, variant, "compensated")
                    for a, b in zip(lit[:2], com[:2]):
                        worst = max(worst, float(np.abs(a - b).max() / np.abs(a).max()))
    print(f"n {n} e {e} no_pv {no_pv}: worst relative |compensated - literal| {worst:.3g}")
    assert worst <= 1e-10


@functools.lru_cache(maxsize=None)
def _claim(n, e, S):
    """per non-islanding (scenario, outage): the AC severity and worst line (Newton on the reduced grid), the 1P1Q ones and the DC
    screen's, with ratings of 1.2 x the scenario's largest base current"""
    ei, bt, rx, spec = _inputs(n, e, S, 3)
    isl = R.islands(bt, ei)
    rows = []
    for s in range(S):
        vm0, th0, status = A.base_state(bt, spec[s], ei, rx[s], "xb")
        assert status >= 0
        base_cur, _ = A.currents(A.state32(vm0, th0, bt, spec[s]), ei, rx[s])
        ratings = np.full(e, 1.2 * base_cur.max())
        dc_post, _ = R.lodf(bt, spec[s], ei, rx[s])
        dc_sev, dc_worst, _ = R.summarise(dc_post, ratings, isl)
        tables = {"ac": np.zeros((e, e)), "fd": np.zeros((e, e))}
        for k in np.flatnonzero(isl == 0):
            truth = A.newton_outage(bt, spec[s], ei, rx[s], vm0, th0, k)
            assert truth is not None, (s, k)
            vm, th, _ = A.outage_state(bt, spec[s], ei, rx[s], vm0, th0, k, 2, "xb", "compensated")
            tables["ac"][k] = A.currents(A.state32(*truth, bt, spec[s]), ei, rx[s], k)[0]
            tables["fd"][k] = A.currents(A.state32(vm, th, bt, spec[s]), ei, rx[s], k)[0]
        ac_sev, ac_worst, _ = A.summarise(tables["ac"], ratings, isl, dtype=np.float64)
        fd_sev, fd_worst, _ = A.summarise(tables["fd"], ratings, isl, dtype=np.float64)
        for k in np.flatnonzero(isl == 0):
            rows.append((ac_sev[k], fd_sev[k], dc_sev[k], ac_worst[k], fd_worst[k], dc_worst[k]))
    return np.array(rows)


@pytest.mark.parametrize("n,e,S", [(14, 20, 4), (30, 41, 3)])
def test_two_halves_are_ten_times_closer_to_ac_than_the_dc_screen(n, e, S):
    rows = _claim(n, e, S)
    ac, fd, dc = rows[:, 0], rows[:, 1], rows[:, 2]
    err_fd, err_dc = np.abs(fd - ac) / ac, np.abs(dc - ac) / ac
    agree_fd, agree_dc = int((rows[:, 4] == rows[:, 3]).sum()), int((rows[:, 5] == rows[:, 3]).sum())
    print(f"({n}, {e}, {S}): {len(rows)} pairs; relative severity error median / max: DC {np.median(err_dc):.2g} / {err_dc.max():.2g}, "
          f"1P1Q {np.median(err_fd):.2g} / {err_fd.max():.2g}; worst line equals AC's: DC {agree_dc}, 1P1Q {agree_fd}")
    assert np.median(err_fd) < 0.1 * np.median(err_dc)
    assert agree_fd >= agree_dc


def test_forty_halves_reach_the_newton_solution():
    ei, bt, rx, spec = _inputs(14, 20, 1, 3)
    isl = R.islands(bt, ei)
    vm0, th0, _ = A.base_state(bt, spec[0], ei, rx[0], "xb")
    worst = 0.0
    for k in np.flatnonzero(isl == 0):
        vm, th, mis = A.outage_state(bt, spec[0], ei, rx[0], vm0, th0, k, 40, "xb", "compensated")
        tv, tt = A.newton_outage(bt, spec[0], ei, rx[0], vm0, th0, k)
        worst = max(worst, float(np.abs(vm - tv).max()), float(np.abs(th - tt).max()))
    print(f"worst |state after 40 halves - newton| {worst:.3g}")
    assert worst <= 1e-8


def test_voltage_figures_follow_the_rules():
    bt = np.array([0, 2, 1, 2, 2, 2])
    vm = np.array([0.5, 0.95, 0.2, 0.93, 0.93, 1.2], dtype=np.float32)      # the slack and the PV bus do not count
    low, bus, count = A.voltage_figures(vm, bt, 0.94, 1.1)
    assert low == np.float32(0.93) and bus == 3 and count == 3               # a tie goes to the lowest bus
    assert A.voltage_figures(vm, bt, 0.93, 1.2)[2] == 0                      # the limits themselves are inside
    low, bus, count = A.voltage_figures(vm, np.array([0, 1, 1, 1, 1, 1]), 0.9, 1.1)
    assert np.isnan(low) and bus == -1 and count == 0                        # no PQ bus
    vm[4] = np.nan
    low, bus, count = A.voltage_figures(vm, bt, 0.9, 1.1)
    assert np.isnan(low) and bus == 4 and count == 2                         # a NaN is the lowest, counts, and makes vm_min NaN
    vm[1] = np.inf
    assert A.voltage_figures(vm, bt, 0.9, 1.1)[1:] == (1, 3)


def test_abi_surface_and_refusals():
    names = ("pfn_contingency_ac_workspace_bytes", "pfn_contingency_ac_waves", "pfn_contingency_ac")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pfn_hip.h")).read()
    lib = L.load()
    for name in names:
        assert name in L.SYMBOLS and name + "(" in header and hasattr(lib, name)
    cap = int(lib.pfn_powerflow_max_unknowns())
    up16 = lambda v: (v + 15) // 16 * 16                                     # noqa: E731
    mat = lambda m: (m * (m | 1) + 3) // 4 * 4                               # noqa: E731
    slab = up16(4 * (mat(13) + mat(9))) + 2 * up16(8 * 14) + 2 * up16(4 * 14) + up16(4 * 15) + up16(16 * 20) + 16
    assert lib.pfn_contingency_ac_workspace_bytes(8, 14, 20, 9) == 8 * slab
    assert lib.pfn_contingency_ac_workspace_bytes(1, cap + 2, 10, 5) == 0 and lib.pfn_contingency_ac_workspace_bytes(0, 14, 20, 9) == 0
    lds = C.c_int(-1)
    assert lib.pfn_contingency_ac_waves(14, 9, 0, 0, C.byref(lds)) == 16 and lds.value == 1
    assert lib.pfn_contingency_ac_waves(14, 9, 2, 3, C.byref(lds)) == 3 and lds.value == 0
    assert lib.pfn_contingency_ac_waves(118, 100, 0, 0, C.byref(lds)) == 8 and lds.value == 1      # 16 waves' vectors do not fit beside the inverses
    assert lib.pfn_contingency_ac_waves(200, 199, 0, 0, C.byref(lds)) == 16 and lds.value == 0
    assert lib.pfn_contingency_ac_waves(200, 199, 1, 0, C.byref(lds)) == 0
    assert lib.pfn_contingency_ac_waves(cap + 1, cap, 0, 0, C.byref(lds)) == 3 and lds.value == 0  # the vectors of three waves are all that fit
    assert lib.pfn_contingency_ac_waves(cap + 1, cap, 0, 4, C.byref(lds)) == 0
    p = C.c_void_p(256)                                                      # (never followed: every call below is refused first)

    def ac(n_lines=20, n_bus=14, n_pv=4, n_pq=9, variant=0, halves=2, v=(0.9, 1.1), tol=1e-8, route=0, group=0, S=4, ws=p, ws_bytes=1 << 30,
           rx=p, table=p):
        return lib.pfn_contingency_ac(p, n_lines, rx, p, p, None, None, 0, p, S, n_bus, n_pv, n_pq, variant, halves, v[0], v[1], tol, 60, route,
                                      group, p, p, p, p, p, p, p, table, p, p, None, None, p, ws, ws_bytes, None)
    assert ac(halves=-1) == -1 and b"halves" in lib.pfn_last_error()
    assert ac(variant=2) == -1 and b"variant" in lib.pfn_last_error()
    assert ac(v=(1.1, 0.9)) == -1 and b"v_limits" in lib.pfn_last_error()
    assert ac(v=(float("nan"), 1.1)) == -1 and b"v_limits" in lib.pfn_last_error()
    assert ac(n_pq=8) == -1 and b"exactly one slack" in lib.pfn_last_error()
    assert ac(route=3) == -1 and b"route" in lib.pfn_last_error()
    assert ac(group=17) == -1 and b"group" in lib.pfn_last_error()
    assert ac(tol=0.0) == -1 and b"tol" in lib.pfn_last_error()
    assert ac(n_bus=cap + 2, n_pv=0, n_pq=cap + 1) == -1 and b"dense" in lib.pfn_last_error()
    assert ac(n_lines=300, n_bus=200, n_pv=0, n_pq=199, route=1) == -1 and b"bytes of LDS" in lib.pfn_last_error()
    assert ac(ws_bytes=4 * slab - 1) == -2 and b"workspace" in lib.pfn_last_error()
    assert ac(ws=None) == -2 and b"workspace" in lib.pfn_last_error()
    assert ac(rx=C.c_void_p(260)) == -1 and b"aligned" in lib.pfn_last_error()
    assert ac(table=C.c_void_p(272)) == -1 and b"32-byte" in lib.pfn_last_error()
    assert ac(ws=C.c_void_p(264)) == -1 and b"aligned" in lib.pfn_last_error()
    assert ac(S=0) == 0


def test_the_python_wrapper_refuses_bad_arguments_on_the_host():
    from poweflownet_amd.utils.contingency import ACContingencyResult, contingency_screen_ac
    ei, bt, rx, spec = make_physical_inputs(5, 6, 1, seed=1)
    call = lambda **kw: contingency_screen_ac(bt, spec, ei, rx, **kw)         # noqa: E731  (CPU tensors: nothing may get as far as them)
    for kw, word in (({"halves": -1}, "halves"), ({"halves": 1.5}, "halves"), ({"halves": True}, "halves"), ({"variant": "fdxb"}, "variant"),
                     ({"v_limits": (1.1, 0.9)}, "v_limits"), ({"v_limits": 1.0}, "v_limits"), ({"route": "sparse"}, "route"),
                     ({"group": 0}, "group"), ({"group": 17}, "group"), ({"keep_state": 1}, "keep_state")):
        with pytest.raises(ValueError, match=word):
            call(**kw)
    cap = int(L.load().pfn_powerflow_max_unknowns())
    with pytest.raises(ValueError, match="max_unknowns"):
        contingency_screen_ac(bt, torch.zeros(1, cap + 2, 4, dtype=torch.float64), ei, rx)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call()
    sev = torch.tensor([[0.5, float("inf"), 2.0, float("nan")]])
    z = torch.zeros(1, 4, dtype=torch.int32)
    res = ACContingencyResult(severity=sev, worst_line=z, overloads=z, vm_min=sev, vm_min_bus=z, v_violations=z, mismatch=sev.double(), islands=z[0],
                              base_table=None, status=z[:, 0], residual=None, post_current=None, post_state=None, route="lds")
    assert res.ranking(4)[0].tolist() == [[3, 1, 2, 0]]
