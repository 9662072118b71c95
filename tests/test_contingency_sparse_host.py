"""The sparse route of the N-1 screen without a GPU: the C ABI carries the two symbols and refuses what it must before anything is
launched, the workspace formula holds on both block placements, `contingency_screen` and `verify_contingencies` refuse bad arguments
before they touch a device, and the numpy float32 restatement of one lane's arithmetic (tests/contingency_sparse_ref.py) stays within
the bound the GPU test holds the kernel to -- the expectation the device figures of DESIGN 7v are compared with."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.synth import make_physical_inputs
from poweflownet_amd.utils.contingency import contingency_screen
from poweflownet_amd.utils.powerflow import sparse_plan
from tests import contingency_ref as R
from tests import contingency_sparse_ref as CS
from tests.test_gpu_contingency_sparse import C_BOUND

LDS_BYTES = 159 * 1024                                                      # what a workgroup may take (kLdsCuBytes - kLdsReserve)


def _inputs(n, e, S=1):
    ei, bt, rx, spec = make_physical_inputs(n, e, S, seed=1)
    return bt, spec, ei, rx


@pytest.mark.parametrize("n,e", [(14, 20), (118, 186), (1100, 1530)])
def test_the_float32_restatement_of_a_lane_meets_the_yardstick(n, e):
    bt, spec, ei, rx = (t.numpy() for t in _inputs(n, e))
    isl = R.islands(bt, ei)
    den = R.lodf(bt, spec[0], ei, rx[0])[1]
    assert (isl > 0).any() and np.abs(den[isl == 0]).min() >= 0.05
    worst = CS.worst_ratio(bt, spec[0], ei, rx[0], isl, literal=n <= 118)
    print(f"n {n} e {e}: numpy float32 lanes, worst |post flow - f64| / u {worst:.3g} (C = {C_BOUND:g})")
    assert worst <= C_BOUND


def test_a_lane_sees_the_slack_as_zeros_and_a_bridge_as_a_vanishing_denominator():
    bt, spec, ei, rx = (t.numpy() for t in _inputs(14, 20))
    plan = CS.dc_plan(bt, ei)
    isl = R.islands(bt, ei)
    post, den = CS.lanes(plan, CS.factor(plan, bt, spec[0], ei, rx[0]), ei, rx[0], R.base_flow(bt, spec[0], ei, rx[0]))
    assert post.dtype == np.float32 and post.shape == (20, 20) and (np.diagonal(post) == 0).all()
    assert (np.abs(den[isl > 0]) < 1e-5).all() and (np.abs(den[isl == 0]) >= 0.05).all()
    slack = int(np.flatnonzero(bt == 0)[0])
    assert ((ei == slack).any(axis=0)).any()                                # (a line at the slack is among them)


def test_abi_surface_workspace_formula_and_refusals():
    names = ("pfn_contingency_sparse_workspace_bytes", "pfn_contingency_sparse")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pfn_hip.h")).read()
    lib = L.load()
    for name in names:
        assert name in L.SYMBOLS and name + "(" in header and hasattr(lib, name)
    assert lib.pfn_abi_version() == 8
    bt, spec, ei, rx = _inputs(14, 20)
    plan = sparse_plan(bt, ei, mode="dc")
    h = C.addressof(plan.header)
    n, e, m, nnz = 14, 20, 13, plan.nnz

    def slab(S, n=n, m=m, nnz=nnz, e=e):
        return S * ((8 * (2 * n + m) + 4 * nnz + 20 * e + 15) // 16 * 16)
    size = lib.pfn_contingency_sparse_workspace_bytes
    # the LDS placement: the scenarios' slabs alone; the global one: a block of 256 (m + 1) bytes per workgroup on top, the
    # workgroups the lesser of the items (scenarios x tiles of 64 outages) and `groups`
    assert size(8, e, h, 0, 0) == size(8, e, h, 1, 0) == size(8, e, h, 1, 5) == slab(8)
    assert size(8, e, h, 2, 3) == slab(8) + 3 * 256 * n and size(8, e, h, 2, 100) == slab(8) + 8 * 256 * n
    assert size(2, e, h, 2, 0) == slab(2) + 2 * 256 * n                    # (the default: no more workgroups than items)
    assert size(0, e, h, 0, 0) == 0 and size(8, e + 1, h, 0, 0) == 0 and size(8, e, h, 3, 0) == 0 and size(8, e, h, 0, -1) == 0
    big_bt, _, big_ei, _ = _inputs(1100, 1530)
    big = sparse_plan(big_bt, big_ei, mode="dc")
    assert 256 * 1100 > LDS_BYTES and big.m == 1099
    per = slab(1, 1100, 1099, big.nnz, 1530)
    assert size(3, 1530, C.addressof(big.header), 0, 7) == 3 * per + 7 * 256 * 1100                       # "auto" is global there
    assert size(3, 1530, C.addressof(big.header), 0, 1000) == 3 * per + 3 * 24 * 256 * 1100                # 24 tiles per scenario
    ac = sparse_plan(bt, ei, mode="ac")
    assert size(8, e, C.addressof(ac.header), 0, 0) == 0                                                  # not a mode-1 plan

    p = C.c_void_p(256)                                                      # (never followed: every call below is refused first)

    def call(n_lines=e, n_bus=n, n_pv=4, n_pq=9, tol=1e-8, S=4, ws=p, ws_bytes=1 << 30, header=h, plan_dev=p, threads=0, block=0, groups=0,
             max_iter=10):
        return lib.pfn_contingency_sparse(p, n_lines, p, p, p, None, 0, p, S, n_bus, n_pv, n_pq, tol, max_iter, p, p, p, p, p, None, p, ws, ws_bytes,
                                          header, plan_dev, threads, block, groups, None)
    assert call(header=None) == -1 and b"null plan header" in lib.pfn_last_error()
    assert call(header=C.addressof(ac.header)) == -1 and b"mode-1" in lib.pfn_last_error()
    junk = (C.c_int32 * 32)()
    assert call(header=C.addressof(junk)) == -1 and b"not a sparse power-flow plan" in lib.pfn_last_error()
    assert call(n_pq=8) == -1 and b"exactly one slack" in lib.pfn_last_error()
    assert call(n_lines=21) == -1 and b"the plan is for 14 buses and 20 lines" in lib.pfn_last_error()
    assert call(n_bus=15, n_pq=10) == -1 and b"the plan is for" in lib.pfn_last_error()
    assert call(block=3) == -1 and b"block_route" in lib.pfn_last_error()
    assert call(groups=-1) == -1 and b"groups" in lib.pfn_last_error()
    assert call(threads=128) == -1 and b"threads" in lib.pfn_last_error()
    assert call(tol=0.0) == -1 and b"tol" in lib.pfn_last_error()
    assert call(max_iter=-1) == -1 and b"max_iter" in lib.pfn_last_error()
    assert call(S=-1) == -1 and b"sample count" in lib.pfn_last_error()
    assert call(plan_dev=None) == -1 and b"null pointer" in lib.pfn_last_error()
    assert call(ws=C.c_void_p(264)) == -1 and b"aligned" in lib.pfn_last_error()
    assert call(ws=None, ws_bytes=0) == -2 and b"workspace" in lib.pfn_last_error()
    assert call(ws_bytes=slab(4) - 1) == -2 and b"workspace" in lib.pfn_last_error()
    assert call(block=2, ws_bytes=slab(4)) == -2 and b"workspace" in lib.pfn_last_error()                   # the blocks are missing
    assert call(S=0) == 0
    bh = C.addressof(big.header)
    assert lib.pfn_contingency_sparse(p, 1530, p, p, p, None, 0, p, 1, 1100, 0, 1099, 1e-8, 10, p, p, p, p, p, None, p, p, 1 << 30, bh, p, 0, 1, 0,
                                      None) == -1 and b"bytes of LDS" in lib.pfn_last_error()
    # the dense entry and its text stay
    assert lib.pfn_contingency_dc(p, 20, p, p, p, None, 0, p, 4, 1100, 0, 1099, 1e-8, 10, 0, p, p, p, p, p, None, p, None, 0, None) == -1
    assert b"the sparse route is not built" in lib.pfn_last_error()


def test_python_argument_errors():
    bt, spec, ei, rx = _inputs(14, 20, 2)
    dc, ac = sparse_plan(bt, ei, mode="dc"), sparse_plan(bt, ei, mode="ac")
    with pytest.raises(ValueError, match="needs plan=sparse_plan"):
        contingency_screen(bt, spec, ei, rx, route="sparse")
    with pytest.raises(ValueError, match="mode 'dc'"):
        contingency_screen(bt, spec, ei, rx, route="sparse", plan=ac)
    with pytest.raises(ValueError, match="the plan is for"):
        contingency_screen(bt, spec, ei[:, :19], rx[:, :19], route="sparse", plan=dc)
    other = _inputs(15, 20, 2)
    with pytest.raises(ValueError, match="the plan is for"):
        contingency_screen(*other, route="sparse", plan=dc)
    for kw, text in (({"block": "shared"}, "block"), ({"groups": 0}, "groups"), ({"groups": 2.5}, "groups"), ({"groups": True}, "groups"),
                     ({"threads": 128}, "threads")):
        with pytest.raises(ValueError, match=text):
            contingency_screen(bt, spec, ei, rx, route="sparse", plan=dc, **kw)
    with pytest.raises(ValueError, match="route must be one of"):
        contingency_screen(bt, spec, ei, rx, route="dense")
    for kw in ({"plan": dc}, {"block": "lds"}, {"groups": 4}, {"threads": 64}):  # the sparse route's options on another route
        with pytest.raises(ValueError, match="route='sparse' only"):
            contingency_screen(bt, spec, ei, rx, **kw)
    with pytest.raises(RuntimeError):                                       # good arguments: the device check is next (no CPU path)
        contingency_screen(bt, spec, ei, rx, route="sparse", plan=dc)
