"""The sparse route of the AC N-1 screen without a GPU: the C ABI carries the three symbols, the block and workspace sizes follow their
formulas, the C entry and `contingency_screen_ac(route="sparse")` refuse what they must before anything is launched, and the
yardstick's compensated form -- the one the GPU test uses beyond the dense cap, where rebuilding both matrices per outage is out of
reach -- equals its literal form at (1100, 1530)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.synth import make_physical_inputs
from poweflownet_amd.utils.contingency import contingency_screen_ac
from poweflownet_amd.utils.powerflow import sparse_plan
from tests import contingency_ac_ref as A

LDS_BYTES = 159 * 1024                                                      # what a workgroup may take (kLdsCuBytes - kLdsReserve)


def _inputs(n, e, S=1):
    ei, bt, rx, spec = make_physical_inputs(n, e, S, seed=1)
    return bt, spec, ei, rx


def _sample_bytes(n, rhs, nnz):
    """a sample's slab of the sparse fast-decoupled solver: fp64 vm, th, sp, sq [n], F [rhs], then both fp32 factors"""
    return (8 * (4 * n + rhs) + 4 * nnz + 15) // 16 * 16


def _block_bytes(n, rhs):
    """an outage block: theta, Vm [n] and g, w [rhs], each row 64 doubles"""
    return 512 * (2 * n + 2 * rhs)


def test_abi_surface_and_size_formulas():
    names = ("pfn_contingency_ac_sparse_block_bytes", "pfn_contingency_ac_sparse_workspace_bytes", "pfn_contingency_ac_sparse")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pfn_hip.h")).read()
    lib = L.load()
    for name in names:
        assert name in L.SYMBOLS and name + "(" in header and hasattr(lib, name)
    assert lib.pfn_abi_version() == L.ABI_VERSION == 8
    bt, spec, ei, rx = _inputs(14, 20)
    plan = sparse_plan(bt, ei, mode="fd")
    h = C.addressof(plan.header)
    n, e, rhs = 14, 20, max(plan.m, plan.m_q)
    assert (plan.m, plan.m_q) == (13, int((bt == 2).sum()))
    size, block = lib.pfn_contingency_ac_sparse_workspace_bytes, lib.pfn_contingency_ac_sparse_block_bytes
    assert block(h) == _block_bytes(n, rhs) <= LDS_BYTES
    slab = _sample_bytes(n, rhs, plan.nnz)
    assert slab == lib.pfn_powerflow_sparse_fd_workspace_bytes(1, h)        # the solver's own slab: the base launch is its launch
    # the LDS placement: the scenarios' slabs alone; the global one: a block per workgroup behind them, the workgroups the lesser of
    # the items (scenarios x tiles of 64 outages) and `groups`
    assert size(8, e, h, 0, 0) == size(8, e, h, 1, 0) == size(8, e, h, 1, 5) == 8 * slab
    assert size(8, e, h, 2, 3) == 8 * slab + 3 * _block_bytes(n, rhs) and size(8, e, h, 2, 100) == 8 * slab + 8 * _block_bytes(n, rhs)
    assert size(2, e, h, 2, 0) == 2 * slab + 2 * _block_bytes(n, rhs)       # (the default: no more workgroups than items)
    assert size(0, e, h, 0, 0) == 0 and size(8, e + 1, h, 0, 0) == 0 and size(8, e, h, 3, 0) == 0 and size(8, e, h, 0, -1) == 0
    dc = sparse_plan(bt, ei, mode="dc")
    junk = (C.c_int32 * 32)()
    assert size(8, e, C.addressof(dc.header), 0, 0) == 0 and size(8, e, C.addressof(junk), 0, 0) == 0 and size(8, e, None, 0, 0) == 0
    assert block(C.addressof(dc.header)) == 0 and block(None) == 0
    big_bt, _, big_ei, _ = _inputs(1100, 1530)
    big = sparse_plan(big_bt, big_ei, mode="fd")
    bh = C.addressof(big.header)
    assert block(bh) == _block_bytes(1100, 1099) > LDS_BYTES
    per = _sample_bytes(1100, 1099, big.nnz)
    assert size(3, 1530, bh, 0, 7) == 3 * per + 7 * block(bh)               # "auto" is global there
    assert size(3, 1530, bh, 0, 1000) == 3 * per + 3 * 24 * block(bh)       # 24 tiles per scenario
    assert size(3, 1530, bh, 1, 0) == 0                                     # the forced LDS placement is refused


def test_the_c_entry_refuses_before_any_launch():
    lib = L.load()
    bt, spec, ei, rx = _inputs(14, 20)
    plan = sparse_plan(bt, ei, mode="fd")
    h = C.addressof(plan.header)
    n, e, rhs = 14, 20, 13
    n_pq = int((bt == 2).sum())
    slab = _sample_bytes(n, rhs, plan.nnz)
    p = C.c_void_p(256)                                                      # (never followed: every call below is refused first)

    def ac(n_lines=e, n_bus=n, n_pv=n - 1 - n_pq, n_pq=n_pq, variant=0, halves=2, v=(0.9, 1.1), tol=1e-8, max_iter=60, header=h, plan_dev=p,
           threads=0, block=0, groups=0, S=4, ws=p, ws_bytes=1 << 30, rx=p, table=p):
        return lib.pfn_contingency_ac_sparse(p, n_lines, rx, p, p, None, None, 0, p, S, n_bus, n_pv, n_pq, variant, halves, v[0], v[1], tol, max_iter,
                                             header, plan_dev, threads, block, groups, p, p, p, p, p, p, p, table, p, p, None, None, p, ws, ws_bytes, None)
    assert ac(header=None) == -1 and b"null plan header" in lib.pfn_last_error()
    dc = sparse_plan(bt, ei, mode="dc")
    assert ac(header=C.addressof(dc.header)) == -1 and b"not a fast-decoupled" in lib.pfn_last_error()
    junk = (C.c_int32 * 32)()
    assert ac(header=C.addressof(junk)) == -1 and b"not a fast-decoupled" in lib.pfn_last_error()
    assert ac(n_lines=21) == -1 and b"the plan is for 14 buses and 20 lines" in lib.pfn_last_error()
    assert ac(n_bus=15, n_pq=n_pq + 1) == -1 and b"the plan is for" in lib.pfn_last_error()
    assert ac(n_pq=n_pq - 1) == -1 and b"exactly one slack" in lib.pfn_last_error()
    assert ac(halves=-1) == -1 and b"halves" in lib.pfn_last_error()
    assert ac(variant=2) == -1 and b"variant" in lib.pfn_last_error()
    assert ac(v=(1.1, 0.9)) == -1 and b"v_limits" in lib.pfn_last_error()
    assert ac(v=(float("nan"), 1.1)) == -1 and b"v_limits" in lib.pfn_last_error()
    assert ac(tol=0.0) == -1 and b"tol" in lib.pfn_last_error()
    assert ac(max_iter=-1) == -1 and b"max_iter" in lib.pfn_last_error()
    assert ac(block=3) == -1 and b"block_route" in lib.pfn_last_error()
    assert ac(groups=-1) == -1 and b"groups" in lib.pfn_last_error()
    assert ac(threads=128) == -1 and b"threads" in lib.pfn_last_error()
    assert ac(S=-1) == -1 and b"bad sizes" in lib.pfn_last_error()
    assert ac(plan_dev=None) == -1 and b"null pointer" in lib.pfn_last_error()
    assert ac(ws_bytes=4 * slab - 1) == -2 and b"workspace" in lib.pfn_last_error()
    assert ac(ws=None, ws_bytes=0) == -2 and b"workspace" in lib.pfn_last_error()
    assert ac(block=2, ws_bytes=4 * slab) == -2 and b"workspace" in lib.pfn_last_error()                  # the blocks are missing
    assert ac(rx=C.c_void_p(260)) == -1 and b"aligned" in lib.pfn_last_error()
    assert ac(table=C.c_void_p(272)) == -1 and b"32-byte" in lib.pfn_last_error()
    assert ac(ws=C.c_void_p(264)) == -1 and b"aligned" in lib.pfn_last_error()
    assert ac(plan_dev=C.c_void_p(264)) == -1 and b"aligned" in lib.pfn_last_error()
    assert ac(S=0) == 0
    big_bt, _, big_ei, _ = _inputs(1100, 1530)
    big = sparse_plan(big_bt, big_ei, mode="fd")
    big_pq = int((big_bt == 2).sum())
    assert lib.pfn_contingency_ac_sparse(p, 1530, p, p, p, None, None, 0, p, 1, 1100, 1099 - big_pq, big_pq, 0, 2, 0.9, 1.1, 1e-8, 60,
                                         C.addressof(big.header), p, 0, 1, 0, p, p, p, p, p, p, p, p, p, p, None, None, p, p, 1 << 40, None) == -1
    assert b"bytes of LDS" in lib.pfn_last_error()
    # the dense entry keeps its signature and its refusal beyond the cap
    cap = int(lib.pfn_powerflow_max_unknowns())
    assert lib.pfn_contingency_ac(p, 20, p, p, p, None, None, 0, p, 4, cap + 2, 0, cap + 1, 0, 2, 0.9, 1.1, 1e-8, 60, 0, 0, p, p, p, p, p, p, p, p, p, p,
                                  None, None, p, p, 1 << 30, None) == -1 and b"dense" in lib.pfn_last_error()


def test_the_python_wrapper_refuses_bad_arguments_on_the_host():
    bt, spec, ei, rx = _inputs(14, 20, 2)
    fd, dc = sparse_plan(bt, ei, mode="fd"), sparse_plan(bt, ei, mode="dc")
    call = lambda **kw: contingency_screen_ac(bt, spec, ei, rx, route="sparse", **kw)   # noqa: E731  (CPU tensors: nothing may get as far as them)
    with pytest.raises(ValueError, match="route 'sparse' needs plan=sparse_plan"):
        call()
    with pytest.raises(ValueError, match="mode 'fd'"):
        call(plan=dc)
    with pytest.raises(ValueError, match="the plan is for"):
        contingency_screen_ac(bt, spec, ei[:, :19], rx[:, :19], route="sparse", plan=fd)
    other = _inputs(15, 20, 2)
    with pytest.raises(ValueError, match="the plan is for"):
        contingency_screen_ac(*other, route="sparse", plan=fd)
    for kw, text in (({"block": "shared"}, "block"), ({"groups": 0}, "groups"), ({"groups": 2.5}, "groups"), ({"groups": True}, "groups"),
                     ({"threads": 128}, "threads"), ({"group": 4}, "group"), ({"halves": -1}, "halves"), ({"variant": "fdxb"}, "variant"),
                     ({"v_limits": (1.1, 0.9)}, "v_limits"), ({"keep_state": 1}, "keep_state")):
        with pytest.raises(ValueError, match=text):
            call(plan=fd, **kw)
    for kw in ({"plan": fd}, {"block": "lds"}, {"groups": 4}, {"threads": 64}):          # the sparse route's options on another route
        with pytest.raises(ValueError, match="route='sparse' only"):
            contingency_screen_ac(bt, spec, ei, rx, **kw)
    with pytest.raises(ValueError, match="route must be one of"):
        contingency_screen_ac(bt, spec, ei, rx, route="dense")
    # beyond the dense cap without a plan: still the refusal that names max_unknowns, and it names the way out
    cap = int(L.load().pfn_powerflow_max_unknowns())
    with pytest.raises(ValueError, match="max_unknowns.*route='sparse'"):
        contingency_screen_ac(bt, torch.zeros(1, cap + 2, 4, dtype=torch.float64), ei, rx)
    with pytest.raises(RuntimeError, match="no CPU fallback"):              # good arguments: the device check is next (no CPU path)
        call(plan=fd)


def test_the_compensated_form_equals_the_literal_one_beyond_the_dense_cap():
    """eight outages of (1100, 1530): the rank-1-compensated inverses against deleting the line and rebuilding both matrices"""
    n, e = 1100, 1530
    ei, bt, rx, spec = (t.numpy() for t in make_physical_inputs(n, e, 1, seed=1))
    isl = A.islands(bt, ei)
    ok = np.flatnonzero(isl == 0)
    assert (isl > 0).any() and len(ok) >= 8
    vm0, th0, status = A.base_state(bt, spec[0], ei, rx[0], "xb")
    assert status >= 0
    inv = A.inverses(bt, ei, rx[0], "xb")
    pq = bt == 2
    ends = pq[ei[0]].astype(int) + pq[ei[1]].astype(int)
    chosen = list(ok[:: max(1, len(ok) // 6)][:6]) + [int(ok[ends[ok] == 1][0]), int(ok[ends[ok] == 0][0])]   # both kinds of end among them
    worst = 0.0
    for k in chosen:
        lit = A.outage_state(bt, spec[0], ei, rx[0], vm0, th0, int(k), 2, "xb", "literal")
        com = A.outage_state(bt, spec[0], ei, rx[0], vm0, th0, int(k), 2, "xb", "compensated", inv)
        for a, b in zip(lit[:2], com[:2]):
            worst = max(worst, float(np.abs(a - b).max() / np.abs(a).max()))
    print(f"n {n} e {e}: {len(chosen)} outages, worst relative |compensated - literal| {worst:.3g}")
    assert len(chosen) == 8 and worst <= 1e-10
