"""The sparse route of the N-2 pair screen without a GPU: the C ABI carries the two symbols and refuses what it must before anything
is launched, the workspace formula holds on both block placements and both column placements, `contingency_screen_pairs` refuses
bad arguments before it touches a device -- the two refusals the dense screen's tests hold among them --, and the numpy float32
restatement of one pair's arithmetic (tests/contingency_pairs_sparse_ref.py) stays within the bound the GPU test holds the kernel to:
the expectation the device figures of DESIGN 7x are compared with."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.synth import make_physical_inputs
from poweflownet_amd.utils.contingency import PairContingencyResult, contingency_screen_pairs
from poweflownet_amd.utils.powerflow import sparse_plan
from tests import contingency_pairs_sparse_ref as PS
from tests.test_gpu_contingency_pairs import NORM_CAP, _candidates
from tests.test_gpu_contingency_pairs_sparse import C3
from tests.test_gpu_powerflow import _case

NAMES = ("pfn_contingency_pairs_sparse_workspace_bytes", "pfn_contingency_pairs_sparse")
LDS_BYTES = 159 * 1024                                                      # what a workgroup may take (kLdsCuBytes - kLdsReserve)


def _inputs(n, e, S=1):
    ei, bt, rx, spec = make_physical_inputs(n, e, S, seed=1)
    return bt, spec, ei, rx


def test_both_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pfn_hip.h")).read()
    lib = L.load()
    for name in NAMES:
        assert name in L.SYMBOLS and name + "(" in header and hasattr(lib, name), name
    assert lib.pfn_abi_version() == L.ABI_VERSION == 8
    z = torch.zeros(1)
    res = PairContingencyResult(z, z, z, z, z, z, z, None, "lds")           # (the two new fields have defaults)
    assert res.block is None and res.columns is None and res.flags is None


@pytest.mark.parametrize("n,e,c", [(14, 20, None), (118, 186, 24)])
def test_the_float32_restatement_of_a_pair_meets_the_yardstick(n, e, c):
    case = _case(n, e, 1)
    lines = _candidates(case, c)
    worst, norm, isl = PS.worst_ratio(case.bt, case.spec[0], case.ei, case.rx[0], np.arange(e) if lines is None else lines, literal=True)
    assert (isl > 0).any() and (isl == 0).any() and norm <= NORM_CAP
    print(f"n {n} e {e}: {len(isl)} pairs, numpy float32 columns and pairs, worst |post flow - f64| / u {worst:.3g} (C3 = {C3:g})")
    assert worst <= C3


def test_workspace_formula_on_both_placements_of_block_and_columns():
    size = L.load().pfn_contingency_pairs_sparse_workspace_bytes
    bt, spec, ei, rx = _inputs(70, 100)
    plan = sparse_plan(bt, ei, mode="dc")
    h, n, e, m = C.addressof(plan.header), 70, 100, 69

    def per(c, n=n, m=m, nnz=plan.nnz, e=e):                                 # the N-1 screen's slab, then the column table: each rounded to 16
        return (8 * (2 * n + m) + 4 * nnz + 20 * e + 15) // 16 * 16 + (4 * c * (m + 1) + 15) // 16 * 16
    for c, tiles in ((2, 1), (64, 1), (65, 2)):
        # the block in LDS: the scenarios' slabs and tables alone, wherever the columns sit and whatever `waves`
        assert size(8, e, c, h, 0, 0, 0, 0) == size(8, e, c, h, 1, 5, 1, 16) == size(8, e, c, h, 1, 0, 2, 1) == 8 * per(c)
        # the block in the workspace: 256 (m + 1) bytes per workgroup, the lesser of the items (scenarios x tiles of 64 candidates) and `groups`
        assert size(8, e, c, h, 2, 3, 0, 0) == 8 * per(c) + 3 * 256 * n and size(8, e, c, h, 2, 1000, 2, 4) == 8 * per(c) + 8 * tiles * 256 * n
        assert size(2, e, c, h, 2, 0, 1, 0) == 2 * per(c) + 2 * tiles * 256 * n      # (the default: no more workgroups than items)
    # 0 for what the call would refuse
    assert size(0, e, 8, h, 0, 0, 0, 0) == 0 and size(8, e + 1, 8, h, 0, 0, 0, 0) == 0 and size(8, e, e + 1, h, 0, 0, 0, 0) == 0
    assert size(8, e, 8, h, 3, 0, 0, 0) == 0 and size(8, e, 8, h, 0, -1, 0, 0) == 0 and size(8, e, 8, h, 0, 0, 3, 0) == 0
    for waves in (3, 5, 32, -1):
        assert size(8, e, 8, h, 0, 0, 0, waves) == 0
    ac = sparse_plan(bt, ei, mode="ac")
    assert size(8, e, 8, C.addressof(ac.header), 0, 0, 0, 0) == 0                                      # not a mode-1 plan
    other = sparse_plan(*_inputs(71, 100)[::2], mode="dc")
    assert other.n == 71 and size(8, e, 8, C.addressof(other.header), 0, 0, 0, 0) != 0               # (the entry takes no bus count: the CALL refuses another n)
    big_bt, _, big_ei, _ = _inputs(1100, 1530)
    big = sparse_plan(big_bt, big_ei, mode="dc")
    bh = C.addressof(big.header)
    assert 256 * 1100 > LDS_BYTES and size(3, 1530, 16, bh, 1, 0, 0, 0) == 0                           # the block does not fit
    assert size(3, 1530, 16, bh, 0, 7, 0, 0) == 3 * per(16, 1100, 1099, big.nnz, 1530) + 3 * 256 * 1100   # "auto" is global there; 3 items
    assert size(3, 1530, 16, bh, 0, 7, 1, 16) == size(3, 1530, 16, bh, 0, 7, 0, 0)                    # 17 columns of 1100 fit
    wide_bt, _, wide_ei, _ = _inputs(2400, 3600)
    wide = sparse_plan(wide_bt, wide_ei, mode="dc")                          # (held: the header lives in the plan)
    wh = C.addressof(wide.header)
    assert 4 * 2400 * 17 > LDS_BYTES >= 4 * 2400 * 9
    assert size(1, 3600, 8, wh, 0, 0, 1, 16) == 0 and size(1, 3600, 8, wh, 0, 0, 1, 8) != 0            # 1 + 16 columns do not fit, 1 + 8 do
    assert size(1, 3600, 8, wh, 0, 0, 0, 16) == size(1, 3600, 8, wh, 0, 0, 2, 16) == size(1, 3600, 8, wh, 0, 0, 1, 8)


def test_every_refusal_of_the_c_entry_carries_its_text():
    lib = L.load()
    bt, spec, ei, rx = _inputs(14, 20)
    plan, ac = sparse_plan(bt, ei, mode="dc"), sparse_plan(bt, ei, mode="ac")
    h, n, e = C.addressof(plan.header), 14, 20
    slabs = int(lib.pfn_contingency_pairs_sparse_workspace_bytes(4, e, 6, h, 1, 0, 0, 0))
    assert slabs and int(lib.pfn_contingency_pairs_sparse_workspace_bytes(4, e, 6, h, 2, 0, 0, 0)) == slabs + 4 * 256 * n
    p = C.c_void_p(256)                                                      # (never followed: every call below is refused first)

    def call(n_lines=e, n_bus=n, n_pv=4, n_pq=9, tol=1e-8, S=4, c=6, ws=p, ws_bytes=1 << 30, header=h, plan_dev=p, threads=0, block=0, groups=0,
             columns=0, waves=0, max_iter=10, lines=p):
        return lib.pfn_contingency_pairs_sparse(p, n_lines, p, p, p, None, 0, lines, c, p, S, n_bus, n_pv, n_pq, tol, max_iter, p, p, p, p, p, None, p, ws,
                                                ws_bytes, header, plan_dev, threads, block, groups, columns, waves, None)
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
    assert call(c=21) == -1 and b"21 candidates among 20 lines" in lib.pfn_last_error()
    assert call(c=-1) == -1 and b"candidates" in lib.pfn_last_error()
    assert call(columns=3) == -1 and b"column_route" in lib.pfn_last_error()
    for waves in (3, 32, -1):
        assert call(waves=waves) == -1 and b"waves" in lib.pfn_last_error()
    assert call(plan_dev=None) == -1 and b"null pointer" in lib.pfn_last_error()
    assert call(lines=None) == -1 and b"null pointer" in lib.pfn_last_error()
    assert call(lines=C.c_void_p(258)) == -1 and b"aligned" in lib.pfn_last_error()
    assert call(ws=C.c_void_p(264)) == -1 and b"aligned" in lib.pfn_last_error()
    assert call(ws=None, ws_bytes=0) == -2 and b"workspace" in lib.pfn_last_error()
    assert call(ws_bytes=slabs - 1) == -2 and b"workspace" in lib.pfn_last_error()
    assert call(block=2, ws_bytes=slabs) == -2 and b"workspace" in lib.pfn_last_error()                  # the blocks are missing
    assert call(S=0) == 0
    big_bt, _, big_ei, _ = _inputs(1100, 1530)
    big_plan = sparse_plan(big_bt, big_ei, mode="dc")                        # (held: the header lives in the plan)
    bh = C.addressof(big_plan.header)

    def big(n_lines, n_bus, header, block, columns, waves):
        return lib.pfn_contingency_pairs_sparse(p, n_lines, p, p, p, None, 0, p, 8, p, 1, n_bus, 0, n_bus - 1, 1e-8, 10, p, p, p, p, p, None, p, p, 1 << 30,
                                                header, p, 0, block, 0, columns, waves, None)
    assert big(1530, 1100, bh, 1, 0, 0) == -1 and b"an outage block of 1099 unknowns" in lib.pfn_last_error() and b"bytes of LDS" in lib.pfn_last_error()
    wide_bt, _, wide_ei, _ = _inputs(2400, 3600)
    wide = sparse_plan(wide_bt, wide_ei, mode="dc")
    wh = C.addressof(wide.header)
    assert big(3600, 2400, wh, 0, 1, 16) == -1 and b"column_route 1 (LDS): 17 columns of 2399 unknowns" in lib.pfn_last_error()
    # the dense entry's refusal names the way beyond the cap
    assert lib.pfn_contingency_pairs(p, 20, p, p, p, None, 0, p, 6, p, 4, 1100, 0, 1099, 1e-8, 10, 0, p, p, p, p, p, None, p, p, 1 << 30, None) == -1
    assert b"dense" in lib.pfn_last_error() and b"pfn_contingency_pairs_sparse" in lib.pfn_last_error()


def test_python_argument_errors(monkeypatch):
    bt, spec, ei, rx = _inputs(14, 20, 2)
    dc, ac = sparse_plan(bt, ei, mode="dc"), sparse_plan(bt, ei, mode="ac")
    with pytest.raises(ValueError, match="route.*needs plan=sparse_plan"):   # (the dense screen's test holds "route")
        contingency_screen_pairs(bt, spec, ei, rx, route="sparse")
    with pytest.raises(ValueError, match="mode 'dc'"):
        contingency_screen_pairs(bt, spec, ei, rx, route="sparse", plan=ac)
    with pytest.raises(ValueError, match="the plan is for"):
        contingency_screen_pairs(bt, spec, ei[:, :19], rx[:, :19], route="sparse", plan=dc)
    with pytest.raises(ValueError, match="the plan is for"):
        contingency_screen_pairs(*_inputs(15, 20, 2), route="sparse", plan=dc)
    for kw, text in (({"block": "shared"}, "block"), ({"groups": 0}, "groups"), ({"groups": 2.5}, "groups"), ({"groups": True}, "groups"),
                     ({"threads": 128}, "threads"), ({"columns": "shared"}, "columns"), ({"waves": 3}, "waves"), ({"waves": True}, "waves"),
                     ({"waves": 0}, "waves"), ({"lines": [3, 1]}, "increasing"), ({"lines": [5]}, "two")):
        with pytest.raises(ValueError, match=text):
            contingency_screen_pairs(bt, spec, ei, rx, route="sparse", plan=dc, **kw)
    with pytest.raises(ValueError, match="route must be one of"):
        contingency_screen_pairs(bt, spec, ei, rx, route="dense")
    for kw in ({"plan": dc}, {"block": "lds"}, {"groups": 4}, {"threads": 64}, {"columns": "global"}, {"waves": 4}):   # sparse-only options elsewhere
        with pytest.raises(ValueError, match="route='sparse' only"):
            contingency_screen_pairs(bt, spec, ei, rx, **kw)
        with pytest.raises(ValueError, match="route='sparse' only"):
            contingency_screen_pairs(bt, spec, ei, rx, route="global", **kw)
    with pytest.raises(RuntimeError):                                       # good arguments: the device check is next (no CPU path)
        contingency_screen_pairs(bt, spec, ei, rx, route="sparse", plan=dc, lines=[1, 4, 7], waves=16, columns="global", block="lds", groups=3)
    # "auto" never takes the sparse route: beyond the cap it raises, names n - 1 and max_unknowns(), and points at route="sparse"
    monkeypatch.setattr(L, "require_device", lambda *a, **k: None)           # (the shape checks pass on host tensors; the cap comes next)
    n = int(L.load().pfn_powerflow_max_unknowns()) + 2
    chain = torch.stack([torch.arange(n - 1), torch.arange(1, n)])
    big_bt = torch.tensor([0] + [2] * (n - 1))
    big_spec, big_rx = torch.zeros(1, n, 4, dtype=torch.float64), torch.ones(1, n - 1, 2, dtype=torch.float64)
    for route in ("auto", "lds", "global"):
        with pytest.raises(ValueError, match=rf"{n - 2}.*max_unknowns.*route='sparse'"):
            contingency_screen_pairs(big_bt, big_spec, chain, big_rx, lines=[0, 1, 2], route=route)
