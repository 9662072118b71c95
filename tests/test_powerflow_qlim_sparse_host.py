"""The host side of the sparse Q-limited solve without a GPU: `qlim_plan` (utils/powerflow.py) builds the plan of the type row with
every non-slack bus PQ -- header m == 2 (n - 1), byte-equal to `sparse_plan(all_pq, ...)`, a `CoverPlan` for per-sample lists -- and
refuses rows whose slacks differ; `solve_power_flow_qlim(route="sparse")` refuses the wrong plan before anything touches a device;
the library sizes the workspace and refuses a plan that is not the all-PQ one."""
import ctypes as C

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.synth import make_physical_inputs
from poweflownet_amd.utils.powerflow import CoverPlan, SparsePlan, cover_plan, qlim_plan, solve_power_flow_qlim, sparse_plan
from tests import topology_ref as T


def _all_pq(bt):
    return torch.where(bt == 0, 0, 2).to(torch.int32)


@pytest.mark.parametrize("n,e", [(5, 6), (14, 20), (118, 186)])
def test_the_plan_is_the_all_pq_rows(n, e):
    ei, bt, _, _ = make_physical_inputs(n, e, 0, 1)
    assert int((bt == 1).sum()) >= 1
    plan = qlim_plan(bt, ei)
    assert isinstance(plan, SparsePlan) and (plan.n, plan.e, plan.mode, plan.m) == (n, e, "ac", 2 * (n - 1))
    assert int(plan.header[4]) == 2 * (n - 1) and int(plan.header[5]) == 0
    want = sparse_plan(_all_pq(bt), ei, "ac")
    assert torch.equal(plan.blob, want.blob) and plan.nnz == want.nnz and plan.madds == want.madds
    own = sparse_plan(bt, ei, "ac")
    assert own.m < plan.m and own.nnz < plan.nnz                       # the dead unknowns are paid for in fill
    # [S, n] rows with their own PV sets and the same slack give the same plan; int64 and int32 alike
    rows = torch.stack([bt, _all_pq(bt).long(), bt])
    assert torch.equal(qlim_plan(rows, ei).blob, plan.blob) and torch.equal(qlim_plan(bt.to(torch.int32), ei).blob, plan.blob)
    assert torch.equal(qlim_plan(bt, ei, size_hint=plan.bytes).blob, plan.blob)


def test_per_sample_lists_give_a_cover_plan():
    n, e, S = 14, 20, 4
    ei, bt, _, _ = make_physical_inputs(n, e, S, 1)
    lists, _, status = T.perturb(ei.numpy(), n, S, remove=1, add=1, seed=1)
    assert (status >= 1).all()
    plan = qlim_plan(bt, torch.from_numpy(lists), ei)
    want = cover_plan(_all_pq(bt), torch.from_numpy(lists), "ac", ei)
    assert isinstance(plan, CoverPlan) and plan.plan.m == 2 * (n - 1) and plan.e_base == e and plan.extras >= 1
    assert torch.equal(plan.plan.blob, want.plan.blob) and torch.equal(plan.cover, want.cover) and torch.equal(plan.slot, want.slot)


def test_qlim_plan_refusals():
    ei, bt, _, _ = make_physical_inputs(14, 20, 0, 1)
    moved = bt.clone()
    moved[int((bt == 0).nonzero()[0])], moved[int((bt == 2).nonzero()[0])] = 2, 0
    with pytest.raises(RuntimeError, match="same bus"):
        qlim_plan(torch.stack([bt, moved]), ei)                         # two slack positions
    two = bt.clone()
    two[int((bt == 2).nonzero()[0])] = 0
    with pytest.raises(RuntimeError, match="exactly one slack"):
        qlim_plan(two, ei)
    with pytest.raises(RuntimeError, match="exactly one slack"):
        qlim_plan(torch.full((14,), 2), ei)
    with pytest.raises(RuntimeError, match="bus_type must be"):
        qlim_plan(bt.double(), ei)
    with pytest.raises(RuntimeError, match="bus_type must be"):
        qlim_plan(bt[None, None], ei)
    with pytest.raises(RuntimeError, match="edge_index must be"):
        qlim_plan(bt, ei.T.contiguous())
    with pytest.raises(RuntimeError, match="edge_index must be"):
        qlim_plan(bt, ei.to(torch.int32))
    with pytest.raises(RuntimeError, match="sparse_plan failed"):       # the builder's own refusal: a line outside the grid
        qlim_plan(bt[:13], ei)


def test_solve_refuses_the_wrong_plan_before_a_device_is_touched():
    n, e, S = 14, 20, 2
    ei, bt, rx, spec = make_physical_inputs(n, e, S, 1)
    plan = qlim_plan(bt, ei)
    with pytest.raises(ValueError, match=r"sparse route.*plan=qlim_plan"):
        solve_power_flow_qlim(bt, spec, ei, rx, route="sparse")
    with pytest.raises(ValueError, match="route='sparse' only"):
        solve_power_flow_qlim(bt, spec, ei, rx, plan=plan)
    with pytest.raises(RuntimeError, match="every non-slack bus PQ"):   # the grid's own-types plan: m != 2 (n - 1)
        solve_power_flow_qlim(bt, spec, ei, rx, route="sparse", plan=sparse_plan(bt, ei))
    with pytest.raises(RuntimeError, match="every non-slack bus PQ"):   # another mode
        solve_power_flow_qlim(bt, spec, ei, rx, route="sparse", plan=sparse_plan(_all_pq(bt), ei, "dc"))
    with pytest.raises(RuntimeError, match="the plan is for"):          # another e
        solve_power_flow_qlim(bt, spec, ei[:, :19].contiguous(), rx[:, :19].contiguous(), route="sparse", plan=plan)
    ei5, bt5, rx5, spec5 = make_physical_inputs(5, 6, S, 1)
    with pytest.raises(RuntimeError, match="the plan is for"):          # another n
        solve_power_flow_qlim(bt5, spec5, ei5, rx5, route="sparse", plan=plan)
    lists = ei[None].expand(S, 2, e).contiguous()
    cover = qlim_plan(bt, lists, ei)
    with pytest.raises(RuntimeError, match="CoverPlan goes with per-sample"):
        solve_power_flow_qlim(bt, spec, ei, rx, route="sparse", plan=cover)
    with pytest.raises(RuntimeError, match="CoverPlan goes with per-sample"):
        solve_power_flow_qlim(bt, spec, lists, rx, route="sparse", plan=plan)
    with pytest.raises(RuntimeError, match="plan must be what qlim_plan returns"):
        solve_power_flow_qlim(bt, spec, ei, rx, route="sparse", plan=object())
    with pytest.raises(RuntimeError, match="the plan lives on"):        # a plan on another device than the inputs
        solve_power_flow_qlim(bt, spec, ei, rx, route="sparse", plan=SparsePlan(**{**plan.__dict__, "blob": plan.blob.to("meta")}))
    # the right plan passes every host check: what is left is that there is no CPU solver
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        solve_power_flow_qlim(bt, spec, ei, rx, route="sparse", plan=plan)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        solve_power_flow_qlim(bt, spec, lists, rx, route="sparse", plan=cover)


def test_the_library_sizes_the_sample_and_refuses_other_plans():
    lib = L.load()
    n, e = 118, 186
    ei, bt, _, _ = make_physical_inputs(n, e, 0, 1)
    plan, own = qlim_plan(bt, ei), sparse_plan(bt, ei)
    m, nnz = plan.m, plan.nnz
    sparse = (8 * (4 * n + m) + 4 * nnz + 15) // 16 * 16               # the sparse route's sample (pf_sample_bytes)
    assert lib.pfn_powerflow_sparse_workspace_bytes(3, C.addressof(plan.header)) == 3 * sparse
    assert lib.pfn_powerflow_sparse_qlim_workspace_bytes(3, C.addressof(plan.header)) == 3 * (sparse + (8 * n + 15) // 16 * 16)
    assert lib.pfn_powerflow_sparse_qlim_workspace_bytes(0, C.addressof(plan.header)) == 0
    assert lib.pfn_powerflow_sparse_qlim_workspace_bytes(3, C.addressof(own.header)) == 0
    assert b"every non-slack bus PQ" in lib.pfn_last_error()
    # the entry refuses that plan by its header, before it looks at a pointer
    rc = lib.pfn_powerflow_solve_sparse_qlim(None, e, None, None, None, None, 0, None, None, None, 0, 1, n, 1e-8, 1e-8, 10, 8, C.addressof(own.header),
                                             None, 0, None, None, None, None, None, None, None, 0, None)
    assert rc == -1 and b"every non-slack bus PQ" in lib.pfn_last_error()
    rc = lib.pfn_powerflow_solve_sparse_qlim(None, e, None, None, None, None, 0, None, None, None, 0, 1, n, 1e-8, 1e-8, 10, -1, C.addressof(plan.header),
                                             None, 0, None, None, None, None, None, None, None, 0, None)
    assert rc == -1 and b"max_rounds" in lib.pfn_last_error()
    rc = lib.pfn_powerflow_solve_sparse_qlim(None, e, None, None, None, None, 0, None, None, None, 0, 1, n + 1, 1e-8, 1e-8, 10, 8,
                                             C.addressof(plan.header), None, 0, None, None, None, None, None, None, None, 0, None)
    assert rc == -1 and b"the plan is for" in lib.pfn_last_error()
    rc = lib.pfn_powerflow_solve_sparse_qlim(None, e, None, None, None, None, 0, None, None, None, 0, 0, n, 1e-8, 1e-8, 10, 8, C.addressof(plan.header),
                                             None, 0, None, None, None, None, None, None, None, 0, None)
    assert rc == 0                                                     # no samples: nothing to do, nothing looked at


def test_the_fill_the_dead_unknowns_cost():
    """the figures of DESIGN 7r's table at (118, 186): own types against every non-slack bus PQ, from the host plan builder"""
    ei, bt, _, _ = make_physical_inputs(118, 186, 0, 1)
    own, plan = sparse_plan(bt, ei), qlim_plan(bt, ei)
    print(f"(118, 186): m {own.m} -> {plan.m}, slab positions {own.nnz} -> {plan.nnz}, multiply-adds per factor {own.madds} -> {plan.madds} "
          f"({plan.madds / own.madds:.2f} x)")
    assert (own.m, plan.m) == (195, 234) and (own.nnz, plan.nnz) == (2571, 3868) and (own.madds, plan.madds) == (12144, 23409)
