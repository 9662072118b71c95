"""The sparse power-flow plan (csrc/powerflow_plan.cpp) and its numpy interpreter (tests/powerflow_sparse_ref.py), without a GPU: the
plan is a valid symbolic factorisation -- a permutation, sorted unique columns that hold every Jacobian position and are closed under
elimination, byte-identical between two builds; the interpreter in float64 takes np.linalg.solve's Newton steps; with the kernel's
float32 factor it still converges to 1e-10; bad inputs are PFN_EINVAL with a text."""
import functools

import numpy as np
import pytest

from poweflownet_amd.synth import make_physical_inputs
from tests import powerflow_ref as P
from tests import powerflow_sparse_ref as SP

TOL, MAX_ITER = 1e-10, 10


@functools.lru_cache(maxsize=None)
def _inputs(n, e, types=None, seed=1):
    ei, bt, rx, spec = make_physical_inputs(n, e, 1, seed)
    ei, bt, rx, spec = ei.numpy(), bt.numpy().copy(), rx.numpy()[0], spec.numpy()[0].copy()
    if types == "no_pv":
        bt[bt == 1] = 2
    elif types == "no_pq":
        spec[bt == 2, 0] = 1.02
        bt[bt == 2] = 1
    return ei, bt, rx, spec


@functools.lru_cache(maxsize=None)
def _plan(n, e, types=None, mode=0):
    ei, bt, _, _ = _inputs(n, e, types)
    rc, blob, text = SP.build_plan(bt, ei, mode)
    assert rc == 0 and blob, text
    return blob, SP.Plan(blob)


def _check_valid(plan, bt, ei, mode):
    n, m = plan.n, plan.m
    ang, mag = P.unknowns(bt)
    assert m == len(ang) + (len(mag) if mode == 0 else 0)
    # the order is a permutation of the non-slack buses, the unknowns one of range(m), a bus's theta directly before its Vm
    assert sorted(plan.order.tolist()) == sorted(ang.tolist()) and plan.slack == int(np.flatnonzero(bt == 0)[0])
    numbers = np.concatenate([plan.ua[plan.ua >= 0], plan.uv[plan.uv >= 0]])
    assert sorted(numbers.tolist()) == list(range(m))
    assert np.array_equal(plan.ua >= 0, bt != 0) and np.array_equal(plan.uv >= 0, (bt == 2) & (mode == 0))
    assert (plan.uv[plan.uv >= 0] == plan.ua[plan.uv >= 0] + 1).all()
    assert (np.diff(plan.ua[plan.order]) > 0).all()
    # columns: sorted, unique, in range, the diagonal where the header says
    assert plan.colptr[0] == 0 and plan.colptr[m] == plan.nnz and len(plan.rowidx) == plan.nnz
    nnz_l = madds = longest = 0
    for j in range(m):
        rows = plan.rowidx[plan.colptr[j]:plan.colptr[j + 1]]
        assert (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < m
        assert plan.rowidx[plan.diag[j]] == j and plan.colptr[j] <= plan.diag[j] < plan.colptr[j + 1]
        l = plan.colptr[j + 1] - plan.diag[j] - 1
        nnz_l, madds, longest = nnz_l + l, madds + l * l, max(longest, l)
    assert (plan.nnz_l, plan.madds, plan.max_col) == (nnz_l, madds, longest)
    # every Jacobian position is in the pattern, at the slab position the plan names
    unknown = (plan.ua, plan.uv)
    seen = 0
    for i in range(n):
        for q in range(plan.adjptr[i], plan.adjptr[i + 1]):
            code, j = plan.adj[q]
            assert ei[code & 1, code >> 1] == i and ei[1 - (code & 1), code >> 1] == j
            for c, (ri, cj) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
                r, col, pos = unknown[ri][i], unknown[cj][j], plan.adjpos[q, c]
                assert (pos >= 0) == (r >= 0 and col >= 0)
                if pos >= 0:
                    assert plan.rowidx[pos] == r and plan.col_of[pos] == col
            seen += 1
        for c, (ri, cj) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
            r, col, pos = unknown[ri][i], unknown[cj][i], plan.buspos[i, c]
            assert (pos >= 0) == (r >= 0 and col >= 0)
            if pos >= 0:
                assert plan.rowidx[pos] == r and plan.col_of[pos] == col
    assert seen == 2 * ei.shape[1]
    # closed under elimination: k < i, j with (i, k) and (k, j) present => (i, j) present
    pattern = plan.pattern()
    below = [plan.rowidx[plan.diag[k] + 1:plan.colptr[k + 1]].tolist() for k in range(m)]           # rows i > k of column k
    right = [[] for _ in range(m)]                                                                     # columns j > k of row k
    for j in range(m):
        for k in plan.rowidx[plan.colptr[j]:plan.diag[j]].tolist():
            right[k].append(j)
    for k in range(m):
        assert {(i, j) for i in below[k] for j in right[k]} <= pattern, k


@pytest.mark.parametrize("n,e,types,mode", [(5, 6, None, 0), (14, 20, None, 0), (118, 186, None, 0), (1100, 1530, None, 0), (14, 20, "no_pv", 0),
                                            (14, 20, "no_pq", 0), (5, 6, None, 1), (14, 20, None, 1), (118, 186, None, 1)])
def test_the_plan_is_a_valid_symbolic_factorisation(n, e, types, mode):
    ei, bt, _, _ = _inputs(n, e, types)
    blob, plan = _plan(n, e, types, mode)
    _check_valid(plan, bt, ei, mode)
    rc, again, _ = SP.build_plan(bt, ei, mode)
    assert rc == 0 and again == blob                                       # a pure function of its inputs


def test_the_order_is_minimum_degree_with_ties_to_the_lowest_bus():
    # a path 1 - 2 - 3 - 4 with the slack 0 hanging off bus 2: degrees without the slack are 1, 2, 2, 1 -> bus 1 first; then 2 has
    # degree 1 like 4: the lower id goes; and so on
    ei = np.array([[1, 2, 3, 0], [2, 3, 4, 2]])
    bt = np.array([0, 2, 2, 1, 2])
    rc, blob, text = SP.build_plan(bt, ei)
    assert rc == 0, text
    assert SP.Plan(blob).order.tolist() == [1, 2, 3, 4]
    # a star around bus 3: its leaves go first, lowest id first, the centre once its degree has dropped to theirs
    ei = np.array([[3, 3, 3, 3], [0, 1, 2, 4]])
    rc, blob, text = SP.build_plan(np.array([0, 2, 2, 2, 2]), ei)
    assert rc == 0, text
    assert SP.Plan(blob).order.tolist() == [1, 2, 3, 4]


def test_parallel_lines_and_a_stored_self_pair_do_not_break_it():
    ei, bt, rx, spec = _inputs(14, 20)
    ei2 = np.concatenate([ei, ei[:, :3], ei[::-1, 3:5], np.array([[4], [4]])], axis=1)       # copies, reversed copies, bus 4 to itself
    rc, blob, text = SP.build_plan(bt, ei2)
    assert rc == 0, text
    plan = SP.Plan(blob)
    _check_valid(plan, bt, ei2, 0)
    base = _plan(14, 20)[1]
    assert plan.order.tolist() == base.order.tolist() and np.array_equal(plan.rowidx, base.rowidx)   # the bus graph is the same
    # ... and the interpreter still takes np.linalg.solve's step on the widened line list
    rx2 = np.concatenate([rx, rx[:3], rx[3:5], rx[:1]])
    steps = []
    table, status, _ = SP.newton(plan, bt, spec, ei2, rx2, tol=TOL, max_iter=MAX_ITER, dtype=np.float64, steps=steps)
    assert 1 <= status <= MAX_ITER
    vm, th, F, dx = steps[0]
    assert np.abs(F - _mismatch_vector(vm, th, bt, spec, ei2, rx2)).max() <= 64 * P.EPS64 * P.scale(np.stack([vm, th / P.RAD, spec[:, 2], spec[:, 3]], axis=1), ei2, rx2).max()
    want = np.linalg.solve(P.flow_jacobian(vm, th, bt, ei2, rx2), F)
    assert np.abs(dx - want).max() <= 1e-9 * np.abs(want).max()


def test_a_bus_without_a_line_is_planned_and_is_a_zero_pivot():
    ei, bt, rx, spec = _inputs(14, 20)
    ei2 = np.where(ei == 13, 1, ei)
    rc, blob, text = SP.build_plan(bt, ei2)
    assert rc == 0, text
    plan = SP.Plan(blob)
    _check_valid(plan, bt, ei2, 0)
    assert SP.newton(plan, bt, spec, ei2, rx, tol=TOL, max_iter=MAX_ITER)[1] == -2


def _mismatch_vector(vm, th, bt, spec, ei, rx):
    ang, mag = P.unknowns(bt)
    dp, dq = P.mismatch(np.stack([vm, th / P.RAD, spec[:, 2], spec[:, 3]], axis=1), ei, rx)
    return np.concatenate([dp[ang], dq[mag]])


@pytest.mark.parametrize("n,e", [(14, 20), (118, 186)])
def test_the_float64_interpreter_takes_the_dense_newton_steps(n, e):
    ei, bt, rx, spec = _inputs(n, e)
    plan = _plan(n, e)[1]
    steps = []
    table, status, res = SP.newton(plan, bt, spec, ei, rx, tol=TOL, max_iter=MAX_ITER, dtype=np.float64, steps=steps)
    assert 1 <= status <= MAX_ITER and len(steps) == status and res < TOL
    worst = 0.0
    for vm, th, F, dx in steps:
        # the right-hand side is the yardstick's mismatch up to the rounding of summing it in another form (the last step's dx is of
        # the size of that rounding times ||J^-1||, so the solve is compared on the interpreter's own F)
        cur = np.stack([vm, th / P.RAD, spec[:, 2], spec[:, 3]], axis=1)
        assert np.abs(F - _mismatch_vector(vm, th, bt, spec, ei, rx)).max() <= 64 * P.EPS64 * P.scale(cur, ei, rx).max()
        want = np.linalg.solve(P.flow_jacobian(vm, th, bt, ei, rx), F)
        worst = max(worst, float(np.abs(dx - want).max() / np.abs(want).max()))
    dp, dq = P.mismatch(table, ei, rx)
    ratio = float((np.maximum(np.abs(dp), np.abs(dq)) / (TOL + 64 * P.EPS64 * P.scale(table, ei, rx))).max())
    print(f"n {n}: {status} solves, worst |dx - dense| / max |dx| {worst:.3g}, worst |mismatch| / bound {ratio:.3g}")
    assert worst <= 1e-9 and ratio <= 1.0
    want_table, want_status, _ = P.newton(bt, spec, ei, rx, tol=TOL, max_iter=MAX_ITER)
    assert want_status == status and np.abs(table - want_table).max() <= 1e-9


def test_the_float64_interpreter_in_dc_mode():
    ei, bt, rx, spec = _inputs(14, 20)
    plan = _plan(14, 20, None, 1)[1]
    table, status, res = SP.newton(plan, bt, spec, ei, rx, tol=TOL, max_iter=MAX_ITER, dtype=np.float64)
    assert 1 <= status <= 2 and res < TOL
    want, inv_norm = P.dc_solve(bt, spec, ei, rx)
    F = P.dc_mismatch(table, ei, rx, bt)
    assert (np.abs(F) <= TOL + 64 * P.EPS64 * P.dc_scale(table, ei, rx)).all()
    assert np.abs(table[:, 1] - want[:, 1]).max() * P.RAD <= 2 * TOL * inv_norm and np.isnan(table[:, 3]).all()


@pytest.mark.parametrize("n,e", [(118, 186), (1100, 1530)])
def test_the_float32_factor_converges(n, e):
    ei, bt, rx, spec = _inputs(n, e)
    plan = _plan(n, e)[1]
    table, status, res = SP.newton(plan, bt, spec, ei, rx, tol=TOL, max_iter=MAX_ITER, dtype=np.float32)
    print(f"n {n} m {plan.m}: nnz(L) {plan.nnz_l}, longest column {plan.max_col}, {status} solves with the float32 factor, residual {res:.3g}")
    assert 1 <= status <= MAX_ITER and res < TOL
    dp, dq = P.mismatch(table, ei, rx)
    assert (np.maximum(np.abs(dp), np.abs(dq)) <= TOL + 64 * P.EPS64 * P.scale(table, ei, rx)).all()


def test_bad_inputs_are_einval_with_a_text():
    ei, bt, _, _ = _inputs(14, 20)
    bad_line = ei.copy()
    bad_line[1, 7] = 14
    two_slacks = bt.copy()
    two_slacks[5] = 0
    no_slack = bt.copy()
    no_slack[bt == 0] = 2
    type3 = bt.copy()
    type3[6] = 3
    for types, lines, word in [(bt, bad_line, "outside"), (two_slacks, ei, "slack"), (no_slack, ei, "slack"), (type3, ei, "type 3")]:
        rc, blob, text = SP.build_plan(types, lines)
        assert rc == -1 and blob is None and word in text, (rc, text)
    from poweflownet_amd import _lib as L
    lib = L.load()
    bt32, ei64 = bt.astype(np.int32), np.ascontiguousarray(ei)
    need = lib.pfn_powerflow_sparse_plan_bytes(ei64.ctypes.data, 20, bt32.ctypes.data, 14, 0)
    small = np.full(need, 7, dtype=np.uint8)
    assert lib.pfn_powerflow_sparse_plan(ei64.ctypes.data, 20, bt32.ctypes.data, 14, 0, small.ctypes.data, need - 1) == -1
    assert (small == 7).all() and b"bytes" in lib.pfn_last_error()           # nothing written
    assert lib.pfn_powerflow_sparse_plan(ei64.ctypes.data, 20, bt32.ctypes.data, 14, 2, small.ctypes.data, need) == -1
    assert lib.pfn_powerflow_sparse_plan_bytes(ei64.ctypes.data, 20, bt32.ctypes.data, 14, 2) == 0
    # the workspace size comes from the header alone; a blob that is no plan answers 0
    rc, blob, _ = SP.build_plan(bt, ei)
    head = np.frombuffer(blob, dtype=np.int32)[:SP.HEADER_WORDS].copy()
    plan = SP.Plan(blob)
    per_sample = lib.pfn_powerflow_sparse_workspace_bytes(1, head.ctypes.data)
    assert per_sample >= 8 * (4 * 14 + plan.m) + 4 * plan.nnz and lib.pfn_powerflow_sparse_workspace_bytes(3, head.ctypes.data) == 3 * per_sample
    head[0] ^= 1
    assert lib.pfn_powerflow_sparse_workspace_bytes(1, head.ctypes.data) == 0
