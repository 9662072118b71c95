"""The fast-decoupled sparse plan (csrc/powerflow_plan.cpp pfn_powerflow_sparse_fd_plan) and its numpy interpreter
(tests/powerflow_sparse_fd_ref.py), without a GPU: both halves -- P, B' over the angle buses, and Q, B'' over the PQ buses -- are
valid symbolic factorisations (a permutation, sorted unique columns that hold every matrix position at the slab position the plan
names and are closed under elimination, header counts re-derived, the outer header their totals), P is byte for byte the dc plan,
two builds are byte-identical; the interpreter assembles tests/powerflow_fd_ref.py's B' and B'', in float64 it takes the half-iteration
count of `fast_decoupled` and lands within 2 tol ||J^-1||_inf of its table, with the kernel's float32 factors it still converges to
1e-10 within one half-iteration of the float64 count; bad inputs are PFN_EINVAL with a text and write nothing."""
import functools

import numpy as np
import pytest

from poweflownet_amd.synth import make_physical_inputs
from tests import powerflow_fd_ref as FD
from tests import powerflow_ref as P
from tests import powerflow_sparse_fd_ref as SF
from tests import powerflow_sparse_ref as SP

TOL, MAX_ITER = 1e-10, 60
GRIDS = [(5, 6, None), (14, 20, None), (118, 186, None), (1100, 1530, None), (14, 20, "no_pv"), (14, 20, "no_pq"), (14, 20, "parallel"),
         (14, 20, "lone_pq")]


@functools.lru_cache(maxsize=None)
def _inputs(n, e, kind=None, seed=1):
    ei, bt, rx, spec = make_physical_inputs(n, e, 1, seed)
    return SF.variant_grid(ei.numpy(), bt.numpy(), rx.numpy()[0], spec.numpy()[0], kind)


@functools.lru_cache(maxsize=None)
def _plan(n, e, kind=None, seed=1):
    ei, bt, _, _ = _inputs(n, e, kind, seed)
    rc, blob, text = SF.build_plan(bt, ei)
    assert rc == 0 and blob, text
    return blob, SF.Plan(blob)


def _check_half(half, members, ei):
    """`half` is a valid symbolic factorisation of a matrix with one unknown at each bus of `members` (a boolean mask) and an
    off-diagonal wherever a line joins two of them."""
    n, m = half.n, half.m
    assert m == int(members.sum()) and sorted(half.order.tolist()) == np.flatnonzero(members).tolist()
    assert np.array_equal(half.ua >= 0, members) and (half.uv == -1).all()
    assert sorted(half.ua[members].tolist()) == list(range(m)) and np.array_equal(half.ua[half.order], np.arange(m))
    assert half.colptr[0] == 0 and half.colptr[m] == half.nnz and len(half.rowidx) == half.nnz
    nnz_l = madds = longest = 0
    for j in range(m):
        rows = half.rowidx[half.colptr[j]:half.colptr[j + 1]]
        assert (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < m
        assert half.colptr[j] <= half.diag[j] < half.colptr[j + 1] and half.rowidx[half.diag[j]] == j
        l = half.colptr[j + 1] - half.diag[j] - 1
        nnz_l, madds, longest = nnz_l + l, madds + l * l, max(longest, l)
    assert (half.nnz_l, half.madds, half.max_col) == (nnz_l, madds, longest)
    seen = 0
    for i in range(n):
        for q in range(half.adjptr[i], half.adjptr[i + 1]):
            code, j = half.adj[q]
            assert ei[code & 1, code >> 1] == i and ei[1 - (code & 1), code >> 1] == j
            pos = half.adjpos[q]
            assert (pos[0] >= 0) == bool(members[i] and members[j]) and (pos[1:] == -1).all()
            if pos[0] >= 0:
                assert half.rowidx[pos[0]] == half.ua[i] and half.col_of[pos[0]] == half.ua[j]
            seen += 1
        pos = half.buspos[i]
        assert (pos[0] >= 0) == bool(members[i]) and (pos[1:] == -1).all()
        if pos[0] >= 0:
            assert pos[0] == half.diag[half.ua[i]]
    assert seen == 2 * ei.shape[1]
    pattern = half.pattern()
    below = [half.rowidx[half.diag[k] + 1:half.colptr[k + 1]].tolist() for k in range(m)]
    right = [[] for _ in range(m)]
    for j in range(m):
        for k in half.rowidx[half.colptr[j]:half.diag[j]].tolist():
            right[k].append(j)
    for k in range(m):
        assert {(i, j) for i in below[k] for j in right[k]} <= pattern, k


@pytest.mark.parametrize("n,e,kind", GRIDS)
def test_both_halves_are_valid_symbolic_factorisations(n, e, kind):
    ei, bt, _, _ = _inputs(n, e, kind)
    blob, plan = _plan(n, e, kind)
    assert (plan.n, plan.e, plan.m_p, plan.m_q) == (n, ei.shape[1], n - 1, int((bt == 2).sum()))
    assert plan.slack == int(np.flatnonzero(bt == 0)[0]) == plan.P.slack == plan.Q.slack
    _check_half(plan.P, bt != 0, ei)
    _check_half(plan.Q, bt == 2, ei)
    # the outer header: totals over the halves, the larger longest column, the whole blob's bytes (checked by SF.Plan)
    assert plan.nnz == plan.P.nnz + plan.Q.nnz and plan.nnz_l == plan.P.nnz_l + plan.Q.nnz_l and plan.madds == plan.P.madds + plan.Q.madds
    assert plan.max_col == max(plan.P.max_col, plan.Q.max_col) and plan.header[SP.H_IDX16] == 1 and plan.header[SP.H_N_ADJ] == 2 * ei.shape[1]
    # P is the dc plan of the grid, byte for byte; the line ends of the two halves are the same list
    rc, dc_blob, text = SP.build_plan(bt, ei, 1)
    assert rc == 0 and dc_blob == plan.blob_p, text
    assert np.array_equal(plan.P.adjptr, plan.Q.adjptr) and np.array_equal(plan.P.adj, plan.Q.adj)
    rc, again, _ = SF.build_plan(bt, ei)
    assert rc == 0 and again == blob                                       # a pure function of its inputs
    if kind == "no_pq":
        assert plan.m_q == 0 and plan.Q.nnz == 0 and (plan.Q.ua == -1).all()
    if kind == "lone_pq":
        lone = [j for j in range(plan.m_q) if plan.Q.colptr[j + 1] - plan.Q.colptr[j] == 1]
        assert lone, "no 1 x 1 column in B''"


def test_the_q_order_is_minimum_degree_on_the_graph_induced_on_the_pq_buses():
    # a path 1 - 2 - 3 - 4 - 5 with the slack 0 on bus 1 and bus 3 a PV bus: without 0 and 3 the PQ graph is 1 - 2 and 4 - 5, all
    # of degree 1 -> lowest id first, and each elimination leaves its neighbour at degree 0
    ei = np.array([[0, 1, 2, 3, 4], [1, 2, 3, 4, 5]])
    bt = np.array([0, 2, 2, 1, 2, 2])
    rc, blob, text = SF.build_plan(bt, ei)
    assert rc == 0, text
    plan = SF.Plan(blob)
    assert plan.Q.order.tolist() == [1, 2, 4, 5] and plan.m_q == 4
    assert plan.Q.nnz == 8 and plan.Q.nnz_l == 2                          # two 2 x 2 blocks, the PV bus cuts the path
    assert plan.P.order.tolist() == [1, 2, 3, 4, 5]


@pytest.mark.parametrize("n,e,kind", [(14, 20, None), (14, 20, "parallel"), (14, 20, "lone_pq"), (118, 186, None)])
@pytest.mark.parametrize("variant", ["xb", "bx"])
def test_the_assembled_matrices_are_the_yardsticks(n, e, kind, variant):
    ei, bt, rx, _ = _inputs(n, e, kind)
    plan = _plan(n, e, kind)[1]
    Bp, Bq = FD.fd_matrices(bt, ei, rx, variant)
    wp, wq = SF.weights(rx, variant)
    ang, mag = P.unknowns(bt)
    for half, w, want, buses in ((plan.P, wp, Bp, ang), (plan.Q, wq, Bq, mag)):
        got = SF.dense(half, SF.assemble(half, w, np.float64))[np.ix_(half.ua[buses], half.ua[buses])]
        assert np.abs(got - want).max() <= 8 * P.EPS64 * np.abs(want).max()      # the same sums in another order


@pytest.mark.parametrize("n,e,kind", [(14, 20, None), (14, 20, "no_pv"), (14, 20, "no_pq"), (14, 20, "parallel"), (14, 20, "lone_pq"), (118, 186, None)])
@pytest.mark.parametrize("variant", ["xb", "bx"])
def test_the_float64_interpreter_is_fast_decoupled(n, e, kind, variant):
    """Same half-iteration count; both tables have a mismatch under tol, so to first order J (x_a - x_b) = F_a - F_b and they lie
    within 2 tol ||J^-1||_inf of each other (Vm, and Va in radians) -- the test's own conditioning, no constant."""
    ei, bt, rx, spec = _inputs(n, e, kind)
    plan = _plan(n, e, kind)[1]
    want, want_status, _ = FD.fast_decoupled(bt, spec, ei, rx, variant, tol=TOL, max_iter=MAX_ITER)
    table, status, res = SF.fast_decoupled(plan, bt, spec, ei, rx, variant, tol=TOL, max_iter=MAX_ITER, dtype=np.float64)
    assert 1 <= want_status <= MAX_ITER and status == want_status and res < TOL
    inv_norm = P.jacobian_inverse_norm(want, bt, ei, rx)
    dx = max(np.abs(table[:, 0] - want[:, 0]).max(), np.abs(table[:, 1] - want[:, 1]).max() * P.RAD)
    dp, dq = P.mismatch(table, ei, rx)
    ratio = float((np.maximum(np.abs(dp), np.abs(dq)) / (TOL + 64 * P.EPS64 * P.scale(table, ei, rx))).max())
    print(f"n {n} {kind} {variant}: {status} half-iterations, |x - fast_decoupled| / (2 tol ||J^-1||) {dx / (2 * TOL * inv_norm):.3g}, "
          f"worst |mismatch| / bound {ratio:.3g}")
    assert dx <= 2 * TOL * inv_norm and ratio <= 1.0
    if kind == "no_pq":
        assert np.array_equal(table[:, 0], spec[:, 0])                     # only P halves ran: no Vm moved


@pytest.mark.parametrize("n,e", [(118, 186), (1100, 1530)])
@pytest.mark.parametrize("variant", ["xb", "bx"])
def test_the_float32_factors_converge(n, e, variant):
    ei, bt, rx, spec = _inputs(n, e)
    plan = _plan(n, e)[1]
    table, status, res = SF.fast_decoupled(plan, bt, spec, ei, rx, variant, tol=TOL, max_iter=MAX_ITER, dtype=np.float32)
    _, status64, _ = SF.fast_decoupled(plan, bt, spec, ei, rx, variant, tol=TOL, max_iter=MAX_ITER, dtype=np.float64)
    print(f"n {n} {variant}: m_p {plan.m_p} m_q {plan.m_q}, nnz(L) {plan.P.nnz_l} + {plan.Q.nnz_l}, longest column {plan.max_col}, "
          f"{status} half-iterations with float32 factors ({status64} with float64), residual {res:.3g}")
    assert 1 <= status <= MAX_ITER and res < TOL and abs(status - status64) <= 1
    dp, dq = P.mismatch(table, ei, rx)
    assert (np.maximum(np.abs(dp), np.abs(dq)) <= TOL + 64 * P.EPS64 * P.scale(table, ei, rx)).all()


def test_a_warm_start_and_a_pq_bus_without_a_line():
    ei, bt, rx, spec = _inputs(14, 20)
    plan = _plan(14, 20)[1]
    table, status, _ = SF.fast_decoupled(plan, bt, spec, ei, rx, "xb", tol=TOL, max_iter=MAX_ITER)
    again, status0, res0 = SF.fast_decoupled(plan, bt, spec, ei, rx, "xb", init=table, tol=TOL, max_iter=MAX_ITER)
    assert status >= 1 and status0 == 0 and res0 < TOL
    ei2 = np.where(ei == 13, 1, ei)                                        # bus 13 (PQ) has no line: a zero pivot in both matrices
    assert bt[13] == 2
    rc, blob, text = SF.build_plan(bt, ei2)
    assert rc == 0, text
    assert SF.fast_decoupled(SF.Plan(blob), bt, spec, ei2, rx, "xb", tol=TOL, max_iter=MAX_ITER)[1] == -2


def test_bad_inputs_are_einval_with_a_text_and_write_nothing():
    ei, bt, _, _ = _inputs(14, 20)
    bad_line = ei.copy()
    bad_line[1, 7] = 14
    two_slacks = bt.copy()
    two_slacks[5] = 0
    no_slack = bt.copy()
    no_slack[bt == 0] = 2
    type3 = bt.copy()
    type3[6] = 3
    from poweflownet_amd import _lib as L
    lib = L.load()
    for types, lines, word in [(bt, bad_line, "outside"), (two_slacks, ei, "slack"), (no_slack, ei, "slack"), (type3, ei, "type 3")]:
        rc, blob, text = SF.build_plan(types, lines)
        assert rc == -1 and blob is None and word in text and text.startswith("pfn_powerflow_sparse_fd_plan:"), (rc, text)
        bt32, ei64 = np.ascontiguousarray(types, dtype=np.int32), np.ascontiguousarray(lines, dtype=np.int64)
        big = np.full(1 << 16, 7, dtype=np.uint8)
        assert lib.pfn_powerflow_sparse_fd_plan(ei64.ctypes.data, 20, bt32.ctypes.data, 14, big.ctypes.data, big.size) == -1
        assert (big == 7).all() and word.encode() in lib.pfn_last_error()
    bt32, ei64 = bt.astype(np.int32), np.ascontiguousarray(ei)
    need = lib.pfn_powerflow_sparse_fd_plan_bytes(ei64.ctypes.data, 20, bt32.ctypes.data, 14)
    assert need == len(_plan(14, 20)[0])
    small = np.full(need, 7, dtype=np.uint8)
    assert lib.pfn_powerflow_sparse_fd_plan(ei64.ctypes.data, 20, bt32.ctypes.data, 14, small.ctypes.data, need - 1) == -1
    assert (small == 7).all() and b"bytes" in lib.pfn_last_error()           # nothing written
    assert lib.pfn_powerflow_sparse_fd_plan(ei64.ctypes.data, 20, bt32.ctypes.data, 14, None, need) == -1 and b"null" in lib.pfn_last_error()
    # the workspace size comes from the outer header alone; an ac plan's header, or a blob that is no plan, answers 0 -- and the
    # Newton route's sizer refuses the fd header likewise
    blob, plan = _plan(14, 20)
    head = np.frombuffer(blob, dtype=np.int32)[:SP.HEADER_WORDS].copy()
    per_sample = lib.pfn_powerflow_sparse_fd_workspace_bytes(1, head.ctypes.data)
    assert per_sample >= 8 * (4 * 14 + max(plan.m_p, plan.m_q)) + 4 * plan.nnz and per_sample % 16 == 0
    assert lib.pfn_powerflow_sparse_fd_workspace_bytes(3, head.ctypes.data) == 3 * per_sample
    assert lib.pfn_powerflow_sparse_workspace_bytes(1, head.ctypes.data) == 0
    ac = np.frombuffer(SP.build_plan(bt, ei)[1], dtype=np.int32)[:SP.HEADER_WORDS].copy()
    assert lib.pfn_powerflow_sparse_fd_workspace_bytes(1, ac.ctypes.data) == 0
    head[0] ^= 1
    assert lib.pfn_powerflow_sparse_fd_workspace_bytes(1, head.ctypes.data) == 0


def test_the_symbols_are_declared_and_listed():
    from poweflownet_amd import _lib as L
    names = ("pfn_powerflow_sparse_fd_plan_bytes", "pfn_powerflow_sparse_fd_plan", "pfn_powerflow_sparse_fd_workspace_bytes", "pfn_powerflow_solve_sparse_fd")
    assert all(name in L.SYMBOLS for name in names) and L.load().pfn_abi_version() == 8
