"""The fast-decoupled modes on the sparse route, on the device: `pfn_powerflow_solve_sparse_fd` (csrc/powerflow_sparse_fd.hip) through
`solve_power_flow(mode="fdxb" | "fdbx", route="sparse", plan=sparse_plan(..., "fd"))`, with tol = 1e-10 and max_iter = 60
half-iterations, held to the bounds of tests/test_gpu_powerflow_sparse.py --
  residual   the yardstick's mismatch of the WRITTEN table, at all buses, <= tol + 64 * 2^-52 * scale_i;
  solution   Vm and Va (radians) within 2 tol ||J^-1||_inf of the float64 yardstick's solution (tests/powerflow_fd_ref.py
             `fast_decoupled`) and of the dense route's table;
  count      the half-iterations within +-1 of the float32 interpreter's (tests/powerflow_sparse_fd_ref.py): a float32 factor moves
             the contraction factor by about 1e-7 * cond, so it moves the count only where a residual lands that close to tol
-- at shapes the dense route takes too (m_p = 64 and 65 either side of the 64-column metadata batches among them), at (1100, 1530)
which it refuses, on grids without a PQ bus, without a PV bus, with parallel lines and with a PQ bus between the slack and PV buses
only; warm starts; bit-for-bit independence of a sample from its batch, the workgroup size and who built the plan; failures that stay
local; what raises; hipGraph capture; one sample of the workload size (6470, 9005); speedup_evaluator.py with the route forced.

Measured on an MI355X (bound 1; each test prints its own; DESIGN.md section 7l has the table): at every sample of every shape the
device's half-iteration count, the float32 interpreter's and the float64 yardstick's were IDENTICAL -- xb / bx 14..16 / 13..21 at
(5, 6, 3), 17..25 / 15..19 at (14, 20, 8), 22..29 / 21..23 at (70, 100, 4), 21..35 / 19..23 at (118, 186, 4), 27, 31 / 20, 21 at
(65, 90, 2), 27, 31 / 19, 19 at (66, 92, 2), 43, 41 / 25, 23 at (1100, 1530, 2); worst mismatch / bound 0.98 (the method converges
linearly: the last residual lands just under tol); worst distance to the yardstick's solution 1.1e-5 of its bound, to the dense
route's 5.4e-6, to sparse Newton's at (1100, 1530) 4.6e-4.  Workload size: the float64 yardstick on the host (B' and B'' inverted
once, mat-vecs after that) takes 43 half-iterations of fdxb at tol 1e-8 on (6470, 9005), inside 100, and the device takes 43 in
0.21 s (the test: 0.64 s), so neither case of the (2000, 2784) fallback arose."""
import functools
import re
import time

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.synth import make_physical_inputs
from poweflownet_amd.utils import powerflow as PF
from poweflownet_amd.utils.powerflow import max_unknowns, solve_power_flow, sparse_plan
from tests import powerflow_fd_ref as FD
from tests import powerflow_ref as P
from tests import powerflow_sparse_fd_ref as SF
from tests.powerflow_checks import DEV, TOL, _check_given, _dev, _distance, _residual_ratio, _run

pytestmark = pytest.mark.gpu
MAX_ITER = 60
VARIANT = {"fdxb": "xb", "fdbx": "bx"}


class _Case:
    """Inputs of one shape on the host; the yardstick's solutions, ||J^-1|| and the interpreter's counts computed once, where asked."""

    def __init__(self, n, e, S, seed, load=0.2, kind=None):
        ei, bt, rx, spec = make_physical_inputs(n, e, S, seed, load)
        self.ei, self.bt, self.rx, self.spec = SF.variant_grid(ei.numpy(), bt.numpy(), rx.numpy(), spec.numpy(), kind)
        self.n, self.e, self.S = n, int(self.ei.shape[1]), S

    @functools.lru_cache(maxsize=None)
    def ref(self, mode):
        """([S, n, 4] float64 tables, statuses) of the dense float64 yardstick."""
        out = [FD.fast_decoupled(self.bt, self.spec[s], self.ei, self.rx[s], VARIANT[mode], tol=TOL, max_iter=MAX_ITER) for s in range(self.S)]
        assert all(1 <= st <= MAX_ITER for _, st, _ in out), [st for _, st, _ in out]
        return np.stack([t for t, _, _ in out]), np.array([st for _, st, _ in out])

    @functools.lru_cache(maxsize=None)
    def count32(self, mode):
        """Half-iterations of the interpreter with the kernel's float32 factors."""
        rc, blob, text = SF.build_plan(self.bt, self.ei)
        assert rc == 0, text
        plan = SF.Plan(blob)
        return np.array([SF.fast_decoupled(plan, self.bt, self.spec[s], self.ei, self.rx[s], VARIANT[mode], tol=TOL, max_iter=MAX_ITER,
                                           dtype=np.float32)[1] for s in range(self.S)])

    @functools.cached_property
    def inv_norm(self):
        ref = self.ref("fdxb")[0]
        return np.array([P.jacobian_inverse_norm(ref[s], self.bt, self.ei, self.rx[s]) for s in range(self.S)])

    @functools.cached_property
    def plan(self):
        return sparse_plan(_dev(self.bt), _dev(self.ei), "fd")

    def solve(self, mode="fdxb", rows=slice(None), **kw):
        kw = {"tol": TOL, "max_iter": MAX_ITER, "route": "sparse", **kw}
        if kw["route"] == "sparse" and "plan" not in kw:
            kw["plan"] = self.plan
        threads = kw.pop("threads", None)
        args = (_dev(self.bt), _dev(self.spec[rows]), _dev(self.ei), _dev(self.rx[rows]))
        if threads is not None:                                 # the workgroup size forced: the module's internal entry
            return PF._solve(*args, mode, kw["tol"], kw["max_iter"], kw["route"], kw.get("init"), kw["plan"], threads)
        return solve_power_flow(*args, mode=mode, **kw)


@functools.lru_cache(maxsize=None)
def _case(n, e, S, seed=1, load=0.2, kind=None):
    return _Case(n, e, S, seed, load, kind)


def _check_accuracy(case, mode, res, dense=True):
    S = case.S
    table, status = res.table.cpu().numpy(), res.status.cpu().numpy()
    assert res.route == "sparse" and table.shape == (S, case.n, 4) and table.dtype == np.float64 and int(res.flags.item()) == 0
    assert ((status >= 1) & (status <= MAX_ITER)).all(), status
    assert torch.equal(res.iterations, res.status) and bool((res.residual < TOL).all())
    ref, ref_status = case.ref(mode)
    count32 = case.count32(mode)
    worst_f = _residual_ratio(case, table)
    worst_x = max(float(_distance(table[s], ref[s]) / (2 * TOL * case.inv_norm[s])) for s in range(S))
    worst_d = 0.0
    if dense:
        other = case.solve(mode, route="auto")
        assert other.route in ("lds", "global") and bool((other.status >= 1).all())
        other_table = other.table.cpu().numpy()
        worst_d = max(float(_distance(table[s], other_table[s]) / (2 * TOL * case.inv_norm[s])) for s in range(S))
    _check_given(case, table)
    print(f"sparse {mode} n {case.n} e {case.e} S {S} m_p {case.plan.m} m_q {case.plan.m_q}: half-iterations {status.tolist()} "
          f"(float32 interpreter {count32.tolist()}, float64 yardstick {ref_status.tolist()}), worst |mismatch| / bound {worst_f:.3g}, "
          f"|x - yardstick| / (2 tol ||J^-1||) {worst_x:.3g}, |x - dense route| / same {worst_d:.3g}")
    assert worst_f <= 1.0 and worst_x <= 1.0 and worst_d <= 1.0
    assert (np.abs(status - count32) <= 1).all()
    return table, status


# ------------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("mode", ["fdxb", "fdbx"])
@pytest.mark.parametrize("n,e,S", [(5, 6, 3), (14, 20, 8), (70, 100, 4), (118, 186, 4), (65, 90, 2), (66, 92, 2)])
def test_residual_solution_and_count_against_the_yardsticks_and_the_dense_route(n, e, S, mode):
    case = _case(n, e, S)
    _check_accuracy(case, mode, case.solve(mode))


# -------------------------------------------------------------------------- the shape the dense routes refuse
@pytest.mark.parametrize("mode", ["fdxb", "fdbx"])
def test_beyond_the_dense_cap(mode):
    case = _case(1100, 1530, 2)
    assert (case.n - 1) + int((case.bt == 2).sum()) == 1832 > max_unknowns()
    res = case.solve(mode)
    status, table = res.status.cpu().numpy(), res.table.cpu().numpy()
    assert res.route == "sparse" and ((status >= 1) & (status <= MAX_ITER)).all(), status
    worst = _residual_ratio(case, table)
    _check_given(case, table)
    newton = solve_power_flow(_dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx), tol=TOL, max_iter=10, route="sparse")
    assert bool((newton.status >= 1).all())
    newton_table = newton.table.cpu().numpy()
    worst_x = max(float(_distance(table[s], newton_table[s]) / (4 * TOL * P.jacobian_inverse_norm(newton_table[s], case.bt, case.ei, case.rx[s])))
                  for s in range(case.S))
    plan = case.plan
    print(f"sparse {mode} n 1100 m_p {plan.m} m_q {plan.m_q}: nnz(L) {plan.nnz_l}, longest column {plan.max_col}, {plan.madds} multiply-adds for both factors, "
          f"plan built in {plan.build_s * 1e3:.1f} ms, half-iterations {status.tolist()}, worst |mismatch| / bound {worst:.3g}, "
          f"|x - sparse Newton| / (4 tol ||J^-1||) {worst_x:.3g}")
    assert worst <= 1.0 and worst_x <= 1.0
    with pytest.raises(RuntimeError, match="sparse factorisation"):
        case.solve(mode, route="auto")


# ------------------------------------------------------------------------------------------------ degenerate types
@pytest.mark.parametrize("mode", ["fdxb", "fdbx"])
@pytest.mark.parametrize("kind", ["no_pq", "no_pv", "parallel", "lone_pq"])
def test_degenerate_grids(kind, mode):
    case = _case(14, 20, 4, kind=kind)
    table, status = _check_accuracy(case, mode, case.solve(mode))
    assert case.plan.m_q == int((case.bt == 2).sum())
    if kind == "no_pq":                                        # only P halves run, and the status counts them
        assert case.plan.m_q == 0 and np.array_equal(status, case.ref(mode)[1])
        assert np.array_equal(table[:, :, 0], case.spec[:, :, 0])


# ------------------------------------------------------------------------------------------------------ warm start
@pytest.mark.parametrize("mode", ["fdxb", "fdbx"])
def test_warm_starts(mode):
    case = _case(14, 20, 8, seed=3)
    flat = case.solve(mode)
    assert bool((flat.status >= 1).all())
    # a start already under tol: status 0; Vm and everything given return bit for bit, Va makes the trip degrees -> radians -> degrees
    # (x * RAD, then * (1 / RAD): three roundings of half an ulp each), so it returns within 4 * 2^-52 of itself
    again = case.solve(mode, init=flat.table)
    assert again.status.tolist() == [0] * 8 and bool((again.residual < TOL).all())
    got, want = again.table.cpu().numpy(), flat.table.cpu().numpy()
    assert np.array_equal(got[:, :, 0], want[:, :, 0])
    assert (np.abs(got[:, :, 1] - want[:, :, 1]) <= 4 * P.EPS64 * np.abs(want[:, :, 1])).all()
    _check_given(case, got)
    assert _residual_ratio(case, got) <= 1.0
    # a start 1e-3 away (Vm, and radians) costs no more half-iterations than the flat start
    noise = np.random.default_rng(5).normal(size=(8, 14, 2)) * np.array([1e-3, 1e-3 / P.RAD])
    near = case.solve(mode, init=_dev(want[:, :, :2] + noise))
    print(f"{mode}: half-iterations flat {flat.status.tolist()}, from 1e-3 away {near.status.tolist()}")
    assert bool((near.status >= 1).all()) and bool((near.status <= flat.status).all())
    assert _residual_ratio(case, near.table.cpu().numpy()) <= 1.0


# ------------------------------------------------------------------------------------------------------------ bits
def test_a_sample_depends_on_neither_its_batch_nor_the_workgroup_size_nor_who_built_the_plan():
    case = _case(14, 20, 8, seed=3)
    for mode in ("fdxb", "fdbx"):
        whole = case.solve(mode)
        assert bool((whole.status >= 1).all())
        for s in (0, 5):
            alone = case.solve(mode, rows=slice(s, s + 1))
            assert torch.equal(alone.table[0], whole.table[s]) and int(alone.status[0]) == int(whole.status[s])
            assert torch.equal(alone.residual[0], whole.residual[s])
        narrow, wide = case.solve(mode, threads=64), case.solve(mode, threads=256)
        for other in (narrow, wide):
            assert torch.equal(other.table, whole.table) and torch.equal(other.status, whole.status) and torch.equal(other.residual, whole.residual)
        fresh = sparse_plan(_dev(case.bt), _dev(case.ei), mode)                 # "fdxb" / "fdbx" are spellings of "fd"
        assert fresh.mode == "fd" and torch.equal(fresh.blob, case.plan.blob) and (fresh.m, fresh.m_q) == (13, int((case.bt == 2).sum()))
        again = case.solve(mode, plan=fresh)
        assert torch.equal(again.table, whole.table) and torch.equal(again.status, whole.status)
    big = _case(118, 186, 4)                                                     # several elements per thread at 64, idle lanes at 256
    narrow, wide = big.solve("fdxb", threads=64), big.solve("fdxb", threads=256)
    assert bool((narrow.status >= 1).all()) and torch.equal(narrow.table, wide.table) and torch.equal(narrow.status, wide.status)


def test_the_plan_report_fields():
    case = _case(118, 186, 4)
    plan, dc = case.plan, sparse_plan(_dev(case.bt), _dev(case.ei), "dc")
    assert (plan.mode, plan.n, plan.e, plan.m, plan.m_q) == ("fd", 118, 186, 117, int((case.bt == 2).sum())) and dc.m_q == 0
    (m_p, nnz_p, nnz_l_p, madds_p, col_p), (m_q, nnz_q, nnz_l_q, madds_q, col_q) = plan.halves
    assert (m_p, nnz_p, nnz_l_p, madds_p, col_p) == (dc.m, dc.nnz, dc.nnz_l, dc.madds, dc.max_col) and m_q == plan.m_q
    assert (plan.nnz, plan.nnz_l, plan.madds, plan.max_col) == (nnz_p + nnz_q, nnz_l_p + nnz_l_q, madds_p + madds_q, max(col_p, col_q))
    assert plan.bytes == plan.blob.numel() == int(plan.header[13])


# -------------------------------------------------------------------------------------------------------- failures
def test_failures_stay_local():
    n, e = 14, 20
    good, heavy = _case(n, e, 6, seed=4), _case(n, e, 6, seed=4, load=2.0)      # tests/test_gpu_powerflow_sparse.py's recipe: ten times the load
    spec, rx = good.spec.copy(), good.rx.copy()
    spec[5], rx[5] = heavy.spec[5], heavy.rx[5]
    start = np.stack([np.where(good.bt == 2, 1.0, good.spec[:, :, 0]), np.broadcast_to(good.spec[:, good.bt == 0, 1], (6, n))], axis=2)
    wild = start.copy()
    wild[2, np.flatnonzero(good.bt == 2)[0], 1] = np.inf              # (a bus whose start IS read)
    bt, ei = _dev(good.bt), _dev(good.ei)
    for mode in ("fdxb", "fdbx"):
        clean = good.solve(mode, init=_dev(start))
        assert bool((clean.status >= 1).all()) and torch.equal(clean.table, good.solve(mode).table)     # that start IS the flat start
        res = solve_power_flow(bt, _dev(spec), ei, _dev(rx), mode=mode, tol=TOL, max_iter=MAX_ITER, route="sparse", plan=good.plan, init=_dev(wild))
        status = res.status.tolist()
        print(f"{mode}: statuses {status}")
        assert status[5] in (-1, -3) and status[2] == -3 and int(res.flags.item()) == 0
        assert res.iterations.tolist() == [s if s >= 0 else -1 for s in status]
        assert torch.isnan(res.table[5]).all() and torch.isnan(res.table[2]).all()
        keep = [0, 1, 3, 4]
        assert torch.equal(res.table[keep], clean.table[keep]) and torch.equal(res.status[keep], clean.status[keep])
        assert torch.equal(res.residual[keep], clean.residual[keep])
    # a plan for other lines of the same size: the kernel notices, nothing is followed
    other = good.ei.copy()
    other[:, [0, 1]] = other[:, [1, 0]]
    stale = solve_power_flow(bt, _dev(good.spec), _dev(other), _dev(good.rx), mode="fdxb", tol=TOL, max_iter=MAX_ITER, route="sparse", plan=good.plan)
    assert stale.status.tolist() == [-6] * 6 and torch.isnan(stale.table).all() and int(stale.flags.item()) == 0
    # changed bus types, each way round: a PQ bus made PV (the plan holds a B'' unknown that is none), a PV bus made PQ
    for old, new in ((2, 1), (1, 2)):
        types = good.bt.copy()
        types[np.flatnonzero(good.bt == old)[0]] = new
        odd = solve_power_flow(_dev(types), _dev(good.spec), ei, _dev(good.rx), mode="fdbx", tol=TOL, max_iter=MAX_ITER, route="sparse", plan=good.plan)
        assert odd.status.tolist() == [-5] * 6 and torch.isnan(odd.table).all() and int(odd.flags.item()) & 1
    # a PQ bus without a line: a zero pivot in both matrices, as on the dense route
    assert good.bt[13] == 2
    alone = np.where(good.ei == 13, 1, good.ei)
    res = solve_power_flow(bt, _dev(good.spec), _dev(alone), _dev(good.rx), mode="fdxb", tol=TOL, max_iter=MAX_ITER, route="sparse",
                           plan=sparse_plan(bt, _dev(alone), "fd"))
    assert res.status.tolist() == [-2] * 6 and torch.isnan(res.table).all()


# ------------------------------------------------------------------------------------------------------ what raises
def test_what_raises():
    case = _case(14, 20, 8, seed=3)
    ac, dc = sparse_plan(_dev(case.bt), _dev(case.ei), "ac"), sparse_plan(_dev(case.bt), _dev(case.ei), "dc")
    for mode in ("fdxb", "fdbx"):
        with pytest.raises(ValueError, match=r"pass plan=sparse_plan\(bus_type, edge_index, 'fd'\).*dense only"):
            case.solve(mode, plan=None)
        for plan in (ac, dc, _case(5, 6, 3).plan):
            with pytest.raises(RuntimeError, match="the plan is for"):
                case.solve(mode, plan=plan)
    for mode in ("ac", "dc"):
        with pytest.raises(RuntimeError, match="the plan is for"):
            case.solve(mode, plan=case.plan)
    with pytest.raises(RuntimeError, match="one topology"):
        solve_power_flow(_dev(case.bt), _dev(case.spec), _dev(np.stack([case.ei] * 8)), _dev(case.rx), mode="fdxb", route="sparse", plan=case.plan)
    with pytest.raises(ValueError, match="route='sparse' only"):
        case.solve("fdxb", route="auto", plan=case.plan)
    with pytest.raises(ValueError, match="mode must be"):
        sparse_plan(_dev(case.bt), _dev(case.ei), "gs")
    # the library's own refusals: the Newton launcher does not take the fd header, the fd launcher no ac header and no mode 0
    lib, h = L.load(), case.plan.header
    import ctypes as C
    table = torch.zeros(8, 14, 4, dtype=torch.float64, device=DEV)
    status, residual, flags = torch.zeros(8, dtype=torch.int32, device=DEV), torch.zeros(8, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    bt, spec, ei, rx = _dev(case.bt.astype(np.int32)), _dev(case.spec), _dev(case.ei), _dev(case.rx)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)

    def call(fn, header, blob, mode):
        return fn(ei.data_ptr(), 20, rx.data_ptr(), bt.data_ptr(), spec.data_ptr(), None, 8, 14, mode, TOL, MAX_ITER, C.addressof(header),
                  blob.data_ptr(), 0, table.data_ptr(), status.data_ptr(), residual.data_ptr(), flags.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_ptr())
    assert call(lib.pfn_powerflow_solve_sparse, h, case.plan.blob, 0) == -1 and b"not a sparse power-flow plan" in lib.pfn_last_error()
    assert call(lib.pfn_powerflow_solve_sparse_fd, ac.header, ac.blob, 2) == -1 and b"not a fast-decoupled" in lib.pfn_last_error()
    assert call(lib.pfn_powerflow_solve_sparse_fd, h, case.plan.blob, 0) == -1 and b"mode must be 2" in lib.pfn_last_error()
    torch.cuda.synchronize()
    assert not table.any() and not status.any()


# --------------------------------------------------------------------------------------------------------- capture
def test_a_solve_is_capturable():
    """No sync, no allocation inside the launch: a hipGraph holding it -- ONE kernel node, so a single branch -- replays the same solve
    into the same tensors, bit for bit."""
    import ctypes as C
    case = _case(14, 20, 8)
    want = case.solve("fdxb")                                  # eager (and the LDS limit of the kernel is raised before the capture)
    assert bool((want.status >= 1).all())
    lib, plan = L.load(), case.plan
    table = torch.zeros(8, 14, 4, dtype=torch.float64, device=DEV)
    status, residual, flags = torch.zeros(8, dtype=torch.int32, device=DEV), torch.zeros(8, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    bt, spec, ei, rx = _dev(case.bt.astype(np.int32)), _dev(case.spec), _dev(case.ei), _dev(case.rx)
    need = int(lib.pfn_powerflow_sparse_fd_workspace_bytes(8, C.addressof(plan.header)))
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            rc = lib.pfn_powerflow_solve_sparse_fd(ei.data_ptr(), 20, rx.data_ptr(), bt.data_ptr(), spec.data_ptr(), None, 8, 14, 2, TOL, MAX_ITER,
                                                   C.addressof(plan.header), plan.blob.data_ptr(), 0, table.data_ptr(), status.data_ptr(),
                                                   residual.data_ptr(), flags.data_ptr(), ws.data_ptr(), need, L.stream_ptr())
    assert rc == 0
    for _ in range(2):
        table.fill_(-7.0)
        status.fill_(99)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(table, want.table) and torch.equal(status, want.status) and torch.equal(residual, want.residual)
    assert int(flags.item()) == 0


# --------------------------------------------------------------------------------------------------- workload size
WORKLOAD_TOL, WORKLOAD_YARDSTICK_COUNT = 1e-8, 43


def test_one_sample_of_the_workload_size():
    """(6470, 9005), fdxb, tol 1e-8.  The float64 yardstick (B' and B'' inverted once on the host, mat-vecs after that) takes
    WORKLOAD_YARDSTICK_COUNT half-iterations on this grid; max_iter is that count plus a quarter."""
    case = _case(6470, 9005, 1)
    plan = case.plan
    assert (plan.m, plan.m_q) == (6469, int((case.bt == 2).sum()))
    max_iter = WORKLOAD_YARDSTICK_COUNT + WORKLOAD_YARDSTICK_COUNT // 4
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = case.solve("fdxb", tol=WORKLOAD_TOL, max_iter=max_iter)
    status = res.status.tolist()
    seconds = time.perf_counter() - t0
    table = res.table.cpu().numpy()
    worst = _residual_ratio(case, table, WORKLOAD_TOL)
    print(f"sparse fdxb n 6470 m_p {plan.m} m_q {plan.m_q}: nnz(L) {plan.nnz_l}, longest column {plan.max_col}, {plan.madds / 1e6:.1f} M multiply-adds "
          f"for both factors, plan {plan.bytes / 1e6:.2f} MB built in {plan.build_s:.3f} s, {status[0]} half-iterations (yardstick "
          f"{WORKLOAD_YARDSTICK_COUNT}, max_iter {max_iter}) in {seconds:.3f} s, worst |mismatch| / bound {worst:.3g}")
    assert 1 <= status[0] <= max_iter and worst <= 1.0
    _check_given(case, table)


# ------------------------------------------------------------------------------------------------------ end to end
def test_speedup_evaluator_on_the_sparse_route(tmp_path):
    import dataset_generator
    import speedup_evaluator
    root = str(tmp_path / "solved")
    _run(dataset_generator.main, ["--case", "14", "--samples", "32", "--root", root])
    torch.manual_seed(0)
    text = _run(speedup_evaluator.main, ["--case", "14", "--data-dir", root, "--split", "0.5", "0.25", "0.25", "--hidden_dim", "32",
                                        "--n_gnn_layers", "3", "--K", "2", "--route", "sparse"])
    print(text)
    assert "n/a" not in text and "Number of samples: 8" in text and "Solved on the sparse route" in text
    value = {}
    for name in ("nr", "fdxb", "fdbx", "nr_result_init", "fdxb_result_init", "fdbx_result_init", "dc"):
        sec = re.search(rf"^{name}: (\S+)$", text, flags=re.M)
        row = re.search(rf"^{name} solves: mean (\S+) max (\S+) failures (\d+)$", text, flags=re.M)
        assert sec and row, name
        value[name] = (float(sec.group(1)), float(row.group(1)), int(row.group(2)), int(row.group(3)))
    for name in ("nr", "fdxb", "fdbx", "dc"):                               # flat starts on a solved set: finite, no failure
        sec, mean, most, failed = value[name]
        assert 0 < sec < 1 and np.isfinite(mean) and 1 <= mean <= most and failed == 0, (name, value[name])
    for name in ("nr_result_init", "fdxb_result_init", "fdbx_result_init"):  # a random model's start: finite figures, failures counted
        sec, mean, most, failed = value[name]
        assert 0 < sec < 1 and np.isfinite(mean) and 0 <= mean <= most and 0 <= failed < 8, (name, value[name])
