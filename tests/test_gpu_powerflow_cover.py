"""Per-sample topologies on the sparse power-flow routes, on the device: `pfn_powerflow_cover_map` (csrc/powerflow_cover.hip) and the
masked solves `pfn_powerflow_solve_sparse_masked` / `_fd_masked` through `solve_power_flow(edge_index [S, 2, e], route="sparse",
plan=cover_plan(...))`, with tol = 1e-10.  The map is held to the slot rule of tests/powerflow_cover_ref.py exactly; a null mask and
a mask of ones to the one-topology route bit for bit; the solves -- with NaN in every rx slot a sample does not use -- to the bounds
of tests/test_gpu_powerflow_sparse.py and tests/test_gpu_powerflow_sparse_fd.py as tests/powerflow_checks.py states them, each sample
on its OWN line list:
  residual   the yardstick's mismatch of the WRITTEN table, at all buses, <= tol + 64 * 2^-52 * scale_i;
  solution   Vm and Va (radians) within 2 tol ||J^-1||_inf of the float64 yardstick's solution and of the dense route's table on the
             same per-sample lists; fast-decoupled: the half-iteration count within +-1 of the float32 interpreter's on the sample's
             own plan
-- at (14, 20, 8) R = A = 1 and (118, 186, 4) R = A = 2, at (1100, 1530, 2) which the dense route refuses; a sample's independence
of its batch and of the workgroup size; a line the cover lacks (-6) and a bus a mask islands (-2) fail their sample alone; and
dataset_generator.py -r 1 -a 1 --route sparse end to end.  DESIGN.md section 7p."""
import functools

import numpy as np
import pytest
import torch

from poweflownet_amd.synth import make_physical_inputs
from poweflownet_amd.utils import powerflow as PF
from poweflownet_amd.utils.powerflow import cover_map, cover_plan, max_unknowns, solve_power_flow, sparse_plan
from poweflownet_amd.utils.topology import unsupplied_buses
from tests import powerflow_cover_ref as CR
from tests import powerflow_fd_ref as FD
from tests import powerflow_ref as P
from tests import powerflow_sparse_fd_ref as SF
from tests import topology_ref as T
from tests.powerflow_checks import DEV, TOL, _check_given, _dev, _distance, _residual_ratio, _run

pytestmark = pytest.mark.gpu
MAX_ITER, FD_ITER = 10, 60
VARIANT = {"fdxb": "xb", "fdbx": "bx"}


def _masked_entry(bt, spec, lines, rx, mask, unplaced, mode, iters, plan, threads=0):
    """`pfn_powerflow_solve_sparse_masked` / `_fd_masked` as the C ABI gives them: `lines` [2, e] the plan's list, `mask` uint8 [S, e]
    or None, `unplaced` int32 [S] or None, `plan` a one-topology `SparsePlan` (a cover plan's `.plan`)."""
    import ctypes as C
    from poweflownet_amd import _lib as L
    lib = L.load()
    fd = mode.startswith("fd")
    sizer, entry = ((lib.pfn_powerflow_sparse_fd_workspace_bytes, lib.pfn_powerflow_solve_sparse_fd_masked) if fd
                    else (lib.pfn_powerflow_sparse_workspace_bytes, lib.pfn_powerflow_solve_sparse_masked))
    S, n, e = int(spec.shape[0]), int(spec.shape[1]), int(lines.shape[1])
    assert tuple(rx.shape) == (S, e, 2) and (mask is None or (tuple(mask.shape) == (S, e) and mask.dtype == torch.uint8 and mask.is_contiguous()))
    need = int(sizer(S, C.addressof(plan.header)))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    bt32, spec, lines, rx = bt.to(torch.int32), spec.contiguous(), lines.contiguous(), rx.contiguous()
    out = PF.PowerFlowResult(torch.empty(S, n, 4, dtype=torch.float64, device=DEV), torch.empty(S, dtype=torch.int32, device=DEV), None,
                             torch.empty(S, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), "sparse")
    L.check(entry(lines.data_ptr(), e, rx.data_ptr(), L.ptr(mask), L.ptr(unplaced), bt32.data_ptr(), spec.data_ptr(), None, S, n, PF._MODES[mode],
                  TOL, iters, C.addressof(plan.header), plan.blob.data_ptr(), threads, out.table.data_ptr(), out.status.data_ptr(),
                  out.residual.data_ptr(), out.flags.data_ptr(), ws.data_ptr(), need, L.stream_ptr()), "masked entry")
    torch.cuda.synchronize()
    out.iterations = torch.where(out.status >= 0, out.status, torch.full_like(out.status, -1))
    return out


class _One:
    """sample s of a perturbed case as the `case` tests/powerflow_checks.py takes: its own line list"""

    def __init__(self, case, s):
        self.ei, self.bt, self.rx, self.spec = case.lists[s], case.bt, case.rx[s:s + 1], case.spec[s:s + 1]


class _Case:
    """A base grid with S perturbed samples (R lines removed, A added per sample, an added line with the parameters of the base
    line it copies: the dataset generator's recipe) on the host; yardsticks and plans computed once, where a test asks."""

    def __init__(self, n, e, S, r, a, seed=1):
        ei, bt, rx, spec = make_physical_inputs(n, e, S, seed)
        self.n, self.e, self.S = n, e, S
        self.ei, self.bt, self.spec = ei.numpy(), bt.numpy().copy(), spec.numpy().copy()
        self.lists, source, status = T.perturb(self.ei, n, S, remove=r, add=a, seed=seed)
        assert (status >= 1).all()
        self.rx = np.take_along_axis(rx.numpy(), source.astype(np.int64)[:, :, None], 1)
        self.m = (n - 1) + int((self.bt == 2).sum())

    def one(self, s):
        return _One(self, s)

    @functools.cached_property
    def ref(self):
        out = [P.newton(self.bt, self.spec[s], self.lists[s], self.rx[s], tol=TOL, max_iter=MAX_ITER) for s in range(self.S)]
        assert all(1 <= st <= MAX_ITER for _, st, _ in out), [st for _, st, _ in out]
        return np.stack([t for t, _, _ in out])

    @functools.cached_property
    def inv_norm(self):
        return np.array([P.jacobian_inverse_norm(self.ref[s], self.bt, self.lists[s], self.rx[s]) for s in range(self.S)])

    @functools.lru_cache(maxsize=None)
    def cover(self, mode="ac"):
        return cover_plan(_dev(self.bt), _dev(self.lists), mode, _dev(self.ei))

    def solve(self, mode="ac", rows=slice(None), threads=0, fill=float("nan"), lists=None, plan=None):
        """the cover route, its two launches made here so that every rx slot a sample does not use holds `fill` (NaN); fill None:
        `solve_power_flow` itself (the default workgroup size)"""
        iters = FD_ITER if mode.startswith("fd") else MAX_ITER
        plan = plan or self.cover("fd" if mode.startswith("fd") else mode)
        lists = self.lists if lists is None else lists
        if fill is None:
            assert threads == 0
            return solve_power_flow(_dev(self.bt), _dev(self.spec[rows]), _dev(lists[rows]), _dev(self.rx[rows]), mode=mode, tol=TOL, max_iter=iters,
                                    route="sparse", plan=plan)
        mask, rx_cover, unplaced = cover_map(plan, _dev(lists[rows]), _dev(self.rx[rows]), fill=fill)
        return _masked_entry(_dev(self.bt), _dev(self.spec[rows]), plan.cover, rx_cover, mask, unplaced, mode, iters, plan.plan, threads)

    def residual_ratio(self, table):
        return max(_residual_ratio(self.one(s), table[s:s + 1]) for s in range(table.shape[0]))


@functools.lru_cache(maxsize=None)
def _case(n, e, S, r, a, seed=1):
    return _Case(n, e, S, r, a, seed)


def _same(a, b, rows=slice(None)):
    return (torch.equal(a.table[rows].view(torch.int64), b.table[rows].view(torch.int64)) and torch.equal(a.status[rows], b.status[rows])
            and torch.equal(a.residual[rows].view(torch.int64), b.residual[rows].view(torch.int64)))


# ---------------------------------------------------------- 1. a null mask, a mask of ones and the one-topology route
@pytest.mark.parametrize("mode", ["ac", "dc", "fdxb"])
@pytest.mark.parametrize("n,e,S", [(14, 20, 4), (118, 186, 2)])
def test_a_mask_of_ones_and_a_null_mask_are_the_one_topology_route_bit_for_bit(n, e, S, mode):
    ei, bt, rx, spec = make_physical_inputs(n, e, S, 1)
    d_bt, d_spec, d_ei, d_rx = (t.to(DEV) for t in (bt, spec, ei, rx))
    fd = mode.startswith("fd")
    iters = FD_ITER if fd else MAX_ITER
    plan = sparse_plan(d_bt, d_ei, "fd" if fd else mode)
    today = solve_power_flow(d_bt, d_spec, d_ei, d_rx, mode=mode, tol=TOL, max_iter=iters, route="sparse", plan=plan)
    assert bool((today.status >= 1).all())
    ones = torch.ones(S, e, dtype=torch.uint8, device=DEV)
    masked = _masked_entry(d_bt, d_spec, d_ei, d_rx, ones, None, mode, iters, plan)
    assert _same(masked, today) and int(masked.flags.item()) == 0
    placed = torch.zeros(S, dtype=torch.int32, device=DEV)
    assert _same(_masked_entry(d_bt, d_spec, d_ei, d_rx, ones, placed, mode, iters, plan), today)
    null = _masked_entry(d_bt, d_spec, d_ei, d_rx, None, None, mode, iters, plan)          # null, null: the unmasked entry itself
    assert _same(null, today)


# ------------------------------------------------------------------------------- 2. the map kernel and the slot rule
def _check_map(plan, lists, rx, n):
    mask, rxc, unplaced = cover_map(plan, _dev(lists), _dev(rx), fill=float("nan"))
    want_mask, want_rx, want_unplaced = CR.cover_map(lists, rx, plan.cover.cpu().numpy(), n)
    assert mask.dtype == torch.uint8 and rxc.dtype == torch.float64 and unplaced.dtype == torch.int32
    assert np.array_equal(mask.cpu().numpy(), want_mask) and np.array_equal(unplaced.cpu().numpy(), want_unplaced)
    assert np.array_equal(rxc.cpu().numpy().view(np.int64)[want_mask == 1], want_rx.view(np.int64)[want_mask == 1])
    assert torch.isnan(rxc[mask == 0]).all()                                    # a slot the sample does not use is not written
    again = cover_map(plan, _dev(lists), _dev(rx), fill=float("nan"))
    assert torch.equal(again[0], mask) and torch.equal(again[2], unplaced)
    return want_unplaced


def test_the_map_kernel_is_the_slot_rule_exactly():
    case = _case(14, 20, 8, 1, 1)
    assert case.cover().extras >= 1
    assert _check_map(case.cover(), case.lists, case.rx, 14).tolist() == [0] * 8
    # a plan without a base: every line an extra, the cover sorted by key
    assert _check_map(cover_plan(_dev(case.bt), _dev(case.lists), "ac"), case.lists, case.rx, 14).tolist() == [0] * 8
    # hand-made (5, 6): a doubled pair whose first copy is stored reversed, and a sample with a line the cover lacks
    n = 5
    base = np.array([[0, 1, 3, 2, 4, 1], [1, 2, 2, 4, 0, 3]])
    s0 = np.array([[2, 1, 3, 2, 4, 0], [1, 2, 2, 4, 0, 1]])
    s1 = base.copy()
    bt = np.array([0, 2, 2, 1, 2], dtype=np.int64)
    plan = cover_plan(_dev(bt), _dev(np.stack([s0, s1])), "ac", _dev(base))
    stranger = np.array([[0, 1, 3, 2, 4, 0], [1, 2, 2, 4, 0, 3]])
    outside = np.array([[0, 1, 3, 2, 4, 1], [1, 2, 2, 4, 0, 5]])               # bus 5 does not exist; checked before it indexes anything
    twice = np.array([[0, 1, 3, 2, 4, 3], [1, 2, 2, 4, 0, 3]])                 # one bus twice
    third = np.array([[1, 1, 1, 2, 4, 0], [2, 2, 2, 4, 0, 1]])                 # a third (1, 2) line: the cover holds two
    again = np.array([[0, 1, 3, 2, 4, 0], [1, 2, 2, 4, 0, 4]])                 # (0, 4) twice, the second reversed: the cover holds it ONCE
    thrice = np.array([[0, 1, 3, 4, 4, 0], [1, 2, 2, 0, 0, 4]])                # ... and three times
    lists = np.stack([s0, s1, stranger, outside, twice, third, again, thrice])
    rx = np.random.default_rng(3).uniform(0.01, 0.2, (8, 6, 2))
    assert CR.slots(again, plan.cover.cpu().numpy(), n).tolist() == [0, 1, 2, 3, 4, -1]
    assert CR.slots(thrice, plan.cover.cpu().numpy(), n).tolist() == [0, 1, 2, 4, -1, -1]
    for _ in range(3):                                                          # the FIRST copy keeps the place on every run
        assert _check_map(plan, lists, rx, n).tolist() == [0, 0, 1, 1, 1, 1, 1, 2]
    # the cover is the base alone and the sample holds (1, 2) twice
    plain = cover_plan(_dev(bt), _dev(base[None]), "ac", _dev(base))
    doubled = np.array([[0, 1, 2, 2, 4, 1], [1, 2, 1, 4, 0, 3]])
    assert CR.slots(doubled, base, n).tolist() == [0, 1, -1, 3, 4, 5]
    assert _check_map(plan=plain, lists=doubled[None], rx=rx[:1], n=n).tolist() == [1]


def test_a_line_the_cover_lacks_fails_its_sample_alone():
    case = _case(14, 20, 8, 1, 1)
    clean = case.solve()
    assert bool((clean.status >= 1).all())
    lists = case.lists.copy()
    have = {CR.key(a, b) for a, b in case.cover().cover.cpu().numpy().T}
    a, b = next((a, b) for a in range(14) for b in range(a + 1, 14) if (a, b) not in have)
    lists[2, :, 0] = (b, a)
    res = case.solve(lists=lists)
    assert res.status.tolist()[2] == -6 and torch.isnan(res.table[2]).all() and int(res.flags.item()) == 0
    keep = [0, 1, 3, 4, 5, 6, 7]
    assert _same(res, clean, keep)


def test_a_key_the_sample_holds_more_often_than_the_cover_fails_its_sample_alone():
    """the cover holds the pair once, sample 4 holds it twice: its second copy is unplaced, -6, whichever write landed last"""
    case = _case(14, 20, 8, 1, 1)
    clean = case.solve()
    lists = case.lists.copy()
    lists[4, :, 7] = lists[4, ::-1, 2]                                          # line 7 becomes line 2's pair, reversed
    q = CR.key(*lists[4, :, 2])
    assert sum(CR.key(a, b) == q for a, b in case.cover().cover.cpu().numpy().T) == 1
    mask, _, unplaced = cover_map(case.cover(), _dev(lists), _dev(case.rx), fill=float("nan"))
    assert unplaced.tolist() == [0, 0, 0, 0, 1, 0, 0, 0] and int(mask[4].sum()) == 19
    for mode in ("ac", "fdxb"):
        res, ref = case.solve(mode, lists=lists), (clean if mode == "ac" else case.solve(mode))
        assert res.status.tolist()[4] == -6 and torch.isnan(res.table[4]).all() and int(res.flags.item()) == 0
        assert _same(res, ref, [0, 1, 2, 3, 5, 6, 7])
    public = solve_power_flow(_dev(case.bt), _dev(case.spec), _dev(lists), _dev(case.rx), tol=TOL, max_iter=MAX_ITER, route="sparse", plan=case.cover())
    assert public.status.tolist()[4] == -6 and _same(public, clean, [0, 1, 2, 3, 5, 6, 7])


# ---------------------------------------------------------------- 3. NaN in the unused slots; accuracy on the own list
@pytest.mark.parametrize("n,e,S,ra", [(14, 20, 8, 1), (118, 186, 4, 2)])
def test_newton_with_nan_in_every_unused_slot_meets_the_one_topology_bounds(n, e, S, ra):
    case = _case(n, e, S, ra, ra)
    res = case.solve()
    table, status = res.table.cpu().numpy(), res.status.cpu().numpy()
    assert res.route == "sparse" and table.shape == (S, n, 4) and int(res.flags.item()) == 0
    assert ((status >= 1) & (status <= MAX_ITER)).all(), status
    assert np.isfinite(table).all() and torch.equal(res.iterations, res.status) and bool((res.residual < TOL).all())
    dense = solve_power_flow(_dev(case.bt), _dev(case.spec), _dev(case.lists), _dev(case.rx), tol=TOL, max_iter=MAX_ITER, route="global")
    assert dense.route == "global" and bool((dense.status >= 1).all())
    dense_table = dense.table.cpu().numpy()
    worst_f = case.residual_ratio(table)
    worst_x = max(float(_distance(table[s], case.ref[s]) / (2 * TOL * case.inv_norm[s])) for s in range(S))
    worst_d = max(float(_distance(table[s], dense_table[s]) / (2 * TOL * case.inv_norm[s])) for s in range(S))
    for s in range(S):
        _check_given(case.one(s), table[s:s + 1])
    cover = case.cover()
    print(f"cover ac n {n} e {e} S {S} R = A = {ra}: {cover.extras} extra lines, nnz(L) {cover.plan.nnz_l}, solves {status.tolist()}, "
          f"worst |mismatch| / bound {worst_f:.3g}, |x - yardstick| / (2 tol ||J^-1||) {worst_x:.3g}, |x - dense route| / same {worst_d:.3g}")
    assert worst_f <= 1.0 and worst_x <= 1.0 and worst_d <= 1.0


@pytest.mark.parametrize("n,e,S,ra", [(14, 20, 8, 1), (118, 186, 4, 2)])
def test_dc_with_nan_in_every_unused_slot(n, e, S, ra):
    case = _case(n, e, S, ra, ra)
    res = case.solve("dc")
    table, status = res.table.cpu().numpy(), res.status.cpu().numpy()
    assert ((status >= 1) & (status <= MAX_ITER)).all() and int(res.flags.item()) == 0 and res.route == "sparse"
    dense = solve_power_flow(_dev(case.bt), _dev(case.spec), _dev(case.lists), _dev(case.rx), mode="dc", tol=TOL, max_iter=MAX_ITER, route="global")
    dense_table = dense.table.cpu().numpy()
    worst_f = worst_x = worst_d = 0.0
    for s in range(S):
        F = P.dc_mismatch(table[s], case.lists[s], case.rx[s], case.bt)
        worst_f = max(worst_f, float((np.abs(F) / (TOL + 64 * P.EPS64 * P.dc_scale(table[s], case.lists[s], case.rx[s]))).max()))
        assert np.isnan(table[s, :, 3]).all() and np.isfinite(table[s, :, :3]).all()
        want, inv_norm = P.dc_solve(case.bt, case.spec[s], case.lists[s], case.rx[s])
        worst_x = max(worst_x, float(np.abs(table[s, :, 1] - want[:, 1]).max() * P.RAD / (2 * TOL * inv_norm)))
        worst_d = max(worst_d, float(np.abs(table[s, :, 1] - dense_table[s, :, 1]).max() * P.RAD / (2 * TOL * inv_norm)))
        others = case.bt != 0
        assert np.array_equal(table[s, :, 0], want[:, 0]) and np.array_equal(table[s, others, 2], want[others, 2])
    print(f"cover dc n {n} S {S}: solves {status.tolist()}, worst |mismatch| / bound {worst_f:.3g}, |theta - fp64 solve| / (2 tol ||B'^-1||) "
          f"{worst_x:.3g}, |theta - dense route| / same {worst_d:.3g}")
    assert worst_f <= 1.0 and worst_x <= 1.0 and worst_d <= 1.0


@pytest.mark.parametrize("mode", ["fdxb", "fdbx"])
def test_fast_decoupled_with_nan_in_every_unused_slot(mode):
    n, e, S = 118, 186, 4
    case = _case(n, e, S, 2, 2)
    res = case.solve(mode)
    table, status = res.table.cpu().numpy(), res.status.cpu().numpy()
    assert res.route == "sparse" and int(res.flags.item()) == 0 and ((status >= 1) & (status <= FD_ITER)).all(), status
    assert np.isfinite(table).all() and torch.equal(res.iterations, res.status) and bool((res.residual < TOL).all())
    dense = solve_power_flow(_dev(case.bt), _dev(case.spec), _dev(case.lists), _dev(case.rx), mode=mode, tol=TOL, max_iter=FD_ITER, route="global")
    assert bool((dense.status >= 1).all())
    dense_table = dense.table.cpu().numpy()
    worst_f, worst_x, worst_d, count32, count64 = case.residual_ratio(table), 0.0, 0.0, [], []
    for s in range(S):
        ref, st, _ = FD.fast_decoupled(case.bt, case.spec[s], case.lists[s], case.rx[s], VARIANT[mode], tol=TOL, max_iter=FD_ITER)
        assert 1 <= st <= FD_ITER
        count64.append(st)
        inv_norm = P.jacobian_inverse_norm(ref, case.bt, case.lists[s], case.rx[s])
        worst_x = max(worst_x, float(_distance(table[s], ref) / (2 * TOL * inv_norm)))
        worst_d = max(worst_d, float(_distance(table[s], dense_table[s]) / (2 * TOL * inv_norm)))
        rc, blob, text = SF.build_plan(case.bt, case.lists[s])
        assert rc == 0, text
        count32.append(SF.fast_decoupled(SF.Plan(blob), case.bt, case.spec[s], case.lists[s], case.rx[s], VARIANT[mode], tol=TOL, max_iter=FD_ITER,
                                         dtype=np.float32)[1])
        _check_given(case.one(s), table[s:s + 1])
    print(f"cover {mode} n {n} S {S}: half-iterations {status.tolist()} (float32 interpreter on the own plan {count32}, float64 yardstick "
          f"{count64}), worst |mismatch| / bound {worst_f:.3g}, |x - yardstick| / (2 tol ||J^-1||) {worst_x:.3g}, |x - dense route| / same {worst_d:.3g}")
    assert worst_f <= 1.0 and worst_x <= 1.0 and worst_d <= 1.0
    assert (np.abs(status - np.array(count32)) <= 1).all()


# --------------------------------------------------------------------------------------- 4. beyond the dense cap
def test_beyond_the_dense_cap():
    case = _case(1100, 1530, 2, 1, 1)
    assert case.m == 1832 > max_unknowns()
    res = case.solve()
    status, table = res.status.cpu().numpy(), res.table.cpu().numpy()
    assert ((status >= 0) & (status <= MAX_ITER)).all(), status
    worst = case.residual_ratio(table)
    cover = case.cover()
    print(f"cover ac n 1100 m {case.m}: {cover.extras} extra lines, nnz(L) {cover.plan.nnz_l}, {cover.plan.madds} multiply-adds per factor, "
          f"plan built in {cover.plan.build_s * 1e3:.1f} ms, solves {status.tolist()}, worst |mismatch| / bound {worst:.3g}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------- 5. independence
@pytest.mark.parametrize("mode", ["ac", "fdxb"])
def test_a_sample_depends_on_neither_its_batch_nor_the_workgroup_size(mode):
    case = _case(14, 20, 8, 1, 1)
    whole = case.solve(mode)
    assert bool((whole.status >= 1).all())
    alone = case.solve(mode, rows=slice(3, 4))                                  # the same cover plan, one sample
    assert torch.equal(alone.table[0].view(torch.int64), whole.table[3].view(torch.int64)) and alone.status[0] == whole.status[3]
    assert alone.residual[0].view(torch.int64) == whole.residual[3].view(torch.int64)
    narrow, wide = case.solve(mode, threads=64), case.solve(mode, threads=256)
    assert _same(narrow, whole) and _same(wide, whole)
    assert _same(case.solve(mode, fill=None), whole)                            # what an unused slot holds reaches nothing


# ------------------------------------------------------------------------------------------------ 6. islanding
@pytest.mark.parametrize("mode", ["ac", "dc", "fdxb"])
def test_a_mask_that_islands_a_bus_fails_its_sample_alone(mode):
    case = _case(14, 20, 8, 1, 1)
    clean = case.solve(mode)
    assert bool((clean.status >= 1).all())
    # sample 5 loses every line of a non-slack bus: its other lines and the cover stay as they are
    bus = next(i for i in range(13, 0, -1) if case.bt[i] != 0)
    lists = case.lists.copy()
    cut = (lists[5] == bus).any(0)
    assert 1 <= int(cut.sum()) < 20
    spare = lists[5][:, ~cut][:, 0]
    assert bus not in spare
    lists[5][:, cut] = spare[:, None]                                           # in their place: copies of a line the sample has
    plan = cover_plan(_dev(case.bt), _dev(np.concatenate([case.lists, lists[5:6]])), "fd" if mode.startswith("fd") else mode, _dev(case.ei))
    before = case.solve(mode, plan=plan)
    res = case.solve(mode, lists=lists, plan=plan)
    status = res.status.tolist()
    assert status[5] < 0 and status[5] == -2 and torch.isnan(res.table[5]).all() and int(res.flags.item()) == 0
    keep = [0, 1, 2, 3, 4, 6, 7]
    assert bool((before.status >= 1).all()) and _same(res, before, keep)


# ------------------------------------------------------------------------------------------------ 7. generator
def test_generator_writes_a_balanced_perturbed_set_on_the_sparse_route(tmp_path):
    """fails without the cover route: `--route sparse` with -r / -a raised ValueError"""
    import dataset_generator
    from poweflownet_amd.datasets import PowerFlowData
    root = str(tmp_path / "perturbed")
    text = _run(dataset_generator.main, ["--case", "14", "--samples", "8", "-r", "1", "-a", "1", "--route", "sparse", "--root", root])
    assert "Solved on the sparse route" in text and "Cover plans:" in text and "Failed to converge and drawn again: 0" in text
    node = np.load(tmp_path / "perturbed" / "raw" / "case14perturbed1r1a_node_features.npy")
    edge = np.load(tmp_path / "perturbed" / "raw" / "case14perturbed1r1a_edge_features.npy")
    assert node.shape == (8, 14, 6) and edge.shape == (8, 20, 4) and np.isfinite(node).all() and np.isfinite(edge).all()
    ds = PowerFlowData(root=root, case="14perturbed1r1a", split=[.5, .25, .25], task="train", device=DEV)
    assert len(ds) == 4
    lists = edge[:, :, :2].astype(np.int64).transpose(0, 2, 1).copy()
    assert len({lists[s].tobytes() for s in range(8)}) > 1                      # the samples do have their own line lists
    assert unsupplied_buses(_dev(lists), 14).tolist() == [0] * 8
    bt = node[0, :, 1].astype(np.int64)

    class _Row:
        pass
    worst = 0.0
    for s in range(8):
        row = _Row()
        row.ei, row.bt, row.rx, row.spec = lists[s], bt, edge[s:s + 1, :, 2:], node[s:s + 1, :, 2:]
        worst = max(worst, _residual_ratio(row, node[s:s + 1, :, 2:], tol=1e-8))
    print(f"perturbed set generated on the sparse route: worst |mismatch| / bound {worst:.3g}")
    assert worst <= 1.0
