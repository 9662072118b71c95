"""The host half of the cover route (per-sample topologies on the sparse power-flow route), no GPU: `cover_list` / `cover_plan`
(poweflownet_amd/utils/powerflow.py) against the dictionary restatement of tests/powerflow_cover_ref.py -- base first, the
multiplicity rule, the extras ascending and oriented (min, max) --, the table the map kernel searches against the slot rule,
closure -- every sample's Jacobian block pattern lies inside the cover plan's filled pattern, which is why one plan serves the
chunk --, the chunker's policy, and the refusals that are decided before anything touches a device.  DESIGN.md section 7p."""
import ctypes as C

import numpy as np
import pytest
import torch

from poweflownet_amd.synth import make_physical_inputs
from poweflownet_amd.utils import powerflow as PF
from poweflownet_amd.utils.powerflow import CoverChunker, cover_list, cover_plan, solve_power_flow, sparse_plan
from tests import powerflow_cover_ref as CR
from tests import powerflow_sparse_ref as SP
from tests import topology_ref as T


def _grid(n, e, seed=1):
    ei, bt, _, _ = make_physical_inputs(n, e, 0, seed)
    return ei.numpy(), bt.numpy()


def _perturbed(n, e, S, r, a, seed=5):
    ei, bt = _grid(n, e)
    lists, _, status = T.perturb(ei, n, S, remove=r, add=a, seed=seed)
    assert (status >= 1).all()
    return ei, bt, lists


def _table_slots(plan, sample, last_claim_wins=True):
    """the device lookup in numpy, shortcut and all: a binary search of the line's key in the sorted key table; the line's rank among
    the sample's earlier lines of that key is counted only where the NEXT table entry holds the key too, else taken as 0; every line
    claims its place, a place that two lines claimed is marked -- whichever claim landed last -- and the lines of a marked place
    count their rank after all"""
    keys, slot, n = plan.keys.numpy(), plan.slot.numpy(), plan.n

    def key(j):
        a, b = sample[:, j]
        return -1 if not (0 <= a < n and 0 <= b < n) or a == b else min(a, b) * n + max(a, b)

    def place(j, counted):
        q = key(j)
        if q < 0:
            return -1
        lo = int(np.searchsorted(keys, q, side="left"))
        if lo >= len(keys) or keys[lo] != q:
            return -1
        rank = 0
        if counted or (lo + 1 < len(keys) and keys[lo + 1] == q):
            rank = sum(1 for i in range(j) if key(i) == q)
        return int(slot[lo + rank]) if lo + rank < len(keys) and keys[lo + rank] == q else -1
    e = sample.shape[1]
    claim = {}
    for j in (range(e) if last_claim_wins else reversed(range(e))):
        if place(j, False) >= 0:
            claim[place(j, False)] = j
    marked = {place(j, False) for j in range(e) if place(j, False) >= 0 and claim[place(j, False)] != j}
    return np.array([place(j, place(j, False) in marked) for j in range(e)])


# ------------------------------------------------------------------------------------------------ the cover list
def test_hand_made_cover_base_first_multiplicity_orientation_and_order():
    n = 5
    base = np.array([[0, 1, 3, 2, 4, 1], [1, 2, 2, 4, 0, 3]])               # (3, 2) and (4, 0) stored high-to-low: they stay so
    s0 = np.array([[0, 1, 3, 2, 4, 2], [1, 2, 2, 4, 0, 1]])                 # (1, 3) left, a second (1, 2) came, reversed
    s1 = np.array([[0, 1, 3, 2, 4, 4], [1, 2, 2, 4, 0, 3]])                 # (1, 3) left, (3, 4) came as (4, 3)
    s2 = np.array([[1, 1, 3, 2, 4, 1], [0, 2, 2, 4, 0, 3]])                 # the base, its first line reversed
    got = cover_list(np.stack([s0, s1, s2]), n, base)
    assert np.array_equal(got[:, :6], base)
    assert got[:, 6:].tolist() == [[1, 3], [2, 4]]                          # (1, 2) before (3, 4), each (min, max), each once
    assert np.array_equal(got, CR.cover([s0, s1, s2], base))
    # two parallel lines in one sample need two cover lines; one each in two samples need one
    twice = np.array([[0, 1, 3, 2, 2, 1], [1, 2, 2, 4, 1, 3]])
    assert cover_list(np.stack([twice]), n, base)[:, 6:].tolist() == [[1], [2]]
    assert cover_list(np.stack([s0, s0]), n, base).shape[1] == 7
    # a base line no sample uses stays; without a base the cover is the sorted union
    assert np.array_equal(cover_list(np.stack([s0]), n, base)[:, :6], base)
    assert cover_list(np.stack([s0, s1]), n).tolist() == [[0, 0, 1, 1, 2, 2, 3], [1, 4, 2, 2, 3, 4, 4]]
    assert np.array_equal(cover_list(np.stack([s0, s1]), n), CR.cover([s0, s1]))


@pytest.mark.parametrize("n,e,S,r,a", [(14, 20, 8, 1, 1), (14, 20, 8, 2, 2), (118, 186, 6, 1, 1), (118, 186, 6, 2, 2), (14, 20, 16, 0, 3)])
def test_cover_of_perturbed_sets_against_the_restatement(n, e, S, r, a):
    ei, bt, lists = _perturbed(n, e, S, r, a)
    for base in (ei, None):
        got = cover_list(lists, n, base)
        assert np.array_equal(got, CR.cover(lists, base))
        plan = cover_plan(torch.from_numpy(bt), torch.from_numpy(lists), "ac", None if base is None else torch.from_numpy(base))
        assert np.array_equal(plan.cover.numpy(), got) and plan.e_cover == got.shape[1] and plan.e_base == (e if base is not None else 0)
        assert (plan.plan.n, plan.plan.e, plan.plan.mode, plan.n, plan.mode) == (n, plan.e_cover, "ac", n, "ac")
        keys = plan.keys.numpy()
        assert (np.diff(keys) >= 0).all() and sorted(plan.slot.tolist()) == list(range(plan.e_cover))
        for s in range(S):
            want = CR.slots(lists[s], got, n)
            assert (want >= 0).all() and len(set(want.tolist())) == len(want)        # every line placed, no slot twice
            assert np.array_equal(_table_slots(plan, lists[s]), want)


def test_slot_rule_with_parallel_lines_and_a_line_the_cover_lacks():
    n = 5
    base = np.array([[0, 1, 3, 2, 4, 1], [1, 2, 2, 4, 0, 3]])
    s0 = np.array([[2, 1, 3, 2, 4, 0], [1, 2, 2, 4, 0, 1]])                 # two (1, 2) lines, the first reversed, and (0, 1) last
    s1 = np.array([[0, 1, 3, 2, 4, 1], [1, 2, 2, 4, 0, 3]])
    bt = np.array([0, 2, 2, 1, 2], dtype=np.int64)
    plan = cover_plan(torch.from_numpy(bt), torch.from_numpy(np.stack([s0, s1])), "ac", torch.from_numpy(base))
    assert plan.cover.numpy()[:, 6:].tolist() == [[1], [2]]
    # the sample's FIRST (1, 2) line, stored reversed, takes the base's line 1; its second the extra line 6
    assert CR.slots(s0, plan.cover.numpy(), n).tolist() == [1, 6, 2, 3, 4, 0]
    assert _table_slots(plan, s0).tolist() == [1, 6, 2, 3, 4, 0]
    stranger = np.array([[0, 1, 3, 2, 4, 0], [1, 2, 2, 4, 0, 3]])           # (0, 3) is in no sample of the chunk
    assert CR.slots(stranger, plan.cover.numpy(), n).tolist() == [0, 1, 2, 3, 4, -1]
    assert _table_slots(plan, stranger).tolist() == [0, 1, 2, 3, 4, -1]
    third = np.array([[1, 1, 1, 2, 4, 0], [2, 2, 2, 4, 0, 1]])              # a third (1, 2) line: the cover holds two
    assert _table_slots(plan, third).tolist() == CR.slots(third, plan.cover.numpy(), n).tolist() == [1, 6, -1, 3, 4, 0]
    # the cover holds a key ONCE and the sample twice or three times: the first copy keeps the place, whichever claim lands last
    plain = cover_plan(torch.from_numpy(bt), torch.from_numpy(base[None]), "ac", torch.from_numpy(base))
    doubled = np.array([[0, 1, 2, 2, 4, 1], [1, 2, 1, 4, 0, 3]])
    thrice = np.array([[0, 1, 3, 4, 4, 0], [1, 2, 2, 0, 0, 4]])
    for order in (True, False):
        assert _table_slots(plain, doubled, order).tolist() == CR.slots(doubled, base, n).tolist() == [0, 1, -1, 3, 4, 5]
        assert _table_slots(plain, thrice, order).tolist() == CR.slots(thrice, base, n).tolist() == [0, 1, 2, 4, -1, -1]
        assert _table_slots(plan, thrice, order).tolist() == CR.slots(thrice, plan.cover.numpy(), n).tolist() == [0, 1, 2, 4, -1, -1]
    mask, rxc, unplaced = CR.cover_map([s0, stranger], np.arange(24.0).reshape(2, 6, 2), plan.cover.numpy(), n)
    assert mask.tolist() == [[1, 1, 1, 1, 1, 0, 1], [1, 1, 1, 1, 1, 0, 0]] and unplaced.tolist() == [0, 1]
    assert rxc[0, 6].tolist() == [2.0, 3.0] and rxc[0, 1].tolist() == [0.0, 1.0] and np.isnan(rxc[0, 5]).all()


def test_lines_that_are_no_lines_are_refused():
    bt = torch.tensor([0, 2, 2, 1, 2])
    good = np.array([[0, 1, 3, 2, 4, 1], [1, 2, 2, 4, 0, 3]])
    for bad in ([[0, 1, 3, 2, 4, 1], [1, 2, 2, 4, 0, 5]], [[0, 1, 3, 2, 4, -1], [1, 2, 2, 4, 0, 3]], [[0, 1, 3, 2, 4, 3], [1, 2, 2, 4, 0, 3]]):
        with pytest.raises(RuntimeError, match="cover_plan failed"):
            cover_plan(bt, torch.tensor([good.tolist(), bad]), "ac")
    with pytest.raises(RuntimeError, match="sparse_plan failed.*outside"):        # a base line outside the grid: the builder's refusal
        cover_plan(bt, torch.from_numpy(good[None]), "ac", torch.tensor([[0, 1], [1, 7]]))
    with pytest.raises(RuntimeError, match=r"\(S, 2, e\)"):
        cover_plan(bt, torch.from_numpy(good), "ac")
    with pytest.raises(ValueError, match="mode must be"):
        cover_plan(bt, torch.from_numpy(good[None]), "newton")


# ------------------------------------------------------------------------------------------------------- closure
@pytest.mark.parametrize("n,e", [(14, 20), (118, 186)])
@pytest.mark.parametrize("ra", [1, 2])
def test_every_samples_jacobian_pattern_lies_inside_the_cover_plans_filled_pattern(n, e, ra):
    ei, bt, lists = _perturbed(n, e, 8, ra, ra)
    for mode, code in (("ac", 0), ("dc", 1)):
        cp = cover_plan(torch.from_numpy(bt), torch.from_numpy(lists), mode, torch.from_numpy(ei))
        assert cp.extras >= 1
        plan = SP.Plan(cp.plan.blob.numpy().tobytes())
        assert plan.e == cp.e_cover and plan.mode == code
        filled = plan.pattern()
        unknown = [u for u in (plan.ua, plan.uv)]
        for s in range(len(lists)):
            blocks = {(int(i), int(i)) for i in range(n)} | {(int(a), int(b)) for a, b in lists[s].T} | {(int(b), int(a)) for a, b in lists[s].T}
            mine = {(int(ur[i]), int(uc[j])) for i, j in blocks for ur in unknown for uc in unknown if ur[i] >= 0 and uc[j] >= 0}
            assert mine <= filled, (mode, s, sorted(mine - filled)[:4])
        # ... and the cover's own lines are what the plan was built from: the stale-plan check stays against the cover list
        for i in range(n):
            for q in range(plan.adjptr[i], plan.adjptr[i + 1]):
                code_q, j = plan.adj[q]
                assert cp.cover[code_q & 1, code_q >> 1] == i and cp.cover[1 - (code_q & 1), code_q >> 1] == j


def test_fd_cover_plan_is_one_plan_for_both_variants():
    ei, bt, lists = _perturbed(14, 20, 4, 1, 1)
    for spelling in ("fd", "fdxb", "fdbx"):
        cp = cover_plan(torch.from_numpy(bt), torch.from_numpy(lists), spelling, torch.from_numpy(ei))
        assert cp.mode == cp.plan.mode == "fd" and cp.plan.e == cp.e_cover and len(cp.plan.halves) == 2


# ------------------------------------------------------------------------------------------------------ chunking
def test_the_chunker_finds_a_size_and_keeps_it():
    n, e = 118, 186
    ei, bt, lists = _perturbed(n, e, 48, 1, 2)
    t_bt, t_ei, t_lists = torch.from_numpy(bt), torch.from_numpy(ei), torch.from_numpy(lists)
    base = sparse_plan(t_bt, t_ei)
    loose = CoverChunker(t_bt, t_ei, "ac", max_growth=1e9, start=4)          # everything fits: doubled up to the batch
    got = list(loose.plans(t_lists))
    assert [(r.start, r.stop) for r, _ in got] == [(0, 32), (32, 48)] and loose.size == 32 and loose.base_plan.madds == base.madds
    assert list(loose.plans(t_lists[:40]))[0][0] == slice(0, 32)             # the next batch starts at the size found: no new search
    tight = CoverChunker(t_bt, t_ei, "ac", max_growth=1.0, start=8)          # no growth allowed: halved down to single samples at need
    rows = [r for r, _ in tight.plans(t_lists)]
    assert rows[0].start == 0 and rows[-1].stop == 48 and all(a.stop == b.start for a, b in zip(rows, rows[1:]))
    for r, cp in tight.plans(t_lists[:8]):
        assert r.stop - r.start == 1 or cp.plan.madds <= base.madds
    mid = CoverChunker(t_bt, t_ei, "ac", max_growth=1.5, start=8)
    for r, cp in mid.plans(t_lists):
        assert r.stop - r.start == 1 or mid.growth(cp) <= 1.5
        assert np.array_equal(cp.cover.numpy(), CR.cover(lists[r], ei))
    assert mid.trials >= len(mid.sizes) and sum(mid.sizes) == 48
    with pytest.raises(ValueError, match="max_growth"):
        CoverChunker(t_bt, t_ei, "ac", max_growth=0.5)


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals_are_decided_before_a_device_is_touched():
    ei, bt, lists = _perturbed(14, 20, 4, 1, 1)
    _, _, rx, spec = make_physical_inputs(14, 20, 4, 1)
    t_bt, t_lists = torch.from_numpy(bt), torch.from_numpy(lists)
    with pytest.raises(RuntimeError, match="one topology"):
        solve_power_flow(t_bt, spec, t_lists, rx, route="sparse")
    with pytest.raises(RuntimeError, match="one topology"):
        solve_power_flow(t_bt, spec, t_lists, rx, route="sparse", plan=sparse_plan(t_bt, torch.from_numpy(ei)))
    cover = cover_plan(t_bt, t_lists, "ac", torch.from_numpy(ei))
    with pytest.raises(RuntimeError, match="the plan is for"):               # another mode
        solve_power_flow(t_bt, spec, t_lists, rx, route="sparse", mode="dc", plan=cover)
    with pytest.raises(RuntimeError, match="the plan is for"):
        solve_power_flow(t_bt, spec, t_lists, rx, route="sparse", mode="fdxb", plan=cover)
    ei5, bt5, lists5 = _perturbed(5, 6, 4, 1, 1)
    with pytest.raises(RuntimeError, match="the plan is for"):               # another n
        solve_power_flow(t_bt, spec, t_lists, rx, route="sparse", plan=cover_plan(torch.from_numpy(bt5), torch.from_numpy(lists5), "ac"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):               # a fitting plan: the call goes on to the device check
        solve_power_flow(t_bt, spec, t_lists, rx, route="sparse", plan=cover)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PF.cover_map(cover, t_lists, rx)


def test_the_masked_entries_refuse_what_the_plain_ones_refuse():
    """host-side argument checks of the new C entries: no launch is reached"""
    from poweflownet_amd import _lib as L
    lib = L.load()
    ei, bt = _grid(14, 20)
    plan = sparse_plan(torch.from_numpy(bt), torch.from_numpy(ei))
    head = C.addressof(plan.header)
    rc = lib.pfn_powerflow_solve_sparse_masked(None, 20, None, None, None, None, None, None, 1, 14, 2, 1e-8, 10, head, None, 0, None, None, None,
                                               None, None, 0, None)
    assert rc == -1 and b"mode must be 0" in lib.pfn_last_error()
    rc = lib.pfn_powerflow_solve_sparse_masked(None, 21, None, None, None, None, None, None, 1, 14, 0, 1e-8, 10, head, None, 0, None, None, None,
                                               None, None, 0, None)
    assert rc == -1 and b"the plan is for" in lib.pfn_last_error()
    rc = lib.pfn_powerflow_cover_map(None, 20, None, 1, 0, None, None, 20, None, None, None, None)
    assert rc == -1 and b"bad sizes" in lib.pfn_last_error()
    rc = lib.pfn_powerflow_cover_map(None, 20, None, 1, 14, None, None, 20, None, None, None, None)
    assert rc == -1 and b"null" in lib.pfn_last_error()
    assert lib.pfn_powerflow_cover_map(None, 20, None, 0, 14, None, None, 20, None, None, None, None) == 0      # no samples: nothing to do


# ------------------------------------------------------------------------------- the builder's single-call entry
@pytest.mark.parametrize("n,e", [(5, 6), (14, 20), (118, 186)])
def test_the_single_call_builder_gives_the_two_call_plan_byte_for_byte(n, e):
    from poweflownet_amd import _lib as L
    lib = L.load()
    ei, bt = _grid(n, e)
    ei, bt32 = np.ascontiguousarray(ei), np.ascontiguousarray(bt, dtype=np.int32)
    for mode, code in (("ac", 0), ("dc", 1), ("fd", 2)):
        want = sparse_plan(torch.from_numpy(bt), torch.from_numpy(ei), mode)
        blob = want.blob.numpy().tobytes()
        needed = C.c_size_t(0)
        for room in (0, 64, want.bytes - 16, want.bytes - 1):                # too small (the first: a null buffer): the size comes back
            buf = np.full(max(room, 1), 0xAB, dtype=np.uint8)
            rc = lib.pfn_powerflow_sparse_plan_into(ei.ctypes.data, e, bt32.ctypes.data, n, code, buf.ctypes.data if room else None, room, C.byref(needed))
            assert rc == -2 and needed.value == want.bytes and b"needs" in lib.pfn_last_error(), (mode, room)
        for room in (want.bytes, want.bytes + 1000):
            buf = np.full(room, 0xAB, dtype=np.uint8)
            rc = lib.pfn_powerflow_sparse_plan_into(ei.ctypes.data, e, bt32.ctypes.data, n, code, buf.ctypes.data, room, C.byref(needed))
            assert rc == 0 and needed.value == want.bytes and buf[:want.bytes].tobytes() == blob, (mode, room)
            assert (buf[want.bytes:] == 0xAB).all()                           # nothing behind the plan is touched
        for hint in (1, want.bytes, 3 * want.bytes):
            got = sparse_plan(torch.from_numpy(bt), torch.from_numpy(ei), mode, size_hint=hint)
            assert got.blob.numpy().tobytes() == blob and (got.madds, got.nnz_l, got.max_col, got.bytes, got.halves) == (
                want.madds, want.nnz_l, want.max_col, want.bytes, want.halves)
    needed = C.c_size_t(7)
    buf = np.zeros(1 << 16, dtype=np.uint8)
    bad = ei.copy()
    bad[1, 0] = n
    for args, text in (((bad.ctypes.data, e, bt32.ctypes.data, n, 0), b"outside"), ((bad.ctypes.data, e, bt32.ctypes.data, n, 2), b"outside"),
                       ((ei.ctypes.data, e, bt32.ctypes.data, n, 3), b"mode must be")):
        assert lib.pfn_powerflow_sparse_plan_into(*args, buf.ctypes.data, len(buf), C.byref(needed)) == -1 and text in lib.pfn_last_error()
        assert needed.value == 0
    assert lib.pfn_powerflow_sparse_plan_into(ei.ctypes.data, e, bt32.ctypes.data, n, 0, buf.ctypes.data, len(buf), None) == -1
