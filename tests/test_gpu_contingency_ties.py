"""Ties go to the lowest line -- on the device, on every route.  The rule is spelled once (csrc/contingency_monitor.hpp) and met three
times inside a kernel: a thread's strict > over its ascending lines, the merge of the 64 lanes of a wave, the merge of the waves'
partials in the network's screen.  No other device test puts two EQUAL loadings in different lanes, waves or trips; this one does.

The grid is `make_physical_inputs(118, 186, 2, seed=1)` with 74 exact copies (same end buses, same (r, x)) of one non-bridge,
flow-carrying line appended: 260 lines, of which 75 are parallel and carry the same flow, bit for bit, in every item.  The line order
is permuted so that copies sit at 3, 40, 67, 70 and 259 (the other 70 at 189 .. 258).  The DC kernels stride a wave's 64 lanes over
the lines and the network's kernel 256 threads: against line 3, line 40 is another lane of the same trip, 67 the same lane on its
second trip, 70 another wave of the network's kernel (and another lane on the second trip of the others), 259 the same thread of
the network's kernel on its second trip.  Those FIVE carry one small rating (RATED), so that theirs is the largest loading wherever
they are monitored; every other line, the other copies included, keeps 1.0.  Step j of five takes the rating of the first j of them
to 0 (unmonitored): the winner must be 3, 40, 67, 70, 259 in turn and the severity must keep its bits.

Checked items: the non-islanding outages (pairs) none of whose lines is a copy -- asserted on the host yardstick
(tests/contingency_ref.islands, tests/contingency_pairs_ref.islands) to be at least half of all items before anything runs on the
device.  The pair screens take six candidates, none of them a copy.  Per route and step, from the kernel's own table (`keep_table`):
the copies' entries are bit-equal and the rated ones hold the row's largest loading (preconditions), `worst_line` is the step's
line, `severity` has step 0's bits, `overloads` is the count of loading > 1 over the monitored lines."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

from poweflownet_amd import _lib as L
from poweflownet_amd.utils.contingency import contingency_screen, contingency_screen_model, contingency_screen_pairs
from poweflownet_amd.utils.powerflow import sparse_plan
from tests import contingency_pairs_ref as R2
from tests import contingency_ref as R
from tests.powerflow_checks import DEV, TOL, _dev
from tests.test_gpu_powerflow import _case

pytestmark = pytest.mark.gpu
MAX_ITER = 10
N, E0, S = 118, 186, 2
E = 260
SPOTS = (3, 40, 67, 70, 259)
RATED = 1e-4                                                                  # per unit: the five copies' common rating


class _Grid:
    """the augmented grid on the host, what the yardstick says about it, and its device tensors"""

    def __init__(self):
        case = _case(N, E0, S)
        isl0 = R.islands(case.bt, case.ei)
        f0 = np.abs(np.stack([R.base_flow(case.bt, case.spec[s], case.ei, case.rx[s]) for s in range(S)])).min(axis=0)
        src = int(np.argmax(np.where(isl0 == 0, f0, -1.0)))                   # the non-bridge line that carries the most flow at its least
        assert isl0[src] == 0 and f0[src] > 0
        copies = list(SPOTS) + list(range(E0 + 3, E - 1))                     # where the 75 parallel lines go: the five spots, then 189 .. 258
        assert len(copies) == E - E0 + 1 and len(set(copies)) == len(copies) and max(copies) == E - 1
        self.copy = np.zeros(E, dtype=bool)
        self.copy[copies] = True
        origin = np.full(E, src)                                              # new line -> the line of the case it repeats
        origin[~self.copy] = np.delete(np.arange(E0), src)
        self.bt, self.spec = case.bt, case.spec
        self.ei, self.rx = np.ascontiguousarray(case.ei[:, origin]), np.ascontiguousarray(case.rx[:, origin])
        # ---- the checked items, by the host yardstick
        self.isl = R.islands(self.bt, self.ei)
        assert (self.isl[self.copy] == 0).all()
        self.checked = (self.isl == 0) & ~self.copy
        assert 2 * int(self.checked.sum()) >= E, int(self.checked.sum())
        free = np.flatnonzero(self.checked)
        self.lines = [int(k) for k in free[np.linspace(0, free.size - 1, 6).astype(int)]]
        self.pairs = R2.pair_list(self.lines)
        self.pair_isl = R2.islands(self.bt, self.ei, self.pairs)
        self.pair_checked = self.pair_isl == 0
        assert 2 * int(self.pair_checked.sum()) >= len(self.pairs), self.pair_isl

    @functools.cached_property
    def dev(self):
        return _dev(self.bt), _dev(self.spec), _dev(self.ei), _dev(self.rx)

    @functools.cached_property
    def plan(self):
        return sparse_plan(torch.from_numpy(self.bt), torch.from_numpy(self.ei), mode="dc", device=DEV)

    def ratings(self, step):
        r = np.ones(E)
        r[list(SPOTS)] = RATED
        r[list(SPOTS[:step])] = 0.0
        return _dev(r)


@functools.lru_cache(maxsize=None)
def _grid():
    return _Grid()


class _Stub(nn.Module):
    """a deterministic stand-in for the network: plausible voltages that depend on the bus, the scenario and the outage; it keeps
    what it returned, for the direct calls of the C entry"""

    def __init__(self):
        super().__init__()
        self.out = None

    def forward(self, data):
        B = data.x.shape[0] // N
        per_graph = data.edge_attr.view(B, -1, 2).sum(dim=1).repeat_interleave(N, dim=0)
        row = torch.arange(data.x.shape[0], device=data.x.device, dtype=torch.float32)[:, None]
        vm = 1.0 + 0.05 * torch.sin(0.37 * row + per_graph[:, :1])
        va = 8.0 * torch.cos(0.11 * row + 3.0 * per_graph[:, 1:] + data.x[:, 2:3])
        self.out = torch.cat([vm, va, data.x[:, 2:4] * 0.5], dim=1).float().contiguous()
        return self.out


@functools.lru_cache(maxsize=None)
def _stub_out():
    """the stub's output rows for all S * E items as ONE chunk (it does not depend on the ratings), and the N-1 islands"""
    g, stub = _grid(), _Stub()
    res = contingency_screen_model(stub, *g.dev, chunk=S * E)
    return stub.out, res.islands


def _model(step, route):
    """`pfn_contingency_model_loadings` on the stub's rows with the route forced: (severity, worst_line, overloads, table) [S, E(, E)]"""
    g = _grid()
    bt, spec, ei, rx = g.dev
    out, islands = _stub_out()
    T, ratings = S * E, g.ratings(step)
    sev, table = torch.empty(T, device=DEV), torch.empty(T, E, device=DEV)
    worst, over = torch.empty(T, dtype=torch.int32, device=DEV), torch.empty(T, dtype=torch.int32, device=DEV)
    word, bt32 = torch.zeros(1, dtype=torch.int64, device=DEV), bt.to(torch.int32)
    L.check(L.load().pfn_contingency_model_loadings(out.data_ptr(), bt32.data_ptr(), spec.data_ptr(), ei.data_ptr(), rx.data_ptr(), ratings.data_ptr(), 0,
                                                    islands.data_ptr(), S, N, E, word.data_ptr(), T, None, None, route, sev.data_ptr(), worst.data_ptr(),
                                                    over.data_ptr(), table.data_ptr(), None, L.stream_ptr()), "pfn_contingency_model_loadings")
    return sev.view(S, E), worst.view(S, E), over.view(S, E), table.view(S, E, E)


def _single(step, **kw):
    g = _grid()
    res = contingency_screen(*g.dev, g.ratings(step), tol=TOL, max_iter=MAX_ITER, keep_table=True, **kw)
    assert np.array_equal(res.islands.cpu().numpy(), g.isl) and bool((res.status >= 0).all())
    return res.severity, res.worst_line, res.overloads, res.post_flow


def _pairs(step, **kw):
    g = _grid()
    res = contingency_screen_pairs(*g.dev, g.ratings(step), lines=g.lines, tol=TOL, max_iter=MAX_ITER, keep_table=True, **kw)
    assert np.array_equal(res.islands.cpu().numpy(), g.pair_isl) and bool((res.status >= 0).all())
    return res.severity, res.worst_line, res.overloads, res.post_flow


# route -> (run(step) -> (severity, worst_line, overloads, table), items are pairs, the table holds loadings (the network's) not flows)
ROUTES = {
    "dense N-1 lds": (lambda step: _single(step, route="lds"), False, False),
    "dense N-1 global": (lambda step: _single(step, route="global"), False, False),
    "sparse N-1": (lambda step: _single(step, route="sparse", plan=_grid().plan), False, False),
    "dense N-2": (lambda step: _pairs(step), True, False),
    "sparse N-2": (lambda step: _pairs(step, route="sparse", plan=_grid().plan), True, False),
    "model lds": (lambda step: _model(step, 1), False, True),
    "model direct": (lambda step: _model(step, 2), False, True),
}


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("name", list(ROUTES))
def test_equal_loadings_go_to_the_lowest_monitored_line(name):
    g = _grid()
    run, pairs, loadings = ROUTES[name]
    checked = torch.from_numpy(g.pair_checked if pairs else g.checked).to(DEV)
    out = torch.zeros(len(g.pairs) if pairs else E, E, dtype=torch.bool, device=DEV)            # [item, line]: the item's outaged lines
    if pairs:
        out[torch.arange(len(g.pairs)).repeat_interleave(2), torch.from_numpy(g.pairs).reshape(-1)] = True
    else:
        out[torch.arange(E), torch.arange(E)] = True
    copy, spots = torch.from_numpy(g.copy).to(DEV), list(SPOTS)
    first = None
    for step, want in enumerate(SPOTS):
        sev, worst, over, table = run(step)
        r32 = g.ratings(step).float()
        rows = table[:, checked]                                                                # [S, items, E]
        # ---- preconditions: the copies carry one value, bit for bit; the rated ones hold the largest loading of every checked row
        load = rows if loadings else rows.abs() / r32                                           # (the network's table is the loading already)
        rated = torch.zeros(E, dtype=torch.bool, device=DEV)
        rated[spots[step:]] = True
        for same in ((rated, copy & (r32 == 1)) if loadings else (copy,)):
            cols = rows[:, :, same]
            assert bool(torch.isfinite(cols).all()) and torch.equal(_bits(cols), _bits(cols[:, :, :1]).expand_as(cols)), (name, step)
        monitored = (r32 > 0) & ~out[checked]                                                   # [items, E]
        key = torch.where(monitored, load, torch.full_like(load, -1.0))
        top = key.max(dim=2).values
        assert bool((key[:, :, want] == top).all()) and bool(((key == top[:, :, None]).sum(dim=2) == len(SPOTS) - step).all()), (name, step)
        # ---- the winner, the severity's bits, the overload count
        assert bool((worst[:, checked] == want).all()), (name, step, worst[:, checked].unique().tolist())
        assert torch.equal(_bits(sev[:, checked]), _bits(top)), (name, step)
        assert torch.equal(over[:, checked], (monitored & (load > 1)).sum(dim=2).to(torch.int32)), (name, step)
        first = sev if first is None else first
        assert torch.equal(_bits(sev[:, checked]), _bits(first[:, checked])), (name, step)
