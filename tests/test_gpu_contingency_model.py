"""The network's N-1 screen on the device: `pfn_contingency_model_batch` and `pfn_contingency_model_loadings`
(csrc/contingency_model.hip) and `contingency_screen_model` around them.  Every comparison is BIT FOR BIT against code the project
already trusts -- no tolerance anywhere:
  batch       every tensor of a chunk equals tests/contingency_model_ref.py, which tests/test_contingency_model_host.py holds to
              `PowerFlowData` and its collate;
  loadings    the kept table equals `branch_flows` on the kept (merged) predictions, the reduced lists and float(rx), over the
              ratings, scattered to the original numbering; the three figures equal `summarise_loadings` of that table; islanding
              rows are +inf, -1, -1, NaN;
  AC truth    with a stub that returns the AC solver's table of every item, the table equals `verify_contingencies`' loadings;
  network     with a seeded MaskEmbdMultiMPN, the result equals the composition it replaces on the same chunks;
  graphed     equals eager, and a second call captures nothing.
"Same bits" means: NaN at the same places, equal bits everywhere else.  Grids are `make_physical_inputs(n, e, S, seed=1)`.
Beyond `pfn_contingency_model_lds_max_bus()` (10176 buses) no grid is screened here -- ten thousand outages of a ten-thousand-bus
grid do not fit a few seconds; the direct route that serves such grids is held to the LDS route at the small shapes instead
(`route` of the C entry)."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch
import torch.nn as nn

from poweflownet_amd import _lib as L
from poweflownet_amd.loss import branch_flows
from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
from poweflownet_amd.utils.contingency import (MODEL_CHUNK, ModelContingencyResult, contingency_screen, contingency_screen_model, summarise_loadings,
                                               verify_contingencies)
from tests import contingency_model_ref as R
from tests.powerflow_checks import DEV, TOL, _dev, _run
from tests.test_gpu_powerflow import _case

pytestmark = pytest.mark.gpu
SHAPES = [(3, 3), (5, 6), (14, 20), (118, 186)]
S2 = 2
STATS = {"xymean": torch.tensor([[1.01, -3.0, 0.1, 0.03]]), "xystd": torch.tensor([[0.02, 4.5, 0.25, 0.06]]),
         "edgemean": torch.tensor([[0.017, 0.09]]), "edgestd": torch.tensor([[0.007, 0.035]])}


def _bits(t):
    return t.contiguous().view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def _same_bits(a, b):
    """NaN at the same places, equal bits everywhere else"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(_bits(a)[~na], _bits(b)[~nb])


@functools.lru_cache(maxsize=None)
def _inputs(n, e, S):
    """(case, bus_type, spec, edge_index, rx) of a shape: the host case and its device tensors, once"""
    case = _case(n, e, S)
    return case, _dev(case.bt), _dev(case.spec), _dev(case.ei), _dev(case.rx)


def _floats(v, count, plus=0.0):
    return None if v is None else (C.c_float * count)(*[float(a) for a in (v.float().reshape(-1)[:count] + plus).tolist()])


def _launch_batch(bt, spec, ei, rx, item0, B, stats):
    S, n, e = spec.shape[0], spec.shape[1], ei.shape[1]
    out = {"x": torch.full((B * n, 4), -7.0, device=DEV), "pred_mask": torch.full((B * n, 4), -7.0, device=DEV),
           "bus_type": torch.full((B * n,), -7, dtype=torch.int64, device=DEV),
           "edge_index": torch.full((2, B * (e - 1)), -7, dtype=torch.int64, device=DEV), "edge_attr": torch.full((B * (e - 1), 2), -7.0, device=DEV)}
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    word, bt32 = torch.tensor([item0], dtype=torch.int64, device=DEV), bt.to(torch.int32)
    L.check(L.load().pfn_contingency_model_batch(bt32.data_ptr(), spec.data_ptr(), ei.data_ptr(), rx.data_ptr(), S, n, e, word.data_ptr(),
                                                 B, _floats(stats.get("xystd"), 4, 1e-7), _floats(stats.get("xymean"), 4),
                                                 _floats(stats.get("edgestd"), 2, 1e-7), _floats(stats.get("edgemean"), 2), out["x"].data_ptr(),
                                                 out["pred_mask"].data_ptr(), out["bus_type"].data_ptr(), out["edge_index"].data_ptr(),
                                                 out["edge_attr"].data_ptr(), flags.data_ptr(), L.stream_ptr()), "pfn_contingency_model_batch")
    return out, int(flags.item())


# ------------------------------------------------------------------------------------------------------- batch bits
@pytest.mark.parametrize("n,e", SHAPES)
def test_the_batch_of_a_chunk_equals_the_dataset_and_its_collate(n, e):
    case, bt, spec, ei, rx = _inputs(n, e, S2)
    T = S2 * e
    h = [torch.from_numpy(a) for a in (case.bt, case.spec, case.ei, case.rx)]
    # the whole screen from item 0; a chunk that straddles the two scenarios from a nonzero item; a padded tail; a one-item chunk
    for item0, B in ((0, T), (e - 2, 5), (T - 3, 8), (e, 1)):
        for stats in ({}, STATS):
            got, flags = _launch_batch(bt, spec, ei, rx, item0, B, stats)
            want = R.batch_ref(*h, R.chunk_items(item0, B, S2, e), **stats)
            assert flags == 0
            for name, t in got.items():
                w = want[name].to(DEV)
                assert t.dtype == w.dtype and torch.equal(_bits(t), _bits(w)), (n, e, item0, B, bool(stats), name)


def test_a_line_with_a_bad_bus_id_is_flagged_and_written_inside_its_graph():
    case, bt, spec, ei, rx = _inputs(5, 6, S2)
    bad = ei.clone()
    bad[1, 2] = 5                                                           # line 2 names bus 5 of a 5-bus grid
    got, flags = _launch_batch(bt, spec, bad, rx, 0, 4, {})
    assert flags == 2
    for b, k in enumerate(range(4)):                                        # item b = (scenario 0, outage k = b): line 2 sits at position 2 - (k < 2)
        cols = got["edge_index"][:, b * 5:(b + 1) * 5]
        assert int(cols.min()) >= b * 5 and int(cols.max()) < (b + 1) * 5
        if k != 2:
            assert cols[:, 2 - (k < 2)].tolist() == [b * 5, b * 5]
    islands = torch.empty(6, dtype=torch.int32, device=DEV)
    L.check(L.load().pfn_contingency_islands(bad.data_ptr(), 6, 5, 0, islands.data_ptr(), L.stream_ptr()), "pfn_contingency_islands")
    assert islands.tolist() == [-4] * 6                                     # ... and every item of such a list is overwritten as islanding


# --------------------------------------------------------------------------------------------------- loadings bits
class _Stub(nn.Module):
    """a deterministic stand-in: plausible voltages that depend on the scenario (through x) AND on the outage (through the chunk's
    edge_attr); `nan_at` = (call, chunk position) returns NaN rows for one item"""

    def __init__(self, n, nan_at=None):
        super().__init__()
        self.n, self.nan_at, self.calls = n, nan_at, 0

    def forward(self, data):
        B = data.x.shape[0] // self.n
        per_graph = data.edge_attr.view(B, -1, 2).sum(dim=1).repeat_interleave(self.n, dim=0)       # [B n, 2]
        row = torch.arange(data.x.shape[0], device=data.x.device, dtype=torch.float32)[:, None]
        vm = 1.0 + 0.05 * torch.sin(0.37 * row + per_graph[:, :1])
        va = 8.0 * torch.cos(0.11 * row + 3.0 * per_graph[:, 1:] + data.x[:, 2:3])
        out = torch.cat([vm, va, data.x[:, 2:4] * 0.5], dim=1).float()
        if self.nan_at is not None and self.nan_at[0] == self.calls:
            b = self.nan_at[1]
            out[b * self.n:(b + 1) * self.n] = float("nan")
        self.calls += 1
        return out


def _composition(pred, bt, ei, rx, ratings, islands):
    """`branch_flows` on the kept predictions [S, e, n, 4] over the reduced lists, over the ratings, back in the original numbering;
    `summarise_loadings` of that table; the islanding rows by the screen's rule.  (loading [S, e, e], severity, worst, overloads)"""
    S, e = int(rx.shape[0]), int(ei.shape[1])
    k = torch.arange(e, device=DEV)
    ar = torch.arange(e - 1, device=DEV)
    idx = ar[None, :] + (ar[None, :] >= k[:, None])                         # [e, e - 1]: `_verify_removed`'s rule per outage
    idx = idx[None].expand(S, e, e - 1).reshape(S * e, e - 1)
    lists = ei[:, idx].permute(1, 0, 2).contiguous()                        # [S e, 2, e - 1]
    sc = torch.arange(S, device=DEV).repeat_interleave(e)
    rx_post = rx[sc[:, None], idx].float().contiguous()                     # [S e, e - 1, 2]
    flows = branch_flows(pred.reshape(S * e, -1, 4), lists, rx_post)[0]
    rate = (torch.ones(S, e, device=DEV) if ratings is None else ratings.float().expand(S, e))[sc]
    loading = torch.full((S * e, e), float("nan"), device=DEV)
    loading.scatter_(1, idx, flows[:, :, 0] / rate.gather(1, idx))
    monitored = (rate > 0) & (k[None, :] != k.repeat(S)[:, None])
    sev, worst, over = summarise_loadings(loading, monitored)
    cut = (islands != 0).repeat(S)
    loading[cut] = float("nan")
    sev, worst, over = sev.masked_fill(cut, float("inf")), worst.masked_fill(cut, -1), over.masked_fill(cut, -1)
    return loading.view(S, e, e), sev.view(S, e), worst.view(S, e), over.view(S, e)


def _check_against_composition(res, bt, ei, rx, ratings, what):
    loading, sev, worst, over = _composition(res.predictions, bt, ei, rx, ratings, res.islands)
    assert isinstance(res, ModelContingencyResult) and int(res.flags.item()) == 0
    assert res.loading.dtype == torch.float32 and res.severity.dtype == torch.float32 and res.worst_line.dtype == torch.int32 and res.overloads.dtype == torch.int32
    assert _same_bits(res.loading, loading), what
    assert _same_bits(res.severity, sev) and torch.equal(res.worst_line, worst) and torch.equal(res.overloads, over), what
    cut = res.islands != 0
    assert bool(cut.any()) and bool((~cut).any())
    assert bool(torch.isnan(res.loading[:, cut]).all()) and bool((res.severity[:, cut] == float("inf")).all())
    assert bool((res.worst_line[:, cut] == -1).all()) and bool((res.overloads[:, cut] == -1).all())
    e = int(ei.shape[1])
    assert bool(torch.isnan(res.loading[:, torch.arange(e), torch.arange(e)]).all())           # the outaged line itself


def _ratings(kind, S, e):
    g = torch.Generator().manual_seed(11)
    if kind is None:
        return None
    r = 0.2 + 1.3 * torch.rand((S, e) if kind == "per_scenario" else (e,), generator=g, dtype=torch.float64)
    if kind == "holes":                                                     # a zero, a NaN and a negative rating: unmonitored lines
        r[0], r[1], r[e - 1] = 0.0, float("nan"), -1.0
    return r.to(DEV)


@pytest.mark.parametrize("kind", [None, "per_line", "per_scenario", "holes"])
@pytest.mark.parametrize("n,e", SHAPES)
def test_loadings_and_figures_equal_branch_flows_and_summarise_loadings(n, e, kind):
    case, bt, spec, ei, rx = _inputs(n, e, S2)
    ratings = _ratings(kind, S2, e)
    stats = STATS if kind in ("per_line", "holes") else {}
    chunk = {None: None, "per_line": 7, "per_scenario": e + 1, "holes": 2 * e}[kind]           # the default, a tail, a straddle, one chunk
    res = contingency_screen_model(_Stub(n), bt, spec, ei, rx, ratings, chunk=chunk, keep_table=True, keep_predictions=True, **stats)
    assert res.predictions.shape == (S2, e, n, 4) and res.chunk == min(chunk or MODEL_CHUNK, S2 * e)
    _check_against_composition(res, bt, ei, rx, ratings, (n, e, kind))
    # the kept predictions are the merge: float(spec) where the entry is given, whatever the stub said there
    given = ~torch.tensor(R.PowerFlowData.bus_type_mask)[torch.from_numpy(case.bt)].bool().to(DEV)
    assert torch.equal(res.predictions[:, :, given], spec.float()[:, None].expand(S2, e, n, 4)[:, :, given])
    # without the tables the figures are the same
    bare = contingency_screen_model(_Stub(n), bt, spec, ei, rx, ratings, chunk=chunk, **stats)
    assert bare.loading is None and bare.predictions is None
    assert _same_bits(bare.severity, res.severity) and torch.equal(bare.worst_line, res.worst_line) and torch.equal(bare.overloads, res.overloads)
    if kind == "holes":                                                     # no monitored line at all: (0, -1, 0) where the outage does not island
        none = contingency_screen_model(_Stub(n), bt, spec, ei, rx, torch.zeros(e, dtype=torch.float64, device=DEV), **stats)
        ok = none.islands == 0
        assert bool((none.severity[:, ok] == 0).all()) and bool((none.worst_line[:, ok] == -1).all()) and bool((none.overloads[:, ok] == 0).all())


def test_a_nan_prediction_poisons_its_own_item_only():
    n, e = 14, 20
    case, bt, spec, ei, rx = _inputs(n, e, S2)
    clean = contingency_screen_model(_Stub(n), bt, spec, ei, rx, chunk=16, keep_table=True, keep_predictions=True)
    ok = (clean.islands == 0).nonzero().flatten().tolist()
    k = next(k for k in ok if k >= 4)                                       # a non-islanding outage of scenario 1, second chunk onwards
    item = e + k
    res = contingency_screen_model(_Stub(n, nan_at=(item // 16, item % 16)), bt, spec, ei, rx, chunk=16, keep_table=True, keep_predictions=True)
    _check_against_composition(res, bt, ei, rx, None, "nan")
    assert bool(torch.isnan(res.severity[1, k])) and int(res.worst_line[1, k]) >= 0
    other = torch.ones(S2, e, dtype=torch.bool, device=DEV)
    other[1, k] = False
    assert _same_bits(res.severity[other], clean.severity[other]) and torch.equal(res.worst_line[other], clean.worst_line[other])
    assert not bool(torch.isnan(res.severity[other]).any())


@pytest.mark.parametrize("n,e", [(5, 6), (14, 20)])
def test_the_direct_route_has_the_bits_of_the_lds_route(n, e):
    """the route beyond pfn_contingency_model_lds_max_bus(), forced at shapes a test can afford"""
    case, bt, spec, ei, rx = _inputs(n, e, S2)
    T, lib = S2 * e, L.load()
    g = torch.Generator().manual_seed(3)
    out = (torch.rand(T * n, 4, generator=g) * torch.tensor([0.1, 20.0, 1.0, 1.0]) + torch.tensor([0.95, -10.0, 0.0, 0.0])).to(DEV)
    ratings = _ratings("per_scenario", S2, e)
    islands = torch.empty(e, dtype=torch.int32, device=DEV)
    L.check(lib.pfn_contingency_islands(ei.data_ptr(), e, n, 0, islands.data_ptr(), L.stream_ptr()), "pfn_contingency_islands")
    word, bt32 = torch.zeros(1, dtype=torch.int64, device=DEV), bt.to(torch.int32)
    got = {}
    for route in (1, 2):
        sev, worst, over = torch.empty(T, device=DEV), torch.empty(T, dtype=torch.int32, device=DEV), torch.empty(T, dtype=torch.int32, device=DEV)
        table, pred = torch.empty(T, e, device=DEV), torch.empty(T, n, 4, device=DEV)
        L.check(lib.pfn_contingency_model_loadings(out.data_ptr(), bt32.data_ptr(), spec.data_ptr(), ei.data_ptr(), rx.data_ptr(), ratings.data_ptr(), 1,
                                                   islands.data_ptr(), S2, n, e, word.data_ptr(), T, _floats(STATS["xystd"], 4, 1e-7),
                                                   _floats(STATS["xymean"], 4), route, sev.data_ptr(), worst.data_ptr(), over.data_ptr(),
                                                   table.data_ptr(), pred.data_ptr(), L.stream_ptr()), "pfn_contingency_model_loadings")
        got[route] = (sev, worst, over, table, pred)
    assert all(_same_bits(a, b) for a, b in zip(got[1], got[2]))
    assert bool(torch.isfinite(got[1][0][(islands == 0).repeat(S2)]).all())


def test_wrong_dtypes_and_shapes_are_refused():
    case, bt, spec, ei, rx = _inputs(5, 6, S2)
    stub = _Stub(5)
    with pytest.raises(RuntimeError, match="spec must be float64"):
        contingency_screen_model(stub, bt, spec.float(), ei, rx)
    with pytest.raises(RuntimeError, match="bus_type must be"):
        contingency_screen_model(stub, bt[:4], spec, ei, rx)
    with pytest.raises(RuntimeError, match="edge_index must be int64"):
        contingency_screen_model(stub, bt, spec, ei.int(), rx)
    with pytest.raises(RuntimeError, match="rx must be float64"):
        contingency_screen_model(stub, bt, spec, ei, rx[:1])
    with pytest.raises(RuntimeError, match="ratings must be float64"):
        contingency_screen_model(stub, bt, spec, ei, rx, torch.ones(6, device=DEV))
    with pytest.raises(ValueError, match="one line"):
        contingency_screen_model(stub, bt, spec, ei[:, :1].contiguous(), rx[:, :1].contiguous())

    class _Short(nn.Module):
        def forward(self, data):
            return data.x[:-1]
    with pytest.raises(RuntimeError, match="must return float32"):
        contingency_screen_model(_Short(), bt, spec, ei, rx)


# ------------------------------------------------------------------------------------------------ against AC truth
class _Replay(nn.Module):
    """returns, for every item of the chunk it is called for, that item's row of a table [S e, n, 4]"""

    def __init__(self, table, chunk):
        super().__init__()
        self.table, self.chunk, self.calls = table, chunk, 0

    def forward(self, data):
        T = self.table.shape[0]
        items = torch.arange(self.calls * self.chunk, (self.calls + 1) * self.chunk, device=self.table.device).clamp(max=T - 1)
        self.calls += 1
        return self.table[items].reshape(-1, 4)


@pytest.mark.parametrize("n,e", [(5, 6), (14, 20)])
def test_with_the_ac_tables_as_predictions_the_screen_equals_the_ac_verification(n, e):
    """item order, line renumbering and the merge against something physical: a stub that hands back the AC solver's own table of
    every (scenario, outage) makes the screen's loadings those of `verify_contingencies`, bit for bit"""
    S = 3
    case, bt, spec, ei, rx = _inputs(n, e, S)
    g = torch.Generator().manual_seed(5)
    ratings = (0.3 + torch.rand(e, generator=g, dtype=torch.float64)).to(DEV)
    dc = contingency_screen(bt, spec, ei, rx, ratings, tol=TOL, max_iter=10)
    ok = (dc.islands == 0).nonzero().flatten().tolist()
    pairs = [(s, k) for s in range(S) for k in ok]
    ver = verify_contingencies(dc, bt, spec, ei, rx, ratings, pairs=pairs, tol=TOL, max_iter=10)
    assert bool((ver.status >= 1).all()) and len(pairs) < S * e
    # what the AC table holds at the given entries IS float(spec) there, so the merge leaves the table as the solver wrote it
    table32 = ver.table.float()
    given = ~torch.tensor(R.PowerFlowData.bus_type_mask)[torch.from_numpy(case.bt)].bool().to(DEV)
    assert torch.equal(table32[:, given], spec.float()[ver.pairs[:, 0]][:, given])
    full = torch.zeros(S * e, n, 4, device=DEV)                             # (the islanding items: zeros, overwritten by the verdict)
    full[ver.pairs[:, 0] * e + ver.pairs[:, 1]] = table32
    chunk = e + 3
    res = contingency_screen_model(_Replay(full, chunk), bt, spec, ei, rx, ratings, chunk=chunk, keep_table=True, keep_predictions=True)
    sc, out = ver.pairs[:, 0], ver.pairs[:, 1]
    assert _same_bits(res.predictions[sc, out], table32)
    assert _same_bits(res.loading[sc, out], ver.loading)
    assert _same_bits(res.severity[sc, out], ver.severity) and torch.equal(res.worst_line[sc, out], ver.worst_line)
    assert torch.equal(res.overloads[sc, out], ver.overloads) and torch.equal(res.islands, dc.islands)
    # `verify_contingencies` takes the network's result unchanged; its dc_severity column is then the network's figure
    again = verify_contingencies(res, bt, spec, ei, rx, ratings, top=2, tol=TOL, max_iter=10)
    assert again.pairs.shape == (2 * S, 2) and _same_bits(again.dc_severity, res.severity[again.pairs[:, 0], again.pairs[:, 1]])
    assert _same_bits(again.severity, again.dc_severity)                    # (here the "network" IS the AC solver)


# --------------------------------------------------------------------------------------------------- real network
def _network():
    torch.manual_seed(7)
    return MaskEmbdMultiMPN(4, 2, 4, 16, 2, 2, 0.0).to(DEV)


def _host_composition(model, case, spec, bt, ei, rx, ratings, chunk, stats):
    """the composition the entry replaces, on the same chunks with the model on the same flags: the yardstick's host-built batch,
    model(batch), merge, `branch_flows`, `summarise_loadings`"""
    from poweflownet_amd.data import Batch
    S, n, e = case.S, case.n, case.e
    T = S * e
    h = [torch.from_numpy(a) for a in (case.bt, case.spec, case.ei, case.rx)]
    pred = torch.empty(T, n, 4, device=DEV)
    was = (model.dynamic_topology, model.segment_build, model.training)
    model.dynamic_topology, model.segment_build = True, True
    model.eval()
    try:
        with torch.no_grad():
            for item0 in range(0, T, chunk):
                items = R.chunk_items(item0, chunk, S, e)
                batch = Batch()
                for name, t in R.batch_ref(*h, items, **stats).items():
                    setattr(batch, name, t.to(DEV))
                out = model(batch)
                merged = R.merged_ref(out, bt, spec[torch.tensor(items, device=DEV) // e], stats.get("xymean"), stats.get("xystd"))
                live = min(chunk, T - item0)
                pred[item0:item0 + live] = merged[:live]
    finally:
        model.dynamic_topology, model.segment_build = was[:2]
        model.train(was[2])
    islands = torch.empty(e, dtype=torch.int32, device=DEV)
    L.check(L.load().pfn_contingency_islands(ei.data_ptr(), e, n, 0, islands.data_ptr(), L.stream_ptr()), "pfn_contingency_islands")
    return (pred.view(S, e, n, 4),) + _composition(pred.view(S, e, n, 4), bt, ei, rx, ratings, islands)


@pytest.mark.parametrize("n,e,S,chunks", [(14, 20, 3, (20, 16)), (118, 186, 1, (93, 64))])
def test_a_real_network_equals_the_composition_and_gets_its_flags_back(n, e, S, chunks):
    case, bt, spec, ei, rx = _inputs(n, e, S)
    model = _network()
    ratings = _ratings("per_line", S, e)
    stats = STATS if n == 14 else {}
    for chunk in chunks:                                                    # one that divides S e, one that leaves a tail
        assert (S * e % chunk == 0) == (chunk == chunks[0])
        model.train()
        assert torch.is_grad_enabled() and not model.dynamic_topology and not model.segment_build
        res = contingency_screen_model(model, bt, spec, ei, rx, ratings, chunk=chunk, keep_table=True, keep_predictions=True, **stats)
        assert model.training and all(m.training for m in model.modules()) and torch.is_grad_enabled()
        assert model.dynamic_topology is False and model.segment_build is False
        pred, loading, sev, worst, over = _host_composition(model, case, spec, bt, ei, rx, ratings, chunk, stats)
        assert bool(torch.isfinite(res.predictions).all()) and int(res.flags.item()) == 0
        assert _same_bits(res.predictions, pred) and _same_bits(res.loading, loading), (n, e, chunk)
        assert _same_bits(res.severity, sev) and torch.equal(res.worst_line, worst) and torch.equal(res.overloads, over), (n, e, chunk)
    model.eval()
    model.dynamic_topology = True
    contingency_screen_model(model, bt, spec, ei, rx, ratings, chunk=chunks[0])
    assert not model.training and model.dynamic_topology is True and model.segment_build is False

    class _Raises(nn.Module):
        def forward(self, data):
            raise KeyError("stop")
    model.train()
    broken = nn.Sequential(_Raises())
    broken.train()
    with pytest.raises(KeyError):
        contingency_screen_model(broken, bt, spec, ei, rx)
    assert broken.training and broken[0].training and torch.is_grad_enabled()  # ... also when the forward raises


# --------------------------------------------------------------------------------------------------------- graphed
def test_graphed_equals_eager_and_captures_once():
    n, e, S, chunk = 14, 20, 3, 16                                          # 60 items: three chunks and a tail of 12
    case, bt, spec, ei, rx = _inputs(n, e, S)
    model = _network()
    ratings = _ratings("per_scenario", S, e)
    kw = dict(chunk=chunk, keep_table=True, keep_predictions=True, **STATS)
    fresh = bt.clone()
    with pytest.raises(RuntimeError, match="eagerly once before capturing"):  # the bus_type counts are a host read: eager first
        contingency_screen_model(model, fresh, spec, ei, rx, ratings, graphed=True, **kw)
    eager = contingency_screen_model(model, bt, spec, ei, rx, ratings, **kw)
    assert eager.captures == 0
    first = contingency_screen_model(model, bt, spec, ei, rx, ratings, graphed=True, **kw)
    assert first.captures == 1 and model.dynamic_topology is False and model.segment_build is False
    names = ("severity", "worst_line", "overloads", "islands", "loading", "predictions", "flags")
    assert all(_same_bits(getattr(first, k), getattr(eager, k)) for k in names)
    # a second call, other scenarios of the same shape: the captured chunk is replayed, nothing is captured
    spec2, rx2 = spec.flip(0).contiguous(), rx.flip(0).contiguous()
    second = contingency_screen_model(model, bt, spec2, ei, rx2, ratings, graphed=True, **kw)
    assert second.captures == 1
    eager2 = contingency_screen_model(model, bt, spec2, ei, rx2, ratings, **kw)
    assert all(_same_bits(getattr(second, k), getattr(eager2, k)) for k in names)
    assert all(_same_bits(getattr(first, k), getattr(eager, k)) for k in names)      # (the first answer was not overwritten)
    assert not _same_bits(second.severity, first.severity)


# ---------------------------------------------------------------------------------------------------------- script
def test_the_script_screens_with_a_saved_network(tmp_path, monkeypatch):
    import contingency
    monkeypatch.chdir(tmp_path)
    cfg = {"hidden_dim": 16, "n_gnn_layers": 2, "K": 2, "dropout_rate": 0.0}
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    (tmp_path / "models").mkdir()
    torch.manual_seed(3)
    torch.save({"model_state_dict": MaskEmbdMultiMPN(4, 2, 4, 16, 2, 2, 0.0).state_dict()}, tmp_path / "models" / "model_fresh.pt")
    text = _run(contingency.main, ["--case", "14", "--samples", "2", "--verify-top", "2", "--model-run-id", "fresh", "--cfg_json", str(tmp_path / "cfg.json")])
    assert "islanding outages" in text and "network fresh: 2 scenarios x 20 outages" in text and "scenario 1 network: line" in text
    shapes = {"severity": np.float32, "worst_line": np.int32, "overloads": np.int32}
    for name, dtype in shapes.items():
        a = np.load(tmp_path / "results" / f"case14_contingency_model_{name}.npy")
        assert a.shape == (2, 20) and a.dtype == dtype, name
    # without --model-run-id nothing of it is written
    for f in (tmp_path / "results").iterdir():
        f.unlink()
    _run(contingency.main, ["--case", "14", "--samples", "2", "--verify-top", "2"])
    assert not [f.name for f in (tmp_path / "results").iterdir() if "model" in f.name]
