"""Segment packing of mixed-size batches, everything that needs no GPU: the planner's invariants, the numpy restatement of the
three device kernels (tests/test_gpu_segpack.py holds the kernels to it bit for bit), the size list a Batch carries, and the
block-wise collate of a `case='mixed'` dataset."""
import os
import re

import numpy as np
import pytest
import torch
from hypothesis import given, settings
from hypothesis import strategies as st

from poweflownet_amd import _lib as L
from poweflownet_amd import segpack
from poweflownet_amd.data import Batch, Data, DataLoader
from poweflownet_amd.synth import make_batch, make_graph, make_topology

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the compositions of DESIGN 7c's table: (sizes, segments, padding rows)
COMPOSITIONS = {
    "40x118+88x14": ([118] * 40 + [14] * 88, 51, 66),
    "64x118+64x14": ([118] * 64 + [14] * 64, 72, 48),
    "1x118+127x14": ([118] + [14] * 127, 17, 110),
}


def ball_like_sizes(count=512, seed=0):
    """`count` graph sizes uniform in 1..118 (what explain_epoch's k-hop balls look like)."""
    return [int(v) for v in np.random.default_rng(seed).integers(1, 119, count)]


# ------------------------------------------------------------------------------------ reference implementations
def naive_first_fit_decreasing(sizes):
    """First-fit-decreasing, one graph at a time, stable order by (-size, batch position): (S, start per graph, fill per bin)."""
    S = max(sizes)
    fill, start = [], [0] * len(sizes)
    for g in sorted(range(len(sizes)), key=lambda i: (-sizes[i], i)):
        for b, used in enumerate(fill):
            if used + sizes[g] <= S:
                break
        else:
            fill.append(0)
            b = len(fill) - 1
        start[g] = b * S + fill[b]
        fill[b] += sizes[g]
    return S, start, fill


def np_row_of(plan):
    """(row_of [N], src_of [n_pad]) of a plan: graph g's rows ptr[g] .. ptr[g + 1] sit at start[g] ..., -1 marks padding."""
    row_of = np.empty(plan.n, dtype=np.int32)
    for g in range(plan.n_graphs):
        row_of[plan.ptr[g]:plan.ptr[g + 1]] = plan.start[g] + np.arange(plan.sizes[g])
    src_of = np.full(plan.n_pad, -1, dtype=np.int32)
    src_of[row_of] = np.arange(plan.n, dtype=np.int32)
    return row_of, src_of


def np_pack(plan, x, mask, edge_index):
    """pfn_segpack_pack restated: (x_pad, mask_pad float32, edge_index_pad, row_of, src_of); an id outside [0, N) becomes -1."""
    row_of, src_of = np_row_of(plan)
    x_pad = np.zeros((plan.n_pad, 4), dtype=np.float32)
    mask_pad = np.zeros((plan.n_pad, 4), dtype=np.float32)
    x_pad[row_of] = x
    mask_pad[row_of] = mask.astype(np.float32)
    ok = (edge_index >= 0) & (edge_index < plan.n)
    ei_pad = np.where(ok, row_of[np.where(ok, edge_index, 0)], -1).astype(np.int64)
    return x_pad, mask_pad, ei_pad, row_of, src_of


def np_gather_rows(src_pad, row_of):
    """pfn_segpack_gather_rows restated."""
    return src_pad[row_of]


def np_scatter_rows(src, row_of, n_pad):
    """pfn_segpack_scatter_rows restated: the adjoint of the gather, padding rows zero."""
    out = np.zeros((n_pad, src.shape[1]), dtype=src.dtype)
    out[row_of] = src
    return out


def _branches(n):
    """Stored branches of a synthetic grid of n buses: synth.CASES' count where it lists the size, about 1.6 per bus otherwise."""
    return {118: 186, 14: 20, 1: 0}.get(n, max(n - 1, (n * 186) // 118))      # (one bus: no branch -- a chord needs two ends)


def make_ragged_batch(sizes, seed=0, edgeless=(), isolated=()):
    """A collated batch of synthetic grids with `sizes` nodes each (one topology per size, as every sample of a reference case
    shares its case's).  Graphs at the positions `edgeless` get no edge at all; graphs at `isolated` keep their last node
    without one."""
    graphs = []
    for g, n in enumerate(sizes):
        if n == 1 or g in edgeless:
            topo = torch.zeros(2, 0, dtype=torch.long)
        elif g in isolated:
            topo = make_topology(n - 1, _branches(n - 1), n)
        else:
            topo = make_topology(n, _branches(n), n)
        graphs.append(make_graph(n, topo.shape[1], seed=seed * 7919 + g, edge_index=topo))
    return Batch.from_data_list(graphs)


# ---------------------------------------------------------------------------------------------------- planner
def _check_plan(sizes, p):
    S, start, fill = naive_first_fit_decreasing(sizes)
    assert p.S == S == max(sizes)
    assert list(p.start) == start and list(p.fill) == fill
    assert p.n_seg == len(fill) and p.n_pad == p.n_seg * S and p.n == sum(sizes)
    taken = np.zeros(p.n_pad, dtype=np.int32)
    for g, n in enumerate(sizes):
        if n == 0:
            continue
        a, b = int(p.start[g]), int(p.start[g]) + n
        assert a // S == (b - 1) // S, "a graph lies inside one segment"
        taken[a:b] += 1
    assert taken.max() <= 1, "no two graphs overlap"
    for seg in range(p.n_seg):                      # graphs of a bin contiguous, its padding rows last
        assert (taken[seg * S:seg * S + p.fill[seg]] == 1).all() and (taken[seg * S + p.fill[seg]:(seg + 1) * S] == 0).all()
    row_of, src_of = np_row_of(p)
    assert (row_of == p.host_row_of()).all()
    assert sorted(src_of[src_of >= 0]) == list(range(p.n))


@settings(max_examples=200, deadline=None, derandomize=True)
@given(st.lists(st.integers(min_value=1, max_value=40), min_size=0, max_size=70))
def test_planner_invariants(sizes):
    p = segpack.plan(sizes, max_padding=1e9)        # (no cap: every non-uniform list gets a plan)
    if len(sizes) < 2 or len(set(sizes)) == 1:
        assert p is None
        return
    _check_plan(sizes, p)
    q = segpack.plan(list(sizes), max_padding=1e9)
    assert (q.start == p.start).all() and (q.fill == p.fill).all(), "deterministic"
    capped = segpack.plan(sizes)                    # the default cap: a plan iff n_pad <= 1.25 N
    assert (capped is not None) == (p.n_pad <= 1.25 * p.n)


def test_planner_on_seeded_random_lists():
    rng = np.random.default_rng(5)
    for _ in range(50):
        sizes = [int(v) for v in rng.integers(1, int(rng.integers(3, 200)), int(rng.integers(2, 400)))]
        p = segpack.plan(sizes, max_padding=1e9)
        if p is not None:
            _check_plan(sizes, p)
    _check_plan(ball_like_sizes(), segpack.plan(ball_like_sizes()))


def test_planner_declines_uniform_small_and_overpadded_batches():
    assert segpack.plan([118] * 128) is None
    assert segpack.plan([14]) is None and segpack.plan([]) is None
    assert segpack.plan([118, 14, 14, 14]) is None                         # 236 rows for 160: 47.5 % padding
    p = segpack.plan([118, 14, 14, 14], max_padding=0.5)
    assert p is not None and (p.n_seg, p.n_pad) == (2, 236) and round(100 * p.padding, 1) == 47.5
    assert segpack.plan([118, 14, 14, 14], max_padding=0.47) is None


@pytest.mark.parametrize("name", sorted(COMPOSITIONS))
def test_planner_reproduces_the_design_table(name):
    """Segments and padding rows of DESIGN 7c's table.  `SegPlan.padding` is relative to the REAL rows, n_pad / N - 1, the
    quantity the cap bounds; the share of the padded layout, (n_pad - N) / n_pad, is checked next to it (for 1 x 118 + 127 x 14
    the two readings are 5.8 % and 5.5 %)."""
    sizes, n_seg, pad_rows = COMPOSITIONS[name]
    p = segpack.plan(sizes)
    assert p.S == 118 and p.n_seg == n_seg and p.n_pad - p.n == pad_rows
    of_real = {"40x118+88x14": 1.1, "64x118+64x14": 0.6, "1x118+127x14": 5.8}[name]
    of_padded = {"40x118+88x14": 1.1, "64x118+64x14": 0.6, "1x118+127x14": 5.5}[name]
    assert round(100 * p.padding, 1) == of_real
    assert round(100 * (p.n_pad - p.n) / p.n_pad, 1) == of_padded


def test_ball_like_batches_stay_far_below_the_cap():
    """512 sizes uniform in 1..118: a few per cent of padding, whatever the draw (seed 0, the benchmark's: 283 segments, 5.2 %)."""
    for seed in range(5):
        p = segpack.plan(ball_like_sizes(512, seed))
        assert p is not None and p.S <= 118 and p.padding < 0.10, (seed, p)
    p = segpack.plan(ball_like_sizes(512, 0))
    assert (p.n, p.n_seg, p.n_pad) == (31732, 283, 33394)


def test_numpy_restatement_round_trips():
    b = make_ragged_batch([5, 1, 9, 3, 9], edgeless=(3,), isolated=(2,))
    p = segpack.plan(b._graph_sizes, max_padding=1.0)
    x_pad, mask_pad, ei_pad, row_of, src_of = np_pack(p, b.x.numpy(), b.pred_mask.numpy(), b.edge_index.numpy())
    assert (np_gather_rows(x_pad, row_of) == b.x.numpy()).all()
    assert (np_scatter_rows(b.x.numpy(), row_of, p.n_pad) == x_pad).all()
    assert (x_pad[src_of < 0] == 0).all() and (mask_pad[src_of < 0] == 0).all()
    assert (ei_pad[0] // p.S == ei_pad[1] // p.S).all(), "no edge crosses a multiple of S"
    assert (src_of[ei_pad] == b.edge_index.numpy()).all(), "the same edges in the same order"
    u = np.random.default_rng(0).standard_normal((p.n_pad, 3)).astype(np.float32)      # <gather u, v> == <u, scatter v>
    v = np.random.default_rng(1).standard_normal((p.n, 3)).astype(np.float32)
    assert np.isclose((np_gather_rows(u, row_of) * v).sum(), (u * np_scatter_rows(v, row_of, p.n_pad)).sum(), rtol=1e-5)


# ------------------------------------------------------------------------------------------------- data layer
def test_batch_carries_its_size_list_without_changing_keys_or_len():
    b = make_ragged_batch([14, 5, 14, 7])
    assert b._graph_sizes == (14, 5, 14, 7)
    keys = ["x", "y", "bus_type", "pred_mask", "edge_index", "edge_attr", "batch", "ptr"]
    for other in (b, b.to("cpu"), b.clone(), b.clone().to("cpu")):
        assert other._graph_sizes == (14, 5, 14, 7)
        assert other.keys() == keys and len(other) == 8
    assert make_batch("14", 3)._graph_sizes == (14, 14, 14) and len(make_batch("14", 3)) == 8
    d = Data(x=torch.zeros(3, 4))                   # a plain Data has no size list and carries none
    assert not hasattr(d.to("cpu"), "_graph_sizes") and not hasattr(d.clone(), "_graph_sizes")


def _mixed_root(tmp_path, samples=12):
    """Raw files of the two grid cases `case='mixed'` reads (118v2 and 14v2), with made-up sizes 9 and 4 buses: [from, to, r, x]
    per branch, [index, type, Vm, Va, P, Q] per bus, the topology of a case the same for all its samples."""
    rng = np.random.default_rng(3)
    (tmp_path / "raw").mkdir()
    for case, n, e in (("118v2", 9, 12), ("14v2", 4, 5)):
        src = rng.integers(0, n, e)
        topo = np.stack([src, (src + 1 + rng.integers(0, n - 1, e)) % n], axis=1).astype(np.float32)     # (no self loops)
        edge = np.concatenate([np.broadcast_to(topo, (samples, e, 2)), rng.standard_normal((samples, e, 2)).astype(np.float32)], axis=2)
        node = np.concatenate([np.broadcast_to(np.arange(n, dtype=np.float32)[None, :, None], (samples, n, 1)),
                               rng.integers(0, 3, (samples, n, 1)).astype(np.float32),
                               rng.standard_normal((samples, n, 4)).astype(np.float32)], axis=2)
        np.save(tmp_path / "raw" / f"case{case}_edge_features.npy", edge)
        np.save(tmp_path / "raw" / f"case{case}_node_features.npy", node)
    return str(tmp_path)


def _assert_same_batch(a, b):
    assert a.keys() == b.keys() and len(a) == len(b)
    for k in a.keys():
        u, v = getattr(a, k), getattr(b, k)
        assert u.dtype == v.dtype and u.shape == v.shape and torch.equal(u, v), k
    assert a._graph_sizes == b._graph_sizes


def test_mixed_dataset_collates_by_block_bitwise_like_the_per_sample_rule(tmp_path, monkeypatch):
    from poweflownet_amd.datasets import PowerFlowData
    ds = PowerFlowData(root=_mixed_root(tmp_path), case="mixed", split=[.5, .25, .25], task="train")
    assert len(ds) == 12 and len(ds._blocks) == 2
    order = torch.randperm(len(ds), generator=torch.Generator().manual_seed(4)).tolist()
    cases = [order, order[:5], [0, 1, 2], [7, 8, 11], [11, 0, 11, 6, -1], [3]]
    want = [Batch.from_data_list([ds[i] for i in idx]) for idx in cases]

    def no_per_sample_path(*a, **k):
        raise AssertionError("collate_indices built a sample")
    monkeypatch.setattr(PowerFlowData, "_sample", no_per_sample_path)
    for idx, w in zip(cases, want):
        got = ds.collate_indices(idx)
        _assert_same_batch(got, w)
        assert got._graph_sizes == tuple(9 if (i % 12) < 6 else 4 for i in idx)
    loader = DataLoader(ds, batch_size=5, shuffle=True, generator=torch.Generator().manual_seed(9))
    assert [b.num_graphs for b in loader] == [5, 5, 2]
    with pytest.raises(IndexError):
        ds.collate_indices([0, 12])


def test_mixed_dataset_with_a_transform_keeps_the_per_sample_rule(tmp_path):
    from poweflownet_amd.datasets import PowerFlowData
    calls = []

    def tr(d):
        calls.append(1)
        return d
    ds = PowerFlowData(root=_mixed_root(tmp_path), case="mixed", split=[.5, .25, .25], task="train", transform=tr)
    b = ds.collate_indices([0, 7, 3])
    assert len(calls) == 3 and b._graph_sizes == (9, 4, 9)


def test_segment_packing_is_opt_in():
    from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
    m = MaskEmbdMultiMPN(4, 2, 4, 8, 2, 2, 0.0)
    assert m.segment_packing is False and m.segment_max_padding == 0.25 and m.last_segment_plan is None


# -------------------------------------------------------------------------------------------------------- ABI
def test_segpack_symbols_are_declared_and_exported():
    names = ("pfn_segpack_pack", "pfn_segpack_gather_rows", "pfn_segpack_scatter_rows")
    header = open(os.path.join(ROOT, "include", "pfn_hip.h")).read()
    lib = L.load()
    for n in names:
        assert n in L.SYMBOLS and re.search(rf"\b{n}\s*\(", header) and hasattr(lib, n), n
    assert lib.pfn_abi_version() == 8


def test_segpack_entry_points_validate_their_scalars():
    lib = L.load()
    one = 16          # any non-null, 16-byte aligned value: every call below is refused before a pointer is used
    args = lambda g, n, s, n_pad: (one, one, one, g, n, s, n_pad, one, one, 0, one, 4, one, one, one, one, one, None)  # noqa: E731
    assert lib.pfn_segpack_pack(*args(2, 10, 8, 12)) == -1 and b"multiple" in lib.pfn_last_error()
    assert lib.pfn_segpack_pack(*args(0, 10, 8, 16)) == -1
    assert lib.pfn_segpack_pack(*args(2, 10, 8, 8)) == -1                                    # n_pad < N
    assert lib.pfn_segpack_pack(None, *args(2, 10, 8, 16)[1:]) == -1 and b"null" in lib.pfn_last_error()
    assert lib.pfn_segpack_pack(*args(2, 10, 8, 16)[:7], 8, *args(2, 10, 8, 16)[8:]) == -1 and b"aligned" in lib.pfn_last_error()
    assert lib.pfn_segpack_gather_rows(None, 4, 16, one, one, 4, 10, 4, None) == -1
    assert lib.pfn_segpack_gather_rows(one, 2, 16, one, one, 4, 10, 4, None) == -1           # ld < f
    assert lib.pfn_segpack_scatter_rows(one, 4, 10, one, one, 4, 12, 8, 4, None) == -1 and b"multiple" in lib.pfn_last_error()
    assert lib.pfn_segpack_scatter_rows(one, 4, 10, None, one, 4, 16, 8, 4, None) == -1
