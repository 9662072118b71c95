"""k-hop locality analysis on the device (csrc/khop.hip, poweflownet_amd/utils/explanation.py) against CPU restatements:
networkx BFS for the distances, PyG's k_hop_subgraph(directed=False) over _make_bidirectional for the packed balls, and the
float64 CPU oracle run the reference's way (whole batch, filtered edge list) for the center outputs and explain_epoch."""
import copy

import networkx as nx
import numpy as np
import pytest
import torch

from oracle import ref_cpu
from poweflownet_amd.data import Batch, Data, DataLoader
from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
from poweflownet_amd.synth import make_graph, make_topology
from poweflownet_amd.utils.custom_loss_functions import Masked_L2_loss
from poweflownet_amd.utils.explanation import (KhopGraph, as_uint16, explain_epoch, get_graphinfo, instance_offsets,
                                               khop_center_outputs)
from tests.util import assert_close, record_elementwise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _nx_graph(ei, n):
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(ei.T.tolist())
    return g


def _topology(kind):
    n, e, hub, sym = {"14": (14, 20, 0.0, False), "118": (118, 186, 0.0, False), "6470rte": (6470, 9005, 0.0, False),
                      "6470hub": (6470, 9005, 0.5, False), "118sym": (118, 186, 0.0, True)}[kind]
    ei = make_topology(n, e, seed=3, hub_frac=hub)
    if sym:                                   # a list that already holds both directions (the undirect step doubles it again)
        ei = torch.cat([ei, ei.flip(0)], dim=1)
    return ei, n


# --------------------------------------------------------------------------------------------------- 1. distances
@pytest.mark.parametrize("kind", ["14", "118", "118sym", "6470rte", "6470hub"])
def test_distances_match_networkx_bfs(kind):
    ei, n = _topology(kind)
    g = _nx_graph(ei, n)
    if kind == "6470hub":
        assert max(d for _, d in g.degree()) >= 64
    kg = KhopGraph(ei.to(DEV), n)
    rng = np.random.default_rng(0)
    centers = np.arange(n) if n <= 200 else rng.choice(n, 48, replace=False)
    dist, ecc = kg.distances(torch.tensor(centers, dtype=torch.int32), 65534)
    dist = as_uint16(dist).cpu().numpy()
    capped, _ = kg.distances(torch.tensor(centers, dtype=torch.int32), 2)
    capped = as_uint16(capped).cpu().numpy()
    for i, c in enumerate(centers.tolist()):
        want = np.full(n, 0xFFFF)
        for v, d in nx.single_source_shortest_path_length(g, c).items():
            want[v] = d
        assert (dist[i] == want).all(), (kind, c)
        assert ecc[i].item() == want.max()
        assert (capped[i] == np.where(want <= 2, want, 0xFFFF)).all()
    if n <= 200:
        assert get_graphinfo(type("D", (), {"x": torch.zeros(n, 4), "edge_index": ei})(), device=DEV)[1] == nx.diameter(g)
        assert int(kg.eccentricities().max()) == nx.diameter(g)


def test_graphinfo_diameter_and_disconnected_graphs():
    ei, n = _topology("118")
    d = make_graph(n, ei.shape[1], edge_index=ei)
    num_nodes, diameter, g = get_graphinfo(d, device=DEV)
    assert num_nodes == 118 and diameter == nx.diameter(nx.from_edgelist(ei.T.tolist())) and g.number_of_nodes() == 118
    two = torch.tensor([[0, 1, 3], [1, 2, 4]])                          # two components
    with pytest.raises(ValueError):
        get_graphinfo(type("D", (), {"x": torch.zeros(5, 4), "edge_index": two})(), device=DEV)
    iso = torch.tensor([[0, 1], [1, 2]])                                # bus 3 isolated
    with pytest.raises(ValueError):
        get_graphinfo(type("D", (), {"x": torch.zeros(4, 4), "edge_index": iso})(), device=DEV)
    kg = KhopGraph(torch.zeros(2, 0, dtype=torch.int64, device=DEV), 3)  # no edges at all
    dist, ecc = kg.distances(torch.tensor([0, 2], dtype=torch.int32), 10)
    assert ecc.tolist() == [-1, -1] and as_uint16(dist).tolist() == [[0, 0xFFFF, 0xFFFF], [0xFFFF, 0xFFFF, 0]]


# ---------------------------------------------------------------------------------------------------- 2. packing
def _k_hop_subgraph(node_idx, num_hops, edge_index, num_nodes):
    """torch_geometric.utils.k_hop_subgraph(node_idx, num_hops, edge_index, relabel_nodes=False, num_nodes, directed=False,
    flow='source_to_target'), restated: (subset, edge_mask)."""
    col, row = edge_index
    node_mask = torch.zeros(num_nodes, dtype=torch.bool)
    subsets = [torch.tensor([node_idx])]
    for _ in range(num_hops):
        node_mask.fill_(False)
        node_mask[subsets[-1]] = True
        edge_mask = node_mask[row]
        subsets.append(col[edge_mask])
    subset = torch.cat(subsets).unique()
    node_mask.fill_(False)
    node_mask[subset] = True
    return subset, node_mask[row] & node_mask[col]


def _make_bidirectional(edge_index):
    return torch.cat([edge_index, edge_index.flip([0])], dim=1)


@pytest.mark.parametrize("kind", ["14", "118sym", "6470hub"])
def test_pack_matches_k_hop_subgraph(kind):
    ei, n = _topology(kind)
    kg = KhopGraph(ei.to(DEV), n)
    rng = np.random.default_rng(1)
    centers = rng.choice(n, 6, replace=False).tolist()
    cen = torch.tensor(centers, dtype=torch.int32)
    _, ecc = kg.distances(cen, 65534)
    ecc = ecc.tolist()
    rmax = max(ecc) + 2
    dist, _ = kg.distances(cen, rmax)
    nc, ec = (t.cpu().numpy() for t in kg.histograms(dist, rmax))
    inst = []                                                  # (row, radius, sample): m = 0, a few inside, m = ecc, m > ecc
    for r, c in enumerate(centers):
        for m in sorted({0, 1, min(3, ecc[r]), ecc[r] // 2, ecc[r], ecc[r] + 2}):
            inst.append((r, m, int(rng.integers(0, 3))))
    rows, rad, smp = (np.array(v) for v in zip(*inst))
    ns, es = nc[rows, rad], ec[rows, rad]
    node_ids, pei, eids, cpos, noff, eoff, err = kg.pack(cen, dist, rows, rad, smp, ns, es)
    assert err.item() == 0
    node_ids, pei, eids, cpos = node_ids.cpu(), pei.cpu(), eids.cpu(), cpos.cpu()
    assert noff.cpu().tolist() == instance_offsets(ns).tolist()
    bi = _make_bidirectional(ei)
    for i, (r, m, s) in enumerate(inst):
        subset, emask = _k_hop_subgraph(centers[r], m, bi, n)
        a, b = int(noff[i]), int(noff[i + 1])
        assert node_ids[a:b].tolist() == (subset + s * n).tolist(), (kind, inst[i])
        want_ids = torch.nonzero(emask).flatten()
        ea, eb = int(eoff[i]), int(eoff[i + 1])
        assert eids[ea:eb].tolist() == want_ids.tolist()
        relabel = torch.full((n,), -1, dtype=torch.int64)
        relabel[subset] = torch.arange(subset.numel()) + a
        assert pei[:, ea:eb].tolist() == relabel[bi[:, emask]].tolist()
        assert int(cpos[i]) == a + int((subset == centers[r]).nonzero())
        if m >= ecc[r]:
            assert b - a == n                                  # saturated: the whole (connected) graph


def test_pack_graph_without_edges():
    kg = KhopGraph(torch.zeros(2, 0, dtype=torch.int64, device=DEV), 1)
    cen = torch.tensor([0], dtype=torch.int32)
    dist, ecc = kg.distances(cen, 4)
    assert ecc.tolist() == [0]
    nc, ec = kg.histograms(dist, 4)
    assert nc.tolist() == [[1] * 5] and ec.tolist() == [[0] * 5]
    node_ids, pei, eids, cpos, _, _, err = kg.pack(cen, dist, [0, 0], [0, 4], [0, 2], [1, 1], [0, 0])
    assert err.item() == 0 and node_ids.tolist() == [0, 2] and pei.shape == (2, 0) and cpos.tolist() == [0, 1]


# ----------------------------------------------------------------------------------------- 3. outputs vs oracle
def _models(hidden=12, layers=2, K=2, seed=7):
    torch.manual_seed(seed)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, hidden, layers, K, 0.0).eval()
    model = MaskEmbdMultiMPN(4, 2, 4, hidden, layers, K, 0.0)
    model.load_state_dict(ref.state_dict())
    return model.to(DEV).eval(), copy.deepcopy(ref).double().eval()


def _grid_batch(n, e, samples, seed=0, hub_frac=0.0):
    topo = make_topology(n, e, seed=5, hub_frac=hub_frac)
    return Batch.from_data_list([make_graph(n, e, seed=seed * 1000 + s, edge_index=topo) for s in range(samples)])


def _oracle_ball_output(ref64, batch, center, m, n):
    """The reference's way: the WHOLE batch, the bidirectional list filtered to the ball's edges, not relabelled."""
    bi = _make_bidirectional(batch.edge_index)
    bi_attr = torch.cat([batch.edge_attr, batch.edge_attr.clone()], dim=0)
    _, emask = _k_hop_subgraph(center, m, bi, batch.x.shape[0])
    d = type(batch)(x=batch.x.double(), y=batch.y.double(), pred_mask=batch.pred_mask, bus_type=batch.bus_type,
                    edge_index=bi[:, emask], edge_attr=bi_attr[emask].double(), batch=batch.batch)
    with torch.no_grad():
        return ref64(d)[center]


def test_center_outputs_match_oracle_on_large_grid():
    n, e = 1200, 1750
    batch = _grid_batch(n, e, 2)
    model, ref64 = _models()
    g = _nx_graph(make_topology(n, e, seed=5), n)
    rng = np.random.default_rng(2)
    centers = rng.choice(n, 5, replace=False).tolist()
    ecc = [max(nx.single_source_shortest_path_length(g, c).values()) for c in centers]
    radii = [0, 1, 3, 6, max(ecc) + 1]
    out, counts = khop_center_outputs(model, batch.to(DEV), centers, radii, node_budget=3000)
    assert out.shape == (5, len(radii), 1, 4)
    got, want = [], []
    for i, c in enumerate(centers):
        for j, m in enumerate(radii):
            assert counts[i, j] == sum(1 for d in nx.single_source_shortest_path_length(g, c).values() if d <= m)
            if m <= 6 or i < 2:                                  # the full-graph radius for two centers (oracle cost)
                got.append(out[i, j, 0].cpu())
                want.append(_oracle_ball_output(ref64, batch, c, m, n))
    got, want = torch.stack(got), torch.stack(want)
    assert_close(got, want, what="k-hop center outputs vs fp64 oracle")
    bad, total, worst = record_elementwise(got, want, "k-hop center outputs vs fp64 oracle")
    assert bad <= 1e-3 * total and worst <= 4.0, (bad, total, worst)


# ------------------------------------------------------------------------------------------- 4. explain_epoch
def _reference_explain_epoch(ref64, loader, num_nodes, diameter, num_batches):
    """utils/explanation.py:34-114 restated on the float64 oracle, with this package's two documented differences: the mask
    of Masked_L2_loss is pred_mask[c], m = 0 runs with no edges.  Rows: max(350, n) for n <= 1000."""
    rows = 350 if num_nodes > 1000 else max(350, num_nodes)
    if num_nodes > 1000:
        np.random.choice(350, 350, replace=False)
    losses = torch.zeros((rows, diameter + 1), dtype=torch.float64)
    num_samples = torch.zeros((rows, diameter + 1), dtype=torch.float64)
    nnodes = torch.zeros((rows, diameter + 1))
    for batch_idx, data in enumerate(loader):
        if batch_idx > num_batches:
            break
        sampled = np.random.choice(num_nodes, 350, replace=False).tolist() if num_nodes > 1000 else list(range(num_nodes))
        bi = _make_bidirectional(data.edge_index)
        for k, c in enumerate(sampled):
            for m in range(diameter + 1):
                subset, _ = _k_hop_subgraph(c, m, bi, data.x.shape[0])
                out = _oracle_ball_output(ref64, data, c, m, num_nodes)
                loss = ref_cpu.masked_l2_loss(out, data.y[c].double(), data.pred_mask[c], regularize=False)
                losses[k, m] += loss.item() * len(data)
                num_samples[k, m] += len(data)
                if batch_idx == 0:
                    nnodes[k, m] += subset.shape[0]
    return losses / num_samples, nnodes


def test_explain_epoch_matches_reference_loop():
    n, e = 14, 20
    topo = make_topology(n, e, seed=3)
    dataset = [make_graph(n, e, seed=s, edge_index=topo) for s in range(10)]
    loader = DataLoader(dataset, batch_size=4)
    model, ref64 = _models(hidden=16, layers=3, K=2)
    loss_fn = Masked_L2_loss(regularize=False)
    losses, nnodes, g = explain_epoch(model, loader, loss_fn, device=DEV, num_batches=1)
    diameter = nx.diameter(nx.from_edgelist(topo.T.tolist()))
    assert losses.shape == (350, diameter + 1) and g.number_of_nodes() == n
    want, want_nn = _reference_explain_epoch(ref64, loader, n, diameter, 1)
    assert torch.equal(nnodes, want_nn)
    assert torch.isnan(losses[n:]).all() and not torch.isnan(losses[:n]).any()
    assert_close(losses[:n], want[:n], what="explain_epoch losses vs reference loop on fp64 oracle")
    bad, total, worst = record_elementwise(losses[:n], want[:n], "explain_epoch losses vs reference loop on fp64 oracle")
    assert bad <= 1e-3 * total and worst <= 4.0, (bad, total, worst)


def test_explain_epoch_large_grid_draws_the_reference_centers():
    n, e = 1200, 1750
    topo = make_topology(n, e, seed=5)
    dataset = [make_graph(n, e, seed=s, edge_index=topo) for s in range(2)]
    loader = DataLoader(dataset, batch_size=1)
    model, _ = _models(hidden=8)
    g = _nx_graph(topo, n)
    diameter = nx.diameter(g)
    np.random.seed(42)
    losses, nnodes, _ = explain_epoch(model, loader, Masked_L2_loss(regularize=False), device=DEV, num_batches=0)
    np.random.seed(42)
    np.random.choice(350, 350, replace=False)
    centers = np.random.choice(n, 350, replace=False).tolist()
    assert losses.shape == (350, diameter + 1) and not torch.isnan(losses).any()
    for k in (0, 1, 100, 349):
        lengths = nx.single_source_shortest_path_length(g, centers[k])
        assert nnodes[k].tolist() == [sum(1 for d in lengths.values() if d <= m) for m in range(diameter + 1)]


# ------------------------------------------------------------------------------------ 5. determinism, replication
def test_runs_are_bit_identical_and_saturated_radii_replicate():
    batch = _grid_batch(118, 186, 4, seed=3).to(DEV)
    model, _ = _models(hidden=16, layers=3, K=3)
    centers = list(range(0, 118, 7))
    g = _nx_graph(batch.edge_index[:, :186].cpu(), 118)
    ecc = [max(nx.single_source_shortest_path_length(g, c).values()) for c in centers]
    radii = list(range(max(ecc) + 3))
    a, ca = khop_center_outputs(model, batch, centers, radii, samples=[0, 1, 2, 3], node_budget=700)
    b, cb = khop_center_outputs(model, batch, centers, radii, samples=[0, 1, 2, 3], node_budget=700)
    assert torch.equal(a, b) and torch.equal(ca, cb)
    for i, ec in enumerate(ecc):
        for m in radii[ec + 1:]:
            assert torch.equal(a[i, m], a[i, ec])
            assert ca[i, m] == 118
    # every sample on its own (a batch of one graph) gives the same rows
    for s in range(4):
        single = Batch.from_data_list([_sample(batch.to("cpu"), s, 118, 186)])
        o, _ = khop_center_outputs(model, single.to(DEV), centers, radii)
        assert_close(a[:, :, s], o[:, :, 0], what=f"k-hop outputs: sample {s} of a batch vs on its own")


def _sample(batch, s, n, e):
    sl = slice(s * n, (s + 1) * n)
    return Data(x=batch.x[sl], y=batch.y[sl], bus_type=batch.bus_type[sl], pred_mask=batch.pred_mask[sl],
                edge_index=batch.edge_index[:, s * e:(s + 1) * e] - s * n, edge_attr=batch.edge_attr[s * e:(s + 1) * e])


def test_all_graphs_equals_scoring_each_sample_alone():
    n, e = 14, 20
    topo = make_topology(n, e, seed=4)
    dataset = [make_graph(n, e, seed=100 + s, edge_index=topo) for s in range(4)]
    model, _ = _models(hidden=16, layers=2, K=3)
    loss_fn = Masked_L2_loss(regularize=False)
    all_l, all_nn, _ = explain_epoch(model, DataLoader(dataset, batch_size=4), loss_fn, device=DEV, num_batches=0, all_graphs=True)
    one_l, one_nn, _ = explain_epoch(model, DataLoader(dataset, batch_size=1), loss_fn, device=DEV, num_batches=3)
    assert torch.equal(all_nn, one_nn)
    assert_close(all_l[:n], one_l[:n], what="explain_epoch all_graphs vs one sample per batch")
    other = make_topology(n, e, seed=9)                       # a sample with another topology is refused
    mixed = Batch.from_data_list([dataset[0], make_graph(n, e, seed=1, edge_index=other)]).to(DEV)
    with pytest.raises(ValueError):
        khop_center_outputs(model, mixed, [0], [0, 1], samples=[0, 1])
