"""k-hop locality analysis: counterpart of the reference's `utils/explanation.py` (`explain_epoch`, :34-114; `get_graphinfo`,
:116-123; `_make_bidirectional`, :125-137).  Plotting (`plot_*`, `subplot_*`) is not reproduced.

The reference reruns the model on the WHOLE batch once per (center bus c, hop radius m, batch), each time with the edge list cut
down to the m-hop ball around c (PyG `k_hop_subgraph(directed=False)` over `_make_bidirectional(edge_index)`), and keeps one
output row.  The output at c depends only on the ball, so here every (c, m, sample) instance is packed as a small graph of its
own and a few forwards over batches of balls replace thousands of whole-batch forwards.  The device side is csrc/khop.hip:
BFS distances and eccentricities (`pfn_khop_distances`), the size of every ball at once (`pfn_khop_histograms`) and the
packing (`pfn_khop_pack`); the model forward is the unchanged `MaskEmbdMultiMPN` (any model with its `forward(data)` surface).
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from .. import _lib as L
from ..data import Data
from ..networks.MPN import GraphCSR
from .custom_loss_functions import Masked_L2_loss

NUM_NODE_SAMPLE = 350          # centers per batch of the reference (utils/explanation.py:66)
KHOP_INF = 0xFFFF              # distance of a node that is unreachable or beyond max_hops
DEFAULT_NODE_BUDGET = 1 << 18  # nodes per packed forward


# ================================================================================================ device primitives
class KhopGraph:
    """One graph's adjacency (`pfn_graph_build` mode 1: always undirect) and the three k-hop entry points over it."""

    def __init__(self, edge_index: torch.Tensor, num_nodes: int):
        L.require_device(edge_index, what="edge_index")
        self.edge_index = edge_index.contiguous()
        self.n, self.e = int(num_nodes), int(edge_index.shape[1])
        if self.n <= 0:
            raise ValueError("k-hop analysis of a graph without nodes")
        self.graph = GraphCSR(self.edge_index, self.n, mode=1)      # validated: raises RuntimeError on an id outside [0, n)
        self.device = edge_index.device

    def distances(self, centers: torch.Tensor, max_hops: int, keep_rows: bool = True):
        """(dist, ecc): dist (C, n) int16 holding uint16 hop counts (0xFFFF = unreached / beyond max_hops), or None when
        `keep_rows` is False and a row fits in LDS; ecc (C,) int32, -1 where some node was not reached."""
        lib = L.load()
        centers = centers.to(self.device, torch.int32).contiguous()
        c = centers.numel()
        keep_rows = keep_rows or 2 * self.n > 150 * 1024
        dist = torch.empty(c, self.n, dtype=torch.int16, device=self.device) if keep_rows else None
        ecc = torch.empty(c, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            L.check(lib.pfn_khop_distances(self.graph.ws.data_ptr(), self.n, self.e, centers.data_ptr(), c, int(max_hops),
                                           L.ptr(dist), ecc.data_ptr(), L.stream_ptr()), "pfn_khop_distances")
        return dist, ecc

    def eccentricities(self, chunk: int = 8192) -> torch.Tensor:
        """All-pairs eccentricities (n,) int32 without an n x n table (rows kept only for graphs too large for LDS)."""
        out = []
        for c0 in range(0, self.n, chunk):
            centers = torch.arange(c0, min(self.n, c0 + chunk), dtype=torch.int32, device=self.device)
            out.append(self.distances(centers, min(self.n, KHOP_INF - 1), keep_rows=False)[1])
        return torch.cat(out)

    def histograms(self, dist: torch.Tensor, max_radius: int):
        """(node_count, edge_count), both (C, max_radius + 1) int32, cumulative over the radius."""
        lib = L.load()
        c = dist.shape[0]
        nc = torch.empty(c, max_radius + 1, dtype=torch.int32, device=self.device)
        ec = torch.empty_like(nc)
        with torch.cuda.device(self.device):
            L.check(lib.pfn_khop_histograms(self.graph.ws.data_ptr(), self.n, self.e, dist.data_ptr(), c, int(max_radius),
                                            nc.data_ptr(), ec.data_ptr(), L.stream_ptr()), "pfn_khop_histograms")
        return nc, ec

    def pack(self, centers: torch.Tensor, dist: torch.Tensor, inst_row, inst_radius, inst_sample, node_sizes, edge_sizes,
             err: Optional[torch.Tensor] = None):
        """Packs instances (distance row, radius, batch position) with the given sizes (from `histograms`).  Returns
        (node_ids, edge_index, edge_ids, center_pos, node_off, edge_off, err) on the device; see pfn_khop_pack."""
        lib = L.load()
        dev = self.device
        i32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int32)).to(dev)
        ns, es = np.asarray(node_sizes, dtype=np.int64), np.asarray(edge_sizes, dtype=np.int64)
        node_off, edge_off = instance_offsets(ns), instance_offsets(es)
        ni, tn, te = len(ns), int(node_off[-1]), int(edge_off[-1])
        rows, rad, smp = i32(inst_row), i32(inst_radius), i32(inst_sample)
        noff, eoff = torch.from_numpy(node_off).to(dev), torch.from_numpy(edge_off).to(dev)
        node_ids = torch.empty(tn, dtype=torch.int64, device=dev)
        edge_index = torch.empty(2, te, dtype=torch.int64, device=dev)
        edge_ids = torch.empty(te, dtype=torch.int64, device=dev)
        center_pos = torch.empty(ni, dtype=torch.int64, device=dev)
        if err is None:
            err = torch.zeros(1, dtype=torch.int32, device=dev)
        centers = centers.to(dev, torch.int32).contiguous()
        with torch.cuda.device(dev):
            L.check(lib.pfn_khop_pack(self.graph.ws.data_ptr(), self.n, self.e, self.edge_index.data_ptr(), centers.data_ptr(),
                                      dist.data_ptr(), rows.data_ptr(), rad.data_ptr(), smp.data_ptr(), noff.data_ptr(),
                                      eoff.data_ptr(), ni, te, node_ids.data_ptr(), edge_index.data_ptr(), edge_ids.data_ptr(),
                                      center_pos.data_ptr(), err.data_ptr(), L.stream_ptr()), "pfn_khop_pack")
        return node_ids, edge_index, edge_ids, center_pos, noff, eoff, err


def as_uint16(dist: torch.Tensor) -> torch.Tensor:
    """int16 distance rows as int32 hop counts (0xFFFF = unreached)."""
    return dist.to(torch.int32) & 0xFFFF


# ==================================================================================================== host planning
def instance_offsets(sizes) -> np.ndarray:
    """Exclusive offsets [len(sizes) + 1] of consecutive instances of the given sizes (int64)."""
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def saturation_radius(node_count: np.ndarray) -> np.ndarray:
    """Per center the radius from which the ball stops growing (= its eccentricity in a connected graph): the first r with
    node_count[r + 1] == node_count[r] (no node at distance r + 1, hence none farther), or R when it still grows at R.  Every
    radius beyond it gives the same instance: the ball holds every reachable node, and with them every edge among them."""
    nc = np.asarray(node_count)
    c, nr = nc.shape
    sat = np.full(c, nr - 1, dtype=np.int64)
    if nr > 1:
        flat = nc[:, 1:] == nc[:, :-1]
        has = flat.any(axis=1)
        sat[has] = flat[has].argmax(axis=1)
    return sat


class InstancePlan:
    """The unique (center row, effective radius, sample) instances of a request and their chunks.

    inst_row / inst_radius / inst_sample / node_size / edge_size: per unique instance (saturated radii folded onto the
    saturation radius); index[c, j, s]: the instance that answers (center c, radii[j], sample s); chunks: [start, stop) instance
    ranges of at most `node_budget` nodes (an instance larger than the budget is a chunk of its own)."""

    def __init__(self, node_count, edge_count, radii: Sequence[int], num_samples: int, node_budget: int):
        nc, ec = np.asarray(node_count, dtype=np.int64), np.asarray(edge_count, dtype=np.int64)
        radii = np.asarray(radii, dtype=np.int64)
        if radii.size and (radii.min() < 0 or radii.max() >= nc.shape[1]):
            raise ValueError(f"radii must lie in [0, {nc.shape[1] - 1}]")
        if node_budget <= 0:
            raise ValueError("node_budget must be positive")
        ncent, nrad, ns = nc.shape[0], radii.size, int(num_samples)
        self.sat = saturation_radius(nc)
        self.m_eff = np.minimum(radii[None, :], self.sat[:, None])                    # (C, R)
        keys = self.m_eff + (np.arange(ncent, dtype=np.int64) * nc.shape[1])[:, None]    # row * (Rmax + 1) + m_eff
        uniq, inv = np.unique(keys.reshape(-1), return_inverse=True)                     # ascending (row, m_eff)
        u_row, u_rad = uniq // nc.shape[1], uniq % nc.shape[1]
        nu = uniq.size
        self.inst_row = np.repeat(u_row, ns)                                             # instance = (unique key, sample)
        self.inst_radius = np.repeat(u_rad, ns)
        self.inst_sample = np.tile(np.arange(ns, dtype=np.int64), nu)
        self.node_size = nc[self.inst_row, self.inst_radius]
        self.edge_size = ec[self.inst_row, self.inst_radius]
        self.index = (inv.reshape(ncent, nrad)[:, :, None] * ns + np.arange(ns)[None, None, :]).astype(np.int64)
        self.node_count = nc[np.arange(ncent)[:, None], self.m_eff]                      # (C, R) ball sizes
        self.chunks = []
        start, acc = 0, 0
        for i, sz in enumerate(self.node_size.tolist()):
            if i > start and acc + sz > node_budget:
                self.chunks.append((start, i))
                start, acc = i, 0
            acc += sz
        if self.node_size.size:
            self.chunks.append((start, self.node_size.size))

    @property
    def num_instances(self) -> int:
        return int(self.node_size.size)


# ======================================================================================================= the batch
def _graph0(data):
    """(edge_index, edge rows, n) of graph 0 of a batch: nodes [0, n), the edges whose source lies there, in stored order."""
    x, ei = data.x, data.edge_index
    ptr = getattr(data, "ptr", None)
    batch = getattr(data, "batch", None)
    if torch.is_tensor(ptr) and ptr.numel() > 1:
        n = int(ptr[1] - ptr[0])
    elif torch.is_tensor(batch) and batch.numel() == x.shape[0]:
        n = int((batch == 0).sum())
    else:
        n = int(x.shape[0])
    sel = torch.nonzero(ei[0] < n).flatten()
    return ei.index_select(1, sel).contiguous(), sel, n


def _check_topology(data, ei0, n, samples):
    """The listed batch positions must hold graph 0's topology (same list, shifted by s * n): checked on the device, one sync."""
    e0, E = ei0.shape[1], data.edge_index.shape[1]
    nb = data.x.shape[0] // n if n > 0 else 0
    if n <= 0 or data.x.shape[0] != nb * n or E != nb * e0 or max(samples) >= nb or min(samples) < 0:
        raise ValueError(f"samples {list(samples)[:8]}...: the batch ({data.x.shape[0]} nodes, {E} edges) is not "
                         f"{nb} copies of graph 0's topology ({n} nodes, {e0} edges)")
    if e0 == 0:
        return
    idx = torch.as_tensor(list(samples), dtype=torch.int64, device=ei0.device)
    blocks = data.edge_index.view(2, nb, e0).index_select(1, idx)
    same = (blocks - (idx * n).view(1, -1, 1) == ei0.view(2, 1, e0)).all()
    if not bool(same):
        raise ValueError("samples must share graph 0's topology (the k-hop balls are built from graph 0's edge list)")


def _run_instances(model, data, centers, radii, samples, node_budget):
    """(out (I, F) per unique instance, plan, n): every instance's output row at its center, one forward per chunk."""
    dev = data.x.device
    L.require_device(data.x, data.edge_index, what="explanation batch")
    ei0, sel0, n = _graph0(data)
    centers = [int(c) for c in centers]
    radii = [int(r) for r in radii]
    if not centers or not radii:
        raise ValueError("need at least one center and one radius")
    if min(centers) < 0 or max(centers) >= n:
        raise ValueError(f"centers must be node ids of graph 0, in [0, {n})")
    if min(radii) < 0:
        raise ValueError("radii must be >= 0")
    use = [0] if samples is None else [int(s) for s in samples]
    if samples is not None:
        _check_topology(data, ei0, n, use)
    kg = KhopGraph(ei0, n)
    rmax = min(max(radii), KHOP_INF - 1)
    cen = torch.tensor(centers, dtype=torch.int32, device=dev)
    dist, _ = kg.distances(cen, rmax)
    nc, ec = kg.histograms(dist, rmax)
    plan = InstancePlan(nc.cpu().numpy(), ec.cpu().numpy(), [min(r, rmax) for r in radii], len(use), node_budget)
    e0 = ei0.shape[1]
    if samples is None:
        ea_of = data.edge_attr.index_select(0, sel0)                      # graph 0's rows; sample 0 only
    else:
        ea_of = data.edge_attr.view(data.x.shape[0] // n, e0, -1).index_select(0, torch.as_tensor(use, device=dev)).reshape(len(use) * e0, -1)
    use_t = torch.as_tensor(use, dtype=torch.int64)
    outs, err = [], torch.zeros(1, dtype=torch.int32, device=dev)
    was = model.training
    model.eval()
    try:
        with torch.no_grad():
            for a, b in plan.chunks:
                smp_pos = plan.inst_sample[a:b]                                # position in `use`
                node_ids, edge_index, edge_ids, center_pos, noff, eoff, err = kg.pack(
                    cen, dist, plan.inst_row[a:b], plan.inst_radius[a:b], use_t[smp_pos].numpy(), plan.node_size[a:b],
                    plan.edge_size[a:b], err)
                ni, tn, te = b - a, int(plan.node_size[a:b].sum()), int(plan.edge_size[a:b].sum())
                es = torch.from_numpy(plan.edge_size[a:b]).to(dev)
                ns = torch.from_numpy(plan.node_size[a:b]).to(dev)
                e_smp = torch.repeat_interleave(torch.from_numpy(smp_pos).to(dev), es, output_size=te)
                ea = ea_of.index_select(0, e_smp * e0 + edge_ids.remainder(max(e0, 1)))
                rows = {k: getattr(data, k).index_select(0, node_ids) for k in ("x", "y", "bus_type", "pred_mask")
                        if torch.is_tensor(getattr(data, k, None))}
                packed = Data(**rows, edge_index=edge_index, edge_attr=ea,
                              batch=torch.repeat_interleave(torch.arange(ni, device=dev), ns, output_size=tn))
                # no `ptr`: the balls differ in size, the model takes no segment hint (seg_hint = 0)
                outs.append(model(packed).index_select(0, center_pos))
    finally:
        model.train(was)
    if int(err.item()) != 0:
        raise RuntimeError("pfn_khop_pack: an instance's size disagreed with its planned offsets")
    return torch.cat(outs), plan, n


@torch.no_grad()
def khop_center_outputs(model: nn.Module, data, centers: Sequence[int], radii: Sequence[int],
                        samples: Optional[Sequence[int]] = None, node_budget: int = DEFAULT_NODE_BUDGET):
    """The model's output at each center with the edge list cut down to the center's m-hop ball, for every radius m.

    `centers`: node ids of graph 0; `radii`: hop radii (>= 0); `samples`: batch positions to evaluate (None: graph 0 only, as
    the reference).  Listed samples must share graph 0's topology (checked on the device; ValueError otherwise).  The
    (center, radius, sample) instances are packed in chunks of at most `node_budget` nodes and the UNCHANGED model forward runs
    once per chunk (eval mode, no_grad).  Radii at or beyond a center's eccentricity give the same ball: computed once and
    replicated.  Returns (out, node_counts): out (C, R, S, output_dim) on the device (S = 1 for samples=None), node_counts
    (C, R) int64 -- the reference's `subgraph_nnodes` entries."""
    out, plan, _ = _run_instances(model, data, centers, radii, samples, node_budget)
    idx = torch.from_numpy(plan.index).to(out.device)
    return out[idx], torch.from_numpy(plan.node_count.astype(np.int64))


# ===================================================================================================== graph info
def get_graphinfo(data, device=None):
    """utils/explanation.py:116-123: (num_nodes, diameter, nx_G).  The diameter is the maximum of the device eccentricities
    (all-pairs BFS, pfn_khop_distances); nx_G = networkx.from_edgelist(...) as in the reference, or None without networkx.
    Raises ValueError for a disconnected topology or isolated buses, as nx.diameter does."""
    ei = data.edge_index
    n = int(data.x.shape[0]) if getattr(data, "x", None) is not None else int(ei.max()) + 1
    try:
        import networkx as nx
        nx_G = nx.from_edgelist(ei.T.tolist())
    except ImportError:
        nx_G = None
    dev = torch.device(device) if device is not None else (ei.device if ei.is_cuda else torch.device("cuda"))
    if dev.type == "cpu":
        dev = torch.device("cuda")       # the BFS is a device kernel: there is no CPU path
    ecc = KhopGraph(ei.to(dev), n).eccentricities()
    if bool((ecc < 0).any()):
        raise ValueError("Found infinite path length because the graph is not connected (isolated buses or several components)")
    return n, int(ecc.max()), nx_G


# ================================================================================================== explain_epoch
def _initial_centers(num_nodes: int):
    """utils/explanation.py:67-70 (before the batch loop; its draw is consumed and unused)."""
    if num_nodes > 1000:
        return np.random.choice(NUM_NODE_SAMPLE, NUM_NODE_SAMPLE, replace=False).tolist()
    return np.arange(num_nodes).tolist()


def _batch_centers(num_nodes: int):
    """utils/explanation.py:82-85: a fresh draw per batch for large grids, every bus otherwise."""
    if num_nodes > 1000:
        return np.random.choice(num_nodes, NUM_NODE_SAMPLE, replace=False).tolist()
    return np.arange(num_nodes).tolist()


def sample_centers(num_nodes: int, num_batches: int):
    """The centers of `num_batches` batches, drawn from np.random in the reference's exact call sequence."""
    _initial_centers(num_nodes)
    return [_batch_centers(num_nodes) for _ in range(num_batches)]


@torch.no_grad()
def explain_epoch(model: nn.Module, loader, loss_fn: Callable, device="cpu", num_batches: int = 16, all_graphs: bool = False,
                  node_budget: int = DEFAULT_NODE_BUDGET):
    """Loss at each center bus for each k-hop ball around it (reference utils/explanation.py:34-114).

    Returns (losses / num_samples, subgraph_nnodes, nx_G) with the reference's semantics and quirks: batches 0..num_batches
    INCLUSIVE; only graph 0 of each batch is scored, weighted by len(data); centers are every bus when n <= 1000 (rows >= n of
    the 350-row tables come out NaN, 0/0) and 350 buses drawn with np.random per batch otherwise, in the reference's call
    sequence (a seeded run picks the same centers); subgraph_nnodes is counted on batch 0.

    Differences from the reference:
      * 350 < n <= 1000: the reference indexes past its 350 rows and raises; the tables here have max(350, n) rows.
      * A `Masked_L2_loss` gets the mask `data.pred_mask[c]` (the reference reads `data.x[:, 10:]`, a column range of a stale
        16-wide layout, empty for the 4-wide `x`); any other loss gets (out[c], y[c]) as in the reference.
      * m = 0 is the center with no edges (the oracle's is_directed for E == 0; the reference's indexes edge_index[0, 0]).
      * all_graphs=True (opt-in) scores every graph of each batch with weight 1: the statistic the reference approximates
        with one graph.  It needs every sample of a batch to share graph 0's topology.
    Each ball is packed as its own graph and evaluated in few forwards (khop_center_outputs), not one whole-batch forward
    per (center, radius)."""
    model.eval()
    num_nodes, diameter, nx_G = get_graphinfo(loader.dataset[0], device=device)
    _initial_centers(num_nodes)
    rows = NUM_NODE_SAMPLE if num_nodes > 1000 else max(NUM_NODE_SAMPLE, num_nodes)
    losses = torch.zeros((rows, diameter + 1))
    num_samples = torch.zeros((rows, diameter + 1))
    subgraph_nnodes = torch.zeros((rows, diameter + 1))
    radii = list(range(diameter + 1))
    masked = isinstance(loss_fn, Masked_L2_loss)
    for batch_idx, data in enumerate(loader):
        if batch_idx > num_batches:
            break
        print(f"****** [Batch {batch_idx}]: ******")
        data = data.to(device)
        centers = _batch_centers(num_nodes)
        if all_graphs:
            samples = list(range(data.x.shape[0] // num_nodes))
            weight = 1.0
        else:
            samples, weight = None, float(len(data))
        out, plan, n = _run_instances(model, data, centers, radii, samples, node_budget)
        # one loss per unique instance (saturated radii share theirs), accumulated on the device, read back once
        use = [0] if samples is None else samples
        vals = []
        for i in range(plan.num_instances):
            c = centers[int(plan.inst_row[i])]
            row = use[int(plan.inst_sample[i])] * n + c
            if masked:
                vals.append(loss_fn(out[i], data.y[row], data.pred_mask[row]))
            else:
                vals.append(loss_fn(out[i], data.y[row]))
        vals = torch.stack(vals).double().cpu().numpy()
        per = vals[plan.index]                                             # (C, D + 1, S)
        nc = len(centers)
        losses[:nc] += torch.from_numpy(per.sum(axis=2) * weight).float()
        num_samples[:nc] += per.shape[2] * weight
        if batch_idx == 0:
            subgraph_nnodes[:nc] += torch.from_numpy(plan.node_count).float()
    return (losses / num_samples), subgraph_nnodes, nx_G
