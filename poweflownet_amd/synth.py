"""Synthetic power-grid batches with the tensor layout of `datasets/PowerFlowData.py:171-217`.

No dataset files exist on the target image (and pandapower is absent), so tests and bench.py use
topologies generated as SURVEY.md 8(d) specifies: a random spanning tree (node i attaches to a
uniform j < i, stored parent -> child) plus uniform random chords (self-loops rejected, parallel
edges allowed), one stored edge per branch; bus types / masks follow `datasets/PowerFlowData.py:71-74`.
"""
from __future__ import annotations

import numpy as np
import torch

from .data import Batch, Data

CASES = {"14": (14, 20), "118": (118, 186), "118v2": (118, 186), "6470rte": (6470, 9005)}

# bus_type -> which of (Vm, Va, P, Q) must be predicted; datasets/PowerFlowData.py:71-74
_MASK_TABLE = torch.tensor([[0, 0, 1, 1],      # slack
                            [0, 1, 0, 1],      # PV
                            [1, 1, 0, 0]],     # PQ
                           dtype=torch.long)


def make_topology(n: int, e: int, seed: int = 0, hub_frac: float = 0.0) -> torch.Tensor:
    """(2, e) int64 stored-once edge list, connected.  `hub_frac` > 0 routes that fraction of the
    chords into n/1000 hub nodes (high-degree buses, max degree >= 64 on 6470rte, for the LDS tile sizing case)."""
    if e < n - 1:
        raise ValueError("need at least n-1 edges for a connected grid")
    rng = np.random.default_rng(seed)
    src = np.empty(e, dtype=np.int64)
    dst = np.empty(e, dtype=np.int64)
    for i in range(1, n):
        src[i - 1] = rng.integers(0, i)
        dst[i - 1] = i
    hubs = rng.choice(n, size=max(1, n // 1000), replace=False) if hub_frac > 0 else None
    k = n - 1
    while k < e:
        a = int(rng.integers(0, n))
        if hubs is not None and rng.random() < hub_frac:
            b = int(hubs[rng.integers(0, len(hubs))])
        else:
            b = int(rng.integers(0, n))
        if a == b:
            continue
        src[k], dst[k] = a, b
        k += 1
    return torch.from_numpy(np.stack([src, dst]))


def make_graph(n: int, e: int, seed: int = 0, topo_seed: int = 0, hub_frac: float = 0.0,
               edge_index: torch.Tensor | None = None) -> Data:
    """One normalised sample: y ~ N(0,1); x = y * (1 - mask); edge_attr ~ N(0,1)."""
    if edge_index is None:
        edge_index = make_topology(n, e, topo_seed, hub_frac)
    g = torch.Generator().manual_seed(seed)
    bus_type = torch.full((n,), 2, dtype=torch.long)
    bus_type[::3] = 1
    bus_type[0] = 0
    pred_mask = _MASK_TABLE[bus_type]
    y = torch.randn(n, 4, generator=g)
    x = y * (1 - pred_mask).float()
    edge_attr = torch.randn(edge_index.shape[1], 2, generator=g)
    return Data(x=x, y=y, bus_type=bus_type, pred_mask=pred_mask, edge_index=edge_index, edge_attr=edge_attr)


def make_batch(case: str, batch_size: int, seed: int = 0, hub_frac: float = 0.0, first: int = 0) -> Batch:
    """`batch_size` samples of one case sharing a topology (as every sample of a reference case does),
    collated exactly like the loader would."""
    n, e = CASES[str(case)]
    topo = make_topology(n, e, 0, hub_frac)
    return Batch.from_data_list([make_graph(n, e, seed=seed * 1_000_003 + first + b, edge_index=topo)
                                 for b in range(batch_size)])


def make_physical_inputs(n: int, e: int, num_samples: int, seed: int, load: float = 0.2):
    """Inputs of `utils.powerflow.solve_power_flow` that a power-flow solution exists for: `make_topology(n, e)`'s grid with
    `make_graph`'s bus types, per-unit, demand-positive.  Returns (edge_index [2, e] int64, bus_type [n] int64, rx [S, e, 2] float64,
    spec [S, n, 4] float64 = (Vm, Va in degrees, P, Q) with the entries a bus type does not give left 0).  One
    `np.random.default_rng(seed)` serves the samples one after the other, each drawing in this order: r ~ U(0.005, 0.03),
    x ~ U(0.03, 0.15) per line; Vm ~ U(1.00, 1.05) at the slack and the PV buses; P ~ N(load, 0.1 load) and
    Q ~ N(load / 4, 0.1 load / 4) at the PQ buses; P = -sum(P_pq) / n_pv * U(0.8, 1.2) at the PV buses; the slack's Va is 0.  The
    reference generator's +-20 % / 10 % perturbations (dataset_generator.py) around a made-up base case."""
    edge_index = make_topology(n, e)
    bus_type = torch.full((n,), 2, dtype=torch.long)
    bus_type[::3] = 1
    bus_type[0] = 0
    bt = bus_type.numpy()
    fixed_v, pv, pq = np.flatnonzero(bt != 2), np.flatnonzero(bt == 1), np.flatnonzero(bt == 2)
    rng = np.random.default_rng(seed)
    rx = np.empty((num_samples, e, 2), dtype=np.float64)
    spec = np.zeros((num_samples, n, 4), dtype=np.float64)
    for s in range(num_samples):
        rx[s, :, 0] = rng.uniform(0.005, 0.03, e)
        rx[s, :, 1] = rng.uniform(0.03, 0.15, e)
        spec[s, fixed_v, 0] = rng.uniform(1.00, 1.05, fixed_v.size)
        spec[s, pq, 2] = rng.normal(load, 0.1 * load, pq.size)
        spec[s, pq, 3] = rng.normal(load / 4, 0.1 * load / 4, pq.size)
        if pv.size:
            spec[s, pv, 2] = -spec[s, pq, 2].sum() / pv.size * rng.uniform(0.8, 1.2, pv.size)
    return edge_index, bus_type, torch.from_numpy(rx), torch.from_numpy(spec)


def make_dataset(case: str, num_samples: int, seed: int = 0):
    n, e = CASES[str(case)]
    topo = make_topology(n, e, 0)
    return [make_graph(n, e, seed=seed * 1_000_003 + s, edge_index=topo) for s in range(num_samples)]
