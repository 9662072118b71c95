#!/usr/bin/env python3
"""Wall time of the k-hop locality analysis (poweflownet_amd/utils/explanation.py), not part of bench.py:

  * explain_epoch at synthetic case118v2 x 128, num_batches=16 (17 batches: the reference's bound is inclusive);
  * explain_epoch at synthetic 6470rte x 64, num_batches=1;
  * the reference-style loop on this package -- one whole-batch forward per (center, radius) with the bidirectional edge list
    filtered to the ball (PyG k_hop_subgraph(directed=False) restated in torch on the device) -- timed over its first
    instances and extrapolated to the same workload.

    python tools/explain_bench.py [--ref-instances 24] [--node-budget N]

Prints one JSON line.  Model: MaskEmbdMultiMPN at configs/standard.json (hidden 129, 4 layers, K 3), random weights, eval."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from poweflownet_amd.data import Data, DataLoader  # noqa: E402
from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN  # noqa: E402
from poweflownet_amd.synth import make_dataset  # noqa: E402
from poweflownet_amd.utils.custom_loss_functions import Masked_L2_loss  # noqa: E402
from poweflownet_amd.utils.explanation import DEFAULT_NODE_BUDGET, explain_epoch, get_graphinfo  # noqa: E402


def _ball_edge_mask(center, m, bi, num_nodes):
    """k_hop_subgraph(center, m, bi, directed=False)'s edge mask, on the device."""
    col, row = bi
    node_mask = torch.zeros(num_nodes, dtype=torch.bool, device=bi.device)
    frontier = torch.tensor([center], device=bi.device)
    reached = [frontier]
    for _ in range(m):
        node_mask.fill_(False)
        node_mask[reached[-1]] = True
        reached.append(col[node_mask[row]])
    node_mask.fill_(False)
    node_mask[torch.cat(reached)] = True
    return node_mask[row] & node_mask[col]


def reference_style_seconds_per_instance(model, data, loss_fn, diameter, count):
    """Seconds per (center, radius) of the reference's loop on this package: full-batch forward on the filtered list."""
    n0 = int(data.ptr[1])
    bi = torch.cat([data.edge_index, data.edge_index.flip([0])], dim=1)
    bi_attr = torch.cat([data.edge_attr, data.edge_attr], dim=0)
    done, t0 = 0, None
    for c in range(n0):
        for m in range(diameter + 1):
            if done == 2:                       # two warm-up instances
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            mask = _ball_edge_mask(c, m, bi, data.x.shape[0])
            d = Data(x=data.x, y=data.y, bus_type=data.bus_type, pred_mask=data.pred_mask, edge_index=bi[:, mask],
                     edge_attr=bi_attr[mask], batch=data.batch)
            out = model(d)
            loss_fn(out[c], data.y[c], data.pred_mask[c]).item()
            done += 1
            if done == count + 2:
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / count
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / max(done - 2, 1)


def run_case(case, batch_size, num_batches, model, loss_fn, ref_instances, node_budget, device):
    dataset = make_dataset(case, batch_size * (num_batches + 1), seed=0)
    loader = DataLoader(dataset, batch_size=batch_size)
    n, diameter, _ = get_graphinfo(dataset[0], device=device)
    np.random.seed(0)
    explain_epoch(model, DataLoader(dataset[:batch_size], batch_size=batch_size), loss_fn, device=device, num_batches=0,
                  node_budget=node_budget)                                         # warm-up (allocator, kernel attributes)
    torch.cuda.synchronize()
    np.random.seed(0)
    t0 = time.perf_counter()
    losses, nnodes, _ = explain_epoch(model, loader, loss_fn, device=device, num_batches=num_batches, node_budget=node_budget)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    centers = 350 if n > 1000 else n
    instances = centers * (diameter + 1) * (num_batches + 1)
    first = next(iter(loader)).to(device)
    per = reference_style_seconds_per_instance(model, first, loss_fn, diameter, ref_instances)
    return {"case": case, "batch_size": batch_size, "num_batches": num_batches, "nodes": n, "diameter": diameter,
            "explain_epoch_s": round(wall, 3), "reference_style_instances": instances,
            "reference_style_s_per_instance": round(per, 6), "reference_style_extrapolated_s": round(per * instances, 1),
            "speedup": round(per * instances / wall, 1), "finite_rows": int(torch.isfinite(losses).all(dim=1).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-instances", type=int, default=24)
    ap.add_argument("--node-budget", type=int, default=DEFAULT_NODE_BUDGET)
    ap.add_argument("--cases", default="118v2:128:16,6470rte:64:1")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("explain_bench.py needs a HIP device")
    device = torch.device("cuda")
    torch.manual_seed(0)
    model = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.2).to(device).eval()
    loss_fn = Masked_L2_loss(regularize=False)
    rows = []
    for spec in args.cases.split(","):
        case, bs, nb = spec.split(":")
        rows.append(run_case(case, int(bs), int(nb), model, loss_fn, args.ref_instances, args.node_budget, device))
    print(json.dumps({"explain_bench": rows}))


if __name__ == "__main__":
    main()
