#!/usr/bin/env python3
"""DC-approximation baseline counterpart of the reference's dc_error.py (the comparison line of the paper): how far is the DC power
flow from the AC truth, in the model's own loss?  For the test split of a dataset on disk every sample's own inputs -- the slack's Vm
and Va, the PV buses' Vm and P, the PQ buses' P and Q, its lines' r and x -- are solved with `solve_power_flow(mode="dc")` on the
device (pp.rundcpp's role, dc_error.py:120), the DC table and the dataset's truth are normalised with the split's statistics, and
`Masked_L2_loss(regularize=False)` is taken per sample under the sample's prediction mask with its Vm and Q columns zeroed, as the
reference does (dc_error.py:53-56, 130).  Prints the reference's statistics lines.  The DC table's Q is NaN; under a zeroed mask
column it takes the truth's value.

    python dc_error.py --case 118 --data-dir data [--samples 1000]
"""
import argparse
import sys

import numpy as np


def load_test_split(root, case, samples=None, split=(.5, .2, .3)):
    """(the normalised test split, its raw node rows [S, n, 6], its raw edge rows [S, e, 4]) of `root`'s case, the raw rows cut to the
    first `samples`: every sample's own solver inputs, as the files hold them (speedup_evaluator.py reads them the same way)."""
    from poweflownet_amd.datasets import PowerFlowData
    testset = PowerFlowData(root=root, case=case, split=list(split), task="test")
    pair = testset._raw_pairs()[0]
    edge, node = np.load(pair[0]), np.load(pair[1])
    lens = [int(len(node) * f) for f in split]
    lo = lens[0] + lens[1]
    node, edge = node[lo:lo + lens[2]], edge[lo:lo + lens[2]]
    if samples is not None:
        node, edge = node[:samples], edge[:samples]
    if (node[:, :, 1] != node[:1, :, 1]).any():
        raise RuntimeError("dc_error: the bus types differ between the samples")
    return testset, node, edge


def solver_inputs(node, edge, device, rows=slice(None)):
    """(spec = the truth table [S, n, 4] float64, edge_index [S, 2, e] int64, rx [S, e, 2] float64) of raw rows, on `device`."""
    import torch
    truth = torch.from_numpy(node[rows, :, 2:].astype(np.float64)).to(device)
    ei = torch.from_numpy(edge[rows, :, :2].astype(np.int64).transpose(0, 2, 1).copy()).to(device)
    rx = torch.from_numpy(edge[rows, :, 2:].astype(np.float64).copy()).to(device)
    return truth, ei, rx


def dc_losses(root, case, samples=None, batch=4096, tol=1e-8, max_iter=10, device="cuda:0", split=(.5, .2, .3), route="auto"):
    """Per-sample losses (host float64 array) of the DC solve against the test split of `root`'s case; failed solves raise.  `route`:
    "auto" -- the sparse route where the case has more buses than the dense solver takes -- or "sparse".  There a split whose samples
    share one line list has one plan; a perturbed one (one list per sample) is solved in chunks that share a cover plan each
    (utils/powerflow.py CoverChunker: the file's lists are its input, the first sample's list its base)."""
    import torch
    from poweflownet_amd.datasets import PowerFlowData
    from poweflownet_amd.utils.custom_loss_functions import Masked_L2_loss
    from poweflownet_amd.utils.powerflow import CoverChunker, max_unknowns, solve_power_flow, solve_power_flow_covered, sparse_plan
    if route not in ("auto", "sparse"):
        raise ValueError(f"dc_error: route must be 'auto' or 'sparse', not {route!r}")
    testset, node, edge = load_test_split(root, case, samples, split)
    one_topology = bool((edge[:, :, :2] == edge[:1, :, :2]).all())
    if route == "auto" and node.shape[1] - 1 > max_unknowns():
        route = "sparse"
    plan = chunker = None
    mean, std = testset.xymean[0].double().to(device), testset.xystd[0].double().to(device)
    bus_type = torch.from_numpy(node[0, :, 1].astype(np.int64)).to(device)
    mask = torch.tensor(PowerFlowData.bus_type_mask)[bus_type.cpu()].clone()
    mask[:, 0] = 0
    mask[:, 3] = 0
    mask = mask.to(device)
    loss_fn = Masked_L2_loss(regularize=False)
    out = []
    for s0 in range(0, len(node), batch):
        truth, ei, rx = solver_inputs(node, edge, device, slice(s0, s0 + batch))
        if route == "sparse" and not one_topology:
            chunker = chunker or CoverChunker(bus_type, ei[0].contiguous(), "dc")
            res, _ = solve_power_flow_covered(chunker, truth, ei, rx, mode="dc", tol=tol, max_iter=max_iter)
        else:
            if route == "sparse":
                ei = ei[0].contiguous()
                plan = plan or sparse_plan(bus_type, ei, "dc")
            res = solve_power_flow(bus_type, truth, ei, rx, mode="dc", tol=tol, max_iter=max_iter, route=route, plan=plan)
        if int((res.status < 0).sum()) or int(res.flags.item()):
            raise RuntimeError(f"dc_error: {int((res.status < 0).sum())} DC solves failed (statuses {sorted(set(res.status.tolist()))})")
        dc = res.table.clone()
        dc[:, :, 3] = truth[:, :, 3]
        dc_n, truth_n = ((dc - mean) / std).float(), ((truth - mean) / std).float()
        losses = torch.stack([loss_fn(dc_n[s], truth_n[s], mask) for s in range(dc_n.shape[0])])
        out.append(losses.double().cpu().numpy())
    return np.concatenate(out) if out else np.zeros(0)


def statistics_lines(losses):
    """The reference's statistics lines (dc_error.py:144-152) of one case."""
    stats = (("Average", np.mean), ("Std", np.std), ("Max", np.max), ("Min", np.min), ("Median", np.median),
             ("25th percentile", lambda v: np.percentile(v, 25)), ("75th percentile", lambda v: np.percentile(v, 75)),
             ("95th percentile", lambda v: np.percentile(v, 95)), ("99th percentile", lambda v: np.percentile(v, 99)))
    return [f"{name} losses: {fn(losses)}" for name, fn in stats]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--case", default="118")
    ap.add_argument("--data-dir", default="data")
    ap.add_argument("--samples", type=int, default=None, help="only the first N samples of the test split")
    ap.add_argument("--batch", type=int, default=4096, help="samples per device launch")
    ap.add_argument("--split", type=float, nargs=3, default=[.5, .2, .3], help="train / val / test fractions (the reference's .5 .2 .3)")
    ap.add_argument("--route", default="auto", choices=("auto", "sparse"),
                    help="solver route: auto takes the sparse one where the case exceeds the dense solver; sparse forces it")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dc_error.py needs a HIP device: poweflownet_amd has no CPU solver")
    losses = dc_losses(a.data_dir, a.case, a.samples, a.batch, split=tuple(a.split), route=a.route)
    print(f"Case {a.case} done: {len(losses)} samples")
    for line in statistics_lines(losses):
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
