#!/usr/bin/env python3
"""Dataset generator counterpart of the reference's dataset_generator.py: perturbed power-flow problems on a case's grid, solved,
written as the raw files `PowerFlowData` (and train.py --data-dir) load unchanged.  The reference perturbs a pandapower case and
calls pp.runpp per sample; here the problems come from `synth.make_physical_inputs` (the same +-20 % / 10 % perturbation style around
a made-up per-unit base on the synthetic grid of the case's size) and are solved in device batches by `solve_power_flow`
(csrc/powerflow.hip: Newton-Raphson, one workgroup per sample).  A sample whose status is negative is drawn again -- the
reference's `continue` -- and counted.

    python dataset_generator.py --case 118 --samples 2000 --root data

    <root>/raw/case<case>_node_features.npy   (S, n, 6) float64 [index, type, Vm, Va (degrees), P, Q]
    <root>/raw/case<case>_edge_features.npy   (S, e, 4) float64 [from, to, r, x]

Per-unit, demand-positive, the network model of `PowerImbalance` (no shunts, taps, line charging or Q-limits).  The reference's
topology perturbation (-r / -a) is not here.  Needs a HIP device: there is no CPU solver in this package."""
import argparse
import os
import sys

import numpy as np

GENERATOR_CASES = ("14", "118", "118v2")


def write_raw(root, case, bus_type, edge_index, rx, tables):
    """Write solved tables [S, n, 4] with their line parameters [S, e, 2] in the reference's raw layout; returns the two paths."""
    bus_type, edge_index = np.asarray(bus_type), np.asarray(edge_index)
    rx, tables = np.asarray(rx, dtype=np.float64), np.asarray(tables, dtype=np.float64)
    S, n, e = tables.shape[0], tables.shape[1], edge_index.shape[1]
    assert tables.shape == (S, n, 4) and rx.shape == (S, e, 2) and edge_index.shape == (2, e) and bus_type.shape == (n,)
    node = np.empty((S, n, 6), dtype=np.float64)
    node[:, :, 0] = np.arange(n)
    node[:, :, 1] = bus_type
    node[:, :, 2:] = tables
    edge = np.empty((S, e, 4), dtype=np.float64)
    edge[:, :, :2] = edge_index.T
    edge[:, :, 2:] = rx
    os.makedirs(os.path.join(root, "raw"), exist_ok=True)
    paths = (os.path.join(root, "raw", f"case{case}_node_features.npy"), os.path.join(root, "raw", f"case{case}_edge_features.npy"))
    np.save(paths[0], node)
    np.save(paths[1], edge)
    return paths


def generate(case, samples, seed=0, batch=4096, load=0.2, tol=1e-8, max_iter=10, device="cuda:0", max_rounds=64):
    """(bus_type [n], edge_index [2, e], rx [S, e, 2], tables [S, n, 4], redrawn): `samples` converged samples, host arrays."""
    import torch
    from poweflownet_amd.synth import CASES, make_physical_inputs
    from poweflownet_amd.utils.powerflow import solve_power_flow
    if samples < 1:
        raise ValueError("dataset_generator: --samples must be at least 1")
    n, e = CASES[str(case)]
    keep_rx, keep_t, have, redrawn = [], [], 0, 0
    for rnd in range(max_rounds):
        if have >= samples:
            break
        want = min(batch, samples - have)
        ei, bt, rx, spec = make_physical_inputs(n, e, want, seed * 1_000_003 + rnd, load)
        res = solve_power_flow(bt.to(device), spec.to(device), ei.to(device), rx.to(device), tol=tol, max_iter=max_iter)
        ok = (res.status >= 0).cpu().numpy()
        if int(res.flags.item()) != 0:
            raise RuntimeError("dataset_generator: the solver flagged its bus types")
        keep_rx.append(rx.numpy()[ok])
        keep_t.append(res.table.cpu().numpy()[ok])
        have += int(ok.sum())
        redrawn += int((~ok).sum())
    if have < samples:
        raise RuntimeError(f"dataset_generator: only {have} of {samples} samples converged in {max_rounds} rounds (load {load})")
    return bt.numpy(), ei.numpy(), np.concatenate(keep_rx)[:samples], np.concatenate(keep_t)[:samples], redrawn


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--case", default="118", choices=GENERATOR_CASES)
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--root", default="data")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=4096, help="samples per device launch")
    ap.add_argument("--load", type=float, default=0.2, help="mean active demand of a PQ bus, per-unit")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dataset_generator.py needs a HIP device: poweflownet_amd has no CPU solver")
    bt, ei, rx, tables, redrawn = generate(a.case, a.samples, a.seed, a.batch, a.load)
    paths = write_raw(a.root, a.case, bt, ei, rx, tables)
    print(f"Failed to converge and drawn again: {redrawn}")
    print(f"wrote {a.samples} samples of case{a.case} ({tables.shape[1]} buses, {ei.shape[1]} lines): {paths[0]}, {paths[1]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
