#!/usr/bin/env python3
"""Dataset generator counterpart of the reference's dataset_generator.py: perturbed power-flow problems on a case's grid, solved,
written as the raw files `PowerFlowData` (and train.py --data-dir) load unchanged.  The reference perturbs a pandapower case and
calls pp.runpp per sample; here the problems come from `synth.make_physical_inputs` (the same +-20 % / 10 % perturbation style around
a made-up per-unit base on the synthetic grid of the case's size) and are solved in device batches by `solve_power_flow`
(csrc/powerflow.hip: Newton-Raphson, one workgroup per sample).  A sample whose status is negative is drawn again -- the
reference's `continue` -- and counted.  A case with more unknowns than the dense solver takes (6470rte: 10782) goes through the
sparse route (csrc/powerflow_sparse.hip): its plan is built once and serves every device batch and redraw; --route sparse forces
that route at any size.  With -r / -a every sample has its own topology: the sparse route then solves the samples in chunks
that share one plan each, built on the chunk's cover list -- the base lines and the lines any of its samples adds -- with a
per-sample line mask (utils/powerflow.py cover_plan, CoverChunker); the chunk size follows the fill the added lines cost.
--enforce-q-lims, the reference's ENFORCE_Q_LIMS (`pp.runpp(..., enforce_q_lims=True)`): a PV bus whose reactive output hits a limit
becomes a load bus and the sample is solved again -- inside the one launch of `solve_power_flow_qlim` (csrc/powerflow_qlim.hip) --
and is written as type 2 for THAT sample, as the reference writes it.  The synthetic cases carry no generator data, so --q-limit Q
(per-unit, > 0) puts (-Q, +Q) on every PV bus.  With and without -r / -a; a case beyond the dense solver (6470rte) takes the
sparse route's Q-limited solve (csrc/powerflow_sparse_qlim.hip) on the plan of the grid with every non-slack bus PQ
(utils/powerflow.py qlim_plan), with -r / -a in chunks that share one cover plan each, as above.

    python dataset_generator.py --case 118 --samples 2000 --root data
    python dataset_generator.py --case 118 --samples 2000 --root data -r 1 -a 1
    python dataset_generator.py --case 118 --samples 2000 --root data --enforce-q-lims --q-limit 0.5
    python dataset_generator.py --case 6470rte --samples 256 --root data
    python dataset_generator.py --case 6470rte --samples 256 --root data -r 1 -a 1
    python dataset_generator.py --case 6470rte --samples 256 --root data --enforce-q-lims --q-limit 0.5

    <root>/raw/case<case>_node_features.npy   (S, n, 6) float64 [index, type, Vm, Va (degrees), P, Q]; the type is per sample
    <root>/raw/case<case>_edge_features.npy   (S, e, 4) float64 [from, to, r, x]

-r / -a, the reference's topology perturbation (utils/data_utils.py:12-59): every sample loses r random lines -- drawn again, up to
20 times, while a bus is left unsupplied -- and gains a lines between random bus pairs, each with the parameters of a random
existing line.  The draw is `perturb_topology` (csrc/topology.hip, one workgroup per sample, in front of the solver's launch); a
sample without a connected draw is dropped and counted.  The files are then named case<case>perturbed<r>r<a>a_*, the reference's
naming, and hold e - r + a lines per sample: `PowerFlowData(case="118perturbed1r1a")` and train.py --case 118perturbed1r1a load them.

Per-unit, demand-positive, the network model of `PowerImbalance` (no shunts, taps or line charging).  Needs a HIP device:
there is no CPU solver in this package."""
import argparse
import os
import sys

import numpy as np

GENERATOR_CASES = ("14", "118", "118v2", "6470rte")
SPARSE_BATCH = 1024              # samples per launch on the sparse route: a 6470-bus sample holds 5.4 MB of workspace (5.5 GB)


def write_raw(root, case, bus_type, edge_index, rx, tables):
    """Write solved tables [S, n, 4] with their line parameters [S, e, 2] and lines -- [2, e] for all samples or [S, 2, e] -- in the
    reference's raw layout; returns the two paths.  `bus_type` is [n] for all samples or [S, n], one row per sample (what
    `generate(q_limit=...)` returns: a PV bus that hit its limit is a 2 in its sample's row)."""
    bus_type, edge_index = np.asarray(bus_type), np.asarray(edge_index)
    rx, tables = np.asarray(rx, dtype=np.float64), np.asarray(tables, dtype=np.float64)
    S, n, e = tables.shape[0], tables.shape[1], edge_index.shape[-1]
    assert tables.shape == (S, n, 4) and rx.shape == (S, e, 2) and edge_index.shape in ((2, e), (S, 2, e)) and bus_type.shape in ((n,), (S, n))
    node = np.empty((S, n, 6), dtype=np.float64)
    node[:, :, 0] = np.arange(n)
    node[:, :, 1] = bus_type
    node[:, :, 2:] = tables
    edge = np.empty((S, e, 4), dtype=np.float64)
    edge[:, :, :2] = edge_index.T if edge_index.ndim == 2 else edge_index.transpose(0, 2, 1)
    edge[:, :, 2:] = rx
    os.makedirs(os.path.join(root, "raw"), exist_ok=True)
    paths = (os.path.join(root, "raw", f"case{case}_node_features.npy"), os.path.join(root, "raw", f"case{case}_edge_features.npy"))
    np.save(paths[0], node)
    np.save(paths[1], edge)
    return paths


def generate(case, samples, seed=0, batch=4096, load=0.2, tol=1e-8, max_iter=10, device="cuda:0", max_rounds=64, remove=0, add=0,
             counts=None, route="auto", q_limit=None):
    """(bus_type [n], edge_index, rx [S, e, 2], tables [S, n, 4], redrawn): `samples` converged samples, host arrays.  `edge_index`
    is the grid's [2, e]; with `remove` or `add` above 0 it is [S, 2, e - remove + add], one perturbed line list per sample, and
    rx holds the parameters of those lines.  `counts` (a dict, optional) receives "disconnected": the samples dropped because no
    connected draw was found, "drawn": all samples drawn, and "route": the solver route that ran; with per-sample topologies on
    the sparse route also "chunks": the sizes of the chunks that shared a cover plan, "growth": the largest multiply-add count of a
    cover plan over the base plan's, and "extras": the most lines a cover added.  `route`: "auto" (the sparse route where the case
    has more unknowns than the dense solver takes) or "sparse".  `q_limit` (per-unit, > 0; None: no limits): every PV bus's Q is held
    within (-q_limit, +q_limit) by `solve_power_flow_qlim`; `bus_type` is then [S, n], the types each sample ended with, and `counts`
    receives "switched": the kept samples in which a bus switched, and "q_rounds": the most re-solves a kept sample took.  On the
    sparse route the plan is `qlim_plan`'s, the grid with every non-slack bus PQ (2 (n - 1) unknowns, which also decide "auto"
    then); with per-sample topologies the chunker plans that type row, one cover plan and one Q-limited solve per chunk."""
    import torch
    from poweflownet_amd.synth import CASES, make_physical_inputs
    from poweflownet_amd.utils.powerflow import (CoverChunker, QLimResult, max_unknowns, qlim_plan, solve_power_flow, solve_power_flow_covered,
                                                 solve_power_flow_qlim, sparse_plan)
    from poweflownet_amd.utils.topology import perturb_topology
    if route not in ("auto", "sparse"):
        raise ValueError(f"dataset_generator: route must be 'auto' or 'sparse', not {route!r}")
    if samples < 1:
        raise ValueError("dataset_generator: --samples must be at least 1")
    if remove < 0 or add < 0:
        raise ValueError(f"dataset_generator: cannot remove {remove} and add {add} lines")
    if q_limit is not None and not q_limit > 0:
        raise ValueError(f"dataset_generator: --q-limit must be above 0, not {q_limit!r}")
    n, e = CASES[str(case)]
    perturbed = remove > 0 or add > 0
    plan = chunker = None
    # the route is decided from the grid alone, before a sample is drawn: a draw of no samples gives the lines and the bus types
    ei0, bt0, _, _ = make_physical_inputs(n, e, 0, seed * 1_000_003, load)
    # (with Q-limits every non-slack bus may end PQ: the dense solver is sized for 2 (n - 1) unknowns then)
    if route == "auto" and (2 * (n - 1) if q_limit is not None else (n - 1) + int((bt0 == 2).sum())) > max_unknowns():
        route = "sparse"
    if route == "sparse":
        batch = min(batch, SPARSE_BATCH)
        # with Q-limits the plan is the grid's with every non-slack bus PQ: it serves whichever PV buses a sample switches
        plan_bt = torch.where(bt0 == 0, 0, 2) if q_limit is not None else bt0
        if perturbed:
            chunker = CoverChunker(plan_bt.to(device), ei0.to(device))  # one plan per chunk of samples, on the chunk's cover list
        elif q_limit is not None:
            plan = qlim_plan(bt0.to(device), ei0.to(device))
        else:
            plan = sparse_plan(bt0.to(device), ei0.to(device))   # one grid: built and uploaded once, it serves every batch and redraw
    growth, extras = 1.0, 0
    keep_ei, keep_rx, keep_t, keep_bt, keep_rounds, have, redrawn, drawn, disconnected = [], [], [], [], [], 0, 0, 0, 0
    for rnd in range(max_rounds):
        if have >= samples:
            break
        want = min(batch, samples - have)
        ei, bt, rx, spec = make_physical_inputs(n, e, want, seed * 1_000_003 + rnd, load)
        d_ei, d_rx, d_spec = ei.to(device), rx.to(device), spec.to(device)
        if perturbed:
            # sample numbers run on over the rounds: no draw repeats.  An added line has the parameters of the line it copies
            topo = perturb_topology(d_ei, n, num_samples=want, remove=remove, add=add, seed=seed, first_sample=drawn)
            connected = topo.status >= 1
            if bool((topo.status == -4).any()):
                raise RuntimeError("dataset_generator: the base grid names a bus outside the grid")
            d_ei = topo.edge_index[connected]
            d_rx = torch.gather(d_rx, 1, topo.source.long().clamp(min=0)[:, :, None].expand(-1, -1, 2))[connected]
            d_spec = d_spec[connected]
            disconnected += want - int(d_ei.shape[0])
        drawn += want
        if d_spec.shape[0] == 0:
            continue
        if q_limit is not None:
            limits = torch.tensor([-q_limit, q_limit], dtype=torch.float64, device=device).expand(n, 2)
        if chunker is not None and q_limit is not None:
            # per chunk: one cover plan of the all-PQ row and one Q-limited solve (its map launch and its masked solve)
            covers = list(chunker.plans(d_ei))
            parts = [solve_power_flow_qlim(bt.to(device), d_spec[rows], d_ei[rows], d_rx[rows], limits, tol=tol, max_iter=max_iter,
                                           route="sparse", plan=cover) for rows, cover in covers]
            res = QLimResult(*(torch.cat([getattr(r, f) for r in parts]) for f in ("table", "status", "iterations", "residual")),
                             flags=torch.stack([r.flags for r in parts]).amax(0), route="sparse",
                             bus_type=torch.cat([r.bus_type for r in parts]), rounds=torch.cat([r.rounds for r in parts]))
        elif chunker is not None:
            res, covers = solve_power_flow_covered(chunker, d_spec, d_ei, d_rx, tol=tol, max_iter=max_iter)
        elif q_limit is not None and route == "sparse":
            res = solve_power_flow_qlim(bt.to(device), d_spec, d_ei, d_rx, limits, tol=tol, max_iter=max_iter, route="sparse", plan=plan)
        elif q_limit is not None:
            res = solve_power_flow_qlim(bt.to(device), d_spec, d_ei, d_rx, limits, tol=tol, max_iter=max_iter)
        else:
            res = solve_power_flow(bt.to(device), d_spec, d_ei, d_rx, tol=tol, max_iter=max_iter, route=route, plan=plan)
        if chunker is not None:
            growth = max([growth] + [chunker.growth(c) for _, c in covers])
            extras = max([extras] + [c.extras for _, c in covers])
        ok = res.status >= 0
        if int(res.flags.item()) != 0:
            raise RuntimeError("dataset_generator: the solver flagged its bus types")
        if perturbed:
            keep_ei.append(d_ei[ok].cpu().numpy())
        ok = ok.cpu().numpy()
        keep_rx.append(d_rx.cpu().numpy()[ok])
        keep_t.append(res.table.cpu().numpy()[ok])
        if q_limit is not None:
            keep_bt.append(res.bus_type.cpu().numpy()[ok])
            keep_rounds.append(res.rounds.cpu().numpy()[ok])
        have += int(ok.sum())
        redrawn += int((~ok).sum())
    if counts is not None:
        counts.update(disconnected=disconnected, drawn=drawn, route=route)
        if chunker is not None:
            counts.update(chunks=list(chunker.sizes), growth=growth, extras=extras)
    if have < samples:
        raise RuntimeError(f"dataset_generator: only {have} of {samples} samples converged in {max_rounds} rounds (load {load})")
    lines = np.concatenate(keep_ei)[:samples] if perturbed else ei.numpy()
    types = bt.numpy()
    if q_limit is not None:
        types, q_rounds = np.concatenate(keep_bt)[:samples].astype(np.int64), np.concatenate(keep_rounds)[:samples]
        if counts is not None:
            counts.update(switched=int((types != bt.numpy()).any(axis=1).sum()), q_rounds=int(q_rounds.max()))
    return types, lines, np.concatenate(keep_rx)[:samples], np.concatenate(keep_t)[:samples], redrawn


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--case", default="118", choices=GENERATOR_CASES)
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--root", default="data")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=4096, help="samples per device launch")
    ap.add_argument("--load", type=float, default=0.2, help="mean active demand of a PQ bus, per-unit")
    ap.add_argument("-r", "--num_lines_to_remove", type=int, default=0, help="lines every sample loses (redrawn while a bus is unsupplied)")
    ap.add_argument("-a", "--num_lines_to_add", type=int, default=0, help="lines every sample gains, each a copy of a random line")
    ap.add_argument("--route", default="auto", choices=("auto", "sparse"),
                    help="solver route: auto takes the sparse one where the case exceeds the dense solver; sparse forces it")
    ap.add_argument("--enforce-q-lims", action="store_true",
                    help="a PV bus whose Q hits its limit becomes a load bus for that sample (needs --q-limit)")
    ap.add_argument("--q-limit", type=float, default=None, metavar="Q", help="with --enforce-q-lims: every PV bus's Q stays within (-Q, +Q), per-unit")
    a = ap.parse_args(argv)
    r, add = a.num_lines_to_remove, a.num_lines_to_add
    if r < 0 or add < 0:
        ap.error("-r and -a must be at least 0")
    if a.enforce_q_lims != (a.q_limit is not None) or (a.q_limit is not None and not a.q_limit > 0):
        ap.error("--enforce-q-lims and --q-limit Q (per-unit, above 0) go together")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dataset_generator.py needs a HIP device: poweflownet_amd has no CPU solver")
    counts = {}
    bt, ei, rx, tables, redrawn = generate(a.case, a.samples, a.seed, a.batch, a.load, remove=r, add=add, counts=counts, route=a.route,
                                            q_limit=a.q_limit)
    name = f"{a.case}perturbed{r}r{add}a" if r > 0 or add > 0 else a.case
    paths = write_raw(a.root, name, bt, ei, rx, tables)
    if r > 0 or add > 0:
        print(f"Left a bus unsupplied in every draw and dropped: {counts['disconnected']}")
    print(f"Failed to converge and drawn again: {redrawn}")
    if a.q_limit is not None:
        print(f"Q-limits (-{a.q_limit:g}, +{a.q_limit:g}) at every PV bus: {counts['switched']} sample(s) had a bus switched to a load bus, "
              f"at most {counts['q_rounds']} re-solve(s)")
    if counts["route"] == "sparse":
        print("Solved on the sparse route")
    if "chunks" in counts:
        sizes = counts["chunks"]
        print(f"Cover plans: {len(sizes)} chunk(s) of {min(sizes)}..{max(sizes)} samples, at most {counts['extras']} added lines and "
              f"{counts['growth']:.3f} x the base plan's multiply-adds per factor")
    print(f"wrote {a.samples} samples of case{name} ({tables.shape[1]} buses, {ei.shape[-1]} lines): {paths[0]}, {paths[1]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
