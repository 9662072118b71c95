#!/usr/bin/env python3
"""Topology perturbation: milliseconds and samples per second of `perturb_topology` (ONE `pfn_topology_perturb` launch) at case14
and case118 x 4096 samples for (r, a) in {(1, 0), (3, 2)}, with the mean attempts; beside it the numpy yardstick loop of
tests/topology_ref.py per sample on this host's CPU -- a test yardstick, labelled as what it is: not the reference's
pandapower / networkx loop and not a tuned baseline.  Then a generator round at case118 (draw the physical inputs on the host, draw
the topologies, gather the line parameters, solve) timed piece by piece with and without -r 1 -a 1, and the solver's failure rate
on the perturbed against the static grid.  Not part of bench.py; no threshold (the draw has no predecessor).

    python tools/perturb_bench.py [--samples 4096] [--big-samples 65536] [--calls 200] [--repeats 5] [--cpu-samples 64]

Host wall time with a device synchronise at either end, median of `--repeats` after one warm-up: of ONE call (`ms`: at 4096 samples
mostly the launch and the synchronise), of `--calls` calls back to back per call (`ms_back_to_back`: the kernel where it is longer
than the host's enqueue), and the latter at `--big-samples` samples, where the kernel is most of the time.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def timed(fn, repeats, calls=1):
    """Per-call milliseconds: `calls` back-to-back calls between two synchronises (one call of a 40-us kernel is a measurement of
    the launch and the synchronise), median over `repeats` such windows after a warm-up window."""
    import torch
    per, last = [], None
    for rep in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            last = fn()
        torch.cuda.synchronize()
        if rep:
            per.append((time.perf_counter() - t0) / calls)
    ms = 1e3 * float(np.median(per))
    return last, {"ms": round(ms, 4), "min_ms": round(1e3 * min(per), 4), "max_ms": round(1e3 * max(per), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--big-samples", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-samples", type=int, default=64)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("perturb_bench.py needs a HIP device")
    import dataset_generator
    from poweflownet_amd.synth import CASES, make_physical_inputs, make_topology
    from poweflownet_amd.utils.powerflow import solve_power_flow
    from poweflownet_amd.utils.topology import perturb_topology
    from tests import topology_ref as T
    dev = torch.device("cuda:0")
    S = a.samples
    res = {"device": torch.cuda.get_device_name(0), "samples": S, "max_attempts": 20, "draw": {}}
    for case in ("14", "118"):
        n, e = CASES[case]
        base = make_topology(n, e)
        d_base = base.to(dev)
        for r, add in ((1, 0), (3, 2)):
            topo, t = timed(lambda: perturb_topology(d_base, n, num_samples=S, remove=r, add=add, seed=1), a.repeats)
            status = topo.status.cpu().numpy()
            many = timed(lambda: perturb_topology(d_base, n, num_samples=S, remove=r, add=add, seed=1), a.repeats, a.calls)[1]
            big = timed(lambda: perturb_topology(d_base, n, num_samples=a.big_samples, remove=r, add=add, seed=1), a.repeats, a.calls)[1]
            t.update(samples_per_s=round(S / (t["ms"] * 1e-3)), ms_back_to_back=many["ms"], back_to_back_min_max_ms=[many["min_ms"], many["max_ms"]],
                     samples_per_s_back_to_back=round(S / (many["ms"] * 1e-3)),
                     big={"samples": a.big_samples, "ms_back_to_back": big["ms"], "min_max_ms": [big["min_ms"], big["max_ms"]],
                          "samples_per_s": round(a.big_samples / (big["ms"] * 1e-3))},
                     no_draw=int((status < 0).sum()), mean_attempts=round(float(status[status > 0].mean()), 3))
            k = min(a.cpu_samples, S)
            T.perturb(base.numpy(), n, 1, r, add, seed=1)
            t0 = time.perf_counter()
            T.perturb(base.numpy(), n, k, r, add, seed=1)
            ms = 1e3 * (time.perf_counter() - t0) / k
            t["numpy_yardstick_cpu"] = {"ms_per_sample": round(ms, 4), "samples_per_s": round(1e3 / ms, 1), "samples_timed": k}
            res["draw"][f"case{case}_r{r}_a{add}"] = t

    # one generator round at case118, piece by piece
    n, e = CASES["118"]
    t0 = time.perf_counter()
    ei, bt, rx, spec = make_physical_inputs(n, e, S, seed=0)
    host_ms = 1e3 * (time.perf_counter() - t0)
    d_ei, d_bt, d_rx, d_spec = (x.to(dev) for x in (ei, bt, rx, spec))
    rnd = {"host_inputs_ms": round(host_ms, 1)}
    topo, rnd["draw"] = timed(lambda: perturb_topology(d_ei, n, num_samples=S, remove=1, add=1, seed=0), a.repeats)
    g_rx, rnd["gather_rx"] = timed(lambda: torch.gather(d_rx, 1, topo.source.long().clamp(min=0)[:, :, None].expand(-1, -1, 2)), a.repeats)
    static, rnd["solve_static"] = timed(lambda: solve_power_flow(d_bt, d_spec, d_ei, d_rx), a.repeats)
    pert, rnd["solve_perturbed"] = timed(lambda: solve_power_flow(d_bt, d_spec, topo.edge_index, g_rx), a.repeats)
    ok = (topo.status >= 1)
    for name, r_ in (("static", static), ("perturbed", pert)):
        st = r_.status[ok] if name == "perturbed" else r_.status
        good = st[st >= 0]
        rnd[f"solver_failed_{name}"] = int((st < 0).sum())
        rnd[f"solver_mean_iterations_{name}"] = round(float(good.float().mean()), 3)
    rnd["no_draw"] = int((~ok).sum())
    rnd["draw_share_of_device_round"] = round(rnd["draw"]["ms"] / (rnd["draw"]["ms"] + rnd["gather_rx"]["ms"] + rnd["solve_perturbed"]["ms"]), 5)
    res["generator_round_case118"] = rnd
    # the generator as a whole (host draws, copies and the final read-back included)
    for name, kw in (("static", {}), ("r1_a1", dict(remove=1, add=1))):
        dataset_generator.generate("118", S, **kw)
        per = []
        for _ in range(5):
            counts = {}
            t0 = time.perf_counter()
            redrawn = dataset_generator.generate("118", S, counts=counts, **kw)[4]
            per.append(time.perf_counter() - t0)
        sec = float(np.median(per))
        res[f"generator_case118_{name}"] = {"s": round(sec, 3), "min_s": round(min(per), 3), "max_s": round(max(per), 3),
                                            "samples_per_s": round(S / sec), "redrawn": redrawn, "disconnected": counts.get("disconnected", 0)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
