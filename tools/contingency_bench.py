#!/usr/bin/env python3
"""N-1 screening: time per (scenario, outage) of `contingency_screen` (two launches: one B' inverse per scenario, then line outage
distribution factors) at case118 and case14 x 4096 scenarios, beside the BRUTE-FORCE path on the same build:
`solve_power_flow(mode="dc")` over explicit per-outage line lists, one [2, e - 1] list per (scenario, non-islanding outage), on a
scenario count small enough to hold.  Not part of bench.py; no threshold.

    python tools/contingency_bench.py [--samples 4096] [--brute-solves 4096] [--repeats 7] [--processes 3] [--case 118 --case 14]

Protocol: every case is measured in `--processes` FRESH child processes; in each, after one warm-up of both paths, the two are timed
alternately `--repeats` times (host wall clock around the call, a device synchronise at either end) and the child reports its
medians; the parent reports the median over the children and their spread (min .. max).  `keep_table` is off: the screen writes
three numbers per (scenario, outage), the brute force a bus table per solve.  tol 1e-8, max_iter 10.  One JSON line.

    python tools/contingency_bench.py --route sparse [--shape 118x186 --shape 600x835 --shape 6470x9005] [--samples 64]
                                      [--groups-sweep 1 4 16] [--brute-pairs 64]

The sparse route (`contingency_screen(route="sparse")`), same protocol.  Per shape (buses x lines, synthetic scenarios) a
row per block placement that the shape allows and per `groups` = the given multiples of the compute units (the default placement
only): the plan's build time, the wall time of the three launches, the base and the outage launch apart (the library's event
brackets, a pass of their own), pairs per second.  Beside it, alternating in the same child: the dense screen where the shape is
within its cap, else the brute force the parent commit has there -- `solve_power_flow(mode="dc", route="sparse", plan=<cover plan of
the base list>)` over explicit per-outage lists of `--brute-pairs` non-islanding outages spread evenly over the list, scaled per
pair.

    python tools/contingency_bench.py --pairs [--candidates 16] [--samples 4096] [--brute-solves 4096] [--case 118 --case 14]

The N-2 pair screen (`contingency_screen_pairs`), same protocol: the candidates are the `--candidates` non-islanding single
outages with the largest severity over the scenarios (the N-1 screen's, unrated), every pair of them is screened -- three launches:
pair islands, one B' inverse per scenario, the rank-2 updates -- on the route "auto" picks and, where that is "lds", on the forced
"global" route too; time per (scenario, pair), the base and the pair launch apart (the library's event brackets, a pass of their
own), beside the brute force: `solve_power_flow(mode="dc")` over explicit [2, e - 2] lists, one per (scenario, non-islanding pair).

    python tools/contingency_bench.py --pairs --route sparse [--shape 118x186 --shape 6470x9005] [--samples 64] [--candidates 64]
                                      [--waves-sweep 1 2 4 8 16] [--brute-pairs 64]

The pair screen on the sparse route (`contingency_screen_pairs(route="sparse")`), same protocol.  Per shape a row per
`waves` of the sweep and per column placement the shape allows with it: the wall time of the four launches, the islands, base,
columns and pairs launch apart (the library's event brackets, a pass of their own) and the pair-islands launch's share.  Beside it,
alternating in the same child: the dense pair screen where the shape is within its cap, else the brute force the parent commit has
there -- `solve_power_flow(mode="dc", route="sparse", plan=<cover plan of the base list>)` over explicit [2, e - 2] lists of
`--brute-pairs` non-islanding pairs spread evenly over the pair list, one per scenario, scaled per pair.

    python tools/contingency_bench.py --model [--graphed] [--chunk 64 128 186 256 372 512 744] [--model-samples 16] [--ac-outages 16]
                                      [--case 118 --case 14]

The network's screen (`contingency_screen_model`), same protocol, with the random-weight MaskEmbdMultiMPN of
configs/standard.json (bits do not matter for time).  Per case, alternating in the same child: (a) the entry for every `--chunk` of
the sweep, eager and -- with --graphed -- replayed from its captured chunk; (b) the composition it replaces, per chunk of the same
size: torch index-built reduced lists and normalisation, the forward with the adjacency rebuilt on the generic route, the merge,
`branch_flows`, `summarise_loadings`; (c) `contingency_screen` (DC) for the same scenarios; (d) `solve_power_flow(mode="ac")` over
explicit per-outage lists of `--ac-outages` non-islanding outages spread evenly over the list, for every scenario, scaled per pair.

    python tools/contingency_bench.py --ac [--ac-samples 16] [--case 118 --case 14]

The AC screen (`contingency_screen_ac`), same protocol, ALL outages of `--ac-samples` scenarios.  Per case, alternating in
the same child: the screen with `halves` 2 and 4 (three launches each: islands, base, outages), the base and the outage launch apart
(the library's event brackets, a pass of their own); the path it replaces, `solve_power_flow(mode="ac", init=<the base solution>)`
over explicit reduced lists of every (scenario, non-islanding outage), built as `verify_contingencies` builds them (the build is not
timed); and `contingency_screen` (DC) for the same scenarios.  tol 1e-8; the screen's base solve may take 60 half-iterations, the
Newton solves 10 iterations.  The screen has no predecessor: no threshold.

    python tools/contingency_bench.py --ac --route sparse [--shape 118x186 --shape 6470x9005] [--ac-samples 16] [--groups-sweep 1 2 4]
                                      [--brute-pairs 64]

The AC screen on the sparse route (`contingency_screen_ac(route="sparse")`), same protocol.  Per shape a row per
multiple of the compute units in the sweep (4 is the default `groups`): the screen with `halves` 2 and 4, the base and the outage
launch apart (the library's event brackets, a pass of their own; `dominant_launch` names the larger), beside -- alternating in the
same child -- the path it replaces, `solve_power_flow(mode="ac", route="sparse", init=<the base solution>)` through ONE cover plan
over explicit reduced lists: every (scenario, non-islanding outage) where the shape is within the dense cap, else `--brute-pairs`
outages spread evenly over the list, one scenario each, scaled per pair (`newton_scaled_to_all_ms`); and, within the dense cap, the
dense AC screen.

    python tools/contingency_bench.py --units [--unit-lines 10] [--samples 4096] [--brute-solves 4096] [--case 118 --case 14]

The generator-outage screen (`contingency_screen_units`), same protocol: the units are the PV buses, each losing
max(-P, 0), the lost output shared among the others in equal parts.  Timed alternately in the same child: the screen with the units
alone; with `--unit-lines` > 0 the screen with that many candidate lines behind every unit (the non-islanding single outages with
the largest severity over the scenarios, as --pairs chooses them); the parent commit's `contingency_screen` at the same batch,
which prices the shared base solve and inverse; and the BRUTE FORCE -- `solve_power_flow(mode="dc")` over explicitly modified
`spec` tables, one per (scenario, unit), and over those tables with explicit reduced line lists, one per (scenario, unit, line) --
on scenario counts small enough for about `--brute-solves` solves each, scaled per item."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def child(case, samples, brute_solves, repeats):
    import torch
    from poweflownet_amd.synth import CASES, make_physical_inputs
    from poweflownet_amd.utils.contingency import contingency_screen
    from poweflownet_amd.utils.powerflow import solve_power_flow
    dev = torch.device("cuda:0")
    n, e = CASES[case]
    ei, bt, rx, spec = (t.to(dev) for t in make_physical_inputs(n, e, samples, seed=0))
    res = contingency_screen(bt, spec, ei, rx)                             # (warm-up; its islands choose the brute force's outages)
    outages = torch.nonzero(res.islands == 0).flatten()
    K = int(outages.numel())
    Sb = max(1, min(samples, brute_solves // K))                          # about `brute_solves` DC solves, whatever the case
    # the brute force's inputs, built once and not timed: scenario s, outage k -> sample s * K + k of [Sb K, 2, e - 1] lists
    ar = torch.arange(e - 1, device=dev)
    idx = ar[None, :] + (ar[None, :] >= outages[:, None])                  # [K, e - 1]
    lists = ei[:, idx].permute(1, 0, 2).repeat(Sb, 1, 1).contiguous()
    rx_b = rx[:Sb][:, idx].reshape(Sb * K, e - 1, 2).contiguous()
    spec_b = spec[:Sb].repeat_interleave(K, dim=0).contiguous()
    brute = solve_power_flow(bt, spec_b, lists, rx_b, mode="dc")           # (warm-up)
    assert bool((res.status >= 0).all()) and bool((brute.status >= 0).all())

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    t_screen, t_brute = [], []
    for _ in range(repeats):
        t_screen.append(timed(lambda: contingency_screen(bt, spec, ei, rx)))
        t_brute.append(timed(lambda: solve_power_flow(bt, spec_b, lists, rx_b, mode="dc")))
    screen_us = 1e6 * statistics.median(t_screen) / (samples * e)           # (the screen serves the islanding outages too)
    brute_us = 1e6 * statistics.median(t_brute) / (Sb * K)
    print(json.dumps({"case": case, "buses": n, "lines": e, "route": res.route, "scenarios": samples, "outages": e, "non_islanding": K,
                      "brute_scenarios": Sb, "brute_solves": Sb * K, "screen_ms": 1e3 * statistics.median(t_screen),
                      "brute_ms": 1e3 * statistics.median(t_brute), "screen_us_per_pair": screen_us, "brute_us_per_pair": brute_us,
                      "ratio": brute_us / screen_us}))


def child_ac(case, samples, repeats):
    import torch
    from poweflownet_amd import _lib as L
    from poweflownet_amd.synth import CASES, make_physical_inputs
    from poweflownet_amd.utils.contingency import contingency_screen, contingency_screen_ac
    from poweflownet_amd.utils.powerflow import solve_power_flow
    dev = torch.device("cuda:0")
    n, e = CASES[case]
    ei, bt, rx, spec = (t.to(dev) for t in make_physical_inputs(n, e, samples, seed=0))
    res = contingency_screen_ac(bt, spec, ei, rx)                          # (warm-up; its islands choose the replaced path's outages)
    contingency_screen_ac(bt, spec, ei, rx, halves=4)
    dc = contingency_screen(bt, spec, ei, rx)
    outages = torch.nonzero(res.islands == 0).flatten()
    K = int(outages.numel())
    # the replaced path's inputs, built once and not timed: scenario s, outage k -> sample s * K + k of [S K, 2, e - 1] lists
    ar = torch.arange(e - 1, device=dev)
    idx = ar[None, :] + (ar[None, :] >= outages[:, None])                  # [K, e - 1]
    lists = ei[:, idx].permute(1, 0, 2).repeat(samples, 1, 1).contiguous()
    rx_b = rx[:, idx].reshape(samples * K, e - 1, 2).contiguous()
    spec_b = spec.repeat_interleave(K, dim=0).contiguous()
    init_b = res.base_table[:, :, :2].repeat_interleave(K, dim=0).contiguous()
    newton = solve_power_flow(bt, spec_b, lists, rx_b, mode="ac", init=init_b)      # (warm-up)
    assert bool((res.status >= 0).all()) and bool((dc.status >= 0).all())
    solved = newton.status >= 0

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    runs = {"halves2": lambda: contingency_screen_ac(bt, spec, ei, rx), "halves4": lambda: contingency_screen_ac(bt, spec, ei, rx, halves=4),
            "newton": lambda: solve_power_flow(bt, spec_b, lists, rx_b, mode="ac", init=init_b), "dc": lambda: contingency_screen(bt, spec, ei, rx)}
    times = {k: [] for k in runs}
    for _ in range(repeats):
        for k, fn in runs.items():
            times[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    launches = {}
    for halves in (2, 4):                                                  # the launches apart: a pass of its own
        L.profile_enable(True)
        contingency_screen_ac(bt, spec, ei, rx, halves=halves)
        rep = L.profile_report()
        L.profile_enable(False)
        launches[halves] = {k: round(rep[k]["ms"], 4) for k in ("contingency_islands", "contingency_ac_base", "contingency_ac_outages") if k in rep}
    T = samples * e
    print(json.dumps({"case": case, "buses": n, "lines": e, "scenarios": samples, "outages": e, "non_islanding": K, "placement": res.route,
                      "waves": res.group, "halves2_ms": 1e3 * med["halves2"], "halves4_ms": 1e3 * med["halves4"], "newton_ms": 1e3 * med["newton"],
                      "dc_ms": 1e3 * med["dc"], "halves2_us_per_pair": 1e6 * med["halves2"] / T, "halves4_us_per_pair": 1e6 * med["halves4"] / T,
                      "newton_us_per_pair": 1e6 * med["newton"] / (samples * K), "dc_us_per_pair": 1e6 * med["dc"] / T,
                      "newton_solves": samples * K, "newton_failed": int((~solved).sum()), "newton_iterations_max": int(newton.status.max()),
                      "base_halves_max": int(res.status.max()), "launches_halves2_ms": launches[2], "launches_halves4_ms": launches[4]}))


def main_ac(a):
    out = {"tol": 1e-8, "repeats": a.repeats, "processes": a.processes, "cases": {}}
    for case in a.case or ["118", "14"]:
        kids = []
        for _ in range(a.processes):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-ac", case, "--ac-samples", str(a.ac_samples), "--repeats",
                                str(a.repeats)], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit(f"contingency_bench: the AC child for case {case} failed:\n{r.stdout}\n{r.stderr}")
            kids.append(json.loads(r.stdout.strip().splitlines()[-1]))
        row = dict(kids[0])
        for key in [k for k in kids[0] if k.endswith("_ms") and not k.startswith("launches") or k.endswith("_us_per_pair")]:
            vals = [x[key] for x in kids]
            row[key], row[key + "_spread"] = round(statistics.median(vals), 4), [round(min(vals), 4), round(max(vals), 4)]
        for h in ("halves2", "halves4"):
            row["newton_over_" + h] = round(row["newton_us_per_pair"] / row[h + "_us_per_pair"], 3)
            row[h + "_over_dc"] = round(row[h + "_us_per_pair"] / row["dc_us_per_pair"], 3)
        out["cases"][case] = row
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out))
    return 0


def child_ac_sparse(shape, samples, groups_x, brute_pairs, repeats):
    import torch
    from poweflownet_amd import _lib as L
    from poweflownet_amd.synth import make_physical_inputs
    from poweflownet_amd.utils.contingency import contingency_screen_ac
    from poweflownet_amd.utils.powerflow import cover_plan, max_unknowns, solve_power_flow, sparse_plan
    dev = torch.device("cuda:0")
    n, e = (int(v) for v in shape.split("x"))
    ei, bt, rx, spec = (t.to(dev) for t in make_physical_inputs(n, e, samples, seed=0))
    plan = sparse_plan(bt, ei, mode="fd")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    kw = {"route": "sparse", "plan": plan, "groups": groups_x * cus if groups_x else None}
    res = contingency_screen_ac(bt, spec, ei, rx, **kw)                    # (warm-up; its islands choose the replaced path's outages)
    contingency_screen_ac(bt, spec, ei, rx, halves=4, **kw)
    assert bool((res.status >= 0).all())
    # the replaced path: Newton from the base solution over explicit reduced lists under ONE cover plan; every non-islanding outage
    # of every scenario where the dense solver would take them too, else `brute_pairs` outages spread evenly, one scenario each
    dense = n - 1 <= max_unknowns()
    ok = torch.nonzero(res.islands == 0).flatten()
    outages = ok if dense else ok[torch.linspace(0, ok.numel() - 1, min(brute_pairs, ok.numel())).long()]
    K = int(outages.numel())
    ar = torch.arange(e - 1, device=dev)
    idx = ar[None, :] + (ar[None, :] >= outages[:, None])                  # [K, e - 1]
    if dense:
        lists = ei[:, idx].permute(1, 0, 2).repeat(samples, 1, 1).contiguous()
        rx_b = rx[:, idx].reshape(samples * K, e - 1, 2).contiguous()
        spec_b = spec.repeat_interleave(K, dim=0).contiguous()
        init_b = res.base_table[:, :, :2].repeat_interleave(K, dim=0).contiguous()
    else:
        sc = torch.arange(K, device=dev) % samples
        lists = ei[:, idx].permute(1, 0, 2).contiguous()
        rx_b, spec_b, init_b = rx[sc[:, None], idx].contiguous(), spec[sc].contiguous(), res.base_table[sc][:, :, :2].contiguous()
    T = int(lists.shape[0])
    cover = cover_plan(bt, ei[None], mode="ac", base=ei)
    runs = {"halves2": lambda: contingency_screen_ac(bt, spec, ei, rx, **kw), "halves4": lambda: contingency_screen_ac(bt, spec, ei, rx, halves=4, **kw),
            "newton": lambda: solve_power_flow(bt, spec_b, lists, rx_b, mode="ac", route="sparse", plan=cover, init=init_b)}
    if dense:
        runs["dense2"] = lambda: contingency_screen_ac(bt, spec, ei, rx)
        runs["dense4"] = lambda: contingency_screen_ac(bt, spec, ei, rx, halves=4)
    newton = runs["newton"]()                                              # (warm-up)
    for fn in runs.values():
        fn()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    times = {k: [] for k in runs}
    for _ in range(repeats):
        for k, fn in runs.items():
            times[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    launches = {}
    for halves in (2, 4):                                                  # the launches apart: event brackets, a pass of their own
        L.profile_enable(True)
        contingency_screen_ac(bt, spec, ei, rx, halves=halves, **kw)
        rep = L.profile_report()
        L.profile_enable(False)
        launches[halves] = {k: round(v["ms"], 4) for k, v in rep.items() if k.startswith(("contingency_", "powerflow_sparse_fd"))}
    P = samples * e
    row = {"buses": n, "lines": e, "scenarios": samples, "outages": e, "non_islanding": int(ok.numel()), "block": res.block, "groups_x_cus": groups_x,
           "cus": cus, "nnz_l": plan.nnz_l, "plan_build_s": plan.build_s, "halves2_ms": 1e3 * med["halves2"], "halves4_ms": 1e3 * med["halves4"],
           "newton_ms": 1e3 * med["newton"], "halves2_us_per_pair": 1e6 * med["halves2"] / P, "halves4_us_per_pair": 1e6 * med["halves4"] / P,
           "newton_us_per_pair": 1e6 * med["newton"] / T, "newton_solves": T, "newton_scaled_to_all_ms": 1e3 * med["newton"] / T * samples * int(ok.numel()),
           "newton_failed": int((newton.status < 0).sum()), "newton_iterations_max": int(newton.status.max()), "base_halves_max": int(res.status.max()),
           "launches_halves2_ms": launches[2], "launches_halves4_ms": launches[4]}
    if dense:
        row.update({"dense2_ms": 1e3 * med["dense2"], "dense4_ms": 1e3 * med["dense4"], "dense2_us_per_pair": 1e6 * med["dense2"] / P,
                    "dense4_us_per_pair": 1e6 * med["dense4"] / P})
    print(json.dumps(row))


def main_ac_sparse(a):
    out = {"tol": 1e-8, "repeats": a.repeats, "processes": a.processes, "rows": []}
    for shape in a.shape or ["118x186", "6470x9005"]:
        for gx in ([1, 2, 4] if a.groups_sweep is None else a.groups_sweep):
            kids = []
            for _ in range(a.processes):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-ac-sparse", shape, "--ac-samples", str(a.ac_samples), "--groups-x",
                                    str(gx), "--brute-pairs", str(a.brute_pairs), "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=1100)
                if r.returncode != 0:
                    raise SystemExit(f"contingency_bench: the AC child for {shape} x{gx} failed:\n{r.stdout}\n{r.stderr}")
                kids.append(json.loads(r.stdout.strip().splitlines()[-1]))
            row = dict(kids[0])
            for key in [k for k in kids[0] if k.endswith("_ms") and not k.startswith("launches") or k.endswith("_us_per_pair")]:
                vals = [x[key] for x in kids]
                row[key], row[key + "_spread"] = round(statistics.median(vals), 4), [round(min(vals), 4), round(max(vals), 4)]
            for h in ("halves2", "halves4"):
                row["newton_over_" + h] = round(row["newton_us_per_pair"] / row[h + "_us_per_pair"], 3)
            if "dense2_us_per_pair" in row:
                row["sparse_over_dense2"] = round(row["halves2_us_per_pair"] / row["dense2_us_per_pair"], 3)
                row["sparse_over_dense4"] = round(row["halves4_us_per_pair"] / row["dense4_us_per_pair"], 3)
            dom = row["launches_halves2_ms"]
            row["dominant_launch"] = max((k for k in dom if k != "contingency_islands"), key=lambda k: dom[k]) if dom else None
            out["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out))
    return 0


def child_model(case, samples, chunks, graphed, ac_outages, repeats):
    import torch
    from poweflownet_amd.data import Batch
    from poweflownet_amd.datasets import PowerFlowData
    from poweflownet_amd.loss import branch_flows
    from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
    from poweflownet_amd.synth import CASES, make_physical_inputs
    from poweflownet_amd.utils.contingency import contingency_screen, contingency_screen_model, summarise_loadings
    from poweflownet_amd.utils.powerflow import solve_power_flow
    dev = torch.device("cuda:0")
    n, e = CASES[case]
    S, T = samples, samples * e
    ei, bt, rx, spec = (t.to(dev) for t in make_physical_inputs(n, e, S, seed=0))
    with open(os.path.join(HERE, "configs", "standard.json")) as f:
        cfg = json.load(f)
    torch.manual_seed(0)
    model = MaskEmbdMultiMPN(4, 2, 4, int(cfg["hidden_dim"]), int(cfg["n_gnn_layers"]), int(cfg["K"]), float(cfg["dropout_rate"])).to(dev).eval()
    stats = {"xymean": torch.tensor([[1.0, 0.0, 0.0, 0.0]]), "xystd": torch.tensor([[0.05, 5.0, 0.3, 0.1]]),
             "edgemean": torch.tensor([[0.0175, 0.09]]), "edgestd": torch.tensor([[0.007, 0.035]])}
    dc = contingency_screen(bt, spec, ei, rx)                              # (c), warm-up; also the bus_type tensor's eager first call
    ratings = 1.5 * dc.base_flow.abs().max(dim=0).values
    # (d) the AC solves' inputs, built once and not timed
    ok = torch.nonzero(dc.islands == 0).flatten()
    outages = ok[torch.linspace(0, ok.numel() - 1, min(ac_outages, ok.numel())).long()]
    K = int(outages.numel())
    ar = torch.arange(e - 1, device=dev)
    idx_ac = ar[None, :] + (ar[None, :] >= outages[:, None])               # [K, e - 1]
    lists = ei[:, idx_ac].permute(1, 0, 2).repeat(S, 1, 1).contiguous()
    rx_ac = rx[:, idx_ac].reshape(S * K, e - 1, 2).contiguous()
    spec_ac = spec.repeat_interleave(K, dim=0).contiguous()
    assert bool((solve_power_flow(bt, spec_ac, lists, rx_ac, mode="ac").status >= 0).all())      # (warm-up)
    # (b) the composition's constants
    mask = torch.tensor(PowerFlowData.bus_type_mask)[bt.cpu()].float().to(dev)                  # [n, 4]
    xm, xs, em, es = (stats[k].to(dev) for k in ("xymean", "xystd", "edgemean", "edgestd"))
    rate = ratings.float()
    sev_c, worst_c, over_c = (torch.empty(T, dtype=d, device=dev) for d in (torch.float32, torch.int32, torch.int32))

    @torch.no_grad()
    def composition(chunk):
        was = model.dynamic_topology
        model.dynamic_topology = True                                       # (a new line list per chunk: rebuilt on the device, the generic build)
        try:
            for item0 in range(0, T, chunk):
                items = torch.arange(item0, item0 + chunk, device=dev).clamp(max=T - 1)
                s, k = items // e, items % e
                idx = ar[None, :] + (ar[None, :] >= k[:, None])             # [B, e - 1]
                y = spec[s].float()
                b = Batch()
                b.x = ((y * (1.0 - mask) - xm) / (xs + 1e-7)).reshape(-1, 4)
                b.pred_mask, b.bus_type = mask.repeat(chunk, 1), bt.repeat(chunk)
                local = ei[:, idx]                                          # [2, B, e - 1]
                b.edge_index = (local + (torch.arange(chunk, device=dev) * n)[None, :, None]).reshape(2, -1)
                r = rx[s[:, None], idx].float()
                b.edge_attr = ((r - em) / (es + 1e-7)).reshape(-1, 2)
                b.batch = torch.arange(chunk, device=dev).repeat_interleave(n)
                b.ptr = torch.arange(chunk + 1, device=dev) * n
                out = model(b).view(chunk, n, 4)
                pred = torch.where(mask.bool()[None], out * (xs + 1e-7) + xm, y)
                flows = branch_flows(pred, local.permute(1, 0, 2).contiguous(), r.contiguous())[0]
                loading = torch.full((chunk, e), float("nan"), device=dev)
                loading.scatter_(1, idx, flows[:, :, 0] / rate[idx])
                monitored = (rate > 0)[None, :] & (torch.arange(e, device=dev)[None, :] != k[:, None])
                live = min(chunk, T - item0)
                for dst, src in zip((sev_c, worst_c, over_c), summarise_loadings(loading, monitored)):
                    dst[item0:item0 + live] = src[:live]
        finally:
            model.dynamic_topology = was

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    forms = ["eager"] + (["graphed"] if graphed else [])
    runs = {(c, f): (lambda c=c, f=f: contingency_screen_model(model, bt, spec, ei, rx, ratings, chunk=c, graphed=f == "graphed", **stats))
            for c in chunks for f in forms}
    runs.update({(c, "composition"): (lambda c=c: composition(c)) for c in chunks})
    runs[(0, "dc")] = lambda: contingency_screen(bt, spec, ei, rx, ratings)
    runs[(0, "ac")] = lambda: solve_power_flow(bt, spec_ac, lists, rx_ac, mode="ac")
    for fn in runs.values():                                               # warm-up of every shape the timed window uses (captures included)
        fn()
        fn()
    # the entry and the composition agree on what they compute (same items, same rules) before either is timed
    ref = contingency_screen_model(model, bt, spec, ei, rx, ratings, chunk=chunks[0], **stats)
    composition(chunks[0])
    live = (ref.islands == 0).repeat(S)
    assert bool(torch.isfinite(ref.severity.view(-1)[live]).all())
    agree = float((ref.severity.view(-1)[live] - sev_c[live]).abs().max() / ref.severity.view(-1)[live].abs().max())
    times = {key: [] for key in runs}
    for _ in range(repeats):
        for key, fn in runs.items():
            times[key].append(timed(fn))
    med = {key: statistics.median(v) for key, v in times.items()}
    rows = []
    for c in chunks:
        row = {"chunk": c, "composition_ms": 1e3 * med[(c, "composition")]}
        for f in forms:
            row[f + "_ms"] = 1e3 * med[(c, f)]
            row[f + "_us_per_pair"] = 1e6 * med[(c, f)] / T
            row["composition_over_" + f] = med[(c, "composition")] / med[(c, f)]
        rows.append(row)
    ac_us = 1e6 * med[(0, "ac")] / (S * K)
    print(json.dumps({"case": case, "buses": n, "lines": e, "scenarios": S, "items": T, "hidden_dim": int(cfg["hidden_dim"]), "rows": rows,
                      "dc_ms": 1e3 * med[(0, "dc")], "dc_us_per_pair": 1e6 * med[(0, "dc")] / T, "ac_solves": S * K, "ac_ms": 1e3 * med[(0, "ac")],
                      "ac_us_per_pair": ac_us, "entry_vs_composition_max_rel_severity_gap": agree}))


def main_model(a):
    out = {"repeats": a.repeats, "processes": a.processes, "cases": {}}
    for case in a.case or ["118", "14"]:
        kids = []
        for _ in range(a.processes):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-model", case, "--model-samples", str(a.model_samples), "--repeats",
                                str(a.repeats), "--ac-outages", str(a.ac_outages), "--chunk"] + [str(c) for c in a.chunk]
                               + (["--graphed"] if a.graphed else []), capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit(f"contingency_bench: the model child for case {case} failed:\n{r.stdout}\n{r.stderr}")
            kids.append(json.loads(r.stdout.strip().splitlines()[-1]))
        row = dict(kids[0])
        for key in ("dc_ms", "dc_us_per_pair", "ac_ms", "ac_us_per_pair"):
            vals = [x[key] for x in kids]
            row[key], row[key + "_spread"] = round(statistics.median(vals), 4), [round(min(vals), 4), round(max(vals), 4)]
        row["rows"] = []
        for i, first in enumerate(kids[0]["rows"]):
            merged = {"chunk": first["chunk"]}
            for key in [k for k in first if k != "chunk"]:
                vals = [x["rows"][i][key] for x in kids]
                merged[key], merged[key + "_spread"] = round(statistics.median(vals), 4), [round(min(vals), 4), round(max(vals), 4)]
            for f in ("eager", "graphed"):
                if f + "_us_per_pair" in merged:
                    merged["ac_over_" + f] = round(row["ac_us_per_pair"] / merged[f + "_us_per_pair"], 3)
            row["rows"].append(merged)
        fastest = {f: min(row["rows"], key=lambda m: m[f + "_ms"])["chunk"] for f in ("eager", "graphed") if f + "_ms" in row["rows"][0]}
        row["fastest_chunk"] = fastest
        out["cases"][case] = row
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out))
    return 0


def child_pairs(case, samples, candidates, brute_solves, repeats):
    import torch
    from poweflownet_amd import _lib as L
    from poweflownet_amd.synth import CASES, make_physical_inputs
    from poweflownet_amd.utils.contingency import contingency_screen, contingency_screen_pairs
    from poweflownet_amd.utils.powerflow import solve_power_flow
    dev = torch.device("cuda:0")
    n, e = CASES[case]
    ei, bt, rx, spec = (t.to(dev) for t in make_physical_inputs(n, e, samples, seed=0))
    single = contingency_screen(bt, spec, ei, rx)
    sev = torch.where(single.islands[None, :] == 0, single.severity, torch.full_like(single.severity, -1.0)).max(dim=0).values
    lines = sorted(torch.topk(sev, min(candidates, int((single.islands == 0).sum()))).indices.tolist())
    res = contingency_screen_pairs(bt, spec, ei, rx, lines=lines)           # (warm-up; its islands choose the brute force's pairs)
    routes = [res.route] + (["global"] if res.route == "lds" else [])
    for r in routes[1:]:
        contingency_screen_pairs(bt, spec, ei, rx, lines=lines, route=r)    # (warm-up)
    P = int(res.pairs.shape[0])
    out = res.pairs[res.islands == 0]                                       # [K, 2], a < b
    K = int(out.shape[0])
    Sb = max(1, min(samples, brute_solves // K))
    # the brute force's inputs, built once and not timed: scenario s, pair k -> sample s * K + k of [Sb K, 2, e - 2] lists
    idx = torch.arange(e - 2, device=dev)[None, :].expand(K, e - 2)
    for k in range(2):
        idx = idx + (idx >= out[:, k:k + 1])
    lists = ei[:, idx].permute(1, 0, 2).repeat(Sb, 1, 1).contiguous()
    rx_b = rx[:Sb][:, idx].reshape(Sb * K, e - 2, 2).contiguous()
    spec_b = spec[:Sb].repeat_interleave(K, dim=0).contiguous()
    brute = solve_power_flow(bt, spec_b, lists, rx_b, mode="dc")            # (warm-up)
    assert bool((res.status >= 0).all()) and bool((brute.status >= 0).all())

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    t_screen, t_brute = {r: [] for r in routes}, []
    for _ in range(repeats):
        for r in routes:
            t_screen[r].append(timed(lambda: contingency_screen_pairs(bt, spec, ei, rx, lines=lines, route=r)))
        t_brute.append(timed(lambda: solve_power_flow(bt, spec_b, lists, rx_b, mode="dc")))
    row = {"case": case, "buses": n, "lines": e, "scenarios": samples, "candidates": len(lines), "pairs": P, "non_islanding": K,
           "brute_scenarios": Sb, "brute_solves": Sb * K, "brute_ms": 1e3 * statistics.median(t_brute),
           "brute_us_per_pair": 1e6 * statistics.median(t_brute) / (Sb * K)}
    for r in routes:
        L.profile_report(reset=True)
        L.profile_enable(True)                                              # the launches apart: event brackets, a pass of their own
        for _ in range(repeats):
            contingency_screen_pairs(bt, spec, ei, rx, lines=lines, route=r)
        prof = L.profile_report()
        L.profile_enable(False)
        sec = statistics.median(t_screen[r])
        row[r] = {"screen_ms": 1e3 * sec, "screen_us_per_pair": 1e6 * sec / (samples * P), "ratio": row["brute_us_per_pair"] / (1e6 * sec / (samples * P)),
                  "islands_ms": prof["contingency_pair_islands"]["ms"] / repeats, "base_ms": prof["contingency_pairs_base"]["ms"] / repeats,
                  "pairs_ms": prof["contingency_pairs"]["ms"] / repeats}
    row["route"] = routes[0]
    print(json.dumps(row))


def child_units(case, samples, unit_lines, brute_solves, repeats):
    import torch
    from poweflownet_amd.synth import CASES, make_physical_inputs
    from poweflownet_amd.utils.contingency import contingency_screen, contingency_screen_units, unit_outage_spec
    from poweflownet_amd.utils.powerflow import solve_power_flow
    dev = torch.device("cuda:0")
    n, e = CASES[case]
    ei, bt, rx, spec = (t.to(dev) for t in make_physical_inputs(n, e, samples, seed=0))
    single = contingency_screen(bt, spec, ei, rx)                           # (warm-up; its severities choose the candidate lines)
    sev = torch.where(single.islands[None, :] == 0, single.severity, torch.full_like(single.severity, -1.0)).max(dim=0).values
    lines = sorted(torch.topk(sev, min(unit_lines, int((single.islands == 0).sum()))).indices.tolist()) if unit_lines else None
    alone = contingency_screen_units(bt, spec, ei, rx)                      # (warm-up; units=None: the PV buses, unit_p=None: max(-P, 0))
    G = int(alone.units.shape[0])
    part = torch.ones(G, dtype=torch.float64, device=dev)
    kw = {"participation": part}
    alone = contingency_screen_units(bt, spec, ei, rx, **kw)
    lined = contingency_screen_units(bt, spec, ei, rx, lines=lines, **kw) if lines else None
    # the brute force's inputs, built once and not timed: scenario s, unit g -> sample s * G + g of [Sb G, n, 4] tables
    Sb = max(1, min(samples, brute_solves // G))
    sc, g = torch.arange(Sb, device=dev).repeat_interleave(G), torch.arange(G, device=dev).repeat(Sb)
    spec_u = unit_outage_spec(spec[sc], alone.units, alone.unit_p[sc], part.expand(Sb * G, G), g).contiguous()
    rx_u = rx[sc].contiguous()
    brute = solve_power_flow(bt, spec_u, ei, rx_u, mode="dc")               # (warm-up)
    assert bool((alone.status >= 0).all()) and bool((brute.status >= 0).all())
    paths = {"units": lambda: contingency_screen_units(bt, spec, ei, rx, **kw), "n1_screen": lambda: contingency_screen(bt, spec, ei, rx),
             "brute_units": lambda: solve_power_flow(bt, spec_u, ei, rx_u, mode="dc")}
    K = Sl = 0
    if lines:
        out = lined.lines[lined.islands == 0]                                # the non-islanding candidates
        K = int(out.numel())
        Sl = max(1, min(samples, brute_solves // (G * K)))
        ar = torch.arange(e - 1, device=dev)
        idx = ar[None, :] + (ar[None, :] >= out[:, None])                   # [K, e - 1]
        lists = ei[:, idx].permute(1, 0, 2).repeat(Sl * G, 1, 1).contiguous()           # sample (s * G + g) * K + k
        rx_l = rx[:Sl][:, idx].repeat_interleave(G, dim=0).reshape(Sl * G * K, e - 1, 2).contiguous()
        spec_l = spec_u[:Sl * G].repeat_interleave(K, dim=0).contiguous()
        assert bool((solve_power_flow(bt, spec_l, lists, rx_l, mode="dc").status >= 0).all())                # (warm-up)
        paths["unit_lines"] = lambda: contingency_screen_units(bt, spec, ei, rx, lines=lines, **kw)
        paths["brute_unit_lines"] = lambda: solve_power_flow(bt, spec_l, lists, rx_l, mode="dc")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    t = {k: [] for k in paths}
    for _ in range(repeats):
        for k, fn in paths.items():
            t[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    row = {"case": case, "buses": n, "lines": e, "route": alone.route, "scenarios": samples, "units": G, "units_ms": 1e3 * med["units"],
           "n1_screen_ms": 1e3 * med["n1_screen"], "units_us_per_item": 1e6 * med["units"] / (samples * G), "brute_units_scenarios": Sb,
           "brute_units_ms": 1e3 * med["brute_units"], "brute_units_us_per_item": 1e6 * med["brute_units"] / (Sb * G)}
    row["units_ratio"] = row["brute_units_us_per_item"] / row["units_us_per_item"]
    if lines:
        c = len(lines)
        row.update({"candidates": c, "non_islanding": K, "unit_lines_ms": 1e3 * med["unit_lines"],
                    "unit_lines_us_per_item": 1e6 * med["unit_lines"] / (samples * G * (1 + c)), "brute_unit_lines_scenarios": Sl,
                    "brute_unit_lines_ms": 1e3 * med["brute_unit_lines"], "brute_unit_lines_us_per_item": 1e6 * med["brute_unit_lines"] / (Sl * G * K)})
        row["unit_lines_ratio"] = row["brute_unit_lines_us_per_item"] / row["unit_lines_us_per_item"]
    print(json.dumps(row))


def main_units(a):
    out = {"tol": 1e-8, "max_iter": 10, "repeats": a.repeats, "processes": a.processes, "cases": {}}
    for case in a.case or ["118", "14"]:
        rows = []
        for _ in range(a.processes):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-units", case, "--samples", str(a.samples), "--brute-solves",
                                str(a.brute_solves), "--repeats", str(a.repeats), "--unit-lines", str(a.unit_lines)], capture_output=True, text=True,
                               timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"contingency_bench: the units child for case {case} failed:\n{r.stdout}\n{r.stderr}")
            rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        row = dict(rows[0])
        for key in [k for k, v in rows[0].items() if isinstance(v, float)]:
            vals = [x[key] for x in rows]
            row[key], row[key + "_spread"] = round(statistics.median(vals), 4), [round(min(vals), 4), round(max(vals), 4)]
        out["cases"][case] = row
    print(json.dumps(out))
    return 0


def main_pairs(a):
    out = {"tol": 1e-8, "max_iter": 10, "repeats": a.repeats, "processes": a.processes, "cases": {}}
    for case in a.case or ["118", "14"]:
        rows = []
        for _ in range(a.processes):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-pairs", case, "--samples", str(a.samples), "--brute-solves",
                                str(a.brute_solves), "--repeats", str(a.repeats), "--candidates", str(a.candidates)], capture_output=True, text=True,
                               timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"contingency_bench: the pairs child for case {case} failed:\n{r.stdout}\n{r.stderr}")
            rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        row = dict(rows[0])
        for key in ("brute_ms", "brute_us_per_pair"):
            vals = [x[key] for x in rows]
            row[key], row[key + "_spread"] = round(statistics.median(vals), 4), [round(min(vals), 4), round(max(vals), 4)]
        for route in [k for k in ("lds", "global") if k in row]:
            row[route] = dict(row[route])
            for key in list(rows[0][route]):
                vals = [x[route][key] for x in rows]
                row[route][key], row[route][key + "_spread"] = round(statistics.median(vals), 4), [round(min(vals), 4), round(max(vals), 4)]
        out["cases"][case] = row
    print(json.dumps(out))
    return 0


def child_pairs_sparse(shape, samples, candidates, columns, waves, brute_pairs, repeats):
    import torch
    from poweflownet_amd import _lib as L
    from poweflownet_amd.synth import make_physical_inputs
    from poweflownet_amd.utils.contingency import contingency_screen, contingency_screen_pairs
    from poweflownet_amd.utils.powerflow import cover_plan, max_unknowns, solve_power_flow, sparse_plan
    dev = torch.device("cuda:0")
    n, e = (int(v) for v in shape.split("x"))
    ei, bt, rx, spec = (t.to(dev) for t in make_physical_inputs(n, e, samples, seed=0))
    plan = sparse_plan(bt, ei, mode="dc")
    single = contingency_screen(bt, spec, ei, rx, route="sparse", plan=plan)   # (not timed: its severities choose the candidates)
    sev = torch.where(single.islands[None, :] == 0, single.severity, torch.full_like(single.severity, -1.0)).max(dim=0).values
    lines = sorted(torch.topk(sev, min(candidates, int((single.islands == 0).sum()))).indices.tolist())
    kw = {"route": "sparse", "plan": plan, "lines": lines, "columns": columns, "waves": waves}
    res = contingency_screen_pairs(bt, spec, ei, rx, **kw)                  # (warm-up; its islands choose the brute force's pairs)
    assert bool((res.status >= 0).all())
    P = int(res.pairs.shape[0])
    dense = n - 1 <= max_unknowns()
    if dense:
        def other():
            return contingency_screen_pairs(bt, spec, ei, rx, lines=lines)
        other_pairs = samples * P
    else:
        ok = res.pairs[res.islands == 0]
        out = ok[torch.linspace(0, ok.shape[0] - 1, min(brute_pairs, ok.shape[0])).long()]    # [T, 2], a < b
        T = int(out.shape[0])
        idx = torch.arange(e - 2, device=dev)[None, :].expand(T, e - 2)
        for k in range(2):
            idx = idx + (idx >= out[:, k:k + 1])
        lists = ei[:, idx].permute(1, 0, 2).contiguous()
        sc = torch.arange(T, device=dev) % samples
        rx_b, spec_b = rx[sc[:, None], idx].contiguous(), spec[sc].contiguous()
        cover = cover_plan(bt, ei[None], mode="dc", base=ei)

        def other():
            return solve_power_flow(bt, spec_b, lists, rx_b, mode="dc", route="sparse", plan=cover)
        other_pairs = T
    assert bool((other().status >= 0).all())                               # (warm-up)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    t_screen, t_other = [], []
    for _ in range(repeats):
        t_screen.append(timed(lambda: contingency_screen_pairs(bt, spec, ei, rx, **kw)))
        t_other.append(timed(other))
    L.profile_report(reset=True)
    L.profile_enable(True)                                                  # the four launches apart: event brackets, a pass of their own
    for _ in range(repeats):
        contingency_screen_pairs(bt, spec, ei, rx, **kw)
    prof = L.profile_report()
    L.profile_enable(False)
    ms = {k: prof[name]["ms"] / repeats for k, name in (("islands_ms", "contingency_pair_islands"), ("base_ms", "contingency_sparse_base"),
                                                         ("columns_ms", "contingency_pairs_sparse_columns"), ("pairs_ms", "contingency_pairs_sparse"))}
    screen_s, other_s = statistics.median(t_screen), statistics.median(t_other)
    print(json.dumps({"buses": n, "lines": e, "scenarios": samples, "candidates": len(lines), "pairs": P, "block": res.block, "columns": res.columns,
                      "waves": waves or 4, "unknowns": plan.m, "nnz_l": plan.nnz_l, "screen_ms": 1e3 * screen_s, **ms,
                      "islands_share": ms["islands_ms"] / sum(ms.values()), "screen_us_per_pair": 1e6 * screen_s / (samples * P),
                      "other": "dense pair screen" if dense else "brute force", "other_pairs": other_pairs, "other_ms": 1e3 * other_s,
                      "other_us_per_pair": 1e6 * other_s / other_pairs, "ratio": (other_s / other_pairs) / (screen_s / (samples * P))}))


def main_pairs_sparse(a):
    out = {"tol": 1e-8, "max_iter": 10, "repeats": a.repeats, "processes": a.processes, "rows": []}
    for shape in a.shape or ["118x186", "6470x9005"]:
        n = int(shape.split("x")[0])
        for waves in a.waves_sweep:
            for columns in (("lds", "global") if 4 * n * (1 + waves) + 15 <= 159 * 1024 else ("global",)):
                rows = []
                for _ in range(a.processes):
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-pairs-sparse", shape, "--samples", str(a.samples),
                                        "--candidates", str(a.candidates), "--columns", columns, "--waves", str(waves), "--brute-pairs",
                                        str(a.brute_pairs), "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=900)
                    if r.returncode != 0:
                        raise SystemExit(f"contingency_bench: the child for {shape} {columns} waves {waves} failed:\n{r.stdout}\n{r.stderr}")
                    rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
                row = dict(rows[0])
                for key in ("screen_ms", "islands_ms", "base_ms", "columns_ms", "pairs_ms", "islands_share", "screen_us_per_pair", "other_ms",
                            "other_us_per_pair", "ratio"):
                    vals = [x[key] for x in rows]
                    row[key] = round(statistics.median(vals), 5)
                    row[key + "_spread"] = [round(min(vals), 5), round(max(vals), 5)]
                out["rows"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out))
    return 0


def child_sparse(shape, samples, block, groups_x, brute_pairs, repeats):
    import torch
    from poweflownet_amd import _lib as L
    from poweflownet_amd.synth import make_physical_inputs
    from poweflownet_amd.utils.contingency import contingency_screen
    from poweflownet_amd.utils.powerflow import cover_plan, max_unknowns, solve_power_flow, sparse_plan
    dev = torch.device("cuda:0")
    n, e = (int(v) for v in shape.split("x"))
    ei, bt, rx, spec = (t.to(dev) for t in make_physical_inputs(n, e, samples, seed=0))
    plan = sparse_plan(bt, ei, mode="dc")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    kw = {"route": "sparse", "plan": plan, "block": block, "groups": groups_x * cus if groups_x else None}
    res = contingency_screen(bt, spec, ei, rx, **kw)                       # (warm-up)
    assert bool((res.status >= 0).all())
    dense = n - 1 <= max_unknowns()
    if dense:
        def other():
            return contingency_screen(bt, spec, ei, rx)
        other_pairs = samples * e
    else:
        ok = torch.nonzero(res.islands == 0).flatten()
        outages = ok[torch.linspace(0, ok.numel() - 1, min(brute_pairs, ok.numel())).long()]
        T = int(outages.numel())
        ar = torch.arange(e - 1, device=dev)
        idx = ar[None, :] + (ar[None, :] >= outages[:, None])              # [T, e - 1]
        lists = ei[:, idx].permute(1, 0, 2).contiguous()
        sc = torch.arange(T, device=dev) % samples
        rx_b, spec_b = rx[sc[:, None], idx].contiguous(), spec[sc].contiguous()
        cover = cover_plan(bt, ei[None], mode="dc", base=ei)

        def other():
            return solve_power_flow(bt, spec_b, lists, rx_b, mode="dc", route="sparse", plan=cover)
        other_pairs = T
    assert bool((other().status >= 0).all())                               # (warm-up)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    t_screen, t_other = [], []
    for _ in range(repeats):
        t_screen.append(timed(lambda: contingency_screen(bt, spec, ei, rx, **kw)))
        t_other.append(timed(other))
    L.profile_enable(True)                                                  # the two launches apart: event brackets, a pass of their own
    for _ in range(repeats):
        contingency_screen(bt, spec, ei, rx, **kw)
    prof = L.profile_report()
    L.profile_enable(False)
    screen_s, other_s = statistics.median(t_screen), statistics.median(t_other)
    print(json.dumps({"buses": n, "lines": e, "scenarios": samples, "block": res.block, "groups_x_cus": groups_x, "cus": cus, "unknowns": plan.m,
                      "nnz_l": plan.nnz_l, "plan_build_s": plan.build_s, "screen_ms": 1e3 * screen_s,
                      "base_ms": prof["contingency_sparse_base"]["ms"] / repeats, "outages_ms": prof["contingency_sparse_outages"]["ms"] / repeats,
                      "pairs_per_s": samples * e / screen_s, "screen_us_per_pair": 1e6 * screen_s / (samples * e),
                      "other": "dense screen" if dense else "brute force", "other_pairs": other_pairs, "other_ms": 1e3 * other_s,
                      "other_us_per_pair": 1e6 * other_s / other_pairs, "ratio": (other_s / other_pairs) / (screen_s / (samples * e))}))


def main_sparse(a):
    out = {"tol": 1e-8, "max_iter": 10, "repeats": a.repeats, "processes": a.processes, "rows": []}
    for shape in a.shape or ["118x186", "600x835", "6470x9005"]:
        n = int(shape.split("x")[0])
        configs = [(b, 0) for b in (("lds", "global") if 256 * n <= 159 * 1024 else ("global",))] + [("auto", g) for g in ([1, 4, 16] if a.groups_sweep is None else a.groups_sweep)]
        for block, gx in configs:
            rows = []
            for _ in range(a.processes):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-sparse", shape, "--samples", str(a.samples), "--block", block,
                                    "--groups-x", str(gx), "--brute-pairs", str(a.brute_pairs), "--repeats", str(a.repeats)],
                                   capture_output=True, text=True, timeout=900)
                if r.returncode != 0:
                    raise SystemExit(f"contingency_bench: the child for {shape} {block} x{gx} failed:\n{r.stdout}\n{r.stderr}")
                rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
            row = dict(rows[0])
            for key in ("screen_ms", "base_ms", "outages_ms", "pairs_per_s", "screen_us_per_pair", "other_ms", "other_us_per_pair", "ratio", "plan_build_s"):
                vals = [x[key] for x in rows]
                row[key] = round(statistics.median(vals), 4)
                row[key + "_spread"] = [round(min(vals), 4), round(max(vals), 4)]
            out["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--case", action="append", default=None)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--brute-solves", type=int, default=4096, help="the brute force runs about this many DC solves")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--route", default="dense", choices=("dense", "sparse"), help="sparse: contingency_screen(route='sparse'), DESIGN 7v")
    ap.add_argument("--shape", action="append", default=None, help="sparse: BUSESxLINES (repeatable)")
    ap.add_argument("--groups-sweep", type=int, nargs="*", default=None,
                    help="sparse: groups as multiples of the compute units (default 1 4 16; with --ac 1 2 4, 4 being the default groups)")
    ap.add_argument("--brute-pairs", type=int, default=64, help="sparse, beyond the dense cap: the brute force solves this many outages")
    ap.add_argument("--child-sparse", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--block", default="auto", help=argparse.SUPPRESS)
    ap.add_argument("--groups-x", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--pairs", action="store_true", help="the N-2 pair screen, contingency_screen_pairs, DESIGN 7w")
    ap.add_argument("--candidates", type=int, default=16, help="pairs: the K worst non-islanding single outages are the candidates")
    ap.add_argument("--child-pairs", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--waves-sweep", type=int, nargs="*", default=[1, 2, 4, 8, 16], help="pairs, sparse: the pair launch's waves per workgroup")
    ap.add_argument("--child-pairs-sparse", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--columns", default="auto", help=argparse.SUPPRESS)
    ap.add_argument("--waves", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--model", action="store_true", help="the network's screen, contingency_screen_model, DESIGN 7y")
    ap.add_argument("--graphed", action="store_true", help="model: also time the entry replayed from its captured chunk")
    ap.add_argument("--chunk", type=int, nargs="*", default=[64, 128, 186, 256, 372, 512, 744], help="model: the chunk sizes of the sweep")
    ap.add_argument("--model-samples", type=int, default=16, help="model: scenarios")
    ap.add_argument("--ac-outages", type=int, default=16, help="model: the AC solves cover this many non-islanding outages of every scenario")
    ap.add_argument("--child-model", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--ac", action="store_true", help="the AC screen, contingency_screen_ac, DESIGN 7z")
    ap.add_argument("--ac-samples", type=int, default=16, help="ac: scenarios")
    ap.add_argument("--child-ac", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-ac-sparse", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--units", action="store_true", help="the generator-outage screen, contingency_screen_units, DESIGN 7zc")
    ap.add_argument("--unit-lines", type=int, default=0, help="units: also screen every unit followed by each of the K worst single line outages")
    ap.add_argument("--child-units", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.child_units:
        child_units(a.child_units, a.samples, a.unit_lines, a.brute_solves, a.repeats)
        return 0
    if a.units:
        return main_units(a)
    if a.child_ac_sparse:
        child_ac_sparse(a.child_ac_sparse, a.ac_samples, a.groups_x, a.brute_pairs, a.repeats)
        return 0
    if a.ac and a.route == "sparse":
        return main_ac_sparse(a)
    if a.child_ac:
        child_ac(a.child_ac, a.ac_samples, a.repeats)
        return 0
    if a.ac:
        return main_ac(a)
    if a.child_model:
        child_model(a.child_model, a.model_samples, a.chunk, a.graphed, a.ac_outages, a.repeats)
        return 0
    if a.model:
        return main_model(a)
    if a.child_pairs_sparse:
        child_pairs_sparse(a.child_pairs_sparse, a.samples, a.candidates, a.columns, a.waves or None, a.brute_pairs, a.repeats)
        return 0
    if a.pairs and a.route == "sparse":
        return main_pairs_sparse(a)
    if a.child_pairs:
        child_pairs(a.child_pairs, a.samples, a.candidates, a.brute_solves, a.repeats)
        return 0
    if a.pairs:
        return main_pairs(a)
    if a.child_sparse:
        child_sparse(a.child_sparse, a.samples, a.block, a.groups_x, a.brute_pairs, a.repeats)
        return 0
    if a.route == "sparse":
        return main_sparse(a)
    if a.child:
        child(a.child, a.samples, a.brute_solves, a.repeats)
        return 0
    out = {"tol": 1e-8, "max_iter": 10, "repeats": a.repeats, "processes": a.processes, "cases": {}}
    for case in a.case or ["118", "14"]:
        rows = []
        for _ in range(a.processes):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--samples", str(a.samples), "--brute-solves",
                                str(a.brute_solves), "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"contingency_bench: the child for case {case} failed:\n{r.stdout}\n{r.stderr}")
            rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        row = dict(rows[0])
        for key in ("screen_ms", "brute_ms", "screen_us_per_pair", "brute_us_per_pair", "ratio"):
            vals = [x[key] for x in rows]
            row[key] = round(statistics.median(vals), 4)
            row[key + "_spread"] = [round(min(vals), 4), round(max(vals), 4)]
        out["cases"][case] = row
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
