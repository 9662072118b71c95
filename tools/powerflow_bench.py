#!/usr/bin/env python3
"""Batched power-flow solver: samples per second and mean Newton iterations of `solve_power_flow` (ONE `pfn_powerflow_solve` launch)
at case14 and case118 x 4096 samples, AC and DC, on the LDS route and with the global route forced; beside it the float64 numpy
yardstick of tests/powerflow_ref.py per sample on this host's CPU -- a dense np.linalg.solve Newton loop written for the tests,
labelled as what it is: not pandapower, not a tuned CPU solver.  Not part of bench.py; no threshold (there is no predecessor).
After those rows: the fast-decoupled modes (`fdxb`, `fdbx`; max_iter 60 half-iterations, LDS route and global route forced) and
warm starts (`*_warm`: Newton and both fast-decoupled modes started from Newton's solution plus N(0, 1e-3) noise in Vm and radians,
the start a good prediction would give).

    python tools/powerflow_bench.py [--samples 4096] [--repeats 5] [--cpu-samples 16]
    python tools/powerflow_bench.py --route sparse [--case 118 --case 130,200 --case 600,835 --case 6470rte] [--samples 4096]
    python tools/powerflow_bench.py --route sparse --mode fdxb [--mode fdbx] [--case ...]
    python tools/powerflow_bench.py --route sparse --perturbed 1 1 [--case 6470rte] [--chunk 16 --chunk 64 --chunk 256]
    python tools/powerflow_bench.py --q-limit 0.4 --samples 1024 [--case 118 --case 70,100]
    python tools/powerflow_bench.py --route sparse --q-limit 0.4 --samples 256 --big-samples 64 [--case 1100,1530 --case 6470rte]

`--route sparse`: the sparse route (csrc/powerflow_sparse.hip) per `--case` column (a case name or "n,e"; default 118, 130,200,
600,835 and 6470rte): the plan's fill, multiply-adds per factor, size and HOST build time, then ms and ms per sample of the solve
with 64 and with 256 threads per sample and what the default takes, the mean and maximum solve count, and -- where the shape is
under the dense cap -- the dense global route beside it.  6470rte runs 64 samples and `--big-samples` (default 512).
`--mode` (repeatable; default ac and dc): `fdxb` / `fdbx` are the fast-decoupled modes on that route (csrc/powerflow_sparse_fd.hip):
one "fd" plan, reported per half (B' and B'': unknowns, fill, multiply-adds of the one-time factor, longest column), its host build
time, then the same timing rows with max_iter 60 HALF-iterations (mean and maximum count), and `factor_only`: the same launch with
max_iter 0, which assembles and factors both matrices and forms one mismatch -- the one-time share of the solve.

`--perturbed R A`: per-sample topologies on that route (`perturb_topology`'s draw: R lines removed, A added per sample), one
cover plan per chunk of `--chunk` samples (repeatable; default 16, 64 and 256), AC: per chunk size the lines the cover adds, its
nnz(L) and multiply-adds per factor against the base grid's plan, the HOST seconds of the cover plan (the list read, the
elimination, the upload), the seconds of the solve (the map launch and the masked solve: ONE timed call after one warm-up, not a
median), both per sample, the solve counts, and `one_topology`: the same number of samples on the base grid with the base plan.

`--q-limit Q`: the Q-limited solve (`solve_power_flow_qlim`, csrc/powerflow_qlim.hip) with (-Q, +Q) at every PV bus, per `--case`
column (default 118 and 70,100): the re-solves and the total of Jacobian solves (mean and maximum), the buses switched and the
unknowns a sample ends with, ms and ms per sample -- beside the unconstrained `solve_power_flow(mode="ac")` of the SAME batch in
the same process, and `no_limits`: the Q-limited entry with q_limits=None, i.e. what sizing the launch for m_max = 2 (n - 1) costs
by itself.  With `--route sparse` (csrc/powerflow_sparse_qlim.hip; `--case` default 1100,1530 and 6470rte, the latter with
`--big-samples` samples and one timed call): the plan of the grid with every non-slack bus PQ (`qlim_plan`) beside the own-types
plan -- unknowns, fill, multiply-adds per factor, host build time --, then `solve_power_flow(route="sparse")` of the SAME batch in
the same process, `no_limits` and `q_limited` on the all-PQ plan with solves, rounds and switched buses (mean and maximum), the
quantiles of |Q| at the PV buses of the unconstrained solution (what a Q means on this grid), and the ratios DESIGN 7r quotes.

Host wall time around the call with a device synchronise at either end, median of `--repeats` after one warm-up; tol 1e-8,
max_iter 10 (the defaults).  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def _timed(fn, repeats):
    import torch
    per, last = [], None
    for rep in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = fn()
        torch.cuda.synchronize()
        if rep:
            per.append(time.perf_counter() - t0)
    return per, last


def sparse_rows(a):
    """The `--route sparse` table: one column per case."""
    import torch
    from poweflownet_amd.synth import CASES, make_physical_inputs
    from poweflownet_amd.utils import powerflow as PF
    from poweflownet_amd.utils.powerflow import max_unknowns, sparse_plan
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "route": "sparse", "tol": 1e-8, "max_iter": 10, "cases": {}}
    for case in a.case or ["118", "130,200", "600,835", "6470rte"]:
        n, e = CASES[case] if case in CASES else tuple(int(v) for v in case.split(","))
        big = n > 2000
        for samples in ([64, a.big_samples] if big else [a.samples]):
            ei, bt, rx, spec = make_physical_inputs(n, e, samples, seed=0)
            d = [t.to(dev) for t in (bt, spec, ei, rx)]
            out = {"buses": n, "lines": e, "samples": samples}
            for mode in a.mode or ["ac", "dc"]:
                fd = mode.startswith("fd")
                iters = 60 if fd else 10
                plan = sparse_plan(d[0], d[2], mode)
                out[f"{mode}_plan"] = {"unknowns": plan.m, "nnz_l": plan.nnz_l, "slab_positions": plan.nnz, "longest_column": plan.max_col,
                                       "multiply_adds_per_factor": plan.madds, "plan_bytes": plan.bytes,
                                       "factor_bytes_per_sample": 4 * plan.nnz, "host_build_ms": round(1e3 * plan.build_s, 2)}
                if fd:
                    out[f"{mode}_plan"]["halves"] = {name: {"unknowns": m, "slab_positions": nnz, "nnz_l": nnz_l, "multiply_adds_of_the_factor": madds,
                                                            "longest_column": col} for name, (m, nnz, nnz_l, madds, col) in zip(("B'", "B''"), plan.halves)}
                runs = [("sparse_64", "sparse", 64, iters), ("sparse_256", "sparse", 256, iters), ("sparse_default", "sparse", 0, iters)]
                if fd:
                    runs.append(("factor_only", "sparse", 0, 0))
                if plan.m + plan.m_q <= max_unknowns():
                    runs.append(("dense_global", "global", 0, iters))
                for name, route, threads, max_iter in runs:
                    per, last = _timed(lambda: PF._solve(*d, mode, 1e-8, max_iter, route, None, plan if route == "sparse" else None, threads),
                                       1 if big else a.repeats)
                    status = last.status.cpu().numpy()
                    ms = 1e3 * float(np.median(per))
                    ok = status[status >= 0]
                    out[f"{mode}_{name}"] = {"ms": round(ms, 3), "min_ms": round(1e3 * min(per), 3), "max_ms": round(1e3 * max(per), 3),
                                             "ms_per_sample": round(ms / samples, 5), "failed": int((status < 0).sum()),
                                             "mean_iterations": round(float(ok.mean()), 3) if len(ok) else None,
                                             "max_iterations": int(ok.max()) if len(ok) else None}
            res["cases"][f"{case}x{samples}"] = out
            print(json.dumps({f"{case}x{samples}": out}), flush=True)
    print(json.dumps(res), flush=True)


def perturbed_rows(a):
    """The `--route sparse --perturbed R A` table: one row per chunk size."""
    import torch
    from poweflownet_amd.synth import CASES, make_physical_inputs
    from poweflownet_amd.utils.powerflow import cover_plan, solve_power_flow, sparse_plan
    from poweflownet_amd.utils.topology import perturb_topology
    dev = torch.device("cuda:0")
    remove, add = a.perturbed
    res = {"device": torch.cuda.get_device_name(0), "route": "sparse", "perturbed": [remove, add], "tol": 1e-8, "max_iter": 10, "cases": {}}
    for case in a.case or ["6470rte"]:
        n, e = CASES[case] if case in CASES else tuple(int(v) for v in case.split(","))
        chunks = a.chunk or [16, 64, 256]
        ei, bt, rx, spec = make_physical_inputs(n, e, max(chunks), seed=0)
        bt, spec, ei, rx = (t.to(dev) for t in (bt, spec, ei, rx))
        topo = perturb_topology(ei, n, num_samples=max(chunks), remove=remove, add=add, seed=0)
        keep = topo.status >= 1
        lists, prx, pspec = topo.edge_index[keep], torch.gather(rx, 1, topo.source.long().clamp(min=0)[:, :, None].expand(-1, -1, 2))[keep], spec[keep]
        base = sparse_plan(bt, ei, "ac")
        out = {"buses": n, "lines": e, "connected_draws": int(keep.sum()),
               "base_plan": {"nnz_l": base.nnz_l, "multiply_adds_per_factor": base.madds, "longest_column": base.max_col, "host_build_s": round(base.build_s, 3)}}
        for chunk in chunks:
            S = min(chunk, int(lists.shape[0]))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cover = cover_plan(bt, lists[:S], "ac", ei)
            torch.cuda.synchronize()
            plan_s = time.perf_counter() - t0
            per, last = _timed(lambda: solve_power_flow(bt, pspec[:S], lists[:S], prx[:S], route="sparse", plan=cover), 1)
            one, _ = _timed(lambda: solve_power_flow(bt, spec[:S], ei, rx[:S], route="sparse", plan=base), 1)
            status = last.status.cpu().numpy()
            ok = status[status >= 0]
            out[f"chunk_{chunk}"] = {"samples": S, "extras": cover.extras, "nnz_l": cover.plan.nnz_l, "nnz_l_growth": round(cover.plan.nnz_l / base.nnz_l, 4),
                                     "multiply_adds_per_factor": cover.plan.madds, "madds_growth": round(cover.plan.madds / base.madds, 4),
                                     "longest_column": cover.plan.max_col, "plan_s": round(plan_s, 3), "elimination_s": round(cover.plan.build_s, 3),
                                     "solve_s": round(per[0], 4), "plan_ms_per_sample": round(1e3 * plan_s / S, 3),
                                     "solve_ms_per_sample": round(1e3 * per[0] / S, 3), "total_ms_per_sample": round(1e3 * (plan_s + per[0]) / S, 3),
                                     "failed": int((status < 0).sum()), "mean_iterations": round(float(ok.mean()), 3) if len(ok) else None,
                                     "max_iterations": int(ok.max()) if len(ok) else None,
                                     "one_topology": {"solve_s": round(one[0], 4), "solve_ms_per_sample": round(1e3 * one[0] / S, 3)}}
            print(json.dumps({f"{case} chunk {chunk}": out[f"chunk_{chunk}"]}), flush=True)
        res["cases"][case] = out
    print(json.dumps(res), flush=True)


def qlim_rows(a):
    """The `--q-limit` table: one column per case."""
    import torch
    from poweflownet_amd.synth import CASES, make_physical_inputs
    from poweflownet_amd.utils.powerflow import solve_power_flow, solve_power_flow_qlim
    dev = torch.device("cuda:0")
    S = a.samples
    res = {"device": torch.cuda.get_device_name(0), "samples": S, "tol": 1e-8, "max_iter": 10, "max_rounds": 8, "q_limit": a.q_limit, "cases": {}}
    for case in a.case or ["118", "70,100"]:
        n, e = CASES[case] if case in CASES else tuple(int(v) for v in case.split(","))
        ei, bt, rx, spec = make_physical_inputs(n, e, S, seed=0)
        d = [t.to(dev) for t in (bt, spec, ei, rx)]
        limits = torch.tensor([-a.q_limit, a.q_limit], dtype=torch.float64, device=dev).expand(n, 2).contiguous()
        m0 = (n - 1) + int((bt == 2).sum())
        out = {"buses": n, "lines": e, "pv_buses": int((bt == 1).sum()), "unknowns": m0, "unknowns_sized_for": 2 * (n - 1)}

        def row(per, last):
            status = last.status.cpu().numpy()
            ms = 1e3 * float(np.median(per))
            return {"route": last.route, "ms": round(ms, 3), "min_ms": round(1e3 * min(per), 3), "max_ms": round(1e3 * max(per), 3),
                    "ms_per_sample": round(ms / S, 5), "failed": int((status < 0).sum()), "mean_solves": round(float(status[status >= 0].mean()), 3),
                    "max_solves": int(status.max())}
        out["unconstrained_solve_power_flow"] = row(*_timed(lambda: solve_power_flow(*d, mode="ac"), a.repeats))
        out["no_limits"] = row(*_timed(lambda: solve_power_flow_qlim(*d, None), a.repeats))
        per, last = _timed(lambda: solve_power_flow_qlim(*d, limits), a.repeats)
        ok = (last.status >= 0).cpu().numpy()
        rounds, types = last.rounds.cpu().numpy()[ok], last.bus_type.cpu().numpy()[ok]
        switched = (types != bt.numpy()).sum(axis=1)
        out["q_limited"] = dict(row(per, last), mean_rounds=round(float(rounds.mean()), 3), max_rounds=int(rounds.max()),
                                samples_switched=int((switched > 0).sum()), mean_switched=round(float(switched.mean()), 3),
                                max_switched=int(switched.max()), mean_final_unknowns=round(m0 + float(switched.mean()), 2))
        res["cases"][case] = out
    print(json.dumps(res), flush=True)


def qlim_sparse_rows(a):
    """The `--route sparse --q-limit Q` table: one column per case."""
    import torch
    from poweflownet_amd.synth import CASES, make_physical_inputs
    from poweflownet_amd.utils.powerflow import qlim_plan, solve_power_flow, solve_power_flow_qlim, sparse_plan
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "route": "sparse", "tol": 1e-8, "max_iter": 10, "max_rounds": 8, "q_limit": a.q_limit, "cases": {}}
    for case in a.case or ["1100,1530", "6470rte"]:
        n, e = CASES[case] if case in CASES else tuple(int(v) for v in case.split(","))
        big = n > 2000
        S = a.big_samples if big else a.samples
        repeats = 1 if big else a.repeats
        ei, bt, rx, spec = make_physical_inputs(n, e, S, seed=0)
        d = [t.to(dev) for t in (bt, spec, ei, rx)]
        limits = torch.tensor([-a.q_limit, a.q_limit], dtype=torch.float64, device=dev).expand(n, 2).contiguous()
        own, plan = sparse_plan(d[0], d[2], "ac"), qlim_plan(d[0], d[2])
        out = {"buses": n, "lines": e, "samples": S, "pv_buses": int((bt == 1).sum())}
        for name, p in (("own_types_plan", own), ("all_pq_plan", plan)):
            out[name] = {"unknowns": p.m, "slab_positions": p.nnz, "nnz_l": p.nnz_l, "multiply_adds_per_factor": p.madds, "longest_column": p.max_col,
                         "plan_bytes": p.bytes, "factor_bytes_per_sample": 4 * p.nnz, "host_build_ms": round(1e3 * p.build_s, 2)}
        out["slab_growth"], out["madds_growth"] = round(plan.nnz / own.nnz, 4), round(plan.madds / max(own.madds, 1), 4)

        def row(per, last):
            status = last.status.cpu().numpy()
            ms = 1e3 * float(np.median(per))
            ok = status[status >= 0]
            return {"ms": round(ms, 3), "min_ms": round(1e3 * min(per), 3), "max_ms": round(1e3 * max(per), 3), "ms_per_sample": round(ms / S, 5),
                    "failed": int((status < 0).sum()), "mean_solves": round(float(ok.mean()), 3) if len(ok) else None,
                    "max_solves": int(ok.max()) if len(ok) else None}
        per, free = _timed(lambda: solve_power_flow(*d, mode="ac", route="sparse", plan=own), repeats)
        out["unconstrained_solve_power_flow"] = row(per, free)
        q = free.table[:, bt.to(dev) == 1, 3].abs()
        q = q[torch.isfinite(q)]
        out["unconstrained_pv_abs_q_quantiles"] = {k: round(float(torch.quantile(q, v)), 5) for k, v in (("p50", .5), ("p90", .9), ("p99", .99), ("max", 1.))} if q.numel() else None
        out["no_limits"] = row(*_timed(lambda: solve_power_flow_qlim(*d, None, route="sparse", plan=plan), repeats))
        per, last = _timed(lambda: solve_power_flow_qlim(*d, limits, route="sparse", plan=plan), repeats)
        ok = (last.status >= 0).cpu().numpy()
        rounds, types = last.rounds.cpu().numpy()[ok], last.bus_type.cpu().numpy()[ok]
        switched = (types != bt.numpy()).sum(axis=1)
        out["q_limited"] = row(per, last)
        if ok.any():
            out["q_limited"].update(mean_rounds=round(float(rounds.mean()), 3), max_rounds=int(rounds.max()), samples_switched=int((switched > 0).sum()),
                                    mean_switched=round(float(switched.mean()), 3), max_switched=int(switched.max()))
        base = out["unconstrained_solve_power_flow"]
        out["no_limits_over_unconstrained"] = round(out["no_limits"]["ms"] / base["ms"], 4)
        if out["q_limited"]["mean_solves"] and base["mean_solves"]:
            out["q_limited_over_unconstrained"] = round(out["q_limited"]["ms"] / base["ms"], 4)
            out["solves_ratio_times_no_limits_factor"] = round(out["q_limited"]["mean_solves"] / base["mean_solves"] * out["no_limits_over_unconstrained"], 4)
        res["cases"][f"{case}x{S}"] = out
        print(json.dumps({f"{case}x{S}": out}), flush=True)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-samples", type=int, default=16)
    ap.add_argument("--route", default=None, choices=("sparse",), help="the sparse route's table instead of the dense rows")
    ap.add_argument("--case", action="append", default=None, help="with --route sparse: a case name or n,e (repeatable)")
    ap.add_argument("--big-samples", type=int, default=512, help="with --route sparse: the large batch of a case beyond 2000 buses")
    ap.add_argument("--mode", action="append", default=None, choices=("ac", "dc", "fdxb", "fdbx"),
                    help="with --route sparse: the modes to run (repeatable; default ac and dc)")
    ap.add_argument("--perturbed", type=int, nargs=2, default=None, metavar=("R", "A"),
                    help="with --route sparse: per-sample topologies (R lines removed, A added) under one cover plan per chunk")
    ap.add_argument("--chunk", type=int, action="append", default=None, help="with --perturbed: samples per cover plan (repeatable; default 16, 64, 256)")
    ap.add_argument("--q-limit", type=float, default=None, metavar="Q",
                    help="the Q-limited solve with (-Q, +Q) at every PV bus beside the unconstrained one (--case: default 118 and 70,100)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("powerflow_bench.py needs a HIP device")
    if a.q_limit is not None:
        if not a.q_limit > 0 or a.perturbed or a.mode:
            ap.error("--q-limit Q must be above 0 and goes with neither --perturbed nor --mode")
        return qlim_sparse_rows(a) if a.route == "sparse" else qlim_rows(a)
    if a.route == "sparse" and a.perturbed:
        return perturbed_rows(a)
    if a.route == "sparse":
        return sparse_rows(a)
    from poweflownet_amd.synth import CASES, make_physical_inputs
    from poweflownet_amd.utils.powerflow import solve_power_flow
    from tests import powerflow_ref as P
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "samples": a.samples, "tol": 1e-8, "max_iter": 10, "cases": {}}
    for case in ("14", "118"):
        n, e = CASES[case]
        ei, bt, rx, spec = make_physical_inputs(n, e, a.samples, seed=0)
        d = [t.to(dev) for t in (bt, spec, ei, rx)]
        out = {"buses": n, "lines": e, "unknowns_ac": (n - 1) + int((bt == 2).sum()), "unknowns_dc": n - 1}
        for mode in ("ac", "dc"):
            for route in ("auto", "global"):
                per, last = [], None
                for rep in range(a.repeats + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last = solve_power_flow(*d, mode=mode, route=route)
                    torch.cuda.synchronize()
                    if rep:
                        per.append(time.perf_counter() - t0)
                status = last.status.cpu().numpy()
                ms = 1e3 * float(np.median(per))
                out[f"{mode}_{last.route}"] = {"ms": round(ms, 3), "min_ms": round(1e3 * min(per), 3), "max_ms": round(1e3 * max(per), 3),
                                               "samples_per_s": round(a.samples / (ms * 1e-3)), "failed": int((status < 0).sum()),
                                               "mean_iterations": round(float(status[status >= 0].mean()), 3)}
        # the fast-decoupled modes, and warm starts from the solution plus noise
        solved = solve_power_flow(*d, mode="ac").table
        near = solved[:, :, :2] + torch.randn(a.samples, n, 2, dtype=torch.float64, device=dev,
                                              generator=torch.Generator(device=dev).manual_seed(0)) * torch.tensor([1e-3, 1e-3 * 180.0 / np.pi], dtype=torch.float64, device=dev)
        for name, mode, route, init in (("fdxb", "fdxb", "auto", None), ("fdxb", "fdxb", "global", None), ("fdbx", "fdbx", "auto", None),
                                        ("fdbx", "fdbx", "global", None), ("ac_warm", "ac", "auto", near), ("fdxb_warm", "fdxb", "auto", near),
                                        ("fdbx_warm", "fdbx", "auto", near)):
            per, last = [], None
            for rep in range(a.repeats + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last = solve_power_flow(*d, mode=mode, route=route, init=init, max_iter=10 if mode == "ac" else 60)
                torch.cuda.synchronize()
                if rep:
                    per.append(time.perf_counter() - t0)
            status = last.status.cpu().numpy()
            ms = 1e3 * float(np.median(per))
            out[f"{name}_{last.route}"] = {"ms": round(ms, 3), "min_ms": round(1e3 * min(per), 3), "max_ms": round(1e3 * max(per), 3),
                                           "samples_per_s": round(a.samples / (ms * 1e-3)), "failed": int((status < 0).sum()),
                                           "mean_iterations": round(float(status[status >= 0].mean()), 3),
                                           "max_iterations": int(status.max())}
        # the numpy yardstick, one sample at a time on the CPU
        k = min(a.cpu_samples, a.samples)
        ein, btn, rxn, specn = ei.numpy(), bt.numpy(), rx.numpy(), spec.numpy()
        for name, fn in (("ac", lambda s: P.newton(btn, specn[s], ein, rxn[s], tol=1e-8, max_iter=10)),
                         ("dc", lambda s: P.dc_solve(btn, specn[s], ein, rxn[s], norm=False))):
            fn(0)
            t0 = time.perf_counter()
            for s in range(k):
                fn(s)
            ms = 1e3 * (time.perf_counter() - t0) / k
            out[f"{name}_numpy_yardstick_cpu"] = {"ms_per_sample": round(ms, 3), "samples_per_s": round(1e3 / ms, 1), "samples_timed": k}
        res["cases"][case] = out
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
