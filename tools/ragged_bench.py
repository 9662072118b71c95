#!/usr/bin/env python3
"""Mixed-size batches: the segment-packed route against the generic route, not part of bench.py.

    python tools/ragged_bench.py                      this tree, every workload, packed and unpacked: one JSON line
    python tools/ragged_bench.py --ab OTHER_TREE      the same for this tree and for OTHER_TREE's package (a built copy of another
                                                      commit, e.g. the parent), alternating, `--pairs` times each, in fresh
                                                      processes; then the summary table
    python tools/ragged_bench.py --root TREE          the package under TREE instead of this tree's (what --ab starts)

The script uses only what the package had before segment packing existed (Batch.from_data_list, synth, the model, MSELoss,
FlatAdamW), so it runs unchanged against an older tree: there `segment_packing` is an attribute nobody reads and both variants
time the same route.

Workloads (configs/standard.json: hidden 129, 4 layers, K 3; synthetic topologies of synth.CASES' sizes):
  train 64x118+64x14      eager training step: zero_grad, forward, MSELoss, backward, FlatAdamW
  infer 1024x118+1024x14  forward under no_grad
  infer 512 balls         512 graphs with sizes uniform in 1..118 (what explain_epoch packs), forward under no_grad
  train 1x118+3x14        47.5 % padding: the cap rejects it, both variants take the generic route
  train 128x118 uniform   for scale: the flagship batch, which packing never touches
Every workload rotates over four batches of the same composition with edge_index tensors of their own, as a loader hands them
out: every step builds its adjacency on the device, on either route, and the segment plan is computed anew (its cache is emptied
before every step).  Timing: warm-up until the clocks have ramped, then `--windows` windows of device-event time, each at least
`--window-ms` long; per-step median, minimum and maximum over the windows."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--ab", default=None)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--tag", default="tree")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--reuse-plans", action="store_true", help="keep the planner's cache between steps (a loader whose compositions repeat)")
    return ap.parse_args()


# ------------------------------------------------------------------------------------------------------ worker
def _ragged_batch(sizes, seed):
    import torch
    from poweflownet_amd.data import Batch
    from poweflownet_amd.synth import make_graph, make_topology
    topo = {}
    graphs = []
    for g, n in enumerate(sizes):
        if n not in topo:
            e = {118: 186, 14: 20, 1: 0}.get(n, max(n - 1, (n * 186) // 118))
            topo[n] = make_topology(n, e, n) if n > 1 else torch.zeros(2, 0, dtype=torch.long)
        graphs.append(make_graph(n, topo[n].shape[1], seed=seed * 7919 + g, edge_index=topo[n]))
    return Batch.from_data_list(graphs)


def _workloads():
    balls = [int(v) for v in np.random.default_rng(0).integers(1, 119, 512)]
    return [("train 64x118+64x14", [118] * 64 + [14] * 64, True),
            ("infer 1024x118+1024x14", [118] * 1024 + [14] * 1024, False),
            ("infer 512 balls", balls, False),
            ("train 1x118+3x14", [118, 14, 14, 14], True),
            ("train 128x118 uniform", [118] * 128, True)]


def _time(step, windows, window_ms):
    import torch
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        step()
    b.record()
    torch.cuda.synchronize()
    est = max(a.elapsed_time(b) / 20, 1e-3)
    n = max(20, int(np.ceil(window_ms / est)))
    for _ in range(n):                                  # one untimed window: clocks ramped, caches and allocator settled
        step()
    per = []
    for _ in range(windows):
        a.record()
        for _ in range(n):
            step()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b) / n)
    return {"ms": round(float(np.median(per)), 4), "min": round(min(per), 4), "max": round(max(per), 4), "steps": n}


def worker(args):
    sys.path.insert(0, args.root)
    import torch
    from poweflownet_amd import _lib as L
    from poweflownet_amd.loss import MSELoss
    from poweflownet_amd.networks.MPN import GraphCSR, MaskEmbdMultiMPN
    from poweflownet_amd.optim import FlatAdamW
    try:
        from poweflownet_amd import segpack
        forget_plans = segpack._layout_of_sorted.cache_clear
    except ImportError:
        segpack, forget_plans = None, (lambda: None)
    if args.reuse_plans:
        forget_plans = lambda: None     # noqa: E731
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.2).to(dev)
    opt, loss_fn = FlatAdamW(model, lr=1e-4), MSELoss()
    res = {"tag": args.tag, "has_segpack": segpack is not None, "reuse_plans": bool(args.reuse_plans), "workloads": {}}
    for name, sizes, train in _workloads():
        batches = [_ragged_batch(sizes, seed).to(dev) for seed in range(4)]
        state = {"i": 0}

        def step():
            d = batches[state["i"] & 3]
            state["i"] += 1
            forget_plans()
            if train:
                opt.zero_grad()
                loss_fn.attach(model, d.y)
                loss = loss_fn(model(d), d.y)
                loss.backward(loss_fn.unit_grad(loss))
                opt.step()
            else:
                with torch.no_grad():
                    model(d)
        model.train(train)
        row = {"graphs": len(sizes), "nodes": int(sum(sizes))}
        for variant, packing in (("packed", True), ("unpacked", False)):
            model.segment_packing = packing
            row[variant] = _time(step, args.windows, args.window_ms)
            row[variant]["took_packed_route"] = getattr(model, "last_segment_plan", None) is not None
            if not args.no_profile and packing:
                L.profile_report(reset=True)
                L.profile_enable(True)
                for _ in range(8):
                    step()
                torch.cuda.synchronize()
                L.profile_enable(False)
                rep = L.profile_report(reset=True)
                row["profile_us_per_step"] = {k: round(1e3 * v["ms"] / 8, 2) for k, v in rep.items()
                                              if not k.startswith("__") and (k.startswith("segpack") or k.startswith("ea_seg")
                                                                             or k.startswith("seg_lin") or k.startswith("front_seg"))}
        model.segment_packing = True
        # the per-batch adjacency build on its own (device events around pfn_graph_build + the unread segment check)
        plan = getattr(model, "last_segment_plan", None)
        d = batches[0]
        with torch.no_grad():
            model(d)
        plan = getattr(model, "last_segment_plan", None)
        ei, n, hint = d.edge_index, d.x.shape[0], 0
        if plan is not None:
            ei, n, hint = torch.zeros_like(d.edge_index), plan.n_pad, plan.S
            ei.copy_(plan.row_of.long()[d.edge_index])
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for rep in range(2):
            a.record()
            for _ in range(50):
                GraphCSR(ei, n, -1, seg_hint=hint, async_checks=True)
            b.record()
            torch.cuda.synchronize()
        row["adjacency_build_us"] = round(1e3 * a.elapsed_time(b) / 50, 2)
        res["workloads"][name] = row
        del batches
    print(json.dumps(res), flush=True)


# ------------------------------------------------------------------------------------------------------ driver
def driver(args):
    runs = {"tree": [], "other": []}
    for pair in range(args.pairs):
        for tag, root in (("tree", HERE), ("other", os.path.abspath(args.ab))):
            cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--tag", tag, "--windows", str(args.windows),
                   "--window-ms", str(args.window_ms)] + (["--no-profile"] if pair else [])
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                sys.stderr.write(out.stdout + out.stderr)
                raise SystemExit(f"ragged_bench: the {tag} run failed (exit {out.returncode})")
            line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
            print(line, flush=True)
            runs[tag].append(json.loads(line))
    print("\nper-step ms, median of the windows; one column per pair (tree | other), spread = max - min over the pairs' medians")
    print(f"{'workload':26s} {'variant':9s} " + " ".join(f"{'pair ' + str(i):>17s}" for i in range(args.pairs)) + "   tree/other  spread(other)")
    for name in runs["tree"][0]["workloads"]:
        for variant in ("packed", "unpacked"):
            t = [r["workloads"][name][variant]["ms"] for r in runs["tree"]]
            o = [r["workloads"][name]["packed"]["ms"] for r in runs["other"]]          # (the other tree's default route)
            cols = " ".join(f"{a:8.4f}|{b:8.4f}" for a, b in zip(t, o))
            took = runs["tree"][0]["workloads"][name][variant]["took_packed_route"]
            print(f"{name:26s} {variant:9s} {cols}   {np.median(t) / np.median(o):9.3f}  {max(o) - min(o):8.4f}"
                  f"{'   [segment route]' if took else ''}")
    first = runs["tree"][0]["workloads"]
    print("\nkernel classes of the packed route, us per step (profile pass of the first run), and the adjacency build alone:")
    for name, row in first.items():
        print(f"{name:26s} adjacency build {row['adjacency_build_us']:8.2f} us   {row.get('profile_us_per_step', {})}")


if __name__ == "__main__":
    a = _args()
    if a.ab:
        driver(a)
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("ragged_bench.py needs a HIP device")
        worker(a)
