#!/usr/bin/env python3
"""Per-bus error analysis: `bus_error_epoch` (graphed and eager) against the reference-style loop, the histogram launch against the
host's n x 4 np.histogram calls, and the two kernels alone.  Not part of bench.py.

    python tools/error_bench.py                 this tree, one process: one JSON line
    python tools/error_bench.py --procs 3       three fresh processes (the order of the variants alternates between them), then tables

Needs no dataset files: it writes its own sets into a temporary directory -- 4096 samples of case118v2 (batch 128) and 256 samples of
case6470rte (batch 64), one topology each -- and uses configs/standard.json's model with random weights.

(a) one pass over the set, host wall time with a device synchronise at either end, median of `--epochs` passes after `--warm`:
    `bus_error_epoch` through a `GraphedEvalStep`, `bus_error_epoch` eager, and the REFERENCE-STYLE loop run on this package (reference
    error_per_feature.py:127-156: one forward per sample, `.cpu()` per sample, torch.stack, de-normalise and subtract on the host).
(b) `pfn_bus_errors_histogram` at 300 bins over the finished table (wall time incl. the edges' upload) against the n x 4 np.histogram
    calls on the host (reference :401-404), on the same scaled errors; the counts are compared.
(c) device-event time per launch (pfn_profile_*, 200 launches) of the two kernels at both sizes, next to pfn_eval_metrics on the same
    rows.

The driver starts every process under its own `timeout -k 10` and stops at the first one that fails: nothing is started after a
fault."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = (("118v2", 4096, 128), ("6470rte", 256, 64))


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=0, help="the driver: this many fresh worker processes, then the tables")
    ap.add_argument("--epochs", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--flip", type=int, default=0, help="worker: 1 = the reference-style loop first")
    ap.add_argument("--data", default=None, help="directory for the generated sets (made when absent)")
    ap.add_argument("--worker-timeout", type=int, default=420)
    return ap.parse_args()


def make_sets(root):
    sys.path.insert(0, HERE)
    from poweflownet_amd.synth import CASES, make_topology
    for case, S, _ in SETS:
        n, e = CASES[case]
        rng = np.random.default_rng(n)
        node = np.zeros((S, n, 6), dtype=np.float32)
        node[:, :, 0] = np.arange(n)
        node[:, :, 1] = np.where(np.arange(n) == 0, 0, np.where(np.arange(n) % 3 == 0, 1, 2))
        node[:, :, 2:] = rng.normal(size=(S, n, 4)) * np.array([0.05, 10.0, 50.0, 20.0]) + np.array([1.0, 0.0, 30.0, 10.0])
        edge = np.zeros((S, e, 4), dtype=np.float32)
        edge[:, :, :2] = make_topology(n, e).numpy().T
        edge[:, :, 2:] = np.abs(rng.normal(size=(S, e, 2))) * 0.1 + 0.01
        os.makedirs(os.path.join(root, "raw"), exist_ok=True)
        np.save(os.path.join(root, "raw", f"case{case}_edge_features.npy"), edge)
        np.save(os.path.join(root, "raw", f"case{case}_node_features.npy"), node)


def _timed(fn, epochs, warm):
    import torch
    per, last = [], None
    for ep in range(warm + epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = fn()
        torch.cuda.synchronize()
        if ep >= warm:
            per.append(1e3 * (time.perf_counter() - t0))
    return {"ms": round(float(np.median(per)), 3), "min": round(min(per), 3), "max": round(max(per), 3)}, last


def worker(args):
    sys.path.insert(0, HERE)
    import torch
    from poweflownet_amd import _lib as L
    from poweflownet_amd.data import DataLoader
    from poweflownet_amd.datasets import PowerFlowData
    from poweflownet_amd.loss import (_Workspace, bus_error_moments, bus_errors_accumulate, bus_errors_histogram, eval_accumulator,
                                      eval_metrics)
    from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
    from poweflownet_amd.utils.error_analysis import bus_error_epoch, bus_error_histograms, histogram_edges, mask_scale
    from poweflownet_amd.utils.evaluation import GraphedEvalStep
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "flip": args.flip, "sets": {}}
    for case, S, batch in SETS:
        ds = PowerFlowData(root=args.data, case=case, split=[1.0, 0.0, 0.0], task="train", device=dev)
        assert len(ds) == S
        n = int(ds[0].x.shape[0])
        torch.manual_seed(0)
        model = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.2).to(dev).eval()
        loader = DataLoader(ds, batch_size=batch, shuffle=False)
        mean, std = ds.xymean, ds.xystd
        step = GraphedEvalStep(model)

        @torch.no_grad()
        def reference_loop():
            preds, targets = [], []
            for i in range(len(ds)):
                sample = ds.collate_indices([i])                   # (a batch of one: the model reads `batch`)
                preds.append(model(sample).detach().cpu())
                targets.append(sample.y.detach().cpu())
            m, s = mean[0].cpu(), std[0].cpu()
            return (torch.stack(preds, dim=0) * s + m) - (torch.stack(targets, dim=0) * s + m)

        variants = [("graphed", lambda: bus_error_epoch(model, loader, dev, xymean=mean, xystd=std, graph=step)),
                    ("eager", lambda: bus_error_epoch(model, loader, dev, xymean=mean, xystd=std)),
                    ("reference_loop", reference_loop)]
        a, last = {}, {}
        for name, fn in (variants[::-1] if args.flip else variants):
            a[name], last[name] = _timed(fn, args.epochs if name != "reference_loop" else max(2, args.epochs // 3), args.warm if name != "reference_loop" else 1)
        a["graphed_equals_eager"] = bool(torch.equal(last["graphed"].errors, last["eager"].errors) and
                                         torch.equal(last["graphed"].moments, last["eager"].moments))
        a["captures"] = step.captures
        # the reference subtracts two de-normalised values (up to 7.6e-5 relative off in fp32, include/pfn_hip.h); recorded only
        ref = last["reference_loop"].to(dev)
        a["max_abs_diff_to_reference_loop_over_max_abs"] = float((last["graphed"].errors - ref).abs().max() / ref.abs().max())

        # (b) the histograms
        got = last["graphed"]
        scale = mask_scale(got.mask0)
        edges = histogram_edges(got.moments, scale)
        b = {}
        b["device_launch"], (hist, outside) = _timed(lambda: bus_error_histograms(got.errors, edges, scale), args.epochs, args.warm)
        scaled = got.errors.cpu().numpy() * scale.numpy()[None]

        def host_histograms():
            out = np.zeros((n, 4, 300), dtype=np.int64)
            for f in range(4):
                for bus in range(n):
                    out[bus, f], _ = np.histogram(scaled[:, bus, f], bins=edges[f], density=False)
            return out
        b["host_np_histogram"], want = _timed(host_histograms, 3, 1)
        b["calls"] = 4 * n
        b["counts_equal"] = bool(np.array_equal(hist.cpu().numpy(), want))

        # (c) the kernels alone
        k = {}
        rows = n * batch
        o, y = torch.randn(rows, 4, device=dev), torch.randn(rows, 4, device=dev)
        m = ds[0].pred_mask.repeat(batch, 1).contiguous()
        idx = torch.arange(batch, device=dev)
        tabs = torch.empty(2, batch, n, 4, device=dev)
        mom, flags = bus_error_moments(dev, n), torch.zeros(1, dtype=torch.int32, device=dev)
        acc, ws, terms = eval_accumulator(dev, 1, L.EVAL_ACC_DOUBLES).view(-1), _Workspace(L.EVAL_WS_FLOATS), torch.empty(len(L.EVAL_TERMS), device=dev)
        edges_dev = torch.from_numpy(edges).to(dev)
        calls = {
            "bus_errors_accumulate (errors + moments)": ("bus_errors_accumulate", lambda: bus_errors_accumulate(
                o, y, m, n, idx, mom, flags, std=(0.05, 10.0, 50.0, 20.0), mean=(1.0, 0.0, 30.0, 10.0), err_table=tabs[0])),
            "bus_errors_accumulate (both tables)": ("bus_errors_accumulate", lambda: bus_errors_accumulate(
                o, y, m, n, idx, mom, flags, std=(0.05, 10.0, 50.0, 20.0), mean=(1.0, 0.0, 30.0, 10.0), err_table=tabs[0], pred_table=tabs[1])),
            "eval_metrics (same rows)": ("eval_metrics", lambda: eval_metrics(o, y, m, std=(0.05, 10.0, 50.0, 20.0), weight=8.0,
                                                                              first_unweighted=True, acc=acc, terms=terms, workspace=ws)),
            f"bus_errors_histogram ({S} samples, 300 bins)": ("bus_errors_histogram", lambda: bus_errors_histogram(got.errors, edges_dev, scale.to(dev))),
        }
        for title, (klass, call) in calls.items():
            for _ in range(20):
                call()
            torch.cuda.synchronize()
            L.profile_report(True)
            L.profile_enable(True)
            for _ in range(200):
                call()
            rep = L.profile_report(True)
            L.profile_enable(False)
            k[title] = round(1e3 * rep[klass]["ms"] / rep[klass]["count"], 2)
        res["sets"][case] = {"samples": S, "batch": batch, "buses": n, "a_epoch": a, "b_histograms": b, "c_kernel_us": k}
        del step, ds
    print(json.dumps(res), flush=True)


def driver(args, data):
    runs = []
    for p in range(args.procs):
        cmd = ["timeout", "-k", "10", str(args.worker_timeout), sys.executable, os.path.abspath(__file__), "--data", data, "--epochs", str(args.epochs),
               "--warm", str(args.warm), "--flip", str(p % 2)]
        out = subprocess.run(cmd, capture_output=True, text=True)
        if out.returncode != 0:                # a fault, an abort, a time limit: nothing more is started
            sys.stderr.write(out.stdout + out.stderr)
            raise SystemExit(f"error_bench: process {p} failed (exit {out.returncode}); stopping here")
        line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
        print(line, flush=True)
        runs.append(json.loads(line))
    head = " ".join(f"{'proc ' + str(i):>10s}" for i in range(args.procs)) + "     median   spread"

    def row(name, v, unit=None):
        s = f"  {name:52s} " + " ".join(f"{x:10.3f}" for x in v) + f" {np.median(v):10.3f} {max(v) - min(v):8.3f}"
        print(s + (f"   {unit}" if unit else ""))
    for case, S, batch in SETS:
        R = [r["sets"][case] for r in runs]
        print(f"\ncase{case}: {S} samples of {R[0]['buses']} buses, batch {batch}")
        print(f"(a) one pass, ms (host wall time, median of the process's passes)\n  {'':52s} " + head)
        for name in ("graphed", "eager", "reference_loop"):
            v = [r["a_epoch"][name]["ms"] for r in R]
            row(f"{name}", v, f"{S / np.median(v):8.1f} k samples/s")
        print(f"  graphed == eager (bit for bit) in every process: {all(r['a_epoch']['graphed_equals_eager'] for r in R)}; captures {R[0]['a_epoch']['captures']}; "
              f"worst |difference| to the reference-style loop / max |error|: {max(r['a_epoch']['max_abs_diff_to_reference_loop_over_max_abs'] for r in R):.2e}")
        print(f"(b) 300-bin histograms of {4 * R[0]['buses']} (bus, feature) pairs, ms\n  {'':52s} " + head)
        row("pfn_bus_errors_histogram (one launch + edge upload)", [r["b_histograms"]["device_launch"]["ms"] for r in R])
        row(f"{R[0]['b_histograms']['calls']} np.histogram calls on the host", [r["b_histograms"]["host_np_histogram"]["ms"] for r in R])
        print(f"  counts equal in every process: {all(r['b_histograms']['counts_equal'] for r in R)}")
        print(f"(c) us per launch (event brackets, 200 launches)\n  {'':52s} " + head)
        for title in R[0]["c_kernel_us"]:
            row(title, [r["c_kernel_us"][title] for r in R])


if __name__ == "__main__":
    a = _args()
    with tempfile.TemporaryDirectory() as tmp:
        data = a.data or tmp
        if not os.path.exists(os.path.join(data, "raw", f"case{SETS[-1][0]}_node_features.npy")):
            make_sets(data)
        a.data = data
        if a.procs > 0:
            driver(a, data)
        else:
            import torch
            if not torch.cuda.is_available():
                raise SystemExit("error_bench.py needs a HIP device")
            worker(a)
