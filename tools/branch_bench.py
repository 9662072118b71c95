#!/usr/bin/env python3
"""Per-line branch analysis: the branch pass (`branch_errors_of`: ONE `pfn_branch_flows` call over the finished tables, with its
read-back) against the same quantities in vectorised float64 numpy on the host, and against `bus_error_epoch` alone, whose
predictions it reads.  Not part of bench.py.

    python tools/branch_bench.py                 this tree, one process: one JSON line
    python tools/branch_bench.py --procs 3       three fresh processes (the order of the variants alternates between them), one more
                                                 with PFN_BRANCH_NO_LDS=1 (the direct kernel at every size), then tables

Needs no dataset files: it writes its own sets into a temporary directory -- 4096 samples of case118v2 (batch 128) and 256 samples of
case6470rte (batch 64), one topology each -- and uses configs/standard.json's model with random weights.

(a) host wall time with a device synchronise at either end, median of `--epochs` passes after `--warm`:
    `branch pass`      branch_errors_of on the predictions of a finished bus pass: errors [S, e, 4] left on the device, moments read back
    `host numpy`       predictions, y, edge_index, edge_attr `.cpu()`, then (I, P, Q, loss) of both tables, their difference and its six
                       moments per (line, quantity) in vectorised float64 numpy
    `bus_error_epoch`  the bus pass alone (graphed, keep_predictions=True): what the branch pass comes on top of
(b) device-event time per launch (pfn_profile_*, 200 launches) of the flows and the moments kernel at both sizes.

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
    ap.add_argument("--procs", type=int, default=0, help="the driver: this many fresh worker processes (+ one direct-kernel process), then the tables")
    ap.add_argument("--epochs", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--flip", type=int, default=0, help="worker: 1 = the host computation first")
    ap.add_argument("--direct", type=int, default=0, help="worker: 1 = PFN_BRANCH_NO_LDS=1, kernel times only")
    ap.add_argument("--data", default=None, help="directory for the generated sets (made when absent)")
    ap.add_argument("--worker-timeout", type=int, default=300)
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
        edge[:, :, 2] = rng.uniform(0.01, 0.1, (S, e))
        edge[:, :, 3] = rng.uniform(0.05, 0.5, (S, e))
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


def host_flows(table, ei, rx):
    """(I, P, Q, loss) [S, e, 4] in float64 from physical bus rows [S, n, 4], lines [2, e] and (r, x) [S, e, 2]."""
    t = table.astype(np.float64)
    vm, th = t[:, :, 0], t[:, :, 1] * (np.pi / 180.0)
    ev, fv = vm * np.cos(th), vm * np.sin(th)
    ei_, fi_, ej_, fj_ = ev[:, ei[0]], fv[:, ei[0]], ev[:, ei[1]], fv[:, ei[1]]
    r, x = rx[..., 0], rx[..., 1]
    d = r * r + x * x
    g, b = r / d, -x / d
    de, df = ei_ - ej_, fi_ - fj_
    m2 = de * de + df * df
    t1, t2 = ei_ * ej_ - ei_ ** 2 + fi_ * fj_ - fi_ ** 2, fi_ * ej_ - ei_ * fj_
    return np.stack([np.sqrt(m2) / np.sqrt(d), g * t1 + b * t2, g * t2 - b * t1, g * m2], axis=-1)


def worker(args):
    if args.direct:
        os.environ["PFN_BRANCH_NO_LDS"] = "1"
    sys.path.insert(0, HERE)
    import torch
    from poweflownet_amd import _lib as L
    from poweflownet_amd.data import DataLoader
    from poweflownet_amd.datasets import PowerFlowData
    from poweflownet_amd.loss import branch_flows, branch_moments
    from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
    from poweflownet_amd.utils.branch_analysis import _edge_stats, branch_errors_of
    from poweflownet_amd.utils.error_analysis import bus_error_epoch
    from poweflownet_amd.utils.evaluation import GraphedEvalStep, _std4
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "flip": args.flip, "direct": args.direct, "sets": {}}
    for case, S, batch in SETS:
        ds = PowerFlowData(root=args.data, case=case, split=[1.0, 0.0, 0.0], task="train", device=dev)
        assert len(ds) == S
        blk = ds._blocks[0]
        n, e = int(blk.x.shape[1]), int(blk.edge_index.shape[2])
        torch.manual_seed(0)
        model = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.2).to(dev).eval()
        loader = DataLoader(ds, batch_size=batch, shuffle=False)
        stats = dict(xymean=ds.xymean, xystd=ds.xystd, edgemean=ds.edgemean, edgestd=ds.edgestd)
        step = GraphedEvalStep(model)
        bus_pass = lambda: bus_error_epoch(model, loader, dev, xymean=ds.xymean, xystd=ds.xystd, graph=step, keep_errors=False,      # noqa: E731
                                           keep_predictions=True)
        bus = bus_pass()
        std4, mean4 = _std4(ds.xystd), ds.xymean.reshape(-1)[:4].tolist()
        esd, emu = _edge_stats(ds.edgemean, ds.edgestd)
        a = {}
        if not args.direct:
            def host_numpy():
                pred, y = bus.predictions.cpu().numpy(), blk.y.cpu().numpy()
                ei, ea = blk.edge_index[0].cpu().numpy(), blk.edge_attr.cpu().numpy()
                truth = y.astype(np.float64) * np.asarray(std4) + np.asarray(mean4)
                rx = ea.astype(np.float64) * np.asarray(esd) + np.asarray(emu)
                err = host_flows(pred, ei, rx) - host_flows(truth, ei, rx)
                mom = np.stack([np.full(err.shape[1:], float(err.shape[0])), err.sum(0), np.abs(err).sum(0), (err * err).sum(0), err.min(0),
                                err.max(0)], axis=-1)
                return err, mom
            variants = [("branch_pass", lambda: branch_errors_of(bus, loader, **stats)), ("host_numpy", host_numpy),
                        ("bus_error_epoch", bus_pass)]
            last = {}
            for name, fn in (variants[::-1] if args.flip else variants):
                slow = name == "host_numpy"
                a[name], last[name] = _timed(fn, max(3, args.epochs // 2) if slow else args.epochs, 1 if slow else args.warm)
            got, (want_err, want_mom) = last["branch_pass"], last["host_numpy"]
            a["max_abs_diff_to_host_over_max_abs"] = float(np.abs(got.errors.cpu().numpy() - want_err).max() / np.abs(want_err).max())
            a["max_rel_diff_of_sum_abs"] = float((np.abs(got.moments.numpy()[..., 2] - want_mom[..., 2]) / want_mom[..., 2]).max())
        # (b) the kernels alone
        k = {}
        mom, flags = branch_moments(dev, e), torch.zeros(1, dtype=torch.int32, device=dev)
        outs = [torch.empty(S, e, 4, device=dev) for _ in range(3)]
        common = dict(truth=blk.y, truth_normalised=True, std=std4, mean=mean4, edge_std=esd, edge_mean=emu, flags=flags)
        calls = {
            "branch_flows (errors only)": ("branch_flows", lambda: branch_flows(bus.predictions, blk.edge_index[0], blk.edge_attr, errors=outs[2], **common)),
            "branch_flows (three tables)": ("branch_flows", lambda: branch_flows(bus.predictions, blk.edge_index[0], blk.edge_attr, flows_pred=outs[0],
                                                                                  flows_true=outs[1], errors=outs[2], **common)),
            "branch_moments": ("branch_moments", lambda: branch_flows(bus.predictions, blk.edge_index[0], blk.edge_attr, errors=outs[2], moments=mom,
                                                                      **common)),
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
        res["sets"][case] = {"samples": S, "batch": batch, "buses": n, "lines": e, "a_pass": a, "b_kernel_us": k}
        del step, ds
    print(json.dumps(res), flush=True)


def driver(args, data):
    runs, direct = [], None
    for p in range(args.procs + 1):
        last = p == args.procs
        cmd = ["timeout", "-k", "10", str(args.worker_timeout), sys.executable, os.path.abspath(__file__), "--data", data, "--epochs", str(args.epochs),
               "--warm", str(args.warm), "--flip", str(p % 2), "--direct", str(int(last))]
        out = subprocess.run(cmd, capture_output=True, text=True)
        if out.returncode != 0:                # a fault, an abort, a time limit: nothing more is started
            sys.stderr.write(out.stdout + out.stderr)
            raise SystemExit(f"branch_bench: process {p} failed (exit {out.returncode}); stopping here")
        line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
        print(line, flush=True)
        if last:
            direct = json.loads(line)
        else:
            runs.append(json.loads(line))
    head = " ".join(f"{'proc ' + str(i):>10s}" for i in range(args.procs)) + "     median   spread"

    def row(name, v, unit=None):
        s = f"  {name:52s} " + " ".join(f"{x:10.3f}" for x in v) + f" {np.median(v):10.3f} {max(v) - min(v):8.3f}"
        print(s + (f"   {unit}" if unit else ""))
    for case, S, batch in SETS:
        R = [r["sets"][case] for r in runs]
        print(f"\ncase{case}: {S} samples of {R[0]['buses']} buses and {R[0]['lines']} lines, batch {batch}")
        print(f"(a) one pass, ms (host wall time, median of the process's passes)\n  {'':52s} " + head)
        for name, title in (("branch_pass", "branch pass (one call + read-back)"), ("host_numpy", "host numpy float64 after .cpu()"),
                            ("bus_error_epoch", "bus_error_epoch alone (graphed)")):
            row(title, [r["a_pass"][name]["ms"] for r in R])
        print(f"  worst |error - host's| / max |error|: {max(r['a_pass']['max_abs_diff_to_host_over_max_abs'] for r in R):.2e}; "
              f"worst relative difference of a sum |e|: {max(r['a_pass']['max_rel_diff_of_sum_abs'] for r in R):.2e}")
        print(f"(b) us per launch (event brackets, 200 launches)\n  {'':52s} " + head)
        for title in R[0]["b_kernel_us"]:
            row(title, [r["b_kernel_us"][title] for r in R])
        for title, v in direct["sets"][case]["b_kernel_us"].items():
            print(f"  {title + ', direct kernel (one process)':52s} {v:10.3f}")


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
                raise SystemExit("branch_bench.py needs a HIP device")
            worker(a)
