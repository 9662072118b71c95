#!/usr/bin/env python3
"""Measurements behind DESIGN 7s (measured, not asserted; needs the GPU):

  * per-sample forward latency of MPN / GCN / MLP at batch 1, case14 and case118: the wall time of `model(sample)` between two
    device synchronisations, median and spread over `--reps` calls after `--warmup` calls;
  * forward + backward of ONE GCNConv(129, 129) at case118 x 128 (15 104 nodes, 23 808 stored lines): the HIP layer next to the
    same layer composed from torch ops on the device in fp32 (`index_add_` over the list with self loops; the normalisation
    weights are formed once outside the timed window, as the HIP layer's adjacency is).  Device events around `--inner` calls per
    sample, the two versions ALTERNATING within one process, median and spread over `--reps` samples.  The two outputs and weight
    gradients are compared first, so the timed versions compute the same thing.

Prints one JSON line; `--out FILE` also writes it there."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from poweflownet_amd.networks.GCN import GCN, GCNConv
from poweflownet_amd.networks.MLP import MLP
from poweflownet_amd.networks.MPN import GraphCSR, MaskEmbdMultiMPN
from poweflownet_amd.synth import make_batch

DEV = "cuda:0"


def _spread(xs):
    xs = sorted(xs)
    return {"median": statistics.median(xs), "min": xs[0], "p90": xs[min(len(xs) - 1, int(0.9 * len(xs)))], "n": len(xs)}


@torch.no_grad()
def latency(model, sample, warmup, reps):
    for _ in range(warmup):
        model(sample)
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model(sample)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return _spread(out)                                                        # microseconds


def torch_gcn_layer(ei, n):
    """GCNConv's forward as torch device ops (fp32): returns f(x, w, b) -> out."""
    src, dst = ei[0], ei[1]
    keep = src != dst
    loop = torch.arange(n, device=ei.device)
    src, dst = torch.cat([src[keep], loop]), torch.cat([dst[keep], loop])
    deg = torch.zeros(n, device=ei.device).index_add_(0, dst, torch.ones(src.shape[0], device=ei.device))
    dis = deg.pow(-0.5)
    norm = (dis[src] * dis[dst]).unsqueeze(1)

    def f(x, w, b):
        h = x @ w.t()
        return torch.zeros_like(h).index_add_(0, dst, h[src] * norm) + b
    return f


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner                                     # microseconds per call


def layer_bench(warmup, reps, inner):
    data = make_batch("118", 128).to(DEV)
    n, ei = int(data.x.shape[0]), data.edge_index
    torch.manual_seed(0)
    layer = GCNConv(129, 129).to(DEV)
    with torch.no_grad():
        layer.bias.normal_(0.0, 0.1)
    graph = GraphCSR(ei, n, 0)
    x = torch.randn(n, 129, device=DEV, requires_grad=True)
    cot = torch.randn(n, 129, device=DEV)
    w, b = layer.lin.weight, layer.bias
    composed = torch_gcn_layer(ei, n)

    def hip():
        x.grad = w.grad = b.grad = None
        layer.on_graph(graph, x).backward(cot)

    def ref():
        x.grad = w.grad = b.grad = None
        composed(x, w, b).backward(cot)

    hip()
    got = (layer.on_graph(graph, x).detach(), x.grad.clone(), w.grad.clone(), b.grad.clone())
    ref()
    want = (composed(x, w, b).detach(), x.grad.clone(), w.grad.clone(), b.grad.clone())
    agree = [float((g - t).abs().max() / t.abs().max()) for g, t in zip(got, want)]
    for _ in range(warmup):
        hip()
        ref()
    t_hip, t_ref = [], []
    for _ in range(reps):                                                      # alternating, same process
        t_hip.append(timed(hip, inner))
        t_ref.append(timed(ref, inner))
    return {"nodes": n, "stored_edges": int(ei.shape[1]), "hip_us": _spread(t_hip), "torch_us": _spread(t_ref),
            "max_rel_diff_out_gx_gw_gb": agree}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("baselines_bench.py needs a HIP device")
    res = {"latency_us": {}}
    for case, n_bus in (("14", 14), ("118", 118)):
        sample = make_batch(case, 1).to(DEV)
        models = {"MPN": MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.2), "GCN": GCN(4, 4, 129), "MLP": MLP(n_bus * 4, n_bus * 4, 128, 3, 0.2)}
        res["latency_us"][case] = {k: latency(m.to(DEV).eval(), sample, args.warmup, args.reps) for k, m in models.items()}
    res["gcn_conv_129_129_case118_x128_fwd_bwd"] = layer_bench(args.warmup, max(10, args.reps // 4), args.inner)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
