#!/usr/bin/env python3
"""Evaluation epochs: the eager loops against `GraphedEvalStep`, six `evaluate_epoch_v2` passes against one `evaluate_report`
pass, and train.py's epoch including its validation.  Not part of bench.py.

    python tools/eval_bench.py                    this tree: one JSON line
    python tools/eval_bench.py --ab OTHER_TREE    this tree and OTHER_TREE's package (a built copy of another commit, e.g. the parent)
                                                  alternating, `--pairs` times each, in fresh processes; then the tables
    python tools/eval_bench.py --root TREE        the package under TREE instead of this tree's (what --ab starts)
    python tools/eval_bench.py --pairs 3 --self   this tree alone, three fresh processes, then the tables

The script needs no dataset files: it writes its own case118v2 sets (one topology; 4096 training and 1638 validation samples, the
proportion of train.py's .5 / .2 split) into a temporary directory, once per driver run.  configs/standard.json's model, batch 128.

(a) one validation epoch of `evaluate_epoch` (Masked_L2_loss(regularize=False), train.py's validation loss) over the 4096 samples:
    eager, and -- where the tree has it -- replayed through a `GraphedEvalStep`.
(b) test.py's report over the same set: six `evaluate_epoch_v2` passes against one `evaluate_report` pass (eager and graphed).
(c) train.py's epoch: `train_epoch` through a `GraphedTrainStep` over the 4096 training samples, then `evaluate_epoch` over the 1638
    validation samples (eager / graphed); the validation part is also given on its own.
Host wall time with a device synchronise at either end, median of `--epochs` epochs after `--warm` untimed ones.
(k) the two new kernels alone, device-event time per launch (pfn_profile_*), at 15,104 and 241,664 rows.

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
CASE, S_TRAIN, S_VAL, BATCH = "118v2", 4096, 1638, 128      # train.py's split: validation is 20 % against training's 50 %


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--ab", default=None)
    ap.add_argument("--self", dest="self_only", action="store_true", help="the driver with this tree on both sides")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=9)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--tag", default="tree")
    ap.add_argument("--data", default=None, help="directory holding {train,val}/raw/case118v2_*.npy (made when absent)")
    ap.add_argument("--worker-timeout", type=int, default=300)
    return ap.parse_args()


def make_dataset(root):
    for sub, count, seed in (("train", S_TRAIN, 0), ("val", S_VAL, 1)):
        _make_split(os.path.join(root, sub), count, seed)


def _make_split(root, S_ALL, seed):
    sys.path.insert(0, HERE)
    from poweflownet_amd.synth import CASES, make_topology
    n, e = CASES[CASE]
    rng = np.random.default_rng(seed)
    ei = make_topology(n, e).numpy()
    node = np.zeros((S_ALL, n, 6), dtype=np.float32)
    node[:, :, 0] = np.arange(n)
    node[:, :, 1] = np.where(np.arange(n) == 0, 0, np.where(np.arange(n) % 3 == 0, 1, 2))
    node[:, :, 2:] = rng.normal(size=(S_ALL, n, 4)) * np.array([0.05, 10.0, 50.0, 20.0]) + np.array([1.0, 0.0, 30.0, 10.0])
    edge = np.zeros((S_ALL, e, 4), dtype=np.float32)
    edge[:, :, :2] = ei.T
    edge[:, :, 2:] = np.abs(rng.normal(size=(S_ALL, e, 2))) * 0.1 + 0.01
    os.makedirs(os.path.join(root, "raw"), exist_ok=True)
    np.save(os.path.join(root, "raw", f"case{CASE}_edge_features.npy"), edge)
    np.save(os.path.join(root, "raw", f"case{CASE}_node_features.npy"), node)


# ------------------------------------------------------------------------------------------------------ worker
def _timed(fn, epochs, warm):
    import torch
    per, last = [], None
    for ep in range(warm + epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = fn(ep)
        torch.cuda.synchronize()
        if ep >= warm:
            per.append(1e3 * (time.perf_counter() - t0))
    return {"ms": round(float(np.median(per)), 3), "min": round(min(per), 3), "max": round(max(per), 3)}, last


def worker(args):
    sys.path.insert(0, args.root)
    from functools import partial

    import torch
    from poweflownet_amd import _lib as L
    from poweflownet_amd.data import DataLoader
    from poweflownet_amd.datasets import PowerFlowData, denormalize
    from poweflownet_amd.loss import MSELoss
    from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
    from poweflownet_amd.optim import FlatAdamW
    from poweflownet_amd.utils import evaluation as E
    from poweflownet_amd.utils.custom_loss_functions import Masked_L2_loss, MaskedL1, MaskedL2V2, PowerImbalance
    from poweflownet_amd.utils.training import GraphedTrainStep, train_epoch
    dev = torch.device("cuda:0")
    has_new = hasattr(E, "GraphedEvalStep")
    train = PowerFlowData(root=os.path.join(args.data, "train"), case=CASE, split=[1.0, 0.0, 0.0], task="train", device=dev)
    kw = dict(xymean=train.xymean, xystd=train.xystd, edgemean=train.edgemean, edgestd=train.edgestd)
    val = PowerFlowData(root=os.path.join(args.data, "val"), case=CASE, split=[1.0, 0.0, 0.0], task="train", device=dev, **kw)
    assert len(train) == 4096 and len(val) == 1638
    torch.manual_seed(0)
    model = MaskEmbdMultiMPN(4, 2, 4, 129, 4, 3, 0.2).to(dev)
    opt = FlatAdamW(model, lr=1e-4)
    res = {"tag": args.tag, "device": torch.cuda.get_device_name(0), "has_graphed_eval": has_new}
    big = DataLoader(train, batch_size=BATCH, shuffle=False)
    eval_loss = Masked_L2_loss(regularize=False)

    # (a) one validation epoch over 4096 samples
    a = {}
    a["eager"], v_eager = _timed(lambda ep: E.evaluate_epoch(model, big, eval_loss, dev), args.epochs, args.warm)
    if has_new:
        step = E.GraphedEvalStep(model, eval_loss)
        a["graphed"], v_graph = _timed(lambda ep: E.evaluate_epoch(model, big, eval_loss, dev, graph=step), args.epochs, args.warm)
        a["graphed_equals_eager"] = bool(v_graph == v_eager)
        a["captures"] = step.captures
    a["value"] = v_eager
    res["a_validation_epoch"] = a

    # (b) test.py's report
    stats = [t.cpu() for t in train.get_data_means_stds()]
    mean, std = train.xymean, train.xystd

    def six(ep):
        de = partial(denormalize, mean=mean.cpu(), std=std.cpu())        # as test.py hands them over: host tensors
        out = {}
        for title, loss, pre in (("MaskedL2", MaskedL2V2(), None), ("MaskedL2(denorm)", MaskedL2V2(), de), ("MaskedL1(denorm)", MaskedL1(), de)):
            for k, v in E.evaluate_epoch_v2(model, big, loss, dev, pre_loss_fn=pre).items():
                out[f"{title} {k}"] = v
        for name, loss in (("PowerImbalance", PowerImbalance(*stats)), ("Masked_L2_loss", Masked_L2_loss(regularize=False)), ("MSE", MSELoss())):
            t = E.evaluate_epoch_v2(model, big, loss, dev)
            out[name] = t["total"]
            if "ref" in t:
                out[name + "(ref)"] = t["ref"]
        return out
    b = {}
    b["six_passes"], rep6 = _timed(six, args.epochs, args.warm)
    if has_new:
        pi = PowerImbalance(*stats)
        b["one_pass_eager"], rep1 = _timed(lambda ep: E.evaluate_report(model, big, dev, xystd=std, power_imbalance=pi), args.epochs, args.warm)
        rstep = E.GraphedEvalStep(model)
        b["one_pass_graphed"], rep1g = _timed(lambda ep: E.evaluate_report(model, big, dev, xystd=std, power_imbalance=pi, graph=rstep),
                                              args.epochs, args.warm)
        b["graphed_equals_eager"] = bool(rep1g == rep1)
        b["worst_rel_vs_six_passes"] = {("denorm" if d else "normalised"): max(abs(rep1[k] - rep6[k]) / abs(rep6[k]) for k in rep6 if ("denorm" in k) == d)
                                        for d in (False, True)}
    res["b_report"] = b

    # (c) train.py's epoch: training over 4096 samples, validation over 1638
    train_loss = MSELoss()
    gt = GraphedTrainStep(model, train_loss, opt)
    vloader = DataLoader(val, batch_size=BATCH, shuffle=False)
    c = {}
    for variant in ("eager_validation",) + (("graphed_validation",) if has_new else ()):
        ge = E.GraphedEvalStep(model, eval_loss) if variant == "graphed_validation" else None
        kwv = {"graph": ge} if ge is not None else {}
        parts = {"train": [], "val": []}

        def epoch(ep):
            loader = DataLoader(train, batch_size=BATCH, shuffle=True, generator=torch.Generator().manual_seed(ep))
            t0 = time.perf_counter()
            train_epoch(model, loader, train_loss, opt, dev, graph=gt)      # (ends with its read-back)
            t1 = time.perf_counter()
            v = E.evaluate_epoch(model, vloader, eval_loss, dev, **kwv)
            t2 = time.perf_counter()
            if ep >= args.warm:
                parts["train"].append(1e3 * (t1 - t0))
                parts["val"].append(1e3 * (t2 - t1))
            return v
        c[variant], _ = _timed(epoch, args.epochs, args.warm)
        c[variant]["train_ms"] = round(float(np.median(parts["train"])), 3)
        c[variant]["val_ms"] = round(float(np.median(parts["val"])), 3)
        c[variant]["val_share"] = round(c[variant]["val_ms"] / c[variant]["ms"], 4)
    res["c_train_epoch_with_validation"] = c

    # (k) the new kernels alone
    if has_new:
        from poweflownet_amd.loss import _Workspace, eval_accumulate, eval_accumulator, eval_metrics
        k = {}
        for rows in (15104, 241664):
            o, y, x = (torch.randn(rows, 4, device=dev) for _ in range(3))
            m = torch.randint(0, 2, (rows, 4), device=dev)
            acc, ws, mixed = eval_accumulator(dev, 1, L.EVAL_ACC_DOUBLES).view(-1), _Workspace(L.EVAL_WS_FLOATS), torch.empty_like(o)
            terms = torch.empty(len(L.EVAL_TERMS), device=dev)
            for with_mixed in (False, True):
                def call():
                    eval_metrics(o, y, m, x=x if with_mixed else None, std=(0.05, 10.0, 50.0, 20.0), weight=8.0, first_unweighted=True,
                                 acc=acc, mixed_out=mixed if with_mixed else None, terms=terms, workspace=ws)
                for _ in range(50):
                    call()
                torch.cuda.synchronize()
                L.profile_enable(True)
                for _ in range(200):
                    call()
                rep = L.profile_report(True)
                L.profile_enable(False)
                k[f"eval_metrics {rows} rows{' + mixed_out' if with_mixed else ''}"] = round(1e3 * rep["eval_metrics"]["ms"] / rep["eval_metrics"]["count"], 2)
        loss, acc2 = torch.ones((), device=dev), eval_accumulator(dev).view(-1)
        for _ in range(50):
            eval_accumulate(loss, acc2, 8.0)
        torch.cuda.synchronize()
        L.profile_enable(True)
        for _ in range(200):
            eval_accumulate(loss, acc2, 8.0)
        rep = L.profile_report(True)
        L.profile_enable(False)
        k["eval_accumulate"] = round(1e3 * rep["eval_accumulate"]["ms"] / rep["eval_accumulate"]["count"], 2)
        res["k_kernel_us"] = k
    print(json.dumps(res), flush=True)


# ------------------------------------------------------------------------------------------------------ driver
def _row(name, v, unit_count=None):
    s = f"  {name:44s} " + " ".join(f"{x:9.3f}" for x in v) + f" {np.median(v):9.3f} {max(v) - min(v):8.3f}"
    if unit_count:
        s += f" {unit_count / np.median(v):9.0f} k graphs/s"
    print(s)


def _verdict(what, parent, new):
    spread = max(max(parent) - min(parent), max(new) - min(new))
    gain = float(np.median(parent) - np.median(new))
    ok = gain > spread
    print(f"  {what}: gain {gain:8.3f} ms ({100 * gain / np.median(parent):5.1f} %), observed spread {spread:.3f} -> "
          f"{'beats it' if ok else 'inside the spread'}")
    return ok


def driver(args, data):
    runs = {"tree": [], "other": []}
    for pair in range(args.pairs):
        for tag, root in (("tree", HERE), ("other", os.path.abspath(args.ab))):
            cmd = ["timeout", "-k", "10", str(args.worker_timeout), sys.executable, os.path.abspath(__file__), "--root", root, "--tag", tag,
                   "--data", data, "--epochs", str(args.epochs), "--warm", str(args.warm)]
            out = subprocess.run(cmd, capture_output=True, text=True)
            if out.returncode != 0:            # a fault, an abort, a time limit: nothing more is started
                sys.stderr.write(out.stdout + out.stderr)
                raise SystemExit(f"eval_bench: the {tag} run of pair {pair} failed (exit {out.returncode}); stopping here")
            line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
            print(line, flush=True)
            runs[tag].append(json.loads(line))
    T, O = runs["tree"], runs["other"]
    head = " ".join(f"{'pair ' + str(i):>9s}" for i in range(args.pairs)) + "    median   spread"
    print(f"\n(a) evaluate_epoch over 4096 samples, batch {BATCH} (32 batches), ms per epoch (host wall time, median of {args.epochs} epochs)")
    print(f"  {'':44s} " + head)
    pa = [r["a_validation_epoch"]["eager"]["ms"] for r in O]
    _row("other: eager", pa, 4096)
    _row("tree:  eager", [r["a_validation_epoch"]["eager"]["ms"] for r in T], 4096)
    verdicts = {}
    if T[0]["has_graphed_eval"]:
        g = [r["a_validation_epoch"]["graphed"]["ms"] for r in T]
        _row("tree:  graphed (GraphedEvalStep)", g, 4096)
        print(f"  graphed == eager (float equality) in every run: {all(r['a_validation_epoch']['graphed_equals_eager'] for r in T)}")
        verdicts["a"] = _verdict("graphed against the other tree's eager epoch", pa, g)
    print(f"\n(b) test.py's report over the same set, ms")
    print(f"  {'':44s} " + head)
    pb = [r["b_report"]["six_passes"]["ms"] for r in O]
    _row("other: six evaluate_epoch_v2 passes", pb)
    _row("tree:  six evaluate_epoch_v2 passes", [r["b_report"]["six_passes"]["ms"] for r in T])
    if T[0]["has_graphed_eval"]:
        e1 = [r["b_report"]["one_pass_eager"]["ms"] for r in T]
        g1 = [r["b_report"]["one_pass_graphed"]["ms"] for r in T]
        _row("tree:  one evaluate_report pass, eager", e1)
        _row("tree:  one evaluate_report pass, graphed", g1)
        print(f"  worst relative difference to the six passes: {T[0]['b_report']['worst_rel_vs_six_passes']}")
        verdicts["b one pass"] = _verdict("one eager pass against the other tree's six passes", pb, e1)
        verdicts["b graphed"] = _verdict("one graphed pass against the one eager pass", e1, g1)
    print(f"\n(c) train.py's epoch: train_epoch (hipGraph) over 4096 samples + evaluate_epoch over 1638, ms")
    print(f"  {'':44s} " + head)
    pc = [r["c_train_epoch_with_validation"]["eager_validation"]["ms"] for r in O]
    _row("other: epoch, eager validation", pc)
    _row("other:   of which validation", [r["c_train_epoch_with_validation"]["eager_validation"]["val_ms"] for r in O], 1638)
    print(f"  other: validation's share of the epoch: "
          + " ".join(f"{100 * r['c_train_epoch_with_validation']['eager_validation']['val_share']:.1f} %" for r in O))
    _row("tree:  epoch, eager validation", [r["c_train_epoch_with_validation"]["eager_validation"]["ms"] for r in T])
    if T[0]["has_graphed_eval"]:
        gc_ = [r["c_train_epoch_with_validation"]["graphed_validation"]["ms"] for r in T]
        _row("tree:  epoch, graphed validation", gc_)
        _row("tree:    of which validation", [r["c_train_epoch_with_validation"]["graphed_validation"]["val_ms"] for r in T], 1638)
        _row("tree:    of which training", [r["c_train_epoch_with_validation"]["graphed_validation"]["train_ms"] for r in T], 4096)
        verdicts["c"] = _verdict("epoch with graphed validation against the other tree's epoch", pc, gc_)
        print(f"\n(k) the new kernels, us per launch (event brackets, 200 launches): {T[0]['k_kernel_us']}")
        for r in T[1:]:
            print(f"    {r['k_kernel_us']}")
    if verdicts:
        print(f"\nverdict: " + "; ".join(f"({k}) {'faster than the spread' if v else 'NOT faster than the spread'}" for k, v in verdicts.items()))


if __name__ == "__main__":
    a = _args()
    if a.self_only:
        a.ab = HERE
    raw = lambda d: os.path.join(d, "val", "raw", f"case{CASE}_edge_features.npy")      # noqa: E731
    if a.ab:
        with tempfile.TemporaryDirectory() as tmp:
            data = a.data or tmp
            if not os.path.exists(raw(data)):
                make_dataset(data)
            driver(a, data)
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("eval_bench.py needs a HIP device")
        if a.data is None:
            with tempfile.TemporaryDirectory() as tmp:
                make_dataset(tmp)
                a.data = tmp
                worker(a)
        else:
            if not os.path.exists(raw(a.data)):
                make_dataset(a.data)
            worker(a)
