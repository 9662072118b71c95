#!/usr/bin/env python3
"""Solver-against-model comparison, the counterpart of the reference's speedup_evaluator.py: on the test split of a dataset on disk,
how long do the classical solvers take per sample, how long does the model, and how many solves does the model's prediction save
when the solver starts from it?  The reference times `pp.runpp(algorithm="nr", init="auto")` and `pp.rundcpp` per sample on the
host, names `fdbx` / `fdxb` in its algorithm list, and keeps the run from the GNN's prediction (`init="results"`) and the GNN's own
time in a commented-out block; here every row is one batched `solve_power_flow` launch on the device (csrc/powerflow.hip):

    NR flat, NR from the prediction, fdxb / fdbx flat and from the prediction, DC, the model's forward alone,
    `Loss DC` (dc_error.py's: Masked_L2 of the normalised DC table against the NR truth, Vm and Q mask columns zeroed) and
    `Loss result_init` (Masked_L2 of the normalised NR-from-prediction table against the normalised NR-flat table, the samples'
    prediction mask).

    python speedup_evaluator.py --case 118 --data-dir data [--run-id <id>] [--samples 1000] [--split .5 .2 .3] [--route sparse] [--cfg_json configs/standard.json]

Per method: seconds per sample -- DEVICE time around the call from HIP events, one warm-up call excluded, median of 5 --, the
solves used (mean and max over the converged samples; half-iterations in the fast-decoupled rows) and the failures.  tol 1e-8;
max_iter 10 for NR and DC, 60 half-iterations for the fast-decoupled rows.  The checkpoint is models/model_<run-id>.pt (normalised
with `<data-dir>/params/data_params_<run-id>.pt` where it exists); without `--run-id` the model keeps its random initialisation and
the output says so -- the "from the prediction" rows then show what a bad start costs, not what a trained model saves.  The
solver inputs are read as dc_error.py reads them.  No plots.

A case with more unknowns than the dense solver takes (6470rte) runs every solver row on the sparse route (csrc/powerflow_sparse.hip
for NR and DC, csrc/powerflow_sparse_fd.hip for the fast-decoupled rows, which keep the sparse factors of B' and B'' instead of
their dense inverses); `--route sparse` forces that route at any size.  One plan per kind -- "ac", "dc" and one "fd" plan for the
four fast-decoupled rows -- is built once, before the timing.  A perturbed set (one line list per sample) takes the same route in
chunks of samples that share a cover plan each (utils/powerflow.py CoverChunker), planned before the timing too; a row's time then
covers every chunk's map launch and masked solve."""
import os
import sys

import numpy as np

TOL, NR_ITERS, FD_ITERS, REPEATS = 1e-8, 10, 60, 5


def _take(argv, flag, default=None):
    if flag not in argv:
        return default
    i = argv.index(flag)
    value = argv[i + 1]
    del argv[i:i + 2]
    return value


def device_seconds(fn, repeats=REPEATS):
    """(median device seconds of `fn()` over `repeats` calls after one warm-up call, the last call's result)."""
    import torch
    out = fn()
    times = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e-3)
    return float(np.median(times)), out


def evaluate(root, case, model, samples=1000, device="cuda:0", batch_size=128, xy=None, split=(.5, .2, .3), route="auto"):
    """The rows as a dict: name -> {"seconds_per_sample", "solves_mean", "solves_max", "failures"} for the solver rows,
    "GNN" -> {"seconds_per_sample"}, and the two losses.  `xy`: (xymean, xystd, edgemean, edgestd) saved with the run, None: the
    split's own.  `split`: the train / val / test fractions (they must cover the set, as `PowerFlowData` demands).  `route`: "auto"
    (the sparse route where the case is beyond the dense solver) or "sparse"; "route" in the result says which ran."""
    if route not in ("auto", "sparse"):
        raise ValueError(f"speedup_evaluator: route must be 'auto' or 'sparse', not {route!r}")
    import torch
    import dc_error
    from poweflownet_amd.data import DataLoader
    from poweflownet_amd.utils.custom_loss_functions import Masked_L2_loss
    from poweflownet_amd.utils.error_analysis import bus_error_epoch
    from poweflownet_amd.utils.powerflow import CoverChunker, max_unknowns, solve_power_flow, solve_power_flow_covered, sparse_plan
    testset, node, edge = dc_error.load_test_split(root, case, samples, tuple(split))
    if xy is not None:
        testset = type(testset)(root=root, case=case, split=list(split), task="test", xymean=xy[0], xystd=xy[1], edgemean=xy[2], edgestd=xy[3])
    S = len(node)
    testset.to(device)
    mean, std = testset.xymean[0].double().to(device), testset.xystd[0].double().to(device)
    bus_type = torch.from_numpy(node[0, :, 1].astype(np.int64)).to(device)
    spec, ei, rx = dc_error.solver_inputs(node, edge, device)
    # beyond the dense solver: the sparse route, one plan per mode -- for one line list shared by the samples, or, where every sample
    # has its own (a perturbed set), per chunk of samples on the chunk's cover list (planned before the clock starts, as the one is)
    sparse = route == "sparse" or (node.shape[1] - 1) + int((node[0, :, 1] == 2).sum()) > max_unknowns()
    plans, covers = {}, {}
    if sparse and not bool((edge[:, :, :2] == edge[:1, :, :2]).all()):
        for mode in ("ac", "dc", "fd"):
            chunker = CoverChunker(bus_type, ei[0].contiguous(), mode)
            covers[mode] = (chunker, list(chunker.plans(ei)))
        covers["fdxb"] = covers["fdbx"] = covers["fd"]
    elif sparse:
        ei = ei[0].contiguous()
        plans = {mode: sparse_plan(bus_type, ei, mode) for mode in ("ac", "dc", "fd")}
        plans["fdxb"] = plans["fdbx"] = plans["fd"]
    # ---- the model: the de-normalised prediction table of the whole split (rows in file order), then its forward alone
    loader = DataLoader(testset, batch_size=batch_size, shuffle=False)
    pred = bus_error_epoch(model, loader, device, xymean=testset.xymean, xystd=testset.xystd, keep_errors=False, keep_predictions=True)
    if pred.flags & 1:
        raise RuntimeError("speedup_evaluator: a batch named a sample outside the table")
    init = pred.predictions[:S]
    batches = [b.to(device) for b in loader]

    @torch.no_grad()
    def forward():
        for b in batches:
            model(b)
    rows = {"GNN": {"seconds_per_sample": device_seconds(forward)[0] / len(testset)}}
    # ---- the solvers
    tables = {}
    for name, mode, start in (("nr", "ac", None), ("nr_result_init", "ac", init), ("fdxb", "fdxb", None), ("fdbx", "fdbx", None),
                              ("fdxb_result_init", "fdxb", init), ("fdbx_result_init", "fdbx", init), ("dc", "dc", None)):
        iters = FD_ITERS if mode.startswith("fd") else NR_ITERS
        kw = {"route": "sparse", "plan": plans[mode]} if sparse and not covers else {}
        if covers:
            sec, res = device_seconds(lambda: solve_power_flow_covered(covers[mode][0], spec, ei, rx, plans=covers[mode][1], mode=mode, tol=TOL,
                                                                       max_iter=iters, init=start)[0])
        else:
            sec, res = device_seconds(lambda: solve_power_flow(bus_type, spec, ei, rx, mode=mode, tol=TOL, max_iter=iters, init=start, **kw))
        status = res.status.cpu().numpy()
        ok = status[status >= 0]
        rows[name] = {"seconds_per_sample": sec / S, "solves_mean": float(ok.mean()) if len(ok) else float("nan"),
                      "solves_max": int(ok.max()) if len(ok) else -1, "failures": int((status < 0).sum())}
        tables[name] = res.table
    # ---- the losses
    rows["loss_dc"] = float(dc_error.dc_losses(root, case, samples, tol=TOL, max_iter=NR_ITERS, device=device, split=tuple(split)).mean())
    mask = torch.tensor(type(testset).bus_type_mask)[bus_type.cpu()].to(device)
    loss_fn = Masked_L2_loss(regularize=False)
    a, b = ((tables["nr_result_init"] - mean) / std).float(), ((tables["nr"] - mean) / std).float()
    both = (~torch.isnan(a).flatten(1).any(1) & ~torch.isnan(b).flatten(1).any(1)).tolist()
    losses = [float(loss_fn(a[s], b[s], mask)) for s in range(S) if both[s]]
    rows["loss_result_init"] = float(np.mean(losses)) if losses else float("nan")
    rows["samples"] = S
    rows["route"] = "sparse" if sparse else "dense"
    return rows


def report(rows):
    def solver(name):
        r = rows[name]
        return [f"{name}: {r['seconds_per_sample']}",
                f"{name} solves: mean {r['solves_mean']:.3f} max {r['solves_max']} failures {r['failures']}"]
    lines = ["", "", "===========================================", "Results with auto_init:", ""]
    for name in ("nr", "fdxb", "fdbx"):
        lines += solver(name)
    lines += ["-------------------------------------------", f"GNNs:  {rows['GNN']['seconds_per_sample']}",
              "-------------------------------------------", "Results with results init: ", ""]
    for name in ("nr_result_init", "fdxb_result_init", "fdbx_result_init"):
        lines += solver(name)
    lines += [f"Loss result_init: {rows['loss_result_init']}", "-------------------------------------------", "Results DC: ", ""]
    lines += solver("dc")
    lines += [f"Loss DC: {rows['loss_dc']}", "", "", "==========================================="]
    return lines


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    run_id = _take(argv, "--run-id")
    samples = int(_take(argv, "--samples", default=1000))
    route = _take(argv, "--route", default="auto")
    split = (.5, .2, .3)
    if "--split" in argv:
        i = argv.index("--split")
        split = tuple(float(v) for v in argv[i + 1:i + 4])
        del argv[i:i + 4]
    import torch
    from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN, MPN_simplenet
    from poweflownet_amd.utils.argument_parser import argument_parser
    from poweflownet_amd.utils.evaluation import load_model
    args = argument_parser(argv)
    if not torch.cuda.is_available():
        raise SystemExit("speedup_evaluator.py needs a HIP device: poweflownet_amd has no CPU solver and no CPU model")
    device = torch.device("cuda:0")
    model = {"MaskEmbdMultiMPN": MaskEmbdMultiMPN, "MPN_simplenet": MPN_simplenet}[args.model](
        nfeature_dim=4, efeature_dim=2, output_dim=4, hidden_dim=args.hidden_dim, n_gnn_layers=args.n_gnn_layers, K=args.K,
        dropout_rate=args.dropout_rate).to(device).eval()
    xy = None
    print(f"\n\nCase {args.case} is being evaluated...")
    if run_id is not None:
        model, _ = load_model(model, run_id, device)
        params = os.path.join(args.data_dir, "params", f"data_params_{run_id}.pt")
        if os.path.exists(params):
            p = torch.load(params, map_location="cpu")
            xy = tuple(p[k] for k in ("xymean", "xystd", "edgemean", "edgestd"))
    else:
        print("no --run-id: the model keeps its RANDOM initialisation; the rows that start from its prediction show a bad start")
    rows = evaluate(args.data_dir, args.case, model, samples, device, args.batch_size, xy, split, route)
    print(f"Number of samples: {rows['samples']}")
    if rows["route"] == "sparse":
        print("Solved on the sparse route")
    for line in report(rows):
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
