#!/usr/bin/env python3
"""Per-bus error analysis entry, the counterpart of the reference's error_per_feature.py: the de-normalised error of every bus of
every test sample, its per-feature report (overall, load buses, generator buses) and a 300-bin error histogram per (bus, feature),
from ONE device pass over the test split (poweflownet_amd/utils/error_analysis.py).

    python error_per_feature.py --cfg_json configs/standard.json --case 118v2 --data-dir DATA --run-id <id> [--save-predictions]

`--run-id`, `--case`, `--data-dir` and `--cfg_json` replace what the reference hard-codes (error_per_feature.py:38-53, :80).  The
checkpoint is models/model_<run-id>.pt; without one the model keeps its random initialisation.  Data: the test split of
`<data-dir>/raw/case<case>_*.npy` when present (normalised with the run's saved parameters if
`<data-dir>/params/data_params_<run-id>.pt` exists), else `--synthetic-samples` synthetic grids of the case, of which the last 30 %
are the test split (their values are already normalised: errors are then in normalised units).  Writes
results/<case>_{errors,masks,types}.npy -- the three files the reference writes, [S, n, 4] / [S, n, 4] / [S, n] -- and
results/<case>_error_hist.npy [n, 4, nbins] with results/<case>_error_hist_edges.npy [4, nbins + 1]; `--save-predictions` adds
results/<case>_predictions.npy.  `--graphed-eval` replays the per-batch body from a hipGraph.  No plots: the .npy files are what
the reference's plotting half reads.

`--model GCN` / `--model MLP` (with `--with-mask` for a baseline trained so) runs the same analysis on a baseline, as the reference's
script does on its GCN (:109-131): the checkpoint is models/testing/{gcn,mlp}_<case>.pt (train_baselines.py), the pass is the eager one.

`--branch-errors` adds the per-line analysis the reference left commented out (:186-223; utils/branch_analysis.py): the errors of the
line currents, flows and losses the predicted voltages imply, from one more device pass over the finished tables.  It prints their
report after the lines above and writes results/<case>_i_error_table.npy [S, e] (the reference's file name), _branch_errors.npy
[S, e, 4] (I, P, Q, loss), _lines.npy [2, e], _branch_error_hist.npy and _branch_error_hist_edges.npy; `--save-flows` adds
_branch_flows_pred.npy and _branch_flows_true.npy."""
import os
import sys

import numpy as np
import torch

from poweflownet_amd.data import DataLoader
from poweflownet_amd.datasets import PowerFlowData
from poweflownet_amd.networks.GCN import GCN
from poweflownet_amd.networks.MLP import MLP
from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN, MPN_simplenet
from poweflownet_amd.synth import make_dataset
from poweflownet_amd.utils.argument_parser import argument_parser
from poweflownet_amd.utils.error_analysis import bus_error_epoch, bus_error_histograms, histogram_edges, mask_scale, report_lines
from poweflownet_amd.utils.evaluation import GraphedEvalStep, load_model


def _take(argv, flag, has_value=True, default=None):
    if flag not in argv:
        return default
    i = argv.index(flag)
    value = argv[i + 1] if has_value else True
    del argv[i:i + (2 if has_value else 1)]
    return value


@torch.no_grad()
def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    run_id = _take(argv, "--run-id", default="synthetic")
    save_predictions = _take(argv, "--save-predictions", has_value=False, default=False)
    branch_errors = _take(argv, "--branch-errors", has_value=False, default=False)
    save_flows = _take(argv, "--save-flows", has_value=False, default=False)
    nbins = int(_take(argv, "--nbins", default=300))
    out_dir = _take(argv, "--results-dir", default="results")
    with_mask = bool(_take(argv, "--with-mask", has_value=False, default=False))
    args = argument_parser(argv)
    if not torch.cuda.is_available():
        raise SystemExit("error_per_feature.py needs a HIP device: poweflownet_amd has no CPU fallback")
    device = torch.device("cuda")
    xymean = xystd = edgemean = edgestd = None
    raw = os.path.join(args.data_dir, "raw", f"case{args.case}_node_features.npy")
    if os.path.exists(raw):
        params, kw = os.path.join(args.data_dir, "params", f"data_params_{run_id}.pt"), {}
        if os.path.exists(params):
            p = torch.load(params, map_location="cpu")
            kw = {k: p[k] for k in ("xymean", "xystd", "edgemean", "edgestd")}
        testset = PowerFlowData(root=args.data_dir, case=args.case, split=[.5, .2, .3], task="test", device=device, **kw)
        xymean, xystd, edgemean, edgestd = testset.xymean, testset.xystd, testset.edgemean, testset.edgestd
        nin, nout, ne = testset.get_data_dimensions()
    else:
        n = args.synthetic_samples
        testset = make_dataset(args.case, n, seed=0)[int(0.5 * n) + int(0.2 * n):]      # split [.5, .2, .3], as train.py
        nin, nout, ne = 4, 4, 2
    loader = DataLoader(testset, batch_size=args.batch_size, shuffle=False)
    models = {"MaskEmbdMultiMPN": MaskEmbdMultiMPN, "MPN_simplenet": MPN_simplenet}
    baseline = args.model in ("GCN", "MLP")
    if baseline:
        # the reference runs this analysis on its GCN baseline (error_per_feature.py:109-131); checkpoints are what
        # train_baselines.py saves, models/testing/{gcn,mlp}_<case>.pt
        n_bus, f_in = int(testset[0].x.shape[0]), 8 if with_mask else 4
        model = (GCN(nfeature_dim=f_in, output_dim=nout, hidden_dim=129, with_mask=with_mask) if args.model == "GCN"
                 else MLP(n_bus * f_in, n_bus * nout, 128, 3, 0.2, with_mask=with_mask)).to(device)
    else:
        model = models[args.model](nfeature_dim=nin, efeature_dim=ne, output_dim=nout, hidden_dim=args.hidden_dim,
                                   n_gnn_layers=args.n_gnn_layers, K=args.K, dropout_rate=args.dropout_rate).to(device)
    model.eval()
    saved = os.path.join("models", "testing", f"{args.model.lower()}_{args.case}.pt")
    if baseline and os.path.exists(saved):
        model.load_state_dict(torch.load(saved, map_location=device)["model_state_dict"])
    elif baseline:
        print(f"no checkpoint {saved}: the model keeps its random initialisation")
    elif os.path.exists(os.path.join("models", f"model_{run_id}.pt")):
        model, _ = load_model(model, run_id, device)
    else:
        print(f"no checkpoint models/model_{run_id}.pt: the model keeps its random initialisation")
    print(f"Model: {args.model}\nCase: {args.case}\nNumber of samples: {len(testset)}")
    graphed = getattr(args, "graphed_eval", None) is True           # (off unless asked for: one pass cannot repay the captures)
    if baseline and graphed:
        raise SystemExit("--graphed-eval: the baselines run the eager pass only")
    res = bus_error_epoch(model, loader, device, xymean=xymean, xystd=xystd, graph=GraphedEvalStep(model) if graphed else None,
                          keep_errors=True, keep_predictions=bool(save_predictions or branch_errors))
    if res.flags & 1:
        raise SystemExit("error_per_feature.py: a batch named a sample outside the table")
    for key, value in report_lines(res.moments, res.mask0, res.types0).items():
        print(f"{key}: {value}")
    scale = mask_scale(res.mask0)
    edges = histogram_edges(res.moments, scale, nbins=nbins)
    hist, outside = bus_error_histograms(res.errors, edges, scale)
    S = res.num_samples
    os.makedirs(out_dir, exist_ok=True)
    path = lambda name: os.path.join(out_dir, f"{args.case}_{name}.npy")      # noqa: E731
    np.save(path("errors"), res.errors.cpu().numpy())
    np.save(path("masks"), np.broadcast_to(res.mask0.to(torch.float32).numpy(), (S,) + tuple(res.mask0.shape)).copy())
    np.save(path("types"), np.broadcast_to(res.types0.numpy(), (S,) + tuple(res.types0.shape)).copy())
    np.save(path("error_hist"), hist.cpu().numpy())
    np.save(path("error_hist_edges"), edges)
    if save_predictions:
        np.save(path("predictions"), res.predictions.cpu().numpy())
    inside = int(hist.sum())
    print(f"histograms: {nbins} bins per (bus, feature); {inside} of {S * hist.shape[0] * 4} scaled errors inside the range, "
          f"{int(outside[..., 0].sum())} below, {int(outside[..., 1].sum())} above, {int(outside[..., 2].sum())} NaN")
    print(f"wrote {out_dir}/{args.case}_{{errors,masks,types,error_hist,error_hist_edges{',predictions' if save_predictions else ''}}}.npy")
    if branch_errors:
        _branch_part(res, loader, xymean, xystd, edgemean, edgestd, bool(save_flows), nbins, path, out_dir, args.case)
    return 0


def _branch_part(res, loader, xymean, xystd, edgemean, edgestd, save_flows, nbins, path, out_dir, case):
    from poweflownet_amd.utils.branch_analysis import branch_errors_of, branch_report_lines
    br = branch_errors_of(res, loader, xymean=xymean, xystd=xystd, edgemean=edgemean, edgestd=edgestd, keep_flows=save_flows)
    if br.flags & 1:
        print("branch errors: a line names a bus outside the grid; its rows are NaN and left out of the figures")
    for key, value in branch_report_lines(br.moments).items():
        print(f"{key}: {value}")
    edges = histogram_edges(br.moments, nbins=nbins)
    hist, outside = bus_error_histograms(br.errors, edges)
    errors = br.errors.cpu().numpy()
    np.save(path("i_error_table"), np.ascontiguousarray(errors[:, :, 0]))
    np.save(path("branch_errors"), errors)
    np.save(path("lines"), br.lines0.numpy())
    np.save(path("branch_error_hist"), hist.cpu().numpy())
    np.save(path("branch_error_hist_edges"), edges)
    names = "i_error_table,branch_errors,lines,branch_error_hist,branch_error_hist_edges"
    if save_flows:
        np.save(path("branch_flows_pred"), br.flows_pred.cpu().numpy())
        np.save(path("branch_flows_true"), br.flows_true.cpu().numpy())
        names += ",branch_flows_pred,branch_flows_true"
    print(f"branch histograms: {nbins} bins per (line, quantity); {int(hist.sum())} of {errors.size} errors inside the range, "
          f"{int(outside[..., 0].sum())} below, {int(outside[..., 1].sum())} above, {int(outside[..., 2].sum())} NaN")
    print(f"wrote {out_dir}/{case}_{{{names}}}.npy")


if __name__ == "__main__":
    raise SystemExit(main())
