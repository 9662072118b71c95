#!/usr/bin/env python3
"""k-hop locality analysis entry, the counterpart of the reference's explain.py: for every center bus and every hop radius, the
loss at the center when the model sees only the ball of that radius around it (poweflownet_amd/utils/explanation.py).

    python explain.py --cfg_json configs/standard.json --case 118v2 --data-dir DATA --run-id <id> [--num_batches 10] [-bs 128]
    python explain.py --load --case 118v2 --run-id <id>          # reload saved tables

`--run-id`, `--data-dir`, `--case` and `--cfg_json` replace the values the reference hard-codes (explain.py:24-27).  The
checkpoint is models/model_<run-id>.pt; without one (or with `--run-id` omitted) the model keeps its random initialisation.
Data: the test split of `<data-dir>/raw/case<case>_*.npy` when present (normalised with the run's saved parameters if
`<data-dir>/params/data_params_<run-id>.pt` exists), synthetic grids of the case otherwise.  Writes
results/explain/<run-id>/{loss_subgraph,num_nodes_subgraph}_case_<case>.pt.  Plotting is not reproduced."""
import argparse
import os

import numpy as np
import torch

from poweflownet_amd.data import DataLoader
from poweflownet_amd.datasets import PowerFlowData
from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
from poweflownet_amd.synth import make_dataset
from poweflownet_amd.utils.custom_loss_functions import Masked_L2_loss
from poweflownet_amd.utils.evaluation import load_model
from poweflownet_amd.utils.explanation import explain_epoch


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--load", default=False, action=argparse.BooleanOptionalAction, help="load saved tables")
    p.add_argument("--num_batches", default=10, type=int, help="number of batches to evaluate")
    p.add_argument("--batch_size", "-bs", default=128, type=int, help="batch size")
    p.add_argument("--run-id", default="synthetic", type=str)
    p.add_argument("--data-dir", default="data", type=str)
    p.add_argument("--case", default="118v2", type=str)
    p.add_argument("--cfg_json", default="configs/standard.json", type=str)
    p.add_argument("--synthetic-samples", default=None, type=int,
                   help="synthetic test samples when no raw files exist (default: enough for the batches evaluated)")
    p.add_argument("--seed", default=1234, type=int)
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    result_dir = os.path.join("results", "explain", args.run_id)
    loss_path = os.path.join(result_dir, f"loss_subgraph_case_{args.case}.pt")
    nodes_path = os.path.join(result_dir, f"num_nodes_subgraph_case_{args.case}.pt")
    if args.load:
        try:
            loss_subgraph, num_nodes_subgraph = torch.load(loss_path), torch.load(nodes_path)
        except FileNotFoundError:
            print("File not found. Please run without --load first.")
            return 1
    else:
        if not torch.cuda.is_available():
            raise SystemExit("explain.py needs a HIP device: poweflownet_amd has no CPU fallback")
        device = torch.device("cuda")
        torch.manual_seed(args.seed)
        np.random.seed(args.seed)
        cfg = {}
        if os.path.exists(args.cfg_json):
            import json
            with open(args.cfg_json) as f:
                cfg = json.load(f)
        model = MaskEmbdMultiMPN(nfeature_dim=4, efeature_dim=2, output_dim=4, hidden_dim=cfg.get("hidden_dim", 129),
                                 n_gnn_layers=cfg.get("n_gnn_layers", 4), K=cfg.get("K", 3),
                                 dropout_rate=cfg.get("dropout_rate", 0.2)).to(device)
        model.eval()
        if os.path.exists(os.path.join("models", f"model_{args.run_id}.pt")):
            model, _ = load_model(model, args.run_id, device)
        else:
            print(f"no checkpoint models/model_{args.run_id}.pt: the model keeps its random initialisation")
        eval_loss_fn = Masked_L2_loss(regularize=False)
        raw = os.path.join(args.data_dir, "raw", f"case{args.case}_node_features.npy")
        if os.path.exists(raw):
            params = os.path.join(args.data_dir, "params", f"data_params_{args.run_id}.pt")
            kw = {}
            if os.path.exists(params):
                p = torch.load(params, map_location="cpu")
                kw = {k: p[k] for k in ("xymean", "xystd", "edgemean", "edgestd")}
            testset = PowerFlowData(root=args.data_dir, case=args.case, split=[.5, .2, .3], task="test", device=device, **kw)
        else:
            n = args.synthetic_samples or args.batch_size * (args.num_batches + 1)
            testset = make_dataset(args.case, n, seed=2)
        test_loader = DataLoader(testset, batch_size=args.batch_size, shuffle=False)
        loss_subgraph, num_nodes_subgraph, _ = explain_epoch(model, test_loader, eval_loss_fn, device=device,
                                                             num_batches=args.num_batches)
        os.makedirs(result_dir, exist_ok=True)
        torch.save(loss_subgraph, loss_path)
        torch.save(num_nodes_subgraph, nodes_path)
    finite = torch.isfinite(loss_subgraph).all(dim=1)
    mean = loss_subgraph[finite].log().mean(dim=0).exp()                # across nodes, as plot_loss_subgraph
    print(f"case {args.case}: {int(finite.sum())} centers, radii 0..{loss_subgraph.shape[1] - 1}")
    print("geometric-mean loss per radius:", " ".join(f"{v:.4g}" for v in mean.tolist()))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
