#!/usr/bin/env python3
"""Counterpart of the reference's perfomance_evaluator.py (its spelling): per grid case the loss and the per-sample latency of the
MPN, the MLP and GCN baselines and the Tikhonov regulariser, on the first `--samples` samples of the test split.

    python perfomance_evaluator.py --cases 14 118 [6470rte] [--data-dir data] [--models-dir models/testing] [--samples 10]
                                   [--synthetic-samples 32]

Per case it prints the reference's lines -- `Loss of MPN model`, `Execution time of MPN model`, the same pair for MLP and GCN -- and
the Tikhonov pair, which the reference left behind a `continue` (:135); it is cheap here.  Checkpoints
`<models-dir>/{mpn,mlp,gcn}_<case>.pt` (what train.py / train_baselines.py save under `model_state_dict`) are loaded where they
exist; a model without one keeps its random initialisation and the script says so.  A baseline checkpoint trained `--with-mask` is
recognised by its input width.  Data: the test split of `<data-dir>/raw/case<case>_*.npy` when present, else the last 30 % of
`--synthetic-samples` synthetic grids of the case.

The loss is `Masked_L2_loss(regularize=False)` per single-sample batch, averaged.  The latency is the wall time of `model(sample)`
between two device synchronisations, after one warm-up call per model.  The reference reads `time.time()` around an unsynchronised
call (:65-67): that is the time to LAUNCH the forward, not to run it."""
import argparse
import os
import sys
import time

import torch

from poweflownet_amd.data import Batch
from poweflownet_amd.datasets import PowerFlowData
from poweflownet_amd.networks.GCN import GCN
from poweflownet_amd.networks.MLP import MLP
from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
from poweflownet_amd.synth import make_dataset
from poweflownet_amd.utils.baselines import graph_laplacian, tikhonov_operator, tikhonov_regularizer
from poweflownet_amd.utils.custom_loss_functions import Masked_L2_loss

ALPHA = 1.25                                                       # perfomance_evaluator.py:162


def _load(model, path, name):
    if os.path.exists(path):
        model.load_state_dict(torch.load(path, map_location="cpu")["model_state_dict"])
        print(f"{name}: loaded {path}")
    else:
        print(f"{name}: no checkpoint {path}: the model keeps its random initialisation")
    return model


def _saved_width(path, key, default):
    """Input width of a saved baseline (its first weight's columns), `default` without a checkpoint."""
    if not os.path.exists(path):
        return default
    return int(torch.load(path, map_location="cpu")["model_state_dict"][key].shape[1])


@torch.no_grad()
def _measure(fn, samples, loss_fn):
    """(mean loss, mean seconds per sample) of `fn(sample)` over `samples`: one warm-up call, then every call timed between two
    device synchronisations."""
    fn(samples[0])
    torch.cuda.synchronize()
    loss, seconds = 0.0, 0.0
    for sample in samples:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = fn(sample)
        torch.cuda.synchronize()
        seconds += time.perf_counter() - t0
        loss += float(loss_fn(result, sample.y, sample.pred_mask))
    return loss / len(samples), seconds / len(samples)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cases", nargs="+", default=["14", "118"])
    ap.add_argument("--data-dir", default="data")
    ap.add_argument("--models-dir", default=os.path.join("models", "testing"))
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--synthetic-samples", type=int, default=32)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("perfomance_evaluator.py needs a HIP device: poweflownet_amd has no CPU fallback")
    device = torch.device("cuda")
    eval_loss_fn = Masked_L2_loss(regularize=False)
    for case in args.cases:
        print(f"\n\nCase {case} is being evaluated...")
        raw = os.path.join(args.data_dir, "raw", f"case{case}_node_features.npy")
        if os.path.exists(raw):
            testset = PowerFlowData(root=args.data_dir, case=case, split=[.5, .2, .3], task="test", device=device)
        else:
            n = args.synthetic_samples
            testset = make_dataset(case, n, seed=0)[int(0.5 * n) + int(0.2 * n):]     # split [.5, .2, .3], as train.py
        number = min(args.samples, len(testset))
        print(f"Number of samples: {number}")
        samples = [Batch.from_data_list([testset[i]]).to(device) for i in range(number)]      # single-sample batches
        n_bus, path = int(samples[0].x.shape[0]), lambda name: os.path.join(args.models_dir, f"{name}_{case}.pt")  # noqa: E731

        mpn = MaskEmbdMultiMPN(nfeature_dim=4, efeature_dim=2, output_dim=4, hidden_dim=129, n_gnn_layers=4, K=3, dropout_rate=0.2)
        mpn = _load(mpn, path("mpn"), "MPN").to(device).eval()
        loss, seconds = _measure(mpn, samples, eval_loss_fn)
        print(f"Loss of MPN model: {loss}")
        print(f"Execution time of MPN model: {seconds}")

        width = _saved_width(path("mlp"), "layers.0.weight", n_bus * 4)
        mlp = MLP(width, n_bus * 4, 128, 3, 0.2, with_mask=width == n_bus * 8)
        mlp = _load(mlp, path("mlp"), "MLP").to(device).eval()
        loss, seconds = _measure(mlp, samples, eval_loss_fn)
        print(f"Loss of MLP model: {loss}")
        print(f"Execution time of MLP model: {seconds}")

        width = _saved_width(path("gcn"), "conv1.lin.weight", 4)
        gcn = GCN(nfeature_dim=width, output_dim=4, hidden_dim=129, with_mask=width == 8)
        gcn = _load(gcn, path("gcn"), "GCN").to(device).eval()
        loss, seconds = _measure(gcn, samples, eval_loss_fn)
        print(f"Loss of GCN model: {loss}")
        print(f"Execution time of GCN model: {seconds}")

        # the reference builds the Laplacian from the case's adjacency file; here from the sample's own line list (one solve per
        # topology, kept while the next sample has the same list)
        kept = {}

        def tikhonov(sample):
            ei = sample.edge_index
            if kept.get("ei") is None or kept["ei"].shape != ei.shape or not torch.equal(kept["ei"], ei):
                kept["ei"], kept["lap"] = ei, graph_laplacian(ei, n_bus)
                kept["op"] = tikhonov_operator(ALPHA, kept["lap"])
            return tikhonov_regularizer(ALPHA, kept["lap"], sample.x, operator=kept["op"]).float()

        loss, seconds = _measure(tikhonov, samples, eval_loss_fn)
        print(f"Loss of Tikhonov Regularizer: {loss}")
        print(f"Execution time of Tikhonov Regularizer: {seconds}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
