"""Per-line branch-flow and current error analysis: do the predicted bus voltages give the right line currents and line flows?  The
reference meant to report this -- its error_per_feature.py:186-223 builds an `i_error_table` of line-current errors in a Python
double loop over samples x lines and prints its mean and standard deviation, all commented out.  Here it is ONE `pfn_branch_flows`
call over the finished tables: the de-normalised predictions `bus_error_epoch` leaves on the device against the dataset's `y`,
`edge_index` and `edge_attr`.  Four quantities per (sample, stored line i -> j), in PowerImbalance.message's convention with no unit
conversion (`loss.BRANCH_QUANTITIES`): the current magnitude I, the P and Q message of the stored direction, and the series loss
r I^2.  No plots, no shunt, tap or charging terms (the dataset carries only r and x), no data-parallel sharding."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from ..loss import MOMENT_AT as _AT, branch_flows, branch_moments
from .error_analysis import abs_mean_std, bus_error_epoch
from .evaluation import GraphedEvalStep, _mean4, _std4

QUANTITIES = ("Line Current", "Active Flow", "Reactive Flow", "Active Loss")


@dataclass
class BranchErrors:
    """What `branch_error_epoch` returns.  `errors`: [S, e, 4] float32 on the device, prediction minus truth of (I, P, Q, loss);
    `flows_pred` / `flows_true`: the two tables themselves or None; `moments`: host float64 [e, 4, 6] (`loss.BUS_MOMENTS`);
    `flags`: bit 0 = a line named a bus outside the grid (its rows are NaN and left out of the moments); `lines0`: sample 0's line
    list [2, e] on the host."""
    errors: torch.Tensor
    flows_pred: Optional[torch.Tensor]
    flows_true: Optional[torch.Tensor]
    moments: torch.Tensor
    num_samples: int
    flags: int
    lines0: torch.Tensor


def _edge_stats(edgemean, edgestd):
    """(std + 1e-7 formed in fp32, mean) of the branch parameters as host floats: the dataset's inverse."""
    if edgestd is None:
        sd = None
    else:
        t = torch.as_tensor(edgestd, dtype=torch.float32).detach().cpu().reshape(-1, 2)[0]
        sd = [float(v) for v in (t + 1e-7).tolist()]
    mu = None if edgemean is None else [float(v) for v in torch.as_tensor(edgemean, dtype=torch.float32).detach().cpu().reshape(-1, 2)[0].tolist()]
    return sd, mu


def _split_tables(ds, device):
    """(y [S, n, 4], edge_index [2, e] or [S, 2, e], edge_attr [S, e, 2]) of the split on `device`: zero-copy views of the dense block
    of a device-resident single-case split, else the samples stacked once."""
    blocks = getattr(ds, "_blocks", None)
    if blocks is not None and getattr(ds, "_list", None) is None and len(blocks) == 1 and getattr(ds, "transform", None) is None:
        b = blocks[0]
        ei = b.edge_index[0] if b.static_topology else b.edge_index
        return b.y.to(device), ei.to(device), b.edge_attr.to(device)
    items = [ds[i] for i in range(len(ds))]
    e = int(items[0].edge_index.shape[1])
    if any(int(d.edge_index.shape[1]) != e for d in items):
        raise ValueError("branch_error_epoch: the samples of the split have different numbers of lines; the tables are [samples, lines, 4]")
    y = torch.stack([d.y for d in items]).to(device)
    ei = torch.stack([d.edge_index for d in items]).to(device)
    ea = torch.stack([d.edge_attr for d in items]).to(device)
    if bool((ei == ei[:1]).all()):
        ei = ei[0].contiguous()
    return y, ei, ea


@torch.no_grad()
def branch_error_epoch(model, loader, device, xymean=None, xystd=None, edgemean=None, edgestd=None,
                       graph: Optional[GraphedEvalStep] = None, keep_flows: bool = False) -> BranchErrors:
    """`bus_error_epoch(keep_errors=False, keep_predictions=True)` over `loader`, then ONE `branch_flows` call on the prediction table
    and the dataset's `y` / `edge_index` / `edge_attr`: no host loop, one more read-back (moments + flags).  `xymean` / `xystd` /
    `edgemean` / `edgestd`: the dataset's statistics (None: 0 / 1); their inverse is applied as `denormalize` does, with std + 1e-7.
    `graph`: as in `bus_error_epoch`.  `keep_flows`: also return the two flow tables.

    Row s of every table is sample s of the dataset.  The prediction table has that order where the step fills it by dataset index,
    or where the loader does not shuffle; anything else is a ValueError, as is a pass that did not see every sample once.  Mixed
    splits and per-sample masks raise in `bus_error_epoch`.  Where the topology differs between samples the per-sample line lists
    are used: "line k" is then position k of each sample's list, and `lines0` is sample 0's."""
    bus = bus_error_epoch(model, loader, device, xymean=xymean, xystd=xystd, graph=graph, keep_errors=False, keep_predictions=True)
    return branch_errors_of(bus, loader, xymean=xymean, xystd=xystd, edgemean=edgemean, edgestd=edgestd, keep_flows=keep_flows)


@torch.no_grad()
def branch_errors_of(bus, loader, xymean=None, xystd=None, edgemean=None, edgestd=None, keep_flows: bool = False) -> BranchErrors:
    """The second half of `branch_error_epoch` for a caller that has run `bus_error_epoch(keep_predictions=True)` over `loader`
    itself: the ONE `branch_flows` call on `bus.predictions` and the dataset's tables, with the same statistics."""
    if bus.predictions is None:
        raise ValueError("branch_errors_of: the bus pass kept no predictions (bus_error_epoch(keep_predictions=True))")
    ds = loader.dataset
    if not bus.rows_by_index and (getattr(loader, "shuffle", False) or getattr(loader, "shard", None) is not None):
        raise ValueError("branch_error_epoch: the prediction rows follow a shuffling or sharded loader's order, not the dataset's; "
                         "use shuffle=False or a device-resident dataset (whose rows are filled by sample index)")
    if bus.num_samples != len(ds):
        raise ValueError(f"branch_error_epoch: the pass saw {bus.num_samples} of the split's {len(ds)} samples; every sample is needed once")
    y, ei, ea = _split_tables(ds, bus.predictions.device)
    std4 = _std4(xystd)
    mean4 = _mean4(xymean)
    esd, emu = _edge_stats(edgemean, edgestd)
    e = int(ei.shape[-1])
    state = torch.empty(e * 24 + 1, dtype=torch.float64, device=bus.predictions.device)      # moments + the flags word: ONE read-back
    state[:-1].view(e, 4, 6).copy_(branch_moments(state.device, e))
    state[-1:].zero_()
    flows_pred, flows_true, errors, _ = branch_flows(bus.predictions, ei, ea, truth=y, truth_normalised=std4 is not None or mean4 is not None,
                                                     std=std4, mean=mean4, edge_std=esd, edge_mean=emu, flows_pred=keep_flows,
                                                     flows_true=keep_flows, errors=True, moments=state[:-1], flags=state[-1:].view(torch.int32))
    host = state.cpu()
    lines0 = (ei if ei.dim() == 2 else ei[0]).cpu()
    return BranchErrors(errors=errors, flows_pred=flows_pred, flows_true=flows_true, moments=host[:-1].view(e, 4, 6).clone(),
                        num_samples=bus.num_samples, flags=int(host[-1:].view(torch.int32)[0]), lines0=lines0)


def branch_report_lines(moments) -> dict:
    """From the moments [e, 4, 6]: `i_error_table mean` / `i_error_table std`, the mean and population standard deviation of
    |I error| over the whole table -- the two lines the reference's commented code prints (:220-221) --, then per quantity the
    `Absolute Average` / `Absolute Standard Deviation` of its |error|, and the line with the largest |error| and that error.
    One-pass variances in float64 (sum of squares minus squared mean)."""
    m = np.asarray(torch.as_tensor(moments).cpu().numpy() if torch.is_tensor(moments) else moments, dtype=np.float64)
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):                                 # (an empty table: the mean of nothing, NaN)
        def abs_figures(q):
            return abs_mean_std(m[:, q, _AT["count"]].sum(), m[:, q, _AT["sum_abs"]].sum(), m[:, q, _AT["sum_sq"]].sum())
        out["i_error_table mean"], out["i_error_table std"] = abs_figures(0)
        for q, name in enumerate(QUANTITIES):
            out[f"Absolute Average of {name}"], out[f"Absolute Standard Deviation of {name}"] = abs_figures(q)
        for q, name in enumerate(QUANTITIES):
            seen = m[:, q, _AT["count"]] > 0
            lo, hi = np.where(seen, m[:, q, _AT["min"]], 0.0), np.where(seen, m[:, q, _AT["max"]], 0.0)
            worst = np.where(np.abs(lo) > np.abs(hi), lo, hi) if m.shape[0] else np.zeros(0)
            k = int(np.argmax(np.abs(worst))) if worst.size else -1
            out[f"Largest error of {name}: line"] = k
            out[f"Largest error of {name}"] = float(worst[k]) if worst.size else float("nan")
    return out
