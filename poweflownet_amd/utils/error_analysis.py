"""Per-bus error analysis: the counterpart of the reference's error_per_feature.py (:120-172 the de-normalised error of every bus of
every test sample, :247-324 its mean / standard-deviation report, :362-405 the 300-bin histogram per (bus, feature)) from ONE device
pass over the split.  The reference runs one forward and one `.cpu()` per sample and n x 4 `np.histogram` calls on the host; here a
batch is one forward plus one `pfn_bus_errors_accumulate` launch -- replayed from a hipGraph through `GraphedEvalStep`'s `errors`
kind -- and the histograms are one `pfn_bus_errors_histogram` launch.  No plots: the arrays are what the reference's plotting half
reads."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from ..loss import MOMENT_AT as _AT, bus_errors_histogram
from .evaluation import GraphedEvalStep, _mean4, _std4, _step_for

FEATURES = ("Voltage Magnitude", "Voltage Angle", "Active Power", "Reactive Power")
GIVEN_FACTOR = np.float32(0.00001)     # the reference's `masks[masks == 0] = 0.00001` (:258): given entries are scaled, not dropped


@dataclass
class BusErrors:
    """What `bus_error_epoch` returns.  `errors` / `predictions`: [S, n, 4] float32 on the device or None; a row no batch wrote holds
    NaN.  `moments`: host float64 [n, 4, 2, 6] (group 0: predicted entries, group 1: given; `loss.BUS_MOMENTS`).  `flags`: bit 0 =
    a batch named a row outside the table.  `mask0` / `types0`: sample 0's `pred_mask` [n, 4] and `bus_type` [n] on the host.
    `rows_by_index`: a table row is the sample's index in the dataset (else: its position in the loader's order)."""
    errors: Optional[torch.Tensor]
    predictions: Optional[torch.Tensor]
    moments: torch.Tensor
    num_samples: int
    flags: int
    mask0: torch.Tensor
    types0: torch.Tensor
    rows_by_index: bool = False


def _uniform_split(ds):
    """(sample 0's mask, sample 0's bus types, buses, samples) of a split the tables can hold: ONE case, ONE mask for every sample
    (the reference's `np.stack` fails on anything else too, and its report reads sample 0's mask)."""
    if ds is None or not hasattr(ds, "__len__") or len(ds) == 0:
        raise ValueError("bus_error_epoch: the loader needs a non-empty `dataset`")
    blocks = getattr(ds, "_blocks", None)
    if blocks is not None and getattr(ds, "_list", None) is None:
        if len(blocks) != 1:
            raise ValueError(f"bus_error_epoch: a mixed split ({len(blocks)} grid cases) is not covered: the tables are [samples, buses, 4]")
        b = blocks[0]
        if not bool((b.pred_mask == b.pred_mask[:1]).all()):
            raise ValueError("bus_error_epoch: pred_mask differs between the samples of the split; the per-bus tables and the "
                             "report need ONE mask (the report reads sample 0's)")
        return b.pred_mask[0].cpu(), b.bus_type[0].cpu(), int(b.x.shape[1]), len(ds)
    first = ds[0]
    n = int(first.x.shape[0])
    if any(int(ds[i].x.shape[0]) != n for i in range(len(ds))):
        raise ValueError("bus_error_epoch: a mixed split (samples of different sizes) is not covered: the tables are [samples, buses, 4]")
    mask0 = first.pred_mask
    if any(not torch.equal(ds[i].pred_mask, mask0) for i in range(len(ds))):
        raise ValueError("bus_error_epoch: pred_mask differs between the samples of the split; the per-bus tables and the report "
                         "need ONE mask (the report reads sample 0's)")
    return mask0.cpu(), first.bus_type.cpu(), n, len(ds)


@torch.no_grad()
def bus_error_epoch(model, loader, device, xymean=None, xystd=None, graph: Optional[GraphedEvalStep] = None, keep_errors: bool = True,
                    keep_predictions: bool = False) -> BusErrors:
    """One pass over `loader`: per batch one forward and one `pfn_bus_errors_accumulate` launch; ONE read-back (moments + flags).
    `xymean` / `xystd`: the dataset's node statistics (None: 0 / 1): errors are (out - y) * (std + 1e-7), predictions
    `datasets.denormalize(out)` bit for bit.  `graph`: a `GraphedEvalStep(model)` kept by the caller -> the per-batch body is
    replayed from one hipGraph per batch size (kind `errors`; the step's other kinds capture again when their turn comes); None: the
    eager body on the same device buffers.

    Which table row a sample gets: its index in the dataset where the step gathers batches from a device-resident dataset (so a
    shuffling loader fills the same rows), else its position in the loader's order.  Only ONE case with ONE mask for every sample
    (ValueError otherwise)."""
    mask0, types0, n_bus, rows = _uniform_split(getattr(loader, "dataset", None))
    std4 = _std4(xystd)
    mean4 = _mean4(xymean)
    extras = (None if std4 is None else tuple(std4), None if mean4 is None else tuple(mean4), bool(keep_errors),
              bool(keep_predictions), rows, n_bus)
    step = _step_for(graph, model) if graph is not None else GraphedEvalStep(model)
    step._bind("errors", None, None, extras)
    if graph is None:
        step.disabled = True                                       # the eager body, on the step's device buffers
    host, _, _ = step.run_epoch(loader, device)
    num = int(step._pos)
    take = (lambda t: None if t is None else t.clone()) if step.rows_by_index else (lambda t: None if t is None else t[:num].clone())
    return BusErrors(errors=take(step._etab), predictions=take(step._ptab), moments=host[:-1].view(n_bus, 4, 2, 6).clone(),
                     num_samples=num, flags=int(host[-1:].view(torch.int32)[0]), mask0=mask0, types0=types0,
                     rows_by_index=bool(step.rows_by_index))


def mask_scale(mask0) -> torch.Tensor:
    """The reference's scale table (:256-259): sample 0's mask as float32 with every 0 replaced by 1e-5.  [n, 4] float32."""
    m = torch.as_tensor(mask0).to(torch.float32)
    return torch.where(m == 0, torch.tensor(float(GIVEN_FACTOR), dtype=torch.float32, device=m.device), m)


def histogram_edges(moments, scale=None, nbins: int = 300, multiplier=(0.8, 0.8, 0.4, 0.4)) -> np.ndarray:
    """The reference's bin range (:388-398) from the moments: per feature the min and max of the SCALED errors (error * scale[bus,
    feature] in float32; scale >= 0), each times the feature's multiplier (in float64), made symmetric about 0 on the larger
    magnitude; `np.linspace(lo, hi, nbins + 1)`.  Returns float64 [4, nbins + 1].  Moments of ONE group, [rows, 4, 6] (the branch
    table's, utils/branch_analysis.py), are taken as they stand."""
    m = np.asarray(torch.as_tensor(moments).cpu().numpy() if torch.is_tensor(moments) else moments, dtype=np.float64)
    if m.ndim == 3:
        m = m[:, :, None, :]
    n = m.shape[0]
    sc = np.ones((n, 4), dtype=np.float32) if scale is None else np.asarray(torch.as_tensor(scale).cpu().numpy(), dtype=np.float32)
    seen = m[..., _AT["count"]] > 0                                                      # [n, 4, 2]
    # (the moments' min / max are float32 values widened; a float32 product is monotone, so the extreme of the products is the
    # product of the extreme)
    lo_all = np.where(seen, (m[..., _AT["min"]].astype(np.float32) * sc[:, :, None]).astype(np.float64), np.inf)
    hi_all = np.where(seen, (m[..., _AT["max"]].astype(np.float32) * sc[:, :, None]).astype(np.float64), -np.inf)
    edges = np.empty((4, nbins + 1), dtype=np.float64)
    for f in range(4):
        lo, hi = float(lo_all[:, f].min()) * float(multiplier[f]), float(hi_all[:, f].max()) * float(multiplier[f])
        if abs(lo) >= hi:
            hi = abs(lo)
        else:
            lo = -hi
        edges[f] = np.linspace(lo, hi, nbins + 1)
    return edges


def bus_error_histograms(errors: torch.Tensor, edges, scale=None):
    """The reference's n x 4 `np.histogram(errors[:, bus, feature] * scale, bins=edges[feature])` calls (:401-404) in one launch:
    (hist [n, 4, nbins], outside [n, 4, 3] = below the first edge / above the last / NaN), int32 on the device."""
    if scale is not None:
        scale = torch.as_tensor(scale, dtype=torch.float32).to(errors.device)
    return bus_errors_histogram(errors, edges, scale)


def _figures(m, factor, pred_rows, rows) -> dict:
    """Per feature the mean and population standard deviation of |scaled error| over `pred_rows[f]` (the buses sample 0 predicts),
    then mean and standard deviation of ALL scaled errors of `rows`.  scaled error = error * factor[bus, feature]."""
    tot = m.sum(axis=2)                                                                  # both mask groups: [n, 4, 6]
    with np.errstate(invalid="ignore", divide="ignore"):                                 # (nothing selected: the mean of nothing, NaN)
        return _figures_of(tot, factor, pred_rows, rows)


def abs_mean_std(count, sum_abs, sum_sq):
    """Mean and population standard deviation of |e| from the summed moments (count, sum |e|, sum e^2) -- of e itself when given its
    plain sum.  One-pass variance in float64: mean of squares minus squared mean, clamped at 0."""
    mean = sum_abs / count
    msq = sum_sq / count
    return float(mean), float(np.sqrt(max(msq - mean * mean, 0.0)))


def _figures_of(tot, factor, pred_rows, rows) -> dict:
    out = {}
    for f, name in enumerate(FEATURES):
        r = pred_rows[f]
        out[f"Absolute Average of {name}"], out[f"Absolute Standard Deviation of {name}"] = abs_mean_std(
            tot[r, f, _AT["count"]].sum(), (tot[r, f, _AT["sum_abs"]] * factor[r, f]).sum(), (tot[r, f, _AT["sum_sq"]] * factor[r, f] ** 2).sum())
    out["Average of all errors"], out["Standard Deviation of all errors"] = abs_mean_std(
        tot[rows, :, _AT["count"]].sum(), (tot[rows, :, _AT["sum"]] * factor[rows]).sum(), (tot[rows, :, _AT["sum_sq"]] * factor[rows] ** 2).sum())
    return out


def report_lines(moments, mask0, types0) -> dict:
    """The lines the reference prints at :247-310, in its order, from the moments: the four counts of predicted entries and the
    numbers of loads and generators (sample 0), per feature the mean and population standard deviation of |error * mask| over the
    buses sample 0 predicts, the mean and standard deviation of all scaled errors -- given entries count with the factor 1e-5, as in
    the reference -- and then the same figures for the load buses (type 2) and the generator buses (type 1) on their own
    (:313-324), keys prefixed "Loads: " / "Generators: ".  One-pass variances in float64 (sum of squares minus squared mean)."""
    m = np.asarray(torch.as_tensor(moments).cpu().numpy() if torch.is_tensor(moments) else moments, dtype=np.float64)
    mask = np.asarray(torch.as_tensor(mask0).cpu().numpy())
    types = np.asarray(torch.as_tensor(types0).cpu().numpy())
    factor = mask_scale(torch.as_tensor(mask)).numpy().astype(np.float64)               # float32 values, widened
    out = {f"Number of {name}": int((mask[:, f] == 1).sum()) for f, name in enumerate(FEATURES)}
    out["Number of Loads"] = int((types == 2).sum())
    out["Number of Generators"] = int((types == 1).sum())
    everything = np.arange(m.shape[0])
    out.update(_figures(m, factor, [np.where(mask[:, f] == 1)[0] for f in range(4)], everything))
    for title, code in (("Loads", 2), ("Generators", 1)):
        rows = np.where(types == code)[0]
        sub = _figures(m, factor, [rows[mask[rows, f] == 1] for f in range(4)], rows)
        out.update({f"{title}: {k}": v for k, v in sub.items()})
    return out
