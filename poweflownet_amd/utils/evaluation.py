"""`evaluate_epoch` / `load_model` / `num_params` counterparts of the reference's utils/evaluation.py:20-104, plus what the
reference does not have: `GraphedEvalStep` (an evaluation epoch replayed from one hipGraph per batch size, its running sums kept
on the device) and `evaluate_report` (every line test.py prints from ONE pass over the split, `pfn_eval_metrics`)."""
import warnings
from typing import Callable, Optional

import torch
import torch.nn as nn

from .. import _lib as L
from .captured import BatchSource, capture_state, copy_batch, held_adjacencies, no_gc, topologies_gatherable, topology_owners, warm_up
from .custom_loss_functions import Masked_L2_loss, MaskedL1, MaskedL2V2, MixedMSEPoweImbalance, PowerImbalance


def load_model(model: nn.Module, run_id: str, device, models_dir: str = "models"):
    """utils/evaluation.py:20-36: load `model_state_dict` of the best-validation checkpoint of a run."""
    import os
    path = os.path.join(models_dir, f"model_{run_id}.pt")
    # a reference checkpoint stores `args` as an argparse.Namespace (reference train.py:160-165), which torch's default
    # weights_only unpickler rejects; these are the user's own local training artefacts, exactly what the reference loads
    saved = torch.load(path, map_location=device, weights_only=False)
    model.load_state_dict(saved["model_state_dict"])
    return model, saved


def num_params(model: nn.Module) -> int:
    return sum(p.numel() for p in model.parameters() if p.requires_grad)


def _identity(x):
    return x


def _epoch_loss(loss_fn, pre, out, data):
    """The per-batch loss dispatch of `evaluate_epoch` (utils/evaluation.py:60-104)."""
    if isinstance(loss_fn, Masked_L2_loss):
        return loss_fn(pre(out), pre(data.y), data.pred_mask)
    if isinstance(loss_fn, PowerImbalance):
        # (sic) the reference adds pred_mask * (1 - pred_mask), which is zero for 0/1 masks (:88-89); evaluate_epoch_v2 uses x
        masked_out = out * data.pred_mask + data.pred_mask * (1 - data.pred_mask)
        return loss_fn(pre(masked_out), data.edge_index, data.edge_attr)
    if isinstance(loss_fn, MixedMSEPoweImbalance):
        return loss_fn(pre(out), data.edge_index, data.edge_attr, data.y)
    return loss_fn(pre(out), pre(data.y))


def _epoch_terms(loss_fn, pre, out, data) -> dict:
    """The per-batch dispatch of `evaluate_epoch_v2` (utils/evaluation.py:106-165): a dict of loss terms."""
    if isinstance(loss_fn, Masked_L2_loss):
        return {"total": loss_fn(pre(out), pre(data.y), data.pred_mask)}
    if isinstance(loss_fn, (MaskedL2V2, MaskedL1)):
        return loss_fn(pre(out), pre(data.y), data.pred_mask)
    if isinstance(loss_fn, PowerImbalance):
        masked_out = pre(out * data.pred_mask + data.x * (1 - data.pred_mask))
        return {"total": loss_fn(masked_out, data.edge_index, data.edge_attr),
                "ref": loss_fn(data.y, data.edge_index, data.edge_attr)}
    if isinstance(loss_fn, MixedMSEPoweImbalance):
        return {"total": loss_fn(pre(out), data.edge_index, data.edge_attr, data.y)}
    return {"total": loss_fn(pre(out), pre(data.y))}


class _RunningSum:
    """sum_b double(value_b) * w_b of an evaluation loop (w = 1 on the first batch when `first_unweighted`: the quirk of
    evaluate_epoch_v2).  A float32 scalar on a HIP device is added ON the device (`pfn_eval_accumulate`: the same doubles in the
    same order as the host's `total += loss.item() * len(data)`, so the same bits) and the sum is read back once; anything else
    (a host tensor, another dtype) is added on the host as before."""

    def __init__(self, first_unweighted: bool = False):
        self.first_unweighted, self.acc, self.host, self.n = bool(first_unweighted), None, None, 0

    def add(self, value, weight) -> None:
        on_device = torch.is_tensor(value) and value.is_cuda and value.dtype == torch.float32 and value.numel() == 1
        if on_device and self.host is None:
            from ..loss import eval_accumulate, eval_accumulator
            if self.acc is None:
                self.acc = eval_accumulator(value.device).view(-1)
            eval_accumulate(value, self.acc, weight, self.first_unweighted)
        else:
            if self.host is None:                              # (a loop that changes its mind keeps the order of the sum)
                self.host = float(self.acc[0].item()) if self.acc is not None and self.n > 0 else 0.0
            w = 1.0 if (self.first_unweighted and self.n == 0) else weight
            self.host += value.item() * w
        self.n += 1

    def value(self) -> float:
        if self.host is not None:
            return self.host
        return float(self.acc[0].item()) if self.acc is not None else 0.0


# ---------------------------------------------------------------------------------------------- the report
_FAMILY_KEYS = ("total", "balanced total", "vm", "va", "p", "q")      # the dict order of MaskedL2V2 / MaskedL1
# (title test.py prints, first term of the family in L.EVAL_TERMS)
_REPORT_FAMILIES = (("MaskedL2", "l2_total"), ("MaskedL2(denorm)", "l2d_total"), ("MaskedL1(denorm)", "l1d_total"))


def report_keys(power_imbalance: bool = True):
    """The lines test.py prints, in its order (without the value)."""
    keys = [f"{title} {k}" for title, _ in _REPORT_FAMILIES for k in _FAMILY_KEYS]
    if power_imbalance:
        keys += ["PowerImbalance", "PowerImbalance(ref)"]
    return keys + ["Masked_L2_loss", "MSE"]


def report_from_accumulators(acc, num_samples, power_imbalance=None) -> dict:
    """The report of `evaluate_report` from an epoch's accumulators: `acc` = the `len(L.EVAL_TERMS)` running sums of
    `pfn_eval_metrics` (any sequence of floats, in `L.EVAL_TERMS` order: sum_b w_b * term_b), `num_samples` = sum_b len(batch_b)
    (the denominator of evaluate_epoch_v2, whatever weighting filled the sums), `power_imbalance` = (sum of the loss on the mixed
    rows, sum of the loss on the ground truth) or None.  Pure host arithmetic."""
    acc = [float(v) for v in acc]
    if len(acc) < len(L.EVAL_TERMS):
        raise ValueError(f"report_from_accumulators: expected {len(L.EVAL_TERMS)} sums, got {len(acc)}")
    at = {name: i for i, name in enumerate(L.EVAL_TERMS)}
    out = {}
    for title, first in _REPORT_FAMILIES:
        for j, k in enumerate(_FAMILY_KEYS):
            out[f"{title} {k}"] = acc[at[first] + j] / num_samples
    if power_imbalance is not None:
        out["PowerImbalance"] = float(power_imbalance[0]) / num_samples
        out["PowerImbalance(ref)"] = float(power_imbalance[1]) / num_samples
    out["Masked_L2_loss"] = acc[at["ml2_selected"]] / num_samples
    out["MSE"] = acc[at["mse"]] / num_samples
    return out


def _std4(xystd):
    """The four factors `denormalize` multiplies by -- std + 1e-7, formed in fp32 as it does -- as host floats."""
    if xystd is None:
        return None
    t = torch.as_tensor(xystd, dtype=torch.float32).detach().cpu().reshape(-1, 4)[0]
    return [float(v) for v in (t + 1e-7).tolist()]


def _mean4(xymean):
    """The four means `denormalize` adds, as host floats."""
    if xymean is None:
        return None
    return [float(v) for v in torch.as_tensor(xymean, dtype=torch.float32).detach().cpu().reshape(-1, 4)[0].tolist()]


# ------------------------------------------------------------------------------------------------ the step
class _Child:
    """One captured per-batch body: its input tensors, (indexed modes) their BatchSource, the graph and the adjacencies it reads."""
    __slots__ = ("static", "source", "topo_graph", "dynamic", "graph", "held", "n_keys", "pos")

    def __init__(self, static, source=None, dynamic=False):
        self.static, self.source, self.dynamic = static, source, bool(dynamic)
        self.topo_graph = None if source is None else source.topo_graph     # (the adjacency a `topo` source builds into)
        self.graph, self.held, self.n_keys = None, [], len(static)
        self.pos = None                # errors, copied batches: the table rows of the batch (device int64, filled per batch)


def _num_graphs(data) -> int:
    ptr = getattr(data, "ptr", None)
    return 1 if ptr is None else int(ptr.numel()) - 1


def _same_device(a, b) -> bool:
    a, b = torch.device(a), torch.device(b)
    if a.type != b.type:
        return False
    if a.type != "cuda":
        return True
    cur = torch.cuda.current_device()
    return (cur if a.index is None else a.index) == (cur if b.index is None else b.index)


class GraphedEvalStep:
    """The per-batch body of an evaluation epoch (forward -> loss dispatch -> running sum) captured into a hipGraph and replayed:
    the evaluation counterpart of `GraphedTrainStep`.  `model.eval()`, `no_grad`, warm-up on a side stream, one captured child per
    batch size (the short last batch of a split gets its own).  Kept by the caller across epochs and handed to `evaluate_epoch`,
    `evaluate_epoch_v2` or `evaluate_report` as `graph=`; it serves ONE of them with ONE loss at a time (another loss, another
    `pre_loss_fn` or another kind of epoch drops the captured graphs and captures again).

    How a batch gets into the captured inputs (the capture rules are those of utils/captured.py):
      * a `can_gather()` dataset on the model's device is pulled INSIDE the graph (`BatchSource.indexed`, as
        `GraphedTrainStep.step_indexed`), a `can_gather_topologies()` one (one line set per sample) with its adjacency
        (`BatchSource.topo`).  The checks of such a build stay on the device: a bad batch gives a NaN loss instead of an exception;
      * any other loader whose batch has the captured shapes is copied into the captured inputs -- with the captured `edge_index`
        tensor itself the adjacency is the cached one; a loader that hands out a NEW `edge_index` per batch (a list-backed one)
        switches to the dynamic form, where the list is copied too and the adjacency is rebuilt inside the graph (again: a bad
        batch gives a NaN loss instead of an exception);
      * everything else runs the eager body on the same device accumulators: ragged batches (a mixed split), a dataset with a
        per-sample transform, more shapes than `max_children`, a failed capture (with a warning).

    The step leaves the model as it found it (mode, dropout RNG state, gradients, `dynamic_topology`, `segment_build`, an attached
    loss) and captures again when a parameter's storage moved (`FlatAdamW` re-flattens them) -- not when values changed in place.
    `captures` counts the captures."""

    max_children = 8

    def __init__(self, model, loss_fn=None, pre_loss_fn: Optional[Callable] = None):
        self.model, self.loss_fn, self.pre_loss_fn = model, loss_fn, pre_loss_fn
        self.kind = "epoch"            # epoch | v2 | report | errors
        self._extras = None            # report: (std4, PowerImbalance or None); errors: utils/error_analysis.py bus_error_epoch
        self.captures = 0
        self.eager_batches = 0         # batches of the last epoch that ran the eager body
        self.disabled = False
        self.side = None
        self._children = {}            # (mode, shape signature) -> _Child
        self._copy_dynamic = False     # the loader hands out a new edge_index per batch
        self._param_key = None
        self._acc = None               # [32, 2] float64: row i = {sum, batch counter} of term i (epoch: row 0)
        self._racc = None              # report: the accumulator of pfn_eval_metrics
        self._keys = None              # v2: the term names, in the loss's dict order
        self._metrics_ws = None
        # errors (utils/error_analysis.py): the tables the captured launches write, the moments + flags word, the running position
        self._etab = self._ptab = self._mom = None
        self._pos, self._eager_idx, self.rows_by_index = 0, None, False

    # ------------------------------------------------------------------------------------------ plumbing
    def _owners(self):
        """captured.topology_owners of the model, the loss and (report) the PowerImbalance behind `_extras`."""
        return topology_owners(self.model, self.loss_fn, *(self._extras[1:2] if self._extras else ()))

    def _drop_all(self):
        self._children = {}

    def _bind(self, kind, loss_fn, pre_loss_fn, extras=None):
        same = (kind == self.kind and loss_fn is self.loss_fn and pre_loss_fn is self.pre_loss_fn and extras == self._extras)
        if not same:
            self._drop_all()
            self.kind, self.loss_fn, self.pre_loss_fn, self._extras, self._keys = kind, loss_fn, pre_loss_fn, extras, None

    def _check_params(self):
        key = tuple(p.data_ptr() for p in self.model.parameters())
        if key != self._param_key:
            if self._param_key is not None:
                self._drop_all()                      # the captured launches hold the old addresses
            self._param_key = key

    def _buffers(self, device):
        from ..loss import _Workspace, eval_accumulator
        if self._acc is None or self._acc.device != device:
            self._acc = eval_accumulator(device, rows=32)
            self._racc = eval_accumulator(device, rows=1, width=L.EVAL_ACC_DOUBLES).view(-1)
            self._metrics_ws = _Workspace(L.EVAL_WS_FLOATS)
            self._drop_all()
        self._acc.zero_()                             # between epochs, OUTSIDE the graph (no memset nodes in a capture)
        self._racc.zero_()
        if self.kind == "errors":
            self._error_buffers(device)

    def _error_buffers(self, device):
        """The tables ([rows, n_bus, 4], NaN where no sample was written) and the moments of an `errors` epoch, owned by the step
        because the captured launches hold their addresses; the flags word is the int32 behind the moments (one read-back)."""
        from ..loss import reset_bus_error_moments
        _, _, keep_e, keep_p, rows, n_bus = self._extras
        shape = (rows, n_bus, 4)
        if self._mom is None or self._mom.device != device or self._mom.numel() != n_bus * 48 + 1:
            self._mom = torch.empty(n_bus * 48 + 1, dtype=torch.float64, device=device)
            self._etab = self._ptab = None
            self._drop_all()
        for name, keep in (("_etab", keep_e), ("_ptab", keep_p)):
            tab = getattr(self, name)
            if (tab is not None) != keep or (keep and (tuple(tab.shape) != shape or tab.device != device)):
                setattr(self, name, torch.empty(shape, dtype=torch.float32, device=device) if keep else None)
                self._drop_all()
            if keep:
                getattr(self, name).fill_(float("nan"))
        reset_bus_error_moments(self._mom[:-1].view(n_bus, 4, 2, 6))
        self._mom[-1:].zero_()
        self._pos, self._eager_idx = 0, None

    def _error_batch(self, data) -> int:
        """The number of graphs of an `errors` batch; ValueError unless it is a uniform batch of the epoch's case."""
        n_bus = self._extras[5]
        sizes, B = getattr(data, "_graph_sizes", None), _num_graphs(data)
        if (sizes is not None and any(int(v) != n_bus for v in sizes)) or int(data.x.shape[0]) != B * n_bus:
            raise ValueError(f"bus_error_epoch: a batch of {B} graphs with {int(data.x.shape[0])} rows is not a uniform batch of "
                             f"{n_bus}-bus grids (mixed splits are not covered: the tables are [samples, buses, 4])")
        return B

    # -------------------------------------------------------------------------------------- the body
    def _body(self, ch, data):
        """One batch: (indexed modes) pull it, forward, losses, running sums.  Runs under no_grad with the model in eval mode;
        captured as it stands."""
        from ..loss import eval_accumulate, eval_metrics
        if ch is not None and ch.source is not None:
            ch.source.pull(data, self.model)
        out = self.model(data)
        w = float(len(data))
        pre = self.pre_loss_fn or _identity
        if self.kind == "epoch":
            eval_accumulate(_epoch_loss(self.loss_fn, pre, out, data), self._acc[0], w)
        elif self.kind == "v2":
            terms = _epoch_terms(self.loss_fn, pre, out, data)
            keys = tuple(terms)
            if self._keys is None:
                if len(keys) > self._acc.shape[0]:
                    raise RuntimeError(f"GraphedEvalStep: {len(keys)} loss terms, room for {self._acc.shape[0]}")
                self._keys = keys
            elif keys != self._keys:
                raise RuntimeError(f"GraphedEvalStep: the loss returned the terms {keys}, earlier batches {self._keys}")
            for i, k in enumerate(keys):
                eval_accumulate(terms[k], self._acc[i], w, first_unweighted=True)
        elif self.kind == "errors":
            from ..loss import bus_errors_accumulate
            std4, mean4, _, _, table_rows, n_bus = self._extras
            rows = self._eager_idx if ch is None else (ch.source.buffer if ch.source is not None else ch.pos)
            bus_errors_accumulate(out, data.y, data.pred_mask, n_bus, rows, self._mom[:-1], self._mom[-1:].view(torch.int32),
                                  std=std4, mean=mean4, err_table=self._etab, pred_table=self._ptab, table_rows=table_rows)
        else:
            std4, pi = self._extras
            mixed = torch.empty_like(out) if pi is not None else None
            eval_metrics(out, data.y, data.pred_mask, x=data.x if pi is not None else None, std=std4, weight=w,
                         first_unweighted=True, acc=self._racc, mixed_out=mixed, workspace=self._metrics_ws)
            if pi is not None:
                eval_accumulate(pi(mixed, data.edge_index, data.edge_attr), self._acc[0], w, first_unweighted=True)
                eval_accumulate(pi(data.y, data.edge_index, data.edge_attr), self._acc[1], w, first_unweighted=True)

    def _eager(self, data):
        self.eager_batches += 1
        if self.kind == "errors":
            B = self._error_batch(data)
            if self._eager_idx is None:                            # the running position: one index copy per batch
                self._eager_idx = torch.arange(self._pos, self._pos + B).to(data.x.device)
            self._body(None, data)
            self._pos, self._eager_idx = self._pos + B, None
            return len(data)
        self._body(None, data)
        return len(data)

    # ------------------------------------------------------------------------------------ capture
    def _capture(self, ch):
        if self.side is None:
            self.side = torch.cuda.Stream()
        owners = self._owners()
        snap = (self._acc.clone(), self._racc.clone())            # the warm-up passes leave no trace in the running sums
        if self.kind == "errors":
            snap += (self._mom.clone(),)
        with capture_state(owners, self.model, ch.dynamic, ch.topo_graph is not None):
            warm_up(self.side, lambda: self._body(ch, ch.static))
            self._acc.copy_(snap[0])
            self._racc.copy_(snap[1])
            if len(snap) > 2:
                self._mom.copy_(snap[2])
            g = torch.cuda.CUDAGraph()
            with no_gc(), torch.cuda.graph(g):
                self._body(ch, ch.static)
        ch.graph = g
        ch.held = held_adjacencies(owners, ch.topo_graph)
        self.captures += 1

    def _ready(self, key, make):
        """The captured child of `key` (made by `make()` and captured on first use), or None: this batch runs the eager body."""
        ch = self._children.get(key)
        if ch is not None:
            return ch
        if self.disabled or len(self._children) >= self.max_children:
            return None
        ch = make()
        try:
            self._capture(ch)
        except Exception as exc:                                   # noqa: BLE001  (the eager body is always available)
            warnings.warn(f"GraphedEvalStep: hipGraph capture failed ({exc}); running eager launches from here on")
            torch.cuda.synchronize()
            self.disabled = True
            self._drop_all()
            self._acc.zero_()
            self._racc.zero_()
            if self.kind == "errors":
                self._error_buffers(self._mom.device)
            raise _CaptureFailed() from exc
        self._children[key] = ch
        return ch

    # ------------------------------------------------------------------------------------- batches
    def _step_indexed(self, ds, idx, topo: bool):
        B = int(idx.numel())

        def make():
            static = ds.collate_indices(idx.tolist())
            source = BatchSource.topo(ds, idx, static.x.device) if topo else BatchSource.indexed(ds, idx)
            return _Child(static, source, dynamic=topo)
        ch = self._ready(("topo" if topo else "indexed", id(ds), B), make)
        if ch is None:
            self._eager_idx = idx if self.kind == "errors" else None
            return self._eager(ds.collate_indices(idx.tolist()))
        ch.source.buffer.copy_(idx)
        ch.graph.replay()
        self._pos += B
        return ch.n_keys

    def _step_data(self, data):
        sizes = getattr(data, "_graph_sizes", None)
        if not data.x.is_cuda or (sizes is not None and len(sizes) > 1 and min(sizes) != max(sizes)):
            return self._eager(data)
        errors = self.kind == "errors"
        B = self._error_batch(data) if errors else 0
        ptr = getattr(data, "ptr", None)
        sig = (tuple(data.x.shape), tuple(data.edge_index.shape), tuple(data.edge_attr.shape), data.pred_mask.dtype,
               None if ptr is None else tuple(ptr.shape), len(data), str(data.x.device))
        ch = self._children.get(("copy", sig))
        if ch is not None and not ch.dynamic and data.edge_index is not ch.static.edge_index:
            if not hasattr(self.model, "dynamic_topology"):
                return self._eager(data)
            # same shapes, another edge_index tensor: this loader re-collates the topology per batch.  Capture once more with the
            # adjacency build inside the graph; from here on every batch of a captured shape replays
            self._copy_dynamic = True
            del self._children[("copy", sig)]

        def make():
            static = data.clone()
            if not self._copy_dynamic:
                static.edge_index = data.edge_index                # identity matters: the adjacency caches key on it
            ch = _Child(static, dynamic=self._copy_dynamic)
            if errors:
                ch.pos = torch.arange(self._pos, self._pos + B).to(data.x.device)
            return ch
        ch = self._ready(("copy", sig), make)
        if ch is None:
            return self._eager(data)
        if errors:                                                 # the running position: one index copy per batch
            ch.pos.copy_(torch.arange(self._pos, self._pos + B))
            self._pos += B
        copy_batch(ch.static, data, ch.dynamic)
        ch.graph.replay()
        return ch.n_keys

    def _index_mode(self, loader, ds, device):
        """"indexed" / "topo": the batches are gathered inside the graph from the loader's device index batches; None: collated."""
        indexed = hasattr(loader, "index_batches") and ds is not None and getattr(ds, "transform", None) is None
        on_dev = indexed and hasattr(ds, "device") and _same_device(ds.device, device)
        if on_dev and hasattr(ds, "can_gather") and ds.can_gather():
            return "indexed"
        if on_dev and topologies_gatherable(self.model, self._owners(), ds):
            return "topo"
        return None

    def _loop(self, loader, device):
        ds = getattr(loader, "dataset", None)
        if self.disabled:                                          # the plain loop: collate, forward, losses, device sums
            if self.kind == "errors" and self._index_mode(loader, ds, device) is not None:
                # the table row is the SAMPLE index wherever the graphed pass would hold it on the device: the eager pass
                # fills the same rows (one index copy per batch, no read-back)
                self.rows_by_index, n = True, 0
                for rows in loader._index_lists():
                    self._eager_idx = torch.tensor(rows, dtype=torch.long).to(device)
                    n += self._eager(ds.collate_indices(rows))
                return n
            return sum(self._eager(data.to(device)) for data in loader)
        mode = self._index_mode(loader, ds, device)
        if mode is not None:
            self.rows_by_index = True
            return sum(self._step_indexed(ds, idx, mode == "topo") for idx in loader.index_batches(device))
        n = 0
        transform = getattr(ds, "transform", None) is not None
        for data in loader:
            data = data.to(device)
            n += self._eager(data) if transform else self._step_data(data)
        return n

    def run_epoch(self, loader, device):
        """One pass over `loader`: (the step's accumulators as host tensors -- ONE read-back --, sum of len(batch))."""
        model = self.model
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("GraphedEvalStep needs a HIP device (poweflownet_amd has no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        was_training = model.training
        attach = model.__dict__.get("_mse_attach")
        model.eval()
        self.eager_batches, self.rows_by_index = 0, False
        try:
            with torch.no_grad(), torch.cuda.device(device):
                self._check_params()
                self._buffers(device)
                try:
                    n = self._loop(loader, device)
                except _CaptureFailed:
                    n = self._loop(loader, device)                 # (disabled now: every batch runs the eager body)
                if self.kind == "errors":                          # moments + flags word: ONE read-back
                    return self._mom.cpu(), None, n
                return self._acc.cpu(), self._racc.cpu(), n
        finally:
            model.train(was_training)
            if attach is not None:
                model._mse_attach = attach


class _CaptureFailed(Exception):
    pass


# ---------------------------------------------------------------------------------------------- the loops
def _step_for(graph, model):
    if graph.model is not model:
        raise RuntimeError("evaluate: the GraphedEvalStep was built for another model")
    return graph


@torch.no_grad()
def evaluate_epoch(model: nn.Module, loader, loss_fn: Callable, device="cpu", pre_loss_fn: Optional[Callable] = None,
                   graph: Optional[GraphedEvalStep] = None) -> float:
    """`graph`: a `GraphedEvalStep(model)` kept by the caller across epochs -> the per-batch body is replayed from one hipGraph per
    batch size where that is safe (and the model comes back in the mode it was found in).  Either way the running loss is
    accumulated on the device (`pfn_eval_accumulate`) and read back ONCE per epoch: the reference's per-batch `loss.item()` is a
    host sync per batch; the returned value is the same sum of the same doubles in the same order."""
    if graph is not None:
        step = _step_for(graph, model)
        step._bind("epoch", loss_fn, pre_loss_fn)
        acc, _, n = step.run_epoch(loader, device)
        return float(acc[0, 0]) / max(n, 1)
    pre = pre_loss_fn or _identity
    model.eval()
    total, num_samples = _RunningSum(), 0
    for data in loader:
        data = data.to(device)
        loss = _epoch_loss(loss_fn, pre, model(data), data)
        num_samples += len(data)
        total.add(loss, len(data))
    return total.value() / max(num_samples, 1)


@torch.no_grad()
def evaluate_epoch_v2(model: nn.Module, loader, loss_fn: Callable, device="cpu", pre_loss_fn: Optional[Callable] = None,
                      graph: Optional[GraphedEvalStep] = None) -> dict:
    """utils/evaluation.py:106-165: like `evaluate_epoch` but returns a dict of loss terms (`MaskedL2V2` / `MaskedL1` produce
    several; every other loss one, under 'total'; `PowerImbalance` adds 'ref' = the loss of the ground truth).

    Kept quirk (:158-163): the FIRST batch enters the running sums unweighted, later batches weighted by len(data); the sums
    are divided by the total of len(data).  The sums live on the device, one accumulator per term (the quirk is decided there,
    from the accumulator's batch counter), and are read back once.  `graph`: as in `evaluate_epoch`."""
    if graph is not None:
        step = _step_for(graph, model)
        step._bind("v2", loss_fn, pre_loss_fn)
        acc, _, n = step.run_epoch(loader, device)
        return {k: float(acc[i, 0]) / n for i, k in enumerate(step._keys or ())}
    pre = pre_loss_fn or _identity
    model.eval()
    totals, num_samples = None, 0
    for data in loader:
        data = data.to(device)
        terms = _epoch_terms(loss_fn, pre, model(data), data)
        num_samples += len(data)
        if totals is None:
            totals = {k: _RunningSum(first_unweighted=True) for k in terms}
        for k, s in totals.items():
            s.add(terms[k], len(data))
    return {k: s.value() / num_samples for k, s in (totals or {}).items()}


@torch.no_grad()
def evaluate_report(model: nn.Module, loader, device, xystd=None, power_imbalance: Optional[PowerImbalance] = None,
                    graph: Optional[GraphedEvalStep] = None) -> dict:
    """Every line test.py prints (`report_keys`), from ONE pass over `loader`: per batch one forward, one `pfn_eval_metrics`
    launch and -- when a `PowerImbalance` is given -- its two launches (on out * mask + x * (1 - mask) and on y), the sums kept on
    the device with the weighting of `evaluate_epoch_v2` and read back once.  `xystd`: the dataset's node standard deviations for
    the de-normalised lines (None: they equal the normalised ones).  Against six `evaluate_epoch_v2` passes the normalised lines
    differ by the rounding of another summation order; the de-normalised ones are formed from (out - y) * std instead of
    subtracting two de-normalised values, which is closer to the exact value (include/pfn_hip.h)."""
    std4 = _std4(xystd)
    extras = (None if std4 is None else tuple(std4), power_imbalance)
    step = _step_for(graph, model) if graph is not None else GraphedEvalStep(model)
    step._bind("report", None, None, extras)
    if graph is None:
        step.disabled = True                                       # the eager body, on the step's device accumulators
    acc, racc, n = step.run_epoch(loader, device)
    pi = (float(acc[0, 0]), float(acc[1, 0])) if power_imbalance is not None else None
    return report_from_accumulators(racc[:len(L.EVAL_TERMS)].tolist(), n, pi)
