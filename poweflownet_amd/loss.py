"""`MSELoss` and `Masked_L2_loss` with forward and backward fused into one pass over (out, y) (`pfn_mse_loss`,
`pfn_masked_l2_loss`).

Counterpart of `torch.nn.MSELoss()` at train.py:103 as used by the else-branch of train_epoch
(utils/training.py:72): loss = mean((out - y)^2); the gradient 2 (out - y) / numel is produced by the same
kernel that accumulates the loss, so `loss.backward()` costs one scale instead of torch's four small kernels."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib as L


MASKED_L2_WS_FLOATS = 1032     # struct MaskedL2Ws (csrc/reduce.hpp): 4128 bytes

_ONE = {}     # per device: the constant 1 used as the unit loss gradient (immutable after creation)


def _one(device):
    key = (device.type, device.index)
    if key not in _ONE:
        _ONE[key] = torch.ones((), dtype=torch.float32, device=device)
    return _ONE[key]


class _Workspace:
    """Reduction scratch of ONE loss object (partials + an arrival counter that is zero between calls), per device.  Owned
    by the loss module that uses it -- two models / host threads / streams bring two loss objects and share nothing; one
    object serves one call at a time (the rule of pfn_context, include/pfn_hip.h).  Allocated on the first call, i.e. in
    the warm-up steps that precede a hipGraph capture, never inside one."""

    def __init__(self, floats: int):
        self.floats, self._buf = floats, {}

    def on(self, device) -> torch.Tensor:
        key = (device.type, device.index)
        if key not in self._buf:
            self._buf[key] = torch.zeros(self.floats, dtype=torch.float32, device=device)
        return self._buf[key]

    def __reduce__(self):
        return (_Workspace, (self.floats,))


class _MseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, y, wsp):
        L.require_device(out, y, what="MSELoss input")
        out, y = L.f32c(out, "out"), L.f32c(y, "y")
        if out.shape != y.shape:
            raise RuntimeError(f"MSELoss: shape mismatch {tuple(out.shape)} vs {tuple(y.shape)}")
        loss = torch.empty((), dtype=torch.float32, device=out.device)
        grad = torch.empty_like(out) if ctx.needs_input_grad[0] else None
        ws = wsp.on(out.device)
        with torch.cuda.device(out.device):
            L.check(L.load().pfn_mse_loss(out.data_ptr(), y.data_ptr(), out.numel(), loss.data_ptr(), L.ptr(grad),
                                          ws.data_ptr(), ws.numel() * 4, L.stream_ptr()), "pfn_mse_loss")
        ctx.grad = grad
        return loss

    @staticmethod
    def backward(ctx, gloss):
        if ctx.grad is None:
            return None, None, None
        if gloss.data_ptr() == _one(ctx.grad.device).data_ptr():   # MSELoss.unit_grad(): the constant 1, never written
            return ctx.grad, None, None
        return ctx.grad * gloss, None, None


def slot_validity(data):
    """The per-row validity tensor (int32, 1 = the row counts) a slot batch carries (PowerFlowData.slot_template), or None."""
    v = data.__dict__.get("_slot_valid") if hasattr(data, "__dict__") else None
    return v if torch.is_tensor(v) else None


class _RowsLossFn(torch.autograd.Function):
    """MSELoss (mask None) or Masked_L2_loss over the rows with valid != 0 (pfn_mse_loss_rows / pfn_masked_l2_loss_rows): the
    mean's denominators are counted on the device, an invalid row's gradient is exactly 0."""

    @staticmethod
    def forward(ctx, out, y, mask, valid, regularize, regcoeff, wsp):
        L.require_device(out, y, mask, valid, what="slot-batch loss input")
        out, y = L.f32c(out, "out"), L.f32c(y, "y")
        n = out.shape[0]
        if out.dim() != 2 or out.shape[1] != 4 or out.shape != y.shape or (mask is not None and mask.shape != out.shape):
            raise RuntimeError(f"slot-batch loss: out, y (and mask) must be (N, 4); got {tuple(out.shape)} / {tuple(y.shape)}")
        if valid.dtype != torch.int32 or valid.shape != (n,) or not valid.is_contiguous():
            raise RuntimeError(f"slot-batch loss: the validity tensor must be contiguous int32 of shape ({n},)")
        loss = torch.empty((), dtype=torch.float32, device=out.device)
        grad = torch.empty_like(out) if ctx.needs_input_grad[0] else None
        ws = wsp.on(out.device)
        with torch.cuda.device(out.device):
            if mask is None:
                L.check(L.load().pfn_mse_loss_rows(out.data_ptr(), y.data_ptr(), valid.data_ptr(), n, loss.data_ptr(), L.ptr(grad),
                                                   ws.data_ptr(), ws.numel() * 4, L.stream_ptr()), "pfn_mse_loss_rows")
            else:
                if mask.dtype == torch.int64:
                    code = 0
                else:
                    mask, code = mask.to(torch.float32), 1
                mask = mask.contiguous()
                L.check(L.load().pfn_masked_l2_loss_rows(out.data_ptr(), y.data_ptr(), mask.data_ptr(), code, valid.data_ptr(), n,
                                                         int(bool(regularize)), float(regcoeff), loss.data_ptr(), L.ptr(grad),
                                                         ws.data_ptr(), ws.numel() * 4, L.stream_ptr()), "pfn_masked_l2_loss_rows")
        ctx.grad = grad
        return loss

    @staticmethod
    def backward(ctx, gloss):
        if ctx.grad is None:
            return (None,) * 7
        if gloss.data_ptr() == _one(ctx.grad.device).data_ptr():
            return (ctx.grad,) + (None,) * 6
        return (ctx.grad * gloss,) + (None,) * 6


def _check_no_tail(input):
    if getattr(input, "_pfn_mse_tail", None) is not None:
        raise RuntimeError("a slot batch (valid=...) cannot use an attached loss tail: do not call attach() for it")


class MseTail:
    """What `MSELoss.attach` arranged for ONE forward/backward pair of a model (pfn_mpn_backward_mse): the model left its output
    rows unwritten; its backward pass writes `out`, `loss` and `grad_out` in its first launch."""
    __slots__ = ("target", "target_version", "loss", "grad_out", "ws", "masked", "mask")

    def __init__(self, target, loss, grad_out, ws, masked=None, mask=None):
        self.target, self.target_version, self.loss, self.grad_out, self.ws = target, target._version, loss, grad_out, ws
        self.masked, self.mask = masked, mask      # Masked_L2_loss: (regularize, regcoeff) and the mask tensor the model was given


class _MseTailFn(torch.autograd.Function):
    """The loss node of an attached pair: nothing is launched here.  forward hands out the tensor the model's backward pass will
    write the loss into; backward hands the model the (still unwritten) grad_out buffer as the token that says "form it yourself"."""

    @staticmethod
    def forward(ctx, out, tail):
        ctx.tail = tail
        return tail.loss.detach()      # (an alias: returning tail.loss itself would tie loss -> grad_fn -> tail -> loss into a cycle)

    @staticmethod
    def backward(ctx, gloss):
        tail = ctx.tail
        if gloss.data_ptr() != _one(tail.grad_out.device).data_ptr():
            raise RuntimeError("MSELoss.attach(): the attached loss must be differentiated with loss.backward(MSELoss.unit_grad(loss)) "
                               "(a scaled loss needs the plain path: do not call attach)")
        return tail.grad_out, None


class MSELoss(nn.Module):
    """Drop-in for `torch.nn.MSELoss()` (reduction='mean') on HIP tensors."""

    def __init__(self):
        super().__init__()
        self._ws = _Workspace(264)
        self._tail_ws = _Workspace(1028)     # pfn_mpn_backward_mse: 1024 partials + the arrival counter
        self._rows_ws = _Workspace(MASKED_L2_WS_FLOATS)    # pfn_mse_loss_rows (slot batches)

    def attach(self, model, target):
        """Promise of the training loop, made right before `out = model(data)`: the next three statements are
        `loss = self(out, target)`, `loss.backward(self.unit_grad(loss))`, and nobody reads `out` or `loss` before that backward
        has run.  A model that can (`MaskEmbdMultiMPN` on a batch of small graphs, output_dim 4: pfn_mpn_mse_tail_ok) then leaves
        its output Linear to its backward pass, whose first launch forms `out`, the loss and its gradient -- two launches fewer
        per step (train_epoch's per-batch body, utils/training.py:55-77, is exactly this sequence).  One-shot: consumed by the
        next forward whether it could use it or not; where it could not, nothing changes.  Results: `out` and every gradient bit
        for bit those of the plain path, the loss to the rounding of another summation order."""
        if hasattr(model, "_mse_attach"):
            model._mse_attach = (target, self._tail_ws, None, None)

    def forward(self, input, target, valid=None):
        """`valid` (int32 per row, a slot batch's `_slot_valid`): the mean runs over the rows with valid != 0 only."""
        if valid is not None:
            _check_no_tail(input)
            if "_rows_ws" not in self.__dict__:              # (an object unpickled from before slot batches existed)
                self._rows_ws = _Workspace(MASKED_L2_WS_FLOATS)
            return _RowsLossFn.apply(input, target, None, valid, False, 0.0, self._rows_ws)
        tail = getattr(input, "_pfn_mse_tail", None)
        if tail is not None:
            if not (torch.is_tensor(target) and tail.target is target and tail.target_version == target._version
                    and input.shape == target.shape and tail.masked is None):
                raise RuntimeError("MSELoss.attach(): the loss was called with another target (or a modified one) than the one "
                                   "attached -- the model's output rows are not written on this path")
            return _MseTailFn.apply(input, tail)
        return _MseFn.apply(input, target, self._ws)

    @staticmethod
    def unit_grad(loss):
        """The constant 1 on `loss`'s device.  `loss.backward(MSELoss.unit_grad(loss))` is `loss.backward()` without the
        two tiny kernels autograd spends on creating that 1 and multiplying the gradient by it."""
        return _one(loss.device)


class _MaskedL2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, y, mask, regularize, regcoeff, wsp):
        L.require_device(out, y, mask, what="Masked_L2_loss input")
        out, y = L.f32c(out, "output"), L.f32c(y, "target")
        if out.shape != y.shape or mask.shape != out.shape:
            raise RuntimeError(f"Masked_L2_loss: shape mismatch {tuple(out.shape)} / {tuple(y.shape)} / {tuple(mask.shape)}")
        if mask.dtype == torch.int64:
            code = 0
        else:
            mask, code = mask.to(torch.float32), 1
        mask = mask.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=out.device)
        grad = torch.empty_like(out) if ctx.needs_input_grad[0] else None
        ws = wsp.on(out.device)
        with torch.cuda.device(out.device):
            L.check(L.load().pfn_masked_l2_loss(out.data_ptr(), y.data_ptr(), mask.data_ptr(), code, out.numel(), int(bool(regularize)),
                                                float(regcoeff), loss.data_ptr(), L.ptr(grad), ws.data_ptr(), ws.numel() * 4,
                                                L.stream_ptr()), "pfn_masked_l2_loss")
        ctx.grad = grad
        return loss

    @staticmethod
    def backward(ctx, gloss):
        if ctx.grad is None:
            return None, None, None, None, None, None
        if gloss.data_ptr() == _one(ctx.grad.device).data_ptr():
            return ctx.grad, None, None, None, None, None
        return ctx.grad * gloss, None, None, None, None, None


POWER_IMBALANCE_WS_FLOATS = 320


def masked_l2_attach(model, target, mask, regularize, regcoeff, tail_ws):
    """`Masked_L2_loss.attach`: the promise of `MSELoss.attach` for the reference's default training loss
    (utils/custom_loss_functions.py:10-46; dispatch utils/training.py:61-62).  `mask` must be the very tensor the model is about to
    read as `data.pred_mask` (its first launch counts the two index sets of the loss while it converts the mask)."""
    if hasattr(model, "_mse_attach"):
        model._mse_attach = (target, tail_ws, (bool(regularize), float(regcoeff)), mask)


def masked_l2_loss(output, target, mask, regularize=True, regcoeff=1, workspace=None, valid=None):
    """Masked_L2_loss.forward (utils/custom_loss_functions.py:30-46) on HIP tensors: loss and its gradient in two launches
    instead of four `masked_select` compactions, two means and their autograd graph.  `workspace`: the calling loss
    object's `_Workspace(MASKED_L2_WS_FLOATS)` (a throw-away one is made when omitted).  `valid`: as in MSELoss.forward."""
    if valid is not None:
        _check_no_tail(output)
        return _RowsLossFn.apply(output, target, mask, valid, regularize, regcoeff, workspace or _Workspace(MASKED_L2_WS_FLOATS))
    tail = getattr(output, "_pfn_mse_tail", None)
    if tail is not None:
        if not (tail.masked == (bool(regularize), float(regcoeff)) and tail.target is target and tail.target_version == target._version
                and tail.mask is mask and output.shape == target.shape):
            raise RuntimeError("Masked_L2_loss.attach(): the loss was called with another target / mask / setting than the one "
                               "attached -- the model's output rows are not written on this path")
        return _MseTailFn.apply(output, tail)
    return _MaskedL2Fn.apply(output, target, mask, regularize, regcoeff, workspace or _Workspace(MASKED_L2_WS_FLOATS))


def unit_grad(loss):
    """The constant 1 on `loss`'s device: `loss.backward(unit_grad(loss))` == `loss.backward()` minus two tiny kernels."""
    return _one(loss.device)


class _PowerImbalanceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, graph, edge_attr, stats, wsp):
        L.require_device(x, edge_attr, what="PowerImbalance input")
        x, edge_attr = L.f32c(x, "x"), L.f32c(edge_attr, "edge_attr")
        n = x.shape[0]
        if x.dim() != 2 or x.shape[1] != 4 or edge_attr.shape != (graph.e_stored, 2) or graph.num_nodes != n:
            raise RuntimeError(f"PowerImbalance: x must be (N, 4) and edge_attr (E, 2); got {tuple(x.shape)}, {tuple(edge_attr.shape)}")
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        grad = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dpq = torch.empty(max(n, 1), 2, dtype=torch.float32, device=x.device)
        ws = wsp.on(x.device)
        import ctypes as C
        st = (C.c_float * 12)(*stats)
        with torch.cuda.device(x.device):
            L.check(L.load().pfn_power_imbalance(graph.ws.data_ptr(), n, graph.e_stored, x.data_ptr(), edge_attr.data_ptr(), st,
                                                 loss.data_ptr(), L.ptr(grad), dpq.data_ptr(), ws.data_ptr(), ws.numel() * 4,
                                                 L.stream_ptr()), "pfn_power_imbalance")
        ctx.grad = grad
        return loss

    @staticmethod
    def backward(ctx, gloss):
        if ctx.grad is None:
            return None, None, None, None, None
        if gloss.data_ptr() == _one(ctx.grad.device).data_ptr():
            return ctx.grad, None, None, None, None
        return ctx.grad * gloss, None, None, None, None


def power_imbalance(x, graph, edge_attr, stats, workspace=None):
    """PowerImbalance.forward on HIP tensors; `graph` = the GraphCSR of the stored-once edge_index (mode -1), `stats` = 12
    floats {xymean[4], xystd[4], edgemean[2], edgestd[2]}; `workspace` as in masked_l2_loss."""
    return _PowerImbalanceFn.apply(x, graph, edge_attr, stats, workspace or _Workspace(POWER_IMBALANCE_WS_FLOATS))


# ------------------------------------------------------------------------------------------ evaluation metrics
def eval_accumulator(device, rows: int = 1, width: int = 2) -> torch.Tensor:
    """`rows` epoch accumulators of `width` 8-byte slots, zeroed: doubles followed by ONE int64 batch counter (its bits).
    width 2 = what `eval_accumulate` updates ({sum, batches}); `L.EVAL_ACC_DOUBLES` = what `eval_metrics` updates.  Clear it
    between epochs with `zero_()` -- outside a captured graph."""
    return torch.zeros(rows, width, dtype=torch.float64, device=device)


def eval_metrics(out, y, mask, x=None, std=None, weight=1.0, first_unweighted=False, acc=None, mixed_out=None, terms=None,
                 workspace=None):
    """Every evaluation term of one batch in ONE launch (`pfn_eval_metrics`): returns the fp32 tensor of `L.EVAL_TERMS`.
    `std`: four host floats (the de-normalised families use `(out - y) * std`; None = 1).  `acc` (float64, `L.EVAL_ACC_DOUBLES`
    slots): acc[k] += w * terms[k] on the device, w = 1 on the first batch when `first_unweighted`.  `mixed_out` (needs `x`):
    receives out * mask + x * (1 - mask).  `workspace`: a `_Workspace(L.EVAL_WS_FLOATS)` of the caller (a throw-away one
    otherwise).  No host sync; capturable."""
    L.require_device(out, y, mask, x, acc, mixed_out, terms, what="eval_metrics input")
    out, y = L.f32c(out, "out"), L.f32c(y, "y")
    n = out.shape[0]
    if out.dim() != 2 or out.shape[1] != 4 or y.shape != out.shape or mask.shape != out.shape:
        raise RuntimeError(f"eval_metrics: out, y and mask must be (N, 4); got {tuple(out.shape)} / {tuple(y.shape)} / {tuple(mask.shape)}")
    if mask.dtype == torch.int64:
        code = 0
    else:
        mask, code = mask.to(torch.float32), 1
    mask = mask.contiguous()
    if x is not None:
        x = L.f32c(x, "x")
        if x.shape != out.shape:
            raise RuntimeError(f"eval_metrics: x must be {tuple(out.shape)}, got {tuple(x.shape)}")
    if mixed_out is not None and (x is None or mixed_out.dtype != torch.float32 or mixed_out.shape != out.shape
                                  or not mixed_out.is_contiguous()):
        raise RuntimeError("eval_metrics: mixed_out needs x and must be a contiguous float32 tensor of out's shape")
    if acc is not None and (acc.dtype != torch.float64 or acc.numel() != L.EVAL_ACC_DOUBLES or not acc.is_contiguous()):
        raise RuntimeError(f"eval_metrics: acc must be a contiguous float64 tensor of {L.EVAL_ACC_DOUBLES} elements")
    if terms is None:
        terms = torch.empty(len(L.EVAL_TERMS), dtype=torch.float32, device=out.device)
    elif terms.dtype != torch.float32 or terms.numel() != len(L.EVAL_TERMS) or not terms.is_contiguous():
        raise RuntimeError(f"eval_metrics: terms must be a contiguous float32 tensor of {len(L.EVAL_TERMS)} elements")
    std = _host_floats(std, 4, "eval_metrics: std must hold four values")
    ws = (workspace or _Workspace(L.EVAL_WS_FLOATS)).on(out.device)
    with torch.cuda.device(out.device):
        L.check(L.load().pfn_eval_metrics(out.data_ptr(), y.data_ptr(), L.ptr(x), mask.data_ptr(), code, n, std, float(weight),
                                          int(bool(first_unweighted)), terms.data_ptr(), L.ptr(acc), L.ptr(mixed_out),
                                          ws.data_ptr(), ws.numel() * 4, L.stream_ptr()), "pfn_eval_metrics")
    return terms


def eval_accumulate(loss, acc, weight=1.0, first_unweighted=False):
    """acc[0] += double(loss) * w on the device (`pfn_eval_accumulate`; acc: float64 {sum, batch counter}, w = 1 on the first
    batch when `first_unweighted`): the running sum of an evaluation loop without its per-batch `loss.item()`."""
    L.require_device(loss, acc, what="eval_accumulate input")
    if loss.dtype != torch.float32 or loss.numel() != 1:
        raise RuntimeError(f"eval_accumulate: loss must be one float32 value (got {loss.dtype} {tuple(loss.shape)})")
    if acc.dtype != torch.float64 or acc.numel() != 2 or not acc.is_contiguous():
        raise RuntimeError("eval_accumulate: acc must be a contiguous float64 tensor of 2 elements {sum, batch counter}")
    with torch.cuda.device(loss.device):
        L.check(L.load().pfn_eval_accumulate(loss.data_ptr(), float(weight), int(bool(first_unweighted)), acc.data_ptr(),
                                             L.stream_ptr()), "pfn_eval_accumulate")


# ------------------------------------------------------------------------------------------ per-bus error analysis
BUS_MOMENTS = ("count", "sum", "sum_abs", "sum_sq", "min", "max")      # the six values per (bus, feature, mask group)
MOMENT_AT = {k: i for i, k in enumerate(BUS_MOMENTS)}                   # ... and where each sits in the last axis


def bus_error_moments(device, n_bus: int) -> torch.Tensor:
    """The running moments of `bus_errors_accumulate`, cleared: float64 [n_bus, 4, 2, 6] (group 0: mask != 0, group 1: mask == 0;
    `BUS_MOMENTS`), min = +inf and max = -inf.  Clear it between epochs with `reset_bus_error_moments` -- outside a captured graph."""
    return reset_bus_error_moments(torch.empty(int(n_bus), 4, 2, 6, dtype=torch.float64, device=device))


def reset_bus_error_moments(moments: torch.Tensor) -> torch.Tensor:
    moments[..., :4] = 0.0
    moments[..., 4] = float("inf")
    moments[..., 5] = float("-inf")
    return moments


def _host_floats(v, count, complaint):
    """`count` host floats (a sequence or a tensor; None stays None) as a C float array; RuntimeError(`complaint`) on another length."""
    import ctypes as C
    if v is None:
        return None
    v = [float(a) for a in (v.detach().cpu().reshape(-1).tolist() if torch.is_tensor(v) else v)]
    if len(v) != count:
        raise RuntimeError(complaint)
    return (C.c_float * count)(*v)


def bus_errors_accumulate(out, y, mask, n_bus, sample_idx, moments, flags, std=None, mean=None, err_table=None, pred_table=None,
                          table_rows=None):
    """One uniform batch of ONE case (graph g = rows [g n_bus, (g + 1) n_bus) of out / y / mask) in ONE launch
    (`pfn_bus_errors_accumulate`): the de-normalised errors (out - y) * std go to row sample_idx[g] of `err_table`, the predictions
    out * std + mean to that row of `pred_table` (each [rows, n_bus, 4] float32 or None) and into `moments` (`bus_error_moments`).
    `std` / `mean`: four host floats each (None: 1 / 0).  `sample_idx`: device int64 [n_graphs]; an index outside the table sets bit
    0 of `flags` (device int32) and its graph is left out.  `table_rows`: the bound of the indices when no table is given (with a
    table: its rows; neither: the indices are not read and every graph counts).  No host sync; capturable."""
    L.require_device(out, y, mask, sample_idx, moments, flags, err_table, pred_table, what="bus_errors_accumulate input")
    out, y = L.f32c(out, "out"), L.f32c(y, "y")
    n_bus = int(n_bus)
    if out.dim() != 2 or out.shape[1] != 4 or y.shape != out.shape or mask.shape != out.shape:
        raise RuntimeError(f"bus_errors_accumulate: out, y and mask must be (N, 4); got {tuple(out.shape)} / {tuple(y.shape)} / {tuple(mask.shape)}")
    if n_bus <= 0 or out.shape[0] % n_bus != 0:
        raise RuntimeError(f"bus_errors_accumulate: {out.shape[0]} rows are not whole graphs of {n_bus} buses")
    n_graphs = out.shape[0] // n_bus
    if mask.dtype == torch.int64:
        code = 0
    else:
        mask, code = mask.to(torch.float32), 1
    mask = mask.contiguous()
    if sample_idx.dtype != torch.int64 or sample_idx.numel() != n_graphs or not sample_idx.is_contiguous():
        raise RuntimeError(f"bus_errors_accumulate: sample_idx must be a contiguous int64 tensor of {n_graphs} elements")
    rows = None
    for name, tab in (("err_table", err_table), ("pred_table", pred_table)):
        if tab is None:
            continue
        if tab.dtype != torch.float32 or tab.dim() != 3 or tuple(tab.shape[1:]) != (n_bus, 4) or not tab.is_contiguous():
            raise RuntimeError(f"bus_errors_accumulate: {name} must be a contiguous float32 tensor of shape (rows, {n_bus}, 4)")
        if rows is not None and tab.shape[0] != rows:
            raise RuntimeError("bus_errors_accumulate: the two tables must have the same number of rows")
        rows = int(tab.shape[0])
    if rows is None:
        rows = None if table_rows is None else int(table_rows)
    elif table_rows is not None and int(table_rows) != rows:
        raise RuntimeError(f"bus_errors_accumulate: table_rows {int(table_rows)} against tables of {rows} rows")
    if moments.dtype != torch.float64 or moments.numel() != n_bus * 48 or not moments.is_contiguous():
        raise RuntimeError(f"bus_errors_accumulate: moments must be a contiguous float64 tensor of {n_bus} x 4 x 2 x 6 elements")
    if flags.dtype != torch.int32 or flags.numel() < 1:
        raise RuntimeError("bus_errors_accumulate: flags must be an int32 tensor")
    with torch.cuda.device(out.device):
        L.check(L.load().pfn_bus_errors_accumulate(out.data_ptr(), y.data_ptr(), mask.data_ptr(), code, n_graphs, n_bus,
                                                   _host_floats(std, 4, "bus_errors_accumulate: std must hold four values"),
                                                   _host_floats(mean, 4, "bus_errors_accumulate: mean must hold four values"),
                                                   sample_idx.data_ptr() if rows is not None else None, rows if rows is not None else 0, L.ptr(err_table), L.ptr(pred_table),
                                                   moments.data_ptr(), flags.data_ptr(), L.stream_ptr()), "pfn_bus_errors_accumulate")


def bus_errors_histogram(table, edges, scale=None):
    """np.histogram(table[:, b, f] * scale[b, f], bins=edges[f]) for every (bus, feature) of a finished [S, n_bus, 4] float32 table
    in ONE launch (`pfn_bus_errors_histogram`).  `edges`: float64 [4, nbins + 1], increasing (moved to the device); `scale`: float32
    [n_bus, 4] or None.  Returns (hist int32 [n_bus, 4, nbins], outside int32 [n_bus, 4, 3] = below / above / NaN) on the device."""
    L.require_device(table, scale, what="bus_errors_histogram input")
    table = L.f32c(table, "table")
    if table.dim() != 3 or table.shape[2] != 4:
        raise RuntimeError(f"bus_errors_histogram: the table must be (S, n_bus, 4); got {tuple(table.shape)}")
    S, n_bus = int(table.shape[0]), int(table.shape[1])
    if S >= 2 ** 31:
        raise RuntimeError("bus_errors_histogram: counts are 32-bit, the table must hold fewer than 2^31 samples")
    edges = torch.as_tensor(edges, dtype=torch.float64).to(table.device).contiguous()
    if edges.dim() != 2 or edges.shape[0] != 4:
        raise RuntimeError(f"bus_errors_histogram: edges must be (4, nbins + 1); got {tuple(edges.shape)}")
    nbins = int(edges.shape[1]) - 1
    if scale is not None:
        scale = L.f32c(scale, "scale")
        if tuple(scale.shape) != (n_bus, 4):
            raise RuntimeError(f"bus_errors_histogram: scale must be ({n_bus}, 4); got {tuple(scale.shape)}")
    hist = torch.empty(n_bus, 4, max(nbins, 0), dtype=torch.int32, device=table.device)
    outside = torch.empty(n_bus, 4, 3, dtype=torch.int32, device=table.device)
    with torch.cuda.device(table.device):
        L.check(L.load().pfn_bus_errors_histogram(table.data_ptr(), S, n_bus, L.ptr(scale), edges.data_ptr(), nbins, hist.data_ptr(),
                                                  outside.data_ptr(), L.stream_ptr()), "pfn_bus_errors_histogram")
    return hist, outside


# ------------------------------------------------------------------------------------------ per-line branch flows
BRANCH_QUANTITIES = ("I", "P", "Q", "loss")      # the four values per (sample, line): current magnitude, P and Q message, series loss


def branch_moments(device, n_lines: int) -> torch.Tensor:
    """The running moments of `branch_flows`, cleared: float64 [n_lines, 4, 6] (`BRANCH_QUANTITIES` x `BUS_MOMENTS`), min = +inf and
    max = -inf.  Clear it again with `reset_bus_error_moments` -- outside a captured graph."""
    return reset_bus_error_moments(torch.empty(int(n_lines), 4, 6, dtype=torch.float64, device=device))


def branch_flows_lds_max_bus() -> int:
    """The largest n_bus whose rectangular voltages `pfn_branch_flows` keeps in LDS; beyond it the direct kernel runs."""
    return int(L.load().pfn_branch_flows_lds_max_bus())


def branch_flows(pred, edge_index, edge_attr, truth=None, pred_normalised=False, truth_normalised=False, std=None, mean=None,
                 edge_std=None, edge_mean=None, flows_pred=False, flows_true=False, errors=True, moments=None, flags=None):
    """The line currents and flows of finished bus tables in ONE call (`pfn_branch_flows`: a flows launch, and a moments launch when
    `moments` is given).  `pred` / `truth`: float32 [S, n_bus, 4] rows (Vm, Va in degrees, P, Q); a `*_normalised` table is
    de-normalised with the host floats `std` / `mean` (four each; None: 1 / 0).  `edge_index`: int64 local ids, [2, e] for all
    samples or [S, 2, e]; `edge_attr`: float32 (r, x), [e, 2] or [S, e, 2], de-normalised with `edge_std` / `edge_mean` (two each).
    `flows_pred` / `flows_true` / `errors`: True (allocate), False (leave out) or a float32 [S, e, 4] tensor to write; without
    `truth` only `flows_pred` exists (then allocated by default).  `moments`: `branch_moments(device, e)`, accumulated into;
    `flags`: device int32, bit 0 = a line named a bus outside [0, n_bus).  Returns (flows_pred, flows_true, errors, flags), the
    `BRANCH_QUANTITIES` of every (sample, stored line i = edge_index[0] -> j = edge_index[1]).  No host sync; capturable."""
    L.require_device(pred, truth, edge_index, edge_attr, moments, flags, what="branch_flows input")
    pred = L.f32c(pred, "pred")
    if pred.dim() != 3 or pred.shape[2] != 4:
        raise RuntimeError(f"branch_flows: pred must be (S, n_bus, 4); got {tuple(pred.shape)}")
    S, n_bus = int(pred.shape[0]), int(pred.shape[1])
    if truth is not None:
        truth = L.f32c(truth, "truth")
        if truth.shape != pred.shape:
            raise RuntimeError(f"branch_flows: truth {tuple(truth.shape)} against pred {tuple(pred.shape)}")
    else:
        if moments is not None or torch.is_tensor(flows_true) or torch.is_tensor(errors):
            raise RuntimeError("branch_flows: moments, flows_true and errors need a truth table")
        flows_pred, flows_true, errors = (flows_pred if torch.is_tensor(flows_pred) else True), False, False
    if edge_index.dtype != torch.int64 or edge_index.dim() not in (2, 3) or edge_index.shape[-2] != 2:
        raise RuntimeError(f"branch_flows: edge_index must be int64 (2, e) or (S, 2, e); got {edge_index.dtype} {tuple(edge_index.shape)}")
    e = int(edge_index.shape[-1])
    edge_attr = L.f32c(edge_attr, "edge_attr")
    if edge_attr.dim() not in (2, 3) or tuple(edge_attr.shape[-2:]) != (e, 2):
        raise RuntimeError(f"branch_flows: edge_attr must be ({e}, 2) or (S, {e}, 2); got {tuple(edge_attr.shape)}")
    for name, t in (("edge_index", edge_index), ("edge_attr", edge_attr)):
        if t.dim() == 3 and t.shape[0] != S:
            raise RuntimeError(f"branch_flows: per-sample {name} of {t.shape[0]} samples against tables of {S}")
    edge_index = edge_index.contiguous()
    dev = pred.device
    outs = []
    for name, want in (("flows_pred", flows_pred), ("flows_true", flows_true), ("errors", errors)):
        if torch.is_tensor(want):
            if want.dtype != torch.float32 or tuple(want.shape) != (S, e, 4) or not want.is_contiguous() or want.device != dev:
                raise RuntimeError(f"branch_flows: {name} must be a contiguous float32 tensor of shape ({S}, {e}, 4) on {dev}")
            outs.append(want)
        else:
            outs.append(torch.empty(S, e, 4, dtype=torch.float32, device=dev) if want else None)
    ws = None
    if moments is not None:
        if moments.dtype != torch.float64 or moments.numel() != e * 24 or not moments.is_contiguous():
            raise RuntimeError(f"branch_flows: moments must be a contiguous float64 tensor of {e} x 4 x 6 elements")
        if outs[2] is None:
            ws = torch.empty(S, e, 4, dtype=torch.float32, device=dev)
    if flags is None:
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
    elif flags.dtype != torch.int32 or flags.numel() < 1:
        raise RuntimeError("branch_flows: flags must be an int32 tensor")
    std, mean, edge_std, edge_mean = (_host_floats(v, count, f"branch_flows: {what} must hold {count} values")
                                      for v, count, what in ((std, 4, "std"), (mean, 4, "mean"), (edge_std, 2, "edge_std"), (edge_mean, 2, "edge_mean")))
    with torch.cuda.device(dev):
        L.check(L.load().pfn_branch_flows(pred.data_ptr(), int(bool(pred_normalised)), L.ptr(truth), int(bool(truth_normalised)), S, n_bus,
                                          std, mean, edge_index.data_ptr(),
                                          int(edge_index.dim() == 3), e, edge_attr.data_ptr(), int(edge_attr.dim() == 3), edge_std, edge_mean,
                                          L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]), L.ptr(moments), flags.data_ptr(), L.ptr(ws),
                                          0 if ws is None else ws.numel() * 4, L.stream_ptr()), "pfn_branch_flows")
    return outs[0], outs[1], outs[2], flags
