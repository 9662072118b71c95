"""Batched AC / DC / fast-decoupled power flow on the device: `solve_power_flow` is ONE `pfn_powerflow_solve_init` launch
(csrc/powerflow.hip), one workgroup per sample, from a flat start or from a table the caller gives (a model's prediction).  It stands where the reference calls pandapower -- `pp.runpp` in dataset_generator.py, `pp.rundcpp` in
dc_error.py -- for this project's network model: series admittance only, every stored line in both directions, P and Q
demand-positive per-unit, Va in degrees; no shunts, line charging, taps, Q-limits or unit conversion.  The mismatch it drives to zero
is exactly `PowerImbalance`'s dP_i, dQ_i, so a solved table is what that loss calls balanced.  No CPU path."""
from dataclasses import dataclass

import torch

from .. import _lib as L

STATUS = {-1: "not converged in max_iter", -2: "singular Jacobian", -3: "non-finite mismatch", -4: "a line names a bus outside the grid",
          -5: "bus_type disagrees with the counts the launch was sized for"}
_MODES = {"ac": 0, "dc": 1, "fdxb": 2, "fdbx": 3}
_ROUTES = {"auto": 0, "lds": 1, "global": 2}


@dataclass
class PowerFlowResult:
    """`table` [S, n, 4] float64 (Vm, Va in degrees, P, Q; NaN rows where the sample failed), `status` [S] int32 (>= 0: Jacobian
    solves used -- half-iterations in the fast-decoupled modes; < 0: `STATUS`), `iterations` [S] int32 (the status where it is >= 0, else -1), `residual` [S] float64 (the last
    max |F|), `flags` [1] int32 (bit 0: `bus_type` changed under the launch) -- all on the device, nothing read back; `route`: the
    route that ran, "lds" or "global"."""
    table: torch.Tensor
    status: torch.Tensor
    iterations: torch.Tensor
    residual: torch.Tensor
    flags: torch.Tensor
    route: str


def max_unknowns() -> int:
    """The largest m = (n - 1) + n_pq the dense solver takes (global route); beyond it a sparse factorisation is needed."""
    return int(L.load().pfn_powerflow_max_unknowns())


def solve_power_flow(bus_type, spec, edge_index, rx, *, mode="ac", tol=1e-8, max_iter=10, route="auto", init=None) -> PowerFlowResult:
    """Solve S power-flow problems on one grid.  `bus_type` [n] (0 slack, 1 PV, 2 PQ; exactly one slack; shared by the samples),
    `spec` [S, n, 4] float64 (Vm, Va, P, Q: the slack gives Vm and Va, a PV bus Vm and P, a PQ bus P and Q; the rest is ignored),
    `edge_index` int64 local ids [2, e] or [S, 2, e], `rx` [S, e, 2] float64.  mode "ac": Newton-Raphson from a flat start, fp64
    state and residual, fp32 LU of the analytic Jacobian; "dc": the linear B' theta = -P model (B' from 1 / x) refined to the same
    fp64 tolerance, Q NaN.  It stops when max |mismatch| < `tol` or after `max_iter` Jacobian solves.  `route`: "auto", "lds" (the
    matrix in LDS; RuntimeError where it does not fit) or "global" (in a workspace allocated here).

    mode "fdxb" / "fdbx": the fast-decoupled iterations (pandapower's `algorithm="fdxb"` / `"fdbx"`) on the same fp64 state, mismatch
    and tolerance.  B' (angle buses) and B'' (PQ buses) are built and inverted once per sample in fp32 -- XB: B' from 1 / x, B'' from
    x / (r^2 + x^2); BX the other way round -- and a half-iteration is theta -= B'^-1 (dP / Vm), then Vm -= B''^-1 (dQ / Vm),
    alternating, the mismatch re-formed and tested after each.  There `max_iter` and the returned `status` / `iterations` count
    HALF-iterations: the default 10 is Newton's and is usually too few -- 15 to 30 are typical at 1e-8 .. 1e-10, so pass e.g. 60.
    What pandapower uses as the fast-decoupled iteration limit could not be verified where this was written (it is not installed).

    `init`: None for the flat start, or a device table [S, n, >= 2] of any float dtype whose first two columns are (Vm, Va in degrees)
    -- e.g. the de-normalised prediction table of `bus_error_epoch(keep_predictions=True)`; it is cast to float64 on the device, no
    host read.  Only Va at the non-slack buses and Vm at the PQ buses are read ("dc": Va only); the rest comes from `spec`.  A
    non-finite entry fails that sample alone (status -3); a start already under `tol` returns status 0.

    tol = 1e-8 and max_iter = 10 are what pandapower's Newton-Raphson (`pp.runpp(algorithm="nr")`, per-unit mismatch) is believed to
    use; pandapower is not installed where this was written, so that could not be verified.

    One host read (the counts of `bus_type`, which size the launch); no read-back of the results."""
    L.require_device(bus_type, spec, edge_index, rx, what="solve_power_flow input")
    if mode not in _MODES or route not in _ROUTES:
        raise ValueError(f"solve_power_flow: mode must be one of {sorted(_MODES)} and route one of {sorted(_ROUTES)}")
    if spec.dtype != torch.float64 or spec.dim() != 3 or spec.shape[2] != 4:
        raise RuntimeError(f"solve_power_flow: spec must be float64 (S, n, 4); got {spec.dtype} {tuple(spec.shape)}")
    S, n = int(spec.shape[0]), int(spec.shape[1])
    if bus_type.dim() != 1 or bus_type.shape[0] != n or bus_type.dtype not in (torch.int32, torch.int64):
        raise RuntimeError(f"solve_power_flow: bus_type must be an integer tensor of {n} entries; got {bus_type.dtype} {tuple(bus_type.shape)}")
    if edge_index.dtype != torch.int64 or edge_index.dim() not in (2, 3) or edge_index.shape[-2] != 2:
        raise RuntimeError(f"solve_power_flow: edge_index must be int64 (2, e) or (S, 2, e); got {edge_index.dtype} {tuple(edge_index.shape)}")
    e = int(edge_index.shape[-1])
    if edge_index.dim() == 3 and edge_index.shape[0] != S:
        raise RuntimeError(f"solve_power_flow: per-sample edge_index of {edge_index.shape[0]} samples against {S}")
    if rx.dtype != torch.float64 or tuple(rx.shape) != (S, e, 2):
        raise RuntimeError(f"solve_power_flow: rx must be float64 ({S}, {e}, 2); got {rx.dtype} {tuple(rx.shape)}")
    if init is not None:
        L.require_device(init, what="solve_power_flow init")
        if not init.is_floating_point() or init.dim() != 3 or tuple(init.shape[:2]) != (S, n) or init.shape[2] < 2:
            raise RuntimeError(f"solve_power_flow: init must be a float table ({S}, {n}, >= 2); got {init.dtype} {tuple(init.shape)}")
        init = init[:, :, :2].to(torch.float64).contiguous()
    dev = spec.device
    bt = bus_type.to(torch.int32).contiguous()
    counts = torch.bincount(bt.clamp(0, 3).long(), minlength=4).tolist()
    if counts[0] != 1 or counts[3] != 0 or bool((bt < 0).any()):
        raise RuntimeError(f"solve_power_flow: bus_type needs exactly one slack (0) and only types 0, 1, 2; got counts {counts}")
    n_pv, n_pq = counts[1], counts[2]
    spec, rx, edge_index = spec.contiguous(), rx.contiguous(), edge_index.contiguous()
    lib = L.load()
    table = torch.empty(S, n, 4, dtype=torch.float64, device=dev)
    status = torch.empty(S, dtype=torch.int32, device=dev)
    residual = torch.empty(S, dtype=torch.float64, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    need = int(lib.pfn_powerflow_workspace_bytes_mode(S, n, e, n_pq, _MODES[mode], _ROUTES[route]))
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    with torch.cuda.device(dev):
        L.check(lib.pfn_powerflow_solve_init(edge_index.data_ptr(), int(edge_index.dim() == 3), e, rx.data_ptr(), bt.data_ptr(),
                                             spec.data_ptr(), L.ptr(init), S, n, n_pv, n_pq, _MODES[mode], float(tol), int(max_iter),
                                             _ROUTES[route], table.data_ptr(), status.data_ptr(), residual.data_ptr(), flags.data_ptr(),
                                             L.ptr(ws), need, L.stream_ptr()),
                "pfn_powerflow_solve_init")
    return PowerFlowResult(table=table, status=status, iterations=torch.where(status >= 0, status, torch.full_like(status, -1)),
                           residual=residual, flags=flags, route="global" if need else "lds")
