"""Batched AC / DC / fast-decoupled power flow on the device: `solve_power_flow` is ONE `pfn_powerflow_solve_init` launch
(csrc/powerflow.hip), one workgroup per sample, from a flat start or from a table the caller gives (a model's prediction).  It stands where the reference calls pandapower -- `pp.runpp` in dataset_generator.py, `pp.rundcpp` in
dc_error.py -- for this project's network model: series admittance only, every stored line in both directions, P and Q
demand-positive per-unit, Va in degrees; no shunts, line charging, taps, Q-limits or unit conversion.  The mismatch it drives to zero
is exactly `PowerImbalance`'s dP_i, dQ_i, so a solved table is what that loss calls balanced.  No CPU path."""
import ctypes as C
import time
from dataclasses import dataclass

import torch

from .. import _lib as L

# the texts of csrc/powerflow_common.hpp's status enum (PF_NOT_CONVERGED ... PF_STALE_PLAN), which every route's kernel writes
STATUS = {-1: "not converged in max_iter", -2: "singular Jacobian", -3: "non-finite mismatch", -4: "a line names a bus outside the grid",
          -5: "bus_type disagrees with the counts the launch was sized for",
          -6: "the sparse plan was built from another line list or other bus types"}
_MODES = {"ac": 0, "dc": 1, "fdxb": 2, "fdbx": 3}
_ROUTES = {"auto": 0, "lds": 1, "global": 2, "sparse": 3}
_PLAN_HEADER_WORDS = 32          # csrc/powerflow_plan.hpp: n, e, m, mode at words 2..5, slab positions 6, nnz(L) 7, multiply-adds 8 / 9
_FD_PLAN_MODES = ("fd", "fdxb", "fdbx")      # one plan serves both variants: only the weights differ


@dataclass
class PowerFlowResult:
    """`table` [S, n, 4] float64 (Vm, Va in degrees, P, Q; NaN rows where the sample failed), `status` [S] int32 (>= 0: Jacobian
    solves used -- half-iterations in the fast-decoupled modes; < 0: `STATUS`), `iterations` [S] int32 (the status where it is >= 0, else -1), `residual` [S] float64 (the last
    max |F|), `flags` [1] int32 (bit 0: `bus_type` changed under the launch) -- all on the device, nothing read back; `route`: the
    route that ran, "lds", "global" or "sparse"."""
    table: torch.Tensor
    status: torch.Tensor
    iterations: torch.Tensor
    residual: torch.Tensor
    flags: torch.Tensor
    route: str


def max_unknowns() -> int:
    """The largest m = (n - 1) + n_pq the dense solver takes (global route); beyond it a sparse factorisation is needed."""
    return int(L.load().pfn_powerflow_max_unknowns())


@dataclass
class SparsePlan:
    """The symbolic half of the sparse route for ONE grid (csrc/powerflow_plan.cpp): `blob` the plan on the device (uint8), `header`
    its first 32 int32 words on the host, and what a report needs -- `n`, `e`, `m` unknowns, `mode`, `nnz` slab positions per sample,
    `nnz_l` = nnz(L), `madds` multiply-adds of one factorisation, `max_col` the longest L column, `bytes` of the plan, `build_s` the
    host time it took.  mode "fd" (the fast-decoupled plan: B' and B'' side by side): `m` is the order of B' (n - 1), `m_q` that of
    B'' (the PQ buses; 0 in the other modes), `nnz`, `nnz_l`, `madds` and `bytes` are totals over both, `max_col` the larger half's,
    and `halves` holds (m, nnz, nnz_l, madds, max_col) of each half, P first."""
    blob: torch.Tensor
    header: object
    n: int
    e: int
    m: int
    mode: str
    nnz: int
    nnz_l: int
    madds: int
    max_col: int
    bytes: int
    build_s: float
    m_q: int = 0
    halves: tuple = ()


def sparse_plan(bus_type, edge_index, mode="ac") -> SparsePlan:
    """Plan the sparse route for the grid (`bus_type` [n], `edge_index` int64 [2, e]; device or host tensors): one host read of the
    two, a minimum-degree order and the filled pattern built by the library on the host, one upload.  Reuse the plan for every solve
    on that grid and mode ("ac" or "dc").  mode "fd" (also spelled "fdxb" or "fdbx"; the plan's `mode` is "fd" either way): the
    fast-decoupled plan, the symbolic factorisations of B' and B'' in one blob, for `solve_power_flow(mode="fdxb" | "fdbx")`."""
    if mode not in ("ac", "dc") + _FD_PLAN_MODES:
        raise ValueError("sparse_plan: mode must be 'ac', 'dc' or 'fd' ('fdxb' and 'fdbx' are spellings of 'fd')")
    fd = mode in _FD_PLAN_MODES
    if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64 or bus_type.dim() != 1:
        raise RuntimeError(f"sparse_plan: edge_index must be int64 (2, e) and bus_type (n,); got {tuple(edge_index.shape)} and {tuple(bus_type.shape)}")
    dev = edge_index.device if edge_index.is_cuda else bus_type.device
    ei = edge_index.detach().cpu().contiguous()
    bt = bus_type.detach().to(torch.int32).cpu().contiguous()
    lib = L.load()
    e, n = int(ei.shape[1]), int(bt.shape[0])
    t0 = time.perf_counter()
    if fd:
        need = int(lib.pfn_powerflow_sparse_fd_plan_bytes(ei.data_ptr(), e, bt.data_ptr(), n))
    else:
        need = int(lib.pfn_powerflow_sparse_plan_bytes(ei.data_ptr(), e, bt.data_ptr(), n, _MODES[mode]))
    if need == 0:
        raise RuntimeError(f"sparse_plan failed: {lib.pfn_last_error().decode('utf-8', 'replace')}")
    host = torch.empty(need, dtype=torch.uint8)
    if fd:
        L.check(lib.pfn_powerflow_sparse_fd_plan(ei.data_ptr(), e, bt.data_ptr(), n, host.data_ptr(), need), "pfn_powerflow_sparse_fd_plan")
    else:
        L.check(lib.pfn_powerflow_sparse_plan(ei.data_ptr(), e, bt.data_ptr(), n, _MODES[mode], host.data_ptr(), need), "pfn_powerflow_sparse_plan")
    build_s = time.perf_counter() - t0

    def header(at):
        return (C.c_int32 * _PLAN_HEADER_WORDS).from_buffer_copy(host[at:at + 4 * _PLAN_HEADER_WORDS].numpy().tobytes())

    def madds(w):
        return (int(w[9]) << 32) | (int(w[8]) & 0xffffffff)
    h = header(0)
    halves = tuple((int(w[4]), int(w[6]), int(w[7]), madds(w), int(w[11])) for w in (header(int(h[16])), header(int(h[17])))) if fd else ()
    return SparsePlan(blob=host.to(dev), header=h, n=n, e=e, m=int(h[4]), mode="fd" if fd else mode, nnz=int(h[6]), nnz_l=int(h[7]),
                      madds=madds(h), max_col=int(h[11]), bytes=need, build_s=build_s, m_q=int(h[15]) if fd else 0, halves=halves)


def solve_power_flow(bus_type, spec, edge_index, rx, *, mode="ac", tol=1e-8, max_iter=10, route="auto", init=None, plan=None) -> PowerFlowResult:
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

    route "sparse": the same loop beyond `max_unknowns()` -- a sparse fp32 factor under a static minimum-degree order, no pivoting
    (csrc/powerflow_sparse.hip), modes "ac" and "dc", one `[2, e]` line list for all samples.  `plan`: a `sparse_plan(bus_type,
    edge_index, mode)` to reuse; None builds one here (a host read of the grid and a host computation: build it once per grid).  A
    plan for another n, e or mode raises; one for other lines of the same size gives status -6.  "auto" never takes this route.
    Modes "fdxb" / "fdbx" on this route (csrc/powerflow_sparse_fd.hip) keep the sparse fp32 FACTORS of B' and B'' -- factored once
    per sample -- where the dense route keeps their inverses; same half-iterations, `init`, `tol` and `max_iter`.  They need
    `plan=sparse_plan(bus_type, edge_index, "fd")` (one plan serves both variants); without a plan they are dense only: ValueError.

    One host read (the counts of `bus_type`, which size the launch); no read-back of the results."""
    return _solve(bus_type, spec, edge_index, rx, mode, tol, max_iter, route, init, plan, 0)


def _solve(bus_type, spec, edge_index, rx, mode, tol, max_iter, route, init, plan, threads) -> PowerFlowResult:
    """`solve_power_flow` with the sparse route's workgroup size exposed (`threads`: 0 the library's choice, 64 or 256): what
    tools/powerflow_bench.py and the tests measure the two sizes with."""
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
    if route == "sparse":
        fd = mode in ("fdxb", "fdbx")
        if fd and plan is None:
            raise ValueError(f"solve_power_flow: route 'sparse' with mode {mode!r}: pass plan=sparse_plan(bus_type, edge_index, 'fd'); "
                             "without a plan the fast-decoupled modes are dense only")
        if edge_index.dim() == 3:
            raise RuntimeError("solve_power_flow: route 'sparse' takes one (2, e) line list for all samples: a plan belongs to one topology")
        if plan is None:
            plan = sparse_plan(bt, edge_index, mode)
        if not isinstance(plan, SparsePlan) or (plan.n, plan.e, plan.mode) != (n, e, "fd" if fd else mode):
            raise RuntimeError(f"solve_power_flow: the plan is for (n, e, mode) = {(plan.n, plan.e, plan.mode) if isinstance(plan, SparsePlan) else plan!r}; "
                               f"the call has {(n, e, mode)}")
        if plan.blob.device != dev:
            raise RuntimeError(f"solve_power_flow: the plan lives on {plan.blob.device}, the inputs on {dev}")
        sizer, launch, what = ((lib.pfn_powerflow_sparse_fd_workspace_bytes, lib.pfn_powerflow_solve_sparse_fd, "pfn_powerflow_solve_sparse_fd") if fd
                               else (lib.pfn_powerflow_sparse_workspace_bytes, lib.pfn_powerflow_solve_sparse, "pfn_powerflow_solve_sparse"))
        need = int(sizer(S, C.addressof(plan.header))) if S else 0
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            L.check(launch(edge_index.data_ptr(), e, rx.data_ptr(), bt.data_ptr(), spec.data_ptr(), L.ptr(init), S, n,
                           _MODES[mode], float(tol), int(max_iter), C.addressof(plan.header), plan.blob.data_ptr(),
                           int(threads), table.data_ptr(), status.data_ptr(), residual.data_ptr(), flags.data_ptr(),
                           ws.data_ptr(), need, L.stream_ptr()),
                    what)
        return PowerFlowResult(table=table, status=status, iterations=torch.where(status >= 0, status, torch.full_like(status, -1)),
                               residual=residual, flags=flags, route="sparse")
    if plan is not None:
        raise ValueError("solve_power_flow: a plan goes with route='sparse' only")
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
