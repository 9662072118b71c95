"""N-1 line-outage screening on the device: `contingency_screen` asks, for every scenario and every single line outage, how hard the
remaining lines are loaded -- two launches (csrc/contingency.hip): `pfn_contingency_islands`, one workgroup per outage, finds the
outages that cut buses off the slack; `pfn_contingency_dc`, one workgroup per scenario, solves the DC model of
`solve_power_flow(mode="dc")` once, keeps B'^-1 resident and reads every outage's flows off line outage distribution factors.
`verify_contingencies` re-solves chosen (scenario, outage) pairs with the unchanged AC solver on the reduced line lists and reports
the AC current loadings beside the DC screen's.  Beyond the dense cap (n - 1 > `max_unknowns()`) `route="sparse"` keeps the sparse
fp32 FACTOR of B' under a `sparse_plan(..., mode="dc")` and substitutes 64 outages at a time (csrc/contingency_sparse.hip:
`pfn_contingency_sparse`, two launches behind the islands).  `contingency_screen_pairs` is the N-2 screen: every pair of candidate
lines out together, a rank-2 update of the same inverse (csrc/contingency_pairs.hip: `pfn_contingency_pair_islands`,
`pfn_contingency_pairs`) or, with `route="sparse"`, of one substituted column per candidate under the same plan
(csrc/contingency_pairs_sparse.hip: `pfn_contingency_pairs_sparse`); `verify_pair_contingencies` is its AC check.
`contingency_screen_model` asks the NETWORK instead of the DC model: every (scenario, outage) becomes one graph of a batch
(csrc/contingency_model.hip: `pfn_contingency_model_batch`), the model predicts, and `pfn_contingency_model_loadings` turns the
predictions into line currents and the screen's three figures -- reactive flow and voltage magnitude included.
`contingency_screen_ac` is the AC screen by compensated 1P1Q (csrc/contingency_ac.hip: `pfn_contingency_ac`, two launches behind the
islands): the fast-decoupled base solve of `solve_power_flow(mode="fdxb" | "fdbx")` per scenario, then a wave per (scenario, outage)
takes `halves` half-iterations with B'^-1 and B''^-1 corrected for the missing line by a rank-1 update, and reports the loadings
from line currents together with the lowest voltage, the voltage violations and the remaining mismatch; beyond the dense cap
`route="sparse"` with a `sparse_plan(..., mode="fd")` runs the same screen on the sparse fp32 factors of B' and B''
(csrc/contingency_ac_sparse.hip: `pfn_contingency_ac_sparse`), a lane per outage, 64 outages to a one-wave workgroup.
`contingency_screen_units` screens GENERATOR outages under the DC model on the dense routes (csrc/contingency_units.hip:
`pfn_contingency_units`, one launch, one workgroup per scenario): a unit outage changes the right-hand side only, so the resident
inverse answers it with one column, the lost output picked up by the slack or shared among the other units by participation
factors; with `lines` every unit outage is followed by each candidate line outage (distribution factors on the post-unit flows,
the islands launch first).  `verify_unit_contingencies` is its AC check on the shifted specification.  No CPU path."""
import contextlib
import ctypes as C
import operator
from dataclasses import dataclass

import torch
import torch.nn as nn

from .. import _lib as L
from .captured import capture_state, held_adjacencies, no_gc, topology_owners, warm_up
from .powerflow import STATUS, SparsePlan, cover_plan, solve_power_flow  # noqa: F401  (STATUS: the texts of `ContingencyResult.status`)

_ROUTES = {"auto": 0, "lds": 1, "global": 2}
_BLOCKS = {"auto": 0, "lds": 1, "global": 2}
_COLUMNS = {"auto": 0, "lds": 1, "global": 2}
_COUNTS_ATTR = "_pfn_bus_counts"  # on a bus_type tensor: (version, (n_pv, n_pq, slack)) -- one host read per tensor
_COUNTS_EAGER_FIRST = "contingency_screen: the bus_type counts are read on the host once per tensor; call it eagerly once before capturing"


@dataclass
class ContingencyResult:
    """Per (scenario s, outage k): `severity` [S, e] float32 (the largest loading |f_l| / rating_l over the monitored lines l != k;
    +inf where the outage islands buses, NaN where the scenario failed or a loading is not finite), `worst_line` [S, e] int32 (its
    line, ties to the lowest; -1 where none), `overloads` [S, e] int32 (monitored lines with loading > 1; -1 where islanding or
    failed).  `islands` [e] int32: buses cut off the slack by outage k (the line list decides, not the scenario; -4: a line names a
    bus outside the grid).  Per scenario: `base_flow` [S, e] float64 and `status` [S] int32 (>= 0: refinement solves; < 0:
    `utils.powerflow.STATUS`).  `post_flow` [S, e, e] float32 (row = outage, column = line) with `keep_table`, else None.  `flags`
    [1] int32 (bit 0: `bus_type` changed under the launch).  All on the device, nothing read back; `route`: "lds", "global" or
    "sparse" (there `block` says where the outage blocks sat: "lds" or "global")."""
    severity: torch.Tensor
    worst_line: torch.Tensor
    overloads: torch.Tensor
    islands: torch.Tensor
    base_flow: torch.Tensor
    status: torch.Tensor
    post_flow: object
    route: str
    flags: object = None
    block: object = None

    def ranking(self, top):
        """(int64 [S, top] outage ids, [S, top] their severities): per scenario the `top` outages by severity, descending -- NaN
        first (a failure must not hide), then +inf (the islanding outages), ties to the lowest outage id.  Plain torch on the
        tensors' device: it is not hot."""
        return _rank(self.severity, top, "ranking")


@dataclass
class ContingencyVerification:
    """`pairs` [T, 2] int64 (scenario, outage), the AC `table` [T, n, 4] float64 and `status` [T] int32 of `solve_power_flow` on the
    grid without the line, `loading` [T, e] float32 = I_l / rating_l in the ORIGINAL line numbering (NaN at the outaged line),
    `severity` [T] float32 / `worst_line` [T] int32 / `overloads` [T] int32 by the screen's rules, and `dc_severity` [T] float32, the
    screen's figure for the pair."""
    pairs: torch.Tensor
    table: torch.Tensor
    status: torch.Tensor
    loading: torch.Tensor
    severity: torch.Tensor
    worst_line: torch.Tensor
    overloads: torch.Tensor
    dc_severity: torch.Tensor


def _rank(sev, top, who):
    """`ContingencyResult.ranking`'s order over the columns of `sev`"""
    width = int(sev.shape[1])
    if isinstance(top, bool) or not isinstance(top, int) or not 0 <= top <= width:
        raise ValueError(f"{who}: top must be an int in [0, {width}]; got {top!r}")
    # NaN, +inf and the finite values as three classes, then the value: a stable sort keeps the lowest id among equals
    cls = torch.where(torch.isnan(sev), 2, torch.where(torch.isposinf(sev), 1, 0))
    val = torch.where(cls == 0, sev, torch.zeros_like(sev))
    order = torch.sort(val, dim=1, descending=True, stable=True).indices
    order = order.gather(1, torch.sort(cls.gather(1, order), dim=1, descending=True, stable=True).indices)[:, :top]
    return order, sev.gather(1, order)


@dataclass
class PairContingencyResult:
    """Per (scenario s, pair p): `severity` [S, P] float32, `worst_line` [S, P] int32 and `overloads` [S, P] int32 by
    `ContingencyResult`'s rules with BOTH outaged lines unmonitored (+inf, -1, -1 where the pair islands buses; NaN, -1, -1 where the
    scenario failed).  `pairs` [P, 2] int64: the two lines of pair p, in `pair_lines`' order.  `islands` [P] int32: buses cut off
    the slack with both lines removed (-4: a line names a bus outside the grid).  `base_flow` [S, e] float64 and `status` [S] int32
    carry `contingency_screen`'s bits for the same inputs.  `post_flow` [S, P, e] float32 with `keep_table`, else None.  `flags` [1]
    int32 (bit 0: `bus_type` changed under the launch).  All on the device; `route`: "lds", "global" or "sparse" (there `block` says
    where the column launch's blocks sat and `columns` where the pair launch's columns: "lds" or "global")."""
    severity: torch.Tensor
    worst_line: torch.Tensor
    overloads: torch.Tensor
    islands: torch.Tensor
    pairs: torch.Tensor
    base_flow: torch.Tensor
    status: torch.Tensor
    post_flow: object
    route: str
    flags: object = None
    block: object = None
    columns: object = None

    def ranking(self, top):
        """(int64 [S, top] pair indices, [S, top] their severities): `ContingencyResult.ranking`'s order -- NaN first, then +inf,
        then descending, ties to the lowest pair index."""
        return _rank(self.severity, top, "ranking")


def _candidates(lines_or_e, who):
    """the candidate lines as a list of ints: an int e means range(e); else a host sequence or a CPU int64 tensor"""
    if isinstance(lines_or_e, int) and not isinstance(lines_or_e, bool):
        if lines_or_e < 0:
            raise ValueError(f"{who}: a line count must be >= 0; got {lines_or_e}")
        return list(range(lines_or_e))
    if torch.is_tensor(lines_or_e):
        if lines_or_e.device.type != "cpu" or lines_or_e.dtype != torch.int64 or lines_or_e.dim() != 1:
            raise ValueError(f"{who}: lines as a tensor must be a CPU int64 vector; got {lines_or_e.dtype} {tuple(lines_or_e.shape)} on {lines_or_e.device}")
        return lines_or_e.tolist()
    got = list(lines_or_e)
    try:
        if any(isinstance(k, bool) for k in got):
            raise TypeError
        return [operator.index(k) for k in got]                               # (numpy integers too)
    except TypeError:
        raise ValueError(f"{who}: lines must be ints; got {got!r}") from None


def pair_lines(lines_or_e):
    """int64 [P, 2] (CPU): the pairs of the candidate lines (an int e: all of range(e)) in the screen's order -- pair p is
    (lines[i], lines[j]), i < j, row-major in (i, j); P = c (c - 1) / 2."""
    lines = _candidates(lines_or_e, "pair_lines")
    c = len(lines)
    ij = torch.triu_indices(c, c, 1)
    return torch.tensor(lines, dtype=torch.int64)[ij].t().contiguous().reshape(-1, 2)


def pair_index(i, j, c):
    """`pair_lines`' inverse: the index p of the pair of candidate POSITIONS i < j among c candidates (ints or integer tensors)."""
    return i * (2 * c - i - 1) // 2 + (j - i - 1)


def pair_positions(p, c):
    """(i, j), the candidate positions of pair index p among c candidates (a Python int)."""
    if isinstance(p, bool) or not isinstance(p, int) or not 0 <= p < c * (c - 1) // 2:
        raise ValueError(f"pair_positions: pair {p!r} is outside [0, {c * (c - 1) // 2})")
    i = 0
    while p >= c - 1 - i:                                                      # (row i of the upper triangle holds c - 1 - i pairs)
        p -= c - 1 - i
        i += 1
    return i, i + 1 + p


def _bus_counts(bus_type):
    """(n_pv, n_pq, slack) of a device bus_type tensor: ONE host read, kept ON the tensor object with the version it was read at, so
    that a second call with the same, unmodified tensor -- a graph capture after its eager warm-up -- reads nothing.  (Not keyed by
    address: another tensor may come to live where a freed one was.)"""
    kept = getattr(bus_type, _COUNTS_ATTR, None)
    got = kept[1] if kept is not None and kept[0] == bus_type._version else None
    if got is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(_COUNTS_EAGER_FIRST)
        bt = bus_type.long()
        info = torch.cat([torch.bincount(bt.clamp(0, 3), minlength=4), (bt < 0).sum().view(1), (bt == 0).long().argmax().view(1)]).tolist()
        if info[0] != 1 or info[3] != 0 or info[4] != 0:
            raise RuntimeError(f"contingency_screen: bus_type needs exactly one slack (0) and only types 0, 1, 2; got counts {info[:4]}")
        got = (info[1], info[2], info[5])
        setattr(bus_type, _COUNTS_ATTR, (bus_type._version, got))
    return got


def _ratings(ratings, S, e, who):
    if ratings is None:
        return None
    L.require_device(ratings, what=f"{who} ratings")
    if ratings.dtype != torch.float64 or tuple(ratings.shape) not in ((e,), (S, e)):
        raise RuntimeError(f"{who}: ratings must be float64 ({e},) or ({S}, {e}); got {ratings.dtype} {tuple(ratings.shape)}")
    return ratings.contiguous()


def _check(bus_type, spec, edge_index, rx, who):
    L.require_device(bus_type, spec, edge_index, rx, what=f"{who} input")
    if spec.dtype != torch.float64 or spec.dim() != 3 or spec.shape[2] != 4:
        raise RuntimeError(f"{who}: spec must be float64 (S, n, 4); got {spec.dtype} {tuple(spec.shape)}")
    S, n = int(spec.shape[0]), int(spec.shape[1])
    if bus_type.dim() != 1 or bus_type.shape[0] != n or bus_type.dtype not in (torch.int32, torch.int64):
        raise RuntimeError(f"{who}: bus_type must be an integer tensor of {n} entries; got {bus_type.dtype} {tuple(bus_type.shape)}")
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise RuntimeError(f"{who}: edge_index must be int64 (2, e), one line list for all scenarios; got {edge_index.dtype} {tuple(edge_index.shape)}")
    e = int(edge_index.shape[1])
    if rx.dtype != torch.float64 or tuple(rx.shape) != (S, e, 2):
        raise RuntimeError(f"{who}: rx must be float64 ({S}, {e}, 2); got {rx.dtype} {tuple(rx.shape)}")
    if n < 2 or e < 1:
        raise ValueError(f"{who}: a grid of {n} buses and {e} lines has no outage to screen")
    return S, n, e


def _prepare(who, bus_type, spec, edge_index, rx, ratings, plan=None, after_check=None):
    """What the DC screens do with their inputs, in this order: `_check`, `after_check(n, e)` (a screen's own refusals), `_ratings`,
    the plan's device (`route="sparse"`), `_bus_counts`, then int32 `bus_type` and contiguous inputs.  Returns (S, n, e,
    (n_pv, n_pq, slack), bus_type, spec, edge_index, rx, ratings)."""
    S, n, e = _check(bus_type, spec, edge_index, rx, who)
    if after_check is not None:
        after_check(n, e)
    ratings = _ratings(ratings, S, e, who)
    if plan is not None:
        _plan_device(who, plan, spec.device)
    counts = _bus_counts(bus_type)
    return S, n, e, counts, bus_type.to(torch.int32).contiguous(), spec.contiguous(), edge_index.contiguous(), rx.contiguous(), ratings


def _outputs(S, e, items, dev, keep_table):
    """The tensors a DC screen of `items` outages or pairs per scenario fills, as the result's fields: `severity`, `worst_line`,
    `overloads` [S, items], `base_flow` [S, e], `status` [S], `flags` [1] (zeroed) and `post_flow` [S, items, e] or None."""
    return dict(severity=torch.empty(S, items, dtype=torch.float32, device=dev), worst_line=torch.empty(S, items, dtype=torch.int32, device=dev),
                overloads=torch.empty(S, items, dtype=torch.int32, device=dev), base_flow=torch.empty(S, e, dtype=torch.float64, device=dev),
                status=torch.empty(S, dtype=torch.int32, device=dev), flags=torch.zeros(1, dtype=torch.int32, device=dev),
                post_flow=torch.empty(S, items, e, dtype=torch.float32, device=dev) if keep_table else None)


def _outputs_ac(S, n, e, dev, keep_table, keep_state):
    """The tensors an AC screen fills, as the result's fields and IN THE C ENTRIES' ORDER: the seven figures [S, e], `base_table`
    [S, n, 4], `status`, `residual` [S], `post_current` [S, e, e] and `post_state` [S, e, n, 2] or None, `flags` [1] (zeroed)."""
    new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device=dev)       # noqa: E731
    f32, i32, f64 = torch.float32, torch.int32, torch.float64
    return dict(severity=new(f32, S, e), worst_line=new(i32, S, e), overloads=new(i32, S, e), vm_min=new(f32, S, e), vm_min_bus=new(i32, S, e),
                v_violations=new(i32, S, e), mismatch=new(f64, S, e), base_table=new(f64, S, n, 4), status=new(i32, S), residual=new(f64, S),
                post_current=new(f32, S, e, e) if keep_table else None, post_state=new(f32, S, e, n, 2) if keep_state else None,
                flags=torch.zeros(1, dtype=i32, device=dev))


def _islands(edge_index, e, n, slack, out):
    """the launch every screen starts with: `out` [e] int32, what the outage of each line islands (on the current device and stream)"""
    L.check(L.load().pfn_contingency_islands(edge_index.data_ptr(), e, n, slack, out.data_ptr(), L.stream_ptr()), "pfn_contingency_islands")


def _plan_device(who, plan, dev):
    if plan.blob.device != dev:
        raise RuntimeError(f"{who}: the plan lives on {plan.blob.device}, the inputs on {dev}")


def contingency_screen(bus_type, spec, edge_index, rx, ratings=None, *, tol=1e-8, max_iter=10, route="auto", keep_table=False, plan=None,
                       block="auto", groups=None, threads=None) -> ContingencyResult:
    """Screen every single line outage of every scenario under the DC model: `bus_type` [n] (exactly one slack), `spec` [S, n, 4] and
    `rx` [S, e, 2] float64 as `solve_power_flow` takes them, ONE line list `edge_index` int64 [2, e].  `ratings`: float64 per-unit
    current, [e] or [S, e]; None: 1.0 everywhere; a rating that is not > 0 (zero, negative, NaN) leaves its line unmonitored.
    `route`: "auto", "lds" (raises where B'^-1 does not fit LDS) or "global" (forces the workspace slab).  `keep_table`: also return
    the full post-outage flow table [S, e, e].  Two launches; one host read (the bus_type counts, once per tensor); nothing is read
    back.

    `route="sparse"` with `plan=sparse_plan(bus_type, edge_index, mode="dc")`: the same screen beyond `max_unknowns()` -- the same
    fields, definitions and statuses, plus status -6 where the device line list is not the plan's.  Three launches (islands, base,
    outages).  "auto" never takes it; without a plan, with a plan of another mode or of another n / e it raises ValueError.  There
    `block`: where a tile's 64 right-hand sides sit -- "auto" (LDS where 256 n bytes fit, about 600 buses), "lds" (raises where they
    do not) or "global" (a block of the workspace per workgroup); the same bits.  `groups`: the number of one-wave workgroups the
    (scenario, tile) items are dealt to, None: min(S * tiles, 16 * compute units), each with a block of 256 n bytes
    on the global placement; no bit depends on it.  `threads`: the base solve's
    workgroup, None (64, or 256 where the plan's longest L column exceeds 128), 64 or 256."""
    who = "contingency_screen"
    if route == "sparse":
        return _screen_sparse(bus_type, spec, edge_index, rx, ratings, tol, max_iter, keep_table, plan, block, groups, threads)
    if route not in _ROUTES:
        raise ValueError(f"{who}: route must be one of {sorted(_ROUTES) + ['sparse']}")
    if plan is not None or block != "auto" or groups is not None or threads is not None:
        raise ValueError(f"{who}: plan, block, groups and threads go with route='sparse' only")
    S, n, e, (n_pv, n_pq, slack), bt, spec, edge_index, rx, ratings = _prepare(who, bus_type, spec, edge_index, rx, ratings)
    dev = spec.device
    lib = L.load()
    islands = torch.empty(e, dtype=torch.int32, device=dev)
    out = _outputs(S, e, e, dev, keep_table)
    need = int(lib.pfn_contingency_workspace_bytes(S, n, e, _ROUTES[route]))
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    with torch.cuda.device(dev):
        _islands(edge_index, e, n, slack, islands)
        L.check(lib.pfn_contingency_dc(edge_index.data_ptr(), e, rx.data_ptr(), bt.data_ptr(), spec.data_ptr(), L.ptr(ratings),
                                       int(ratings is not None and ratings.dim() == 2), islands.data_ptr(), S, n, n_pv, n_pq, float(tol),
                                       int(max_iter), _ROUTES[route], out["severity"].data_ptr(), out["worst_line"].data_ptr(),
                                       out["overloads"].data_ptr(), out["base_flow"].data_ptr(), out["status"].data_ptr(), L.ptr(out["post_flow"]),
                                       out["flags"].data_ptr(), L.ptr(ws), need, L.stream_ptr()),
                "pfn_contingency_dc")
    return ContingencyResult(islands=islands, route="global" if need else "lds", **out)


def _sparse_options(who, spec, edge_index, plan, block, groups, threads, mode="dc"):
    """what `route="sparse"` asks of its own options, on the host, before anything touches the library: every screen (`mode`: the
    plan it takes -- "dc" for the DC screens, "fd" for the AC one)"""
    if block not in _BLOCKS:
        raise ValueError(f"{who}: block must be one of {sorted(_BLOCKS)}")
    if groups is not None and (isinstance(groups, bool) or not isinstance(groups, int) or not 1 <= groups < 2 ** 31):
        raise ValueError(f"{who}: groups must be None or a positive int; got {groups!r}")
    if threads not in (None, 64, 256):
        raise ValueError(f"{who}: threads must be None, 64 or 256; got {threads!r}")
    if not isinstance(plan, SparsePlan):
        raise ValueError(f"{who}: route 'sparse' needs plan=sparse_plan(bus_type, edge_index, mode={mode!r}); got {plan!r}")
    if plan.mode != mode:
        raise ValueError(f"{who}: route 'sparse' takes a plan of mode {mode!r}; this one has mode {plan.mode!r}")
    if torch.is_tensor(spec) and spec.dim() == 3 and torch.is_tensor(edge_index) and edge_index.dim() == 2:
        if (plan.n, plan.e) != (int(spec.shape[1]), int(edge_index.shape[1])):
            raise ValueError(f"{who}: the plan is for (n, e) = {(plan.n, plan.e)}; the call has {(int(spec.shape[1]), int(edge_index.shape[1]))}")


def _screen_sparse(bus_type, spec, edge_index, rx, ratings, tol, max_iter, keep_table, plan, block, groups, threads) -> ContingencyResult:
    """`contingency_screen(route="sparse")`: islands, base, outages -- three launches, the one host read of `_bus_counts`."""
    who = "contingency_screen"
    _sparse_options(who, spec, edge_index, plan, block, groups, threads)
    S, n, e, (n_pv, n_pq, slack), bt, spec, edge_index, rx, ratings = _prepare(who, bus_type, spec, edge_index, rx, ratings, plan=plan)
    dev = spec.device
    lib = L.load()
    islands = torch.empty(e, dtype=torch.int32, device=dev)
    out = _outputs(S, e, e, dev, keep_table)
    header, g = C.addressof(plan.header), 0 if groups is None else groups
    with torch.cuda.device(dev):
        need = int(lib.pfn_contingency_sparse_workspace_bytes(S, e, header, _BLOCKS[block], g)) if S else 0
        in_lds = block != "global" and (not S or need == int(lib.pfn_contingency_sparse_workspace_bytes(S, e, header, 1, g)))
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        _islands(edge_index, e, n, slack, islands)
        L.check(lib.pfn_contingency_sparse(edge_index.data_ptr(), e, rx.data_ptr(), bt.data_ptr(), spec.data_ptr(), L.ptr(ratings),
                                           int(ratings is not None and ratings.dim() == 2), islands.data_ptr(), S, n, n_pv, n_pq, float(tol),
                                           int(max_iter), out["severity"].data_ptr(), out["worst_line"].data_ptr(), out["overloads"].data_ptr(),
                                           out["base_flow"].data_ptr(), out["status"].data_ptr(), L.ptr(out["post_flow"]), out["flags"].data_ptr(),
                                           ws.data_ptr(), need, header, plan.blob.data_ptr(), 0 if threads is None else threads, _BLOCKS[block], g,
                                           L.stream_ptr()),
                "pfn_contingency_sparse")
    return ContingencyResult(islands=islands, route="sparse", block="lds" if in_lds else "global", **out)


_LINES_KEPT = {}  # (device, candidate tuple) -> (int32 [c] lines, int64 [P, 2] pairs) on the device: a capture after its eager call uploads nothing


def _device_lines(lines, dev):
    key = (str(dev), tuple(lines))
    got = _LINES_KEPT.get(key)
    if got is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("contingency_screen_pairs: the candidate lines are uploaded once per list; call it eagerly once before capturing")
        if len(_LINES_KEPT) >= 16:
            _LINES_KEPT.pop(next(iter(_LINES_KEPT)))
        got = (torch.tensor(lines, dtype=torch.int32).to(dev), pair_lines(lines).to(dev))
        _LINES_KEPT[key] = got
    return got


def contingency_screen_pairs(bus_type, spec, edge_index, rx, ratings=None, *, lines=None, tol=1e-8, max_iter=10, route="auto",
                             keep_table=False, plan=None, block="auto", groups=None, threads=None, columns="auto",
                             waves=None) -> PairContingencyResult:
    """Screen every PAIR of line outages among the candidate `lines` of every scenario under the DC model (N-2): inputs and their
    checks are `contingency_screen`'s.  `lines`: a host sequence or a CPU int64 tensor of line ids, strictly increasing and within
    [0, e), at least two (checked on the host, no device read; ValueError otherwise); None: all lines.  All e lines stay monitored
    whatever the candidates are -- N-1 first, then the pairs among its top outages, is how larger grids are screened.  With c
    candidates there are P = c (c - 1) / 2 pairs in `pair_lines`' order.  `route`: "auto", "lds" (raises where B'^-1 does not fit
    LDS beside the pair launch's vectors) or "global" (the pair launch reads the workspace slab); the same bits.  These are the dense
    routes: beyond `max_unknowns()` they raise.  Three launches; one host read (the bus_type counts, once per tensor); nothing is
    read back.

    `route="sparse"` with `plan=sparse_plan(bus_type, edge_index, mode="dc")`: the same screen beyond `max_unknowns()` from the
    sparse factor of `contingency_screen(route="sparse")` -- the same fields, pair order, definitions and statuses, plus status -6
    where the device line list is not the plan's; `base_flow` and `status` carry that screen's bits.  Four launches (pair islands,
    base, columns, pairs).  "auto" never takes it.  `block`, `groups`, `threads`: as in `contingency_screen`, for the launch that
    substitutes one column per candidate, 64 candidates to a workgroup.  `columns`: where the pair launch keeps the two columns of
    a pair -- "auto" (LDS where 4 n (1 + waves) bytes fit), "lds" (raises where they do not) or "global" (gathered from the
    workspace); `waves`: the pair launch's waves per (scenario, first candidate), None (4), 1, 2, 4, 8 or 16.  No bit depends on
    any of them."""
    who = "contingency_screen_pairs"
    if route == "sparse":
        _sparse_options(who, spec, edge_index, plan, block, groups, threads)
        if columns not in _COLUMNS:
            raise ValueError(f"{who}: columns must be one of {sorted(_COLUMNS)}")
        if isinstance(waves, bool) or waves not in (None, 1, 2, 4, 8, 16):
            raise ValueError(f"{who}: waves must be None, 1, 2, 4, 8 or 16; got {waves!r}")
    elif route not in _ROUTES:
        raise ValueError(f"{who}: route must be one of {sorted(_ROUTES) + ['sparse']}")
    elif plan is not None or block != "auto" or groups is not None or threads is not None or columns != "auto" or waves is not None:
        raise ValueError(f"{who}: plan, block, groups, threads, columns and waves go with route='sparse' only")
    e_given = int(edge_index.shape[1]) if torch.is_tensor(edge_index) and edge_index.dim() == 2 else None
    if lines is not None:                                                     # on the host, before anything touches the library
        lines = _candidates(lines, who)
        if isinstance(lines, list) and len(lines) < 2:
            raise ValueError(f"{who}: a pair needs at least two candidate lines; got {len(lines)}")
        if any(b <= a for a, b in zip(lines, lines[1:])):
            raise ValueError(f"{who}: lines must be strictly increasing (sorted, no duplicates)")
        if lines[0] < 0 or (e_given is not None and lines[-1] >= e_given):
            raise ValueError(f"{who}: lines must lie within [0, {e_given}); got {lines[0]} .. {lines[-1]}")
    def pairs_fit(n, e):
        if e < 2:
            raise ValueError(f"{who}: a grid of {e} line has no pair to screen")
        cap = int(L.load().pfn_powerflow_max_unknowns())
        if route != "sparse" and n - 1 > cap:
            raise ValueError(f"{who}: {n - 1} unknowns per scenario exceed the dense screen's {cap} (max_unknowns()); beyond it: "
                             f"route='sparse' with plan=sparse_plan(bus_type, edge_index, mode='dc')")
    S, n, e, (n_pv, n_pq, slack), bt, spec, edge_index, rx, ratings = _prepare(who, bus_type, spec, edge_index, rx, ratings,
                                                                                plan=plan if route == "sparse" else None, after_check=pairs_fit)
    dev, lib = spec.device, L.load()
    if lines is None:                                                         # all lines: built on the device, nothing uploaded
        c = e
        ij = torch.triu_indices(c, c, 1, device=dev)
        lines_d, pairs = torch.arange(c, dtype=torch.int32, device=dev), ij.t().contiguous()
    else:
        c = len(lines)
        lines_d, pairs = _device_lines(lines, dev)
    P = c * (c - 1) // 2
    islands = torch.empty(P, dtype=torch.int32, device=dev)
    out = dict(islands=islands, pairs=pairs, **_outputs(S, e, P, dev, keep_table))
    figures = [out[k].data_ptr() for k in ("severity", "worst_line", "overloads", "base_flow", "status")]
    figures += [L.ptr(out["post_flow"]), out["flags"].data_ptr()]              # (in the C entries' order)
    per_sample = int(ratings is not None and ratings.dim() == 2)
    with torch.cuda.device(dev):
        L.check(lib.pfn_contingency_pair_islands(edge_index.data_ptr(), e, n, slack, lines_d.data_ptr(), c, islands.data_ptr(), L.stream_ptr()),
                "pfn_contingency_pair_islands")
        if route == "sparse":
            header, g, w = C.addressof(plan.header), 0 if groups is None else groups, 0 if waves is None else waves
            size = lib.pfn_contingency_pairs_sparse_workspace_bytes
            need = int(size(S, e, c, header, _BLOCKS[block], g, _COLUMNS[columns], w)) if S else 0
            # what "auto" took, by what the forced placements would be given: 0 where the call refuses them
            block_lds = block != "global" and int(size(1, e, c, header, 1, g, 2, w)) != 0
            columns_lds = columns != "global" and int(size(1, e, c, header, 2, g, 1, w)) != 0
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            L.check(lib.pfn_contingency_pairs_sparse(edge_index.data_ptr(), e, rx.data_ptr(), bt.data_ptr(), spec.data_ptr(), L.ptr(ratings), per_sample,
                                                     lines_d.data_ptr(), c, islands.data_ptr(), S, n, n_pv, n_pq, float(tol), int(max_iter),
                                                     *figures, ws.data_ptr(), need, header, plan.blob.data_ptr(), 0 if threads is None else threads,
                                                     _BLOCKS[block], g, _COLUMNS[columns], w, L.stream_ptr()),
                    "pfn_contingency_pairs_sparse")
            return PairContingencyResult(route="sparse", block="lds" if block_lds else "global", columns="lds" if columns_lds else "global", **out)
        need = int(lib.pfn_contingency_pairs_workspace_bytes(S, n, e, c, 2)) if S else 0
        in_lds = route != "global" and int(lib.pfn_contingency_pairs_workspace_bytes(1, n, e, c, 1)) != 0
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        L.check(lib.pfn_contingency_pairs(edge_index.data_ptr(), e, rx.data_ptr(), bt.data_ptr(), spec.data_ptr(), L.ptr(ratings), per_sample,
                                          lines_d.data_ptr(), c, islands.data_ptr(), S, n, n_pv, n_pq, float(tol), int(max_iter), _ROUTES[route],
                                          *figures, ws.data_ptr(), need, L.stream_ptr()),
                "pfn_contingency_pairs")
    return PairContingencyResult(route="lds" if in_lds else "global", **out)


def summarise_loadings(loading, monitored):
    """(severity float32 [T], worst_line int32 [T], overloads int32 [T]) of loadings [T, e] over the `monitored` lines by the
    screen's rules: the maximum with ties to the lowest line, a non-finite loading counts as the largest and makes the severity NaN,
    no monitored line gives (0, -1, 0)."""
    e = loading.shape[1]
    ar = torch.arange(e, device=loading.device)
    wild = monitored & ~torch.isfinite(loading)
    key = torch.where(monitored, torch.where(wild, torch.full_like(loading, float("inf")), loading), torch.full_like(loading, -1.0))
    best = key.max(dim=1).values
    worst = torch.where(key == best[:, None], ar, e).min(dim=1).values
    none = ~monitored.any(dim=1)
    severity = torch.where(none, torch.zeros_like(best), torch.where(wild.any(dim=1), torch.full_like(best, float("nan")), best))
    return severity, torch.where(none, -1, worst).to(torch.int32), (monitored & (loading > 1)).sum(dim=1).to(torch.int32)


def _verify_removed(bus_type, spec, edge_index, rx, ratings, S, e, chosen, removed, solver_kw):
    """The AC re-solve both verifications share: row t is scenario chosen[t] with the K = `removed.shape[1]` (1 or 2) lines
    removed[t] (ascending) left out.  The reduced lists and their rx are built on the device, `solve_power_flow(mode="ac")` solves
    them, `loss.branch_flows` gives the line currents and the loadings go back to the original numbering (NaN at the removed lines).
    Returns (solved, loading [T, e] float32, severity, worst_line, overloads)."""
    from ..loss import branch_flows
    dev = spec.device
    T, K = int(removed.shape[0]), int(removed.shape[1])
    ar = torch.arange(e - K, device=dev)
    idx = ar[None, :].expand(T, e - K)
    for k in range(K):                                                         # the lines that stay, in stored order
        idx = idx + (idx >= removed[:, k:k + 1])
    lists = edge_index[:, idx].permute(1, 0, 2).contiguous()                   # [T, 2, e - K]
    rx_post = rx[chosen[:, None], idx].contiguous()                            # [T, e - K, 2]
    if solver_kw.get("route") == "sparse" and solver_kw.get("plan") is None and T:
        # every reduced list is a subset of the base list: ONE cover plan whose cover IS the base list serves all rows
        solver_kw = {**solver_kw, "plan": cover_plan(bus_type, edge_index[None], mode="ac", base=edge_index)}
    solved = solve_power_flow(bus_type, spec[chosen].contiguous(), lists, rx_post, mode="ac", **solver_kw)
    rate = torch.ones(S, e, dtype=torch.float32, device=dev) if ratings is None else ratings.float().expand(S, e)
    rate = rate[chosen]                                                        # [T, e]
    loading = torch.full((T, e), float("nan"), dtype=torch.float32, device=dev)
    if T and e > K:
        flows = branch_flows(solved.table.float(), lists, rx_post.float())[0]  # [T, e - K, 4]: column 0 is the current
        loading.scatter_(1, idx, flows[:, :, 0] / rate.gather(1, idx))
    monitored = (rate > 0) & (torch.arange(e, device=dev)[None, :, None] != removed[:, None, :]).all(dim=2)
    return (solved, loading) + tuple(summarise_loadings(loading, monitored))


def verify_contingencies(result, bus_type, spec, edge_index, rx, ratings=None, *, top=5, pairs=None, **solver_kw) -> ContingencyVerification:
    """AC check of chosen outages of a `contingency_screen` result (same inputs): for every pair (scenario s, outage k) -- `pairs`
    [T, 2], or per scenario the `top` outages of `result.ranking` -- that does not island a bus, the line list without line k and its
    rx are built on the device, `solve_power_flow(mode="ac", **solver_kw)` solves them, `loss.branch_flows` gives the line currents,
    and the loadings I_l / rating_l go back to the original line numbering.  The pairs are chosen on the host (T is small).
    `route="sparse"` without `plan=`: ONE `cover_plan` whose cover is the base list is built here (every reduced list is a subset of
    it); a `plan=` that is given is reused."""
    who = "verify_contingencies"
    S, n, e = _check(bus_type, spec, edge_index, rx, who)
    ratings = _ratings(ratings, S, e, who)
    dev = spec.device
    islands = result.islands.cpu()
    if pairs is None:
        if isinstance(top, bool) or not isinstance(top, int) or top < 0:
            raise ValueError(f"{who}: top must be an int >= 0; got {top!r}")
        order = result.ranking(e)[0].cpu()
        chosen = [(s, k) for s in range(S) for k in [k for k in order[s].tolist() if int(islands[k]) == 0][:top]]
    else:
        chosen = [(int(s), int(k)) for s, k in (pairs.tolist() if torch.is_tensor(pairs) else pairs)]
        for s, k in chosen:
            if not (0 <= s < S and 0 <= k < e):
                raise ValueError(f"{who}: pair ({s}, {k}) is outside ({S} scenarios, {e} lines)")
        chosen = [(s, k) for s, k in chosen if int(islands[k]) == 0]
    pairs_t = torch.tensor(chosen, dtype=torch.int64, device=dev).reshape(-1, 2)
    sc, out = pairs_t[:, 0], pairs_t[:, 1]
    solved, loading, severity, worst, overloads = _verify_removed(bus_type, spec, edge_index, rx, ratings, S, e, sc, out[:, None], solver_kw)
    return ContingencyVerification(pairs=pairs_t, table=solved.table, status=solved.status, loading=loading, severity=severity,
                                   worst_line=worst, overloads=overloads, dc_severity=result.severity[sc, out])


@dataclass
class PairContingencyVerification:
    """`triples` [T, 3] int64 (scenario, line a, line b; a < b), `pair_index` [T] int64 (the pair's column in the screen's result),
    the AC `table` [T, n, 4] float64 and `status` [T] int32 of `solve_power_flow` on the grid without both lines, `loading` [T, e]
    float32 = I_l / rating_l in the ORIGINAL line numbering (NaN at both outaged lines), `severity` / `worst_line` / `overloads` by
    the screen's rules, and `dc_severity` [T] float32, the screen's figure for the pair."""
    triples: torch.Tensor
    pair_index: torch.Tensor
    table: torch.Tensor
    status: torch.Tensor
    loading: torch.Tensor
    severity: torch.Tensor
    worst_line: torch.Tensor
    overloads: torch.Tensor
    dc_severity: torch.Tensor


def verify_pair_contingencies(result, bus_type, spec, edge_index, rx, ratings=None, *, top=5, triples=None,
                              **solver_kw) -> PairContingencyVerification:
    """`verify_contingencies` with two lines removed: AC check of chosen pairs of a `contingency_screen_pairs` result (same inputs).
    `triples` [T, 3] (scenario, line a, line b) name pairs the screen holds (ValueError otherwise), or per scenario the `top` pairs
    of `result.ranking`; pairs that island buses are skipped.  The rows are chosen on the host (T is small)."""
    who = "verify_pair_contingencies"
    S, n, e = _check(bus_type, spec, edge_index, rx, who)
    ratings = _ratings(ratings, S, e, who)
    dev = spec.device
    islands, held = result.islands.cpu().tolist(), result.pairs.cpu().tolist()
    P = len(held)
    if triples is None:
        if isinstance(top, bool) or not isinstance(top, int) or top < 0:
            raise ValueError(f"{who}: top must be an int >= 0; got {top!r}")
        order = result.ranking(P)[0].cpu()
        chosen = [(s, p) for s in range(S) for p in [p for p in order[s].tolist() if islands[p] == 0][:top]]
    else:
        where = {(a, b): p for p, (a, b) in enumerate(held)}
        chosen = []
        for s, a, b in ([tuple(int(v) for v in row) for row in (triples.tolist() if torch.is_tensor(triples) else triples)]):
            a, b = min(a, b), max(a, b)
            if not 0 <= s < S or (a, b) not in where:
                raise ValueError(f"{who}: ({s}, {a}, {b}) is no (scenario, pair) of this screen ({S} scenarios, {P} pairs)")
            chosen.append((s, where[(a, b)]))
        chosen = [(s, p) for s, p in chosen if islands[p] == 0]
    rows = torch.tensor(chosen, dtype=torch.int64, device=dev).reshape(-1, 2)
    sc, pi = rows[:, 0], rows[:, 1]
    removed = result.pairs[pi]                                                 # [T, 2], ascending
    solved, loading, severity, worst, overloads = _verify_removed(bus_type, spec, edge_index, rx, ratings, S, e, sc, removed, solver_kw)
    return PairContingencyVerification(triples=torch.cat([sc[:, None], removed], dim=1), pair_index=pi, table=solved.table, status=solved.status,
                                       loading=loading, severity=severity, worst_line=worst, overloads=overloads,
                                       dc_severity=result.severity[sc, pi])


# ================================================================================ N-1 with the network's prediction
MODEL_CHUNK = 744   # items per chunk where the caller names none: the fastest of tools/contingency_bench.py --model at case118, S = 16
_STEPS_ATTR = "_pfn_contingency_model_steps"  # on the model: {shape key: _ModelScreenStep} of the graphed calls
_MAX_STEPS = 8                                # (GraphedEvalStep.max_children: beyond it the oldest shape is dropped and captured again)


@dataclass
class ModelContingencyResult:
    """`contingency_screen_model`'s answer.  Per (scenario s, outage k), by `ContingencyResult`'s rules but from the NETWORK's
    prediction: `severity` [S, e] float32 (the largest loading I_l / rating_l over the monitored lines l != k, I_l the line current of
    the merged prediction; +inf where the outage islands buses, NaN where a monitored loading is not finite), `worst_line` [S, e]
    int32 (ties to the lowest; -1 where none), `overloads` [S, e] int32 (-1 where islanding).  `islands` [e] int32 as in
    `ContingencyResult`.  `loading` [S, e, e] float32 with `keep_table` (row = outage, column = line in the ORIGINAL numbering; NaN at
    the outaged line and in an islanding row), `predictions` [S, e, n, 4] float32 with `keep_predictions` (the merged, de-normalised
    table: the network's value where the bus type leaves the entry to be predicted, float(spec) where it is given; written for
    islanding outages too, where it means nothing); else None.  `flags` [1] int32 (bit 1: a line names a bus outside the grid).
    `chunk`: the items per chunk that ran; `captures`: graph captures the serving step has made so far (0: eager).

    `verify_contingencies(result, ...)` takes it as it takes a `ContingencyResult` (it reads `islands`, `ranking` and `severity`);
    the `dc_severity` column of its answer then carries THIS screen's figure, the network's, not a DC one."""
    severity: torch.Tensor
    worst_line: torch.Tensor
    overloads: torch.Tensor
    islands: torch.Tensor
    loading: object = None
    predictions: object = None
    flags: object = None
    chunk: int = 0
    captures: int = 0

    def ranking(self, top):
        """`ContingencyResult.ranking`'s order: NaN first, then +inf, then descending, ties to the lowest outage id."""
        return _rank(self.severity, top, "ranking")


def _stat_floats(v, count, what):
    """a statistic of the dataset (a tensor or a sequence, any shape that holds `count` values first) as fp32 host floats, or None"""
    if v is None:
        return None
    t = torch.as_tensor(v, dtype=torch.float32).detach().cpu().reshape(-1)
    if t.numel() < count or t.numel() % count:
        raise ValueError(f"contingency_screen_model: {what} must hold {count} values; got {t.numel()}")
    return t[:count]


def _model_stats(xymean, xystd, edgemean, edgestd):
    """(div4, mean4, ediv2, emean2) as tuples of host floats or None (identity): the divisor std + 1e-7 formed in fp32, as the
    dataset forms it and as `denormalize` multiplies by it"""
    def div(v, count, what):
        t = _stat_floats(v, count, what)
        return None if t is None else tuple(float(a) for a in (t + 1e-7).tolist())

    def mean(v, count, what):
        t = _stat_floats(v, count, what)
        return None if t is None else tuple(float(a) for a in t.tolist())
    return div(xystd, 4, "xystd"), mean(xymean, 4, "xymean"), div(edgestd, 2, "edgestd"), mean(edgemean, 2, "edgemean")


def _c_floats(v):
    return None if v is None else (C.c_float * len(v))(*v)


@contextlib.contextmanager
def _screen_state(model):
    """The state the screen's forwards run in, for the call's duration only: every module in eval mode, no_grad, and -- on a model
    that keeps an adjacency per edge_index (MaskEmbdMultiMPN) -- `dynamic_topology` and `segment_build` on: every chunk has its own
    line lists, rebuilt on the device without a host sync, one workgroup per graph.  Whatever was there before comes back, also when
    the call raises.  Yields the adjacency owners."""
    modes = [(m, m.training) for m in model.modules()]
    owners = topology_owners(model)
    try:
        model.eval()
        with torch.no_grad(), capture_state(owners, model, True, hasattr(model, "segment_build")):
            yield owners
    finally:
        for m, was in modes:
            m.training = was


class _ModelScreenStep:
    """The chunk loop of one screen shape: the batch a chunk's launch fills, the three steps of a chunk, their capture and replay.
    Eager, the kernels read the caller's tensors and each chunk names its first item by a pointer into `starts`; graphed, the step
    owns copies of the inputs (the captured launches hold their addresses) and the host copies the chunk's first item into the ONE
    device word `item0` the captured kernels read, then replays.  A captured chunk is a chain: no parallel branches."""

    def __init__(self, model, S, n, e, B, dev, stats, per_sample, has_ratings, keep_table, keep_predictions, own_inputs):
        from ..data import Batch
        self.model, self.S, self.n, self.e, self.B, self.dev = model, S, n, e, B, dev
        self.stats = stats
        self.c_stats = tuple(_c_floats(v) for v in stats)
        self.per_sample = per_sample
        T = S * e
        self.starts = torch.arange(0, T, B, dtype=torch.int64, device=dev)
        self.item0 = torch.zeros(1, dtype=torch.int64, device=dev)
        batch = Batch()
        batch.x = torch.empty(B * n, 4, dtype=torch.float32, device=dev)
        batch.pred_mask = torch.empty(B * n, 4, dtype=torch.float32, device=dev)
        batch.bus_type = torch.empty(B * n, dtype=torch.int64, device=dev)
        batch.edge_index = torch.empty(2, B * (e - 1), dtype=torch.int64, device=dev)
        batch.edge_attr = torch.empty(B * (e - 1), 2, dtype=torch.float32, device=dev)
        batch.batch = torch.arange(B, device=dev).repeat_interleave(n)      # constants of the chunk shape
        batch.ptr = torch.arange(B + 1, device=dev) * n
        self.batch = batch
        self.islands = torch.empty(e, dtype=torch.int32, device=dev)
        self.severity = torch.empty(S, e, dtype=torch.float32, device=dev)
        self.worst = torch.empty(S, e, dtype=torch.int32, device=dev)
        self.overloads = torch.empty(S, e, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(1, dtype=torch.int32, device=dev)
        self.loading = torch.empty(S, e, e, dtype=torch.float32, device=dev) if keep_table else None
        self.predictions = torch.empty(S, e, n, 4, dtype=torch.float32, device=dev) if keep_predictions else None
        self.bt = self.spec = self.ei = self.rx = self.ratings = None
        self.own = own_inputs
        if own_inputs:
            self.bt = torch.empty(n, dtype=torch.int32, device=dev)
            self.spec = torch.empty(S, n, 4, dtype=torch.float64, device=dev)
            self.ei = torch.empty(2, e, dtype=torch.int64, device=dev)
            self.rx = torch.empty(S, e, 2, dtype=torch.float64, device=dev)
            self.ratings = torch.empty((S, e) if per_sample else (e,), dtype=torch.float64, device=dev) if has_ratings else None
        self.graph, self.held, self.side, self.captures = None, None, None, 0

    def bind(self, bt, spec, ei, rx, ratings, slack):
        """the inputs of this call (eager: taken as they are; graphed: copied into the step's own) and their islands verdict"""
        if self.own:
            self.bt.copy_(bt)
            self.spec.copy_(spec)
            self.ei.copy_(ei)
            self.rx.copy_(rx)
            if ratings is not None:
                self.ratings.copy_(ratings)
        else:
            self.bt, self.spec, self.ei, self.rx, self.ratings = bt, spec, ei, rx, ratings
        self.flags.zero_()
        _islands(self.ei, self.e, self.n, slack, self.islands)

    def chunk(self, item0):
        """the three steps of the chunk whose first item the device word `item0` holds"""
        lib, b, (div4, mean4, ediv2, emean2) = L.load(), self.batch, self.c_stats
        L.check(lib.pfn_contingency_model_batch(self.bt.data_ptr(), self.spec.data_ptr(), self.ei.data_ptr(), self.rx.data_ptr(), self.S, self.n,
                                                self.e, item0.data_ptr(), self.B, div4, mean4, ediv2, emean2, b.x.data_ptr(),
                                                b.pred_mask.data_ptr(), b.bus_type.data_ptr(), b.edge_index.data_ptr(), b.edge_attr.data_ptr(),
                                                self.flags.data_ptr(), L.stream_ptr()), "pfn_contingency_model_batch")
        out = self.model(b)
        if not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (self.B * self.n, 4) or out.device != self.dev:
            raise RuntimeError(f"contingency_screen_model: the model must return float32 ({self.B * self.n}, 4) on {self.dev}; got "
                               f"{getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))}")
        out = out.detach()
        out = out if out.is_contiguous() and out.data_ptr() % 16 == 0 else out.clone(memory_format=torch.contiguous_format)
        L.check(lib.pfn_contingency_model_loadings(out.data_ptr(), self.bt.data_ptr(), self.spec.data_ptr(), self.ei.data_ptr(), self.rx.data_ptr(),
                                                   L.ptr(self.ratings), int(self.per_sample), self.islands.data_ptr(), self.S, self.n, self.e,
                                                   item0.data_ptr(), self.B, div4, mean4, 0, self.severity.data_ptr(), self.worst.data_ptr(),
                                                   self.overloads.data_ptr(), L.ptr(self.loading), L.ptr(self.predictions), L.stream_ptr()),
                "pfn_contingency_model_loadings")

    def run_eager(self):
        for c in range(int(self.starts.numel())):
            self.chunk(self.starts[c:c + 1])

    def run_graphed(self, owners):
        if self.graph is None:
            if self.side is None:
                self.side = torch.cuda.Stream()
            warm_up(self.side, lambda: self.chunk(self.item0))              # (item0 holds 0: chunk 0, which the loop below runs again)
            g = torch.cuda.CUDAGraph()
            with no_gc(), torch.cuda.graph(g):
                self.chunk(self.item0)
            self.graph, self.held = g, held_adjacencies(owners)
            self.captures += 1
        for c in range(int(self.starts.numel())):
            self.item0.copy_(self.starts[c:c + 1])
            self.graph.replay()


def _screen_model_options(model, edge_index, chunk, keep_table, keep_predictions, graphed):
    """what `contingency_screen_model` asks of its own arguments, on the host, before anything touches the library"""
    who = "contingency_screen_model"
    if not isinstance(model, nn.Module):
        raise ValueError(f"{who}: model must be a torch.nn.Module whose forward(batch) returns [N, 4] float32; got {type(model).__name__}")
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, int) or not 1 <= chunk < 2 ** 24):
        raise ValueError(f"{who}: chunk must be None or an int in [1, 2^24); got {chunk!r}")
    for name, v in (("keep_table", keep_table), ("keep_predictions", keep_predictions), ("graphed", graphed)):
        if not isinstance(v, bool):
            raise ValueError(f"{who}: {name} must be a bool; got {v!r}")
    if torch.is_tensor(edge_index) and edge_index.dim() == 2 and edge_index.shape[1] == 1:
        raise ValueError(f"{who}: a grid of one line leaves no line once it is out: nothing to screen")


def contingency_screen_model(model, bus_type, spec, edge_index, rx, ratings=None, *, xymean=None, xystd=None, edgemean=None, edgestd=None,
                             chunk=None, keep_table=False, keep_predictions=False, graphed=False) -> ModelContingencyResult:
    """Screen every single line outage of every scenario with the NETWORK's prediction: `bus_type`, `spec`, `edge_index`, `rx` and
    `ratings` exactly as `contingency_screen` takes them (e >= 2: ValueError otherwise).  `model`: an `nn.Module` on the inputs'
    device whose `forward(batch)` returns [N, 4] float32 for a `data.Batch` carrying x, pred_mask, bus_type, edge_index, edge_attr,
    batch, ptr; it runs in eval mode under no_grad, a `MaskEmbdMultiMPN` with `dynamic_topology` and `segment_build` on, and gets
    all of it back afterwards.  `xymean` / `xystd` / `edgemean` / `edgestd`: the training set's statistics (None: identity); the
    divisor is std + 1e-7 formed in fp32, the dataset's.

    Item t = s * e + k is scenario s without line k; ALL S * e items run, the islanding ones too (static shapes, nothing read back),
    `chunk` consecutive items at a time (None: `MODEL_CHUNK`; never more than S * e), the last chunk padded with repeats of the last
    item whose results are not written.  Per chunk: `pfn_contingency_model_batch` writes the batch the dataset and its collate
    would have built, the model predicts, `pfn_contingency_model_loadings` merges prediction and specification, forms the line
    currents with `branch_flows`' arithmetic and reduces by the screen's rules; `pfn_contingency_islands` runs first and its verdict
    overwrites the islanding items (+inf, -1, -1, a NaN row).  `graphed`: the three steps of a chunk are captured once per shape
    (kept on the model, reused by later calls: `captures` on the result counts them) and replayed for every chunk, the chunk's first
    item written into one device word before each replay; the first call with a new `bus_type` tensor must be eager.  One host read
    (the bus_type counts, once per tensor)."""
    who = "contingency_screen_model"
    _screen_model_options(model, edge_index, chunk, keep_table, keep_predictions, graphed)
    stats = _model_stats(xymean, xystd, edgemean, edgestd)
    S, n, e = _check(bus_type, spec, edge_index, rx, who)
    if e < 2:
        raise ValueError(f"{who}: a grid of one line leaves no line once it is out: nothing to screen")
    ratings = _ratings(ratings, S, e, who)
    if graphed:
        kept = getattr(bus_type, _COUNTS_ATTR, None)
        if kept is None or kept[0] != bus_type._version:
            raise RuntimeError(_COUNTS_EAGER_FIRST)
    _, _, slack = _bus_counts(bus_type)
    dev = spec.device
    bt = bus_type.to(torch.int32).contiguous()
    spec, rx, edge_index = spec.contiguous(), rx.contiguous(), edge_index.contiguous()
    T = S * e
    B = max(1, min(MODEL_CHUNK if chunk is None else chunk, T))
    per_sample = ratings is not None and ratings.dim() == 2
    shape = (S, n, e, B, dev, stats, per_sample, ratings is not None, keep_table, keep_predictions)
    with torch.cuda.device(dev), _screen_state(model) as owners:
        if not graphed or S == 0:
            step = _ModelScreenStep(model, *shape, own_inputs=False)
            step.bind(bt, spec, edge_index, rx, ratings, slack)
            step.run_eager()
        else:
            key = shape + (tuple(p.data_ptr() for p in model.parameters()),)   # (a parameter whose storage moved: capture again)
            steps = model.__dict__.setdefault(_STEPS_ATTR, {})
            step = steps.get(key)
            if step is None:
                if len(steps) >= _MAX_STEPS:
                    steps.pop(next(iter(steps)))
                step = steps[key] = _ModelScreenStep(model, *shape, own_inputs=True)
            step.bind(bt, spec, edge_index, rx, ratings, slack)
            try:
                step.run_graphed(owners)
            except BaseException:
                steps.pop(key, None)                                          # a failed capture leaves nothing half-made behind
                raise
    take = (lambda t: None if t is None else t.clone()) if graphed else (lambda t: t)   # (a graphed step's outputs are overwritten by its next call)
    return ModelContingencyResult(severity=take(step.severity), worst_line=take(step.worst), overloads=take(step.overloads),
                                  islands=take(step.islands), loading=take(step.loading), predictions=take(step.predictions),
                                  flags=take(step.flags), chunk=B, captures=step.captures)


# ================================================================================ N-1 under AC: compensated 1P1Q
_VARIANTS = {"xb": 0, "bx": 1}


@dataclass
class ACContingencyResult:
    """`contingency_screen_ac`'s answer.  Per (scenario s, outage k), by `ContingencyResult`'s rules but from `halves` fast-decoupled
    half-iterations under AC: `severity` [S, e] float32 (the largest loading I_l / rating_l over the monitored lines l != k; +inf
    where the outage islands buses, NaN where the scenario failed or a loading is not finite), `worst_line`, `overloads` [S, e]
    int32; `vm_min` [S, e] float32, `vm_min_bus` [S, e] int32 (the lowest Vm over the PQ buses and its bus, ties to the lowest; NaN /
    -1 without a PQ bus) and `v_violations` [S, e] int32 (PQ buses outside `v_limits`; a non-finite Vm counts and makes `vm_min`
    NaN); `mismatch` [S, e] float64, max |F| of the reduced grid at the final state.  Islanding outages: +inf, -1, -1, NaN voltage
    figures and mismatch, -1 integers; failed scenarios: NaN and -1 throughout.  `islands` [e] int32 as in `ContingencyResult`.  Per
    scenario: `base_table` [S, n, 4] float64, `status` [S] int32 and `residual` [S] float64 -- the bits of
    `solve_power_flow(mode="fd" + variant)`.  `post_current` [S, e, e] float32 (row = outage, column = line, NaN at l = k) with
    `keep_table`, `post_state` [S, e, n, 2] float32 = (Vm, Va in degrees) with `keep_state`, else None.  `flags` [1] int32 (bit 0:
    `bus_type` changed under the launch).  `route`: "lds" or "global", where the outage launch read the two inverses; `group`: its
    waves per workgroup.  `route` "sparse": the screen ran on the sparse factors; `block` then says where the outage blocks sat
    ("lds" or "global") and `group` is 0.  All on the device, nothing read back."""
    severity: torch.Tensor
    worst_line: torch.Tensor
    overloads: torch.Tensor
    vm_min: torch.Tensor
    vm_min_bus: torch.Tensor
    v_violations: torch.Tensor
    mismatch: torch.Tensor
    islands: torch.Tensor
    base_table: torch.Tensor
    status: torch.Tensor
    residual: torch.Tensor
    post_current: object
    post_state: object
    route: str
    flags: object = None
    group: int = 0
    block: object = None

    def ranking(self, top):
        """`ContingencyResult.ranking`'s order: NaN first, then +inf, then descending, ties to the lowest outage id."""
        return _rank(self.severity, top, "ranking")


def _screen_ac_options(variant, halves, v_limits, route, group, keep_table, keep_state):
    """what `contingency_screen_ac` asks of its own arguments, on the host, before anything touches the library"""
    who = "contingency_screen_ac"
    if variant not in _VARIANTS:
        raise ValueError(f"{who}: variant must be one of {sorted(_VARIANTS)}; got {variant!r}")
    if isinstance(halves, bool) or not isinstance(halves, int) or not 0 <= halves < 2 ** 31:
        raise ValueError(f"{who}: halves must be an int >= 0; got {halves!r}")
    try:
        lo, hi = (float(v) for v in v_limits)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: v_limits must be a pair of floats (low, high); got {v_limits!r}") from None
    if not lo <= hi:
        raise ValueError(f"{who}: v_limits must be in order, low <= high; got {v_limits!r}")
    if route != "sparse" and route not in _ROUTES:
        raise ValueError(f"{who}: route must be one of {sorted(_ROUTES) + ['sparse']}")
    if group is not None and (isinstance(group, bool) or not isinstance(group, int) or not 1 <= group <= 16):
        raise ValueError(f"{who}: group must be None or the waves per workgroup, an int in [1, 16]; got {group!r}")
    for name, v in (("keep_table", keep_table), ("keep_state", keep_state)):
        if not isinstance(v, bool):
            raise ValueError(f"{who}: {name} must be a bool; got {v!r}")
    return lo, hi


def contingency_screen_ac(bus_type, spec, edge_index, rx, ratings=None, *, variant="xb", halves=2, v_limits=(0.9, 1.1), tol=1e-8, max_iter=60,
                          init=None, route="auto", group=None, keep_table=False, keep_state=False, plan=None, block="auto", groups=None,
                          threads=None) -> ACContingencyResult:
    """Screen every single line outage of every scenario under AC by compensated 1P1Q: inputs and their checks are
    `contingency_screen`'s.  The base is the fast-decoupled solve of the full grid (`variant` "xb" or "bx", from the flat start or
    `init` [S, n, 2] = (Vm, Va in degrees), to `tol` within `max_iter` half-iterations) -- `solve_power_flow(mode="fd" + variant)`'s
    code and bits.  Every non-islanding outage then takes `halves` half-iterations (P first, alternating) from the base state with
    B'^-1 and B''^-1 corrected for the missing line by a rank-1 update; 2 is the classical 1P1Q, 4 buys about two more digits,
    0 gives the base state's figures with line k unmonitored.  `mismatch` says how far from converged each estimate is.
    `v_limits`: the band of `v_violations`.  `route`: "auto", "lds" (raises where the two inverses do not fit LDS beside the waves'
    vectors) or "global" (read from the workspace); `group`: the outages, one wave each, per workgroup, None: chosen with the
    placement; the same bits whatever the two are.  These are the dense routes: beyond `max_unknowns()` they raise.
    Three launches (islands, base, outages); one host read (the bus_type counts, once per tensor); nothing is read back.  The result
    goes into `verify_contingencies` as a `ContingencyResult` does.

    `route="sparse"` with `plan=sparse_plan(bus_type, edge_index, mode="fd")`: the same screen beyond `max_unknowns()` from the sparse
    fp32 FACTORS of B' and B'' (csrc/contingency_ac_sparse.hip: `pfn_contingency_ac_sparse`) -- the same fields,
    definitions and statuses, plus status -6 where the device line list is not the plan's; every other argument means what it means
    on the dense routes.  The base is `solve_power_flow(mode="fd" + variant, route="sparse", plan=plan)`'s launch and bits; the
    outage launch takes a lane per outage, 64 consecutive outages of a scenario to a one-wave workgroup.  "auto" never takes it;
    without a plan, with a plan of another mode or of another n / e it raises ValueError.  There `block`: where a tile's fp64 vectors
    sit -- "auto" (LDS where the block of about 2048 n bytes fits, up to 80 buses), "lds" (raises where it does not) or "global" (a
    block of the workspace per workgroup); `groups`: the number of one-wave workgroups the (scenario, tile) items are dealt to,
    None: min(S * tiles, 4 * compute units), each with a block of its own on the global placement; `threads`: the base solve's workgroup, None, 64 or 256.  No bit depends on any of the
    three.  `group` does not go with it; the result's `group` is 0 and its `block` "lds" or "global"."""
    who = "contingency_screen_ac"
    lo, hi = _screen_ac_options(variant, halves, v_limits, route, group, keep_table, keep_state)
    sparse = route == "sparse"
    if sparse:
        if group is not None:
            raise ValueError(f"{who}: group goes with the dense routes only; route 'sparse' takes block, groups and threads")
        _sparse_options(who, spec, edge_index, plan, block, groups, threads, mode="fd")
    elif plan is not None or block != "auto" or groups is not None or threads is not None:
        raise ValueError(f"{who}: plan, block, groups and threads go with route='sparse' only")
    if not sparse and torch.is_tensor(spec) and spec.dim() == 3:              # on the host, before anything touches a device
        cap = int(L.load().pfn_powerflow_max_unknowns())
        if int(spec.shape[1]) - 1 > cap:
            raise ValueError(f"{who}: {int(spec.shape[1]) - 1} unknowns per scenario exceed the dense screen's {cap} (max_unknowns()); "
                             f"beyond it: route='sparse' with plan=sparse_plan(bus_type, edge_index, mode='fd')")
    S, n, e, (n_pv, n_pq, slack), bt, spec, edge_index, rx, ratings = _prepare(who, bus_type, spec, edge_index, rx, ratings,
                                                                                plan=plan if sparse else None)
    dev = spec.device
    if init is not None:
        L.require_device(init, what=f"{who} init")
        if init.dtype != torch.float64 or tuple(init.shape) != (S, n, 2) or init.device != dev:
            raise RuntimeError(f"{who}: init must be float64 ({S}, {n}, 2) = (Vm, Va in degrees) on {dev}; got {init.dtype} {tuple(init.shape)}")
        init = init.contiguous()
    lib = L.load()
    in_lds, waves = C.c_int(0), 0
    if sparse:
        header, g = C.addressof(plan.header), 0 if groups is None else groups
        fits = int(lib.pfn_contingency_ac_sparse_workspace_bytes(1, e, header, 1, g)) != 0    # (0: the forced LDS placement is refused)
        if block == "lds" and not fits:
            raise RuntimeError(f"{who}: block 'lds': an outage block of {n} buses needs {int(lib.pfn_contingency_ac_sparse_block_bytes(header))} "
                               f"bytes and does not fit LDS")
        in_lds.value = int(block != "global" and fits)
    else:
        waves = int(lib.pfn_contingency_ac_waves(n, n_pq, _ROUTES[route], 0 if group is None else group, C.byref(in_lds)))
        if waves == 0:
            raise RuntimeError(f"{who}: route {route!r} with group {group!r}: the two inverses of {n} buses and the waves' vectors do not fit LDS")
    out = _outputs_ac(S, n, e, dev, keep_table, keep_state)
    islands = torch.empty(e, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):                                              # (sparse: the default `groups` asks the current device for its compute units)
        if sparse:
            entry, name = lib.pfn_contingency_ac_sparse, "pfn_contingency_ac_sparse"
            need = int(lib.pfn_contingency_ac_sparse_workspace_bytes(S, e, header, _BLOCKS[block], g)) if S else 0
            middle = (header, plan.blob.data_ptr(), 0 if threads is None else threads, _BLOCKS[block], g)
            placed = dict(route="sparse", group=0, block="lds" if in_lds.value else "global")
        else:
            entry, name = lib.pfn_contingency_ac, "pfn_contingency_ac"
            need = int(lib.pfn_contingency_ac_workspace_bytes(S, n, e, n_pq))
            middle = (_ROUTES[route], 0 if group is None else group)
            placed = dict(route="lds" if in_lds.value else "global", group=waves)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        _islands(edge_index, e, n, slack, islands)
        L.check(entry(edge_index.data_ptr(), e, rx.data_ptr(), bt.data_ptr(), spec.data_ptr(), L.ptr(init), L.ptr(ratings),
                      int(ratings is not None and ratings.dim() == 2), islands.data_ptr(), S, n, n_pv, n_pq, _VARIANTS[variant], halves, lo, hi,
                      float(tol), int(max_iter), *middle, *[L.ptr(t) for t in out.values()], ws.data_ptr(), need, L.stream_ptr()), name)
    return ACContingencyResult(islands=islands, **placed, **out)


# ================================================================================ generator outages, alone and with a line outage
_UNITS_KEPT = {}  # (device, unit tuple) -> int32 [G] on the device: a capture after its eager call uploads nothing


@dataclass
class UnitContingencyResult:
    """`contingency_screen_units`' answer.  `units` [G] int64: the bus of every unit; `unit_p` [S, G] float64: the output each outage
    removes; `participation` [G] / [S, G] float64 or None as the call took it.  Per (scenario s, unit g): `severity` [S, G] float32,
    `worst_line` [S, G] int32 and `overloads` [S, G] int32 by `ContingencyResult`'s rules with ALL lines monitored (NaN, -1, -1 where
    the scenario failed).  `base_flow` [S, e] float64 and `status` [S] int32 carry `contingency_screen`'s bits for the same inputs
    where the unit inputs are good; status -3 also where a `unit_p` is not finite or a participation factor is not finite and >= 0.
    `post_flow` [S, G, e] float32 with `keep_table`, else None.  With `lines`: `lines` [c] int64, `islands` [c] int32 (buses the outage
    of candidate line j cuts off the slack), and per (s, g, candidate j) `line_severity` [S, G, c] float32, `line_worst_line`,
    `line_overloads` [S, G, c] int32 (+inf, -1, -1 where the line islands buses) and `line_post_flow` [S, G, c, e] float32 with
    `keep_table`; without: all None.  `flags` [1] int32 (bit 0: `bus_type` changed under the launch).  All on the device, nothing
    read back; `route`: "lds" or "global"."""
    units: torch.Tensor
    unit_p: torch.Tensor
    severity: torch.Tensor
    worst_line: torch.Tensor
    overloads: torch.Tensor
    base_flow: torch.Tensor
    status: torch.Tensor
    post_flow: object
    route: str
    lines: object = None
    islands: object = None
    line_severity: object = None
    line_worst_line: object = None
    line_overloads: object = None
    line_post_flow: object = None
    participation: object = None
    flags: object = None

    def ranking(self, top):
        """(int64 [S, top] unit positions g, [S, top] their severities): `ContingencyResult.ranking`'s order -- NaN first, then
        +inf, then descending, ties to the lowest position."""
        return _rank(self.severity, top, "ranking")

    def line_ranking(self, top):
        """(int64 [S, top, 2] (unit position g, line id k), [S, top] their severities) over the unit x line items, in the same
        order; ties to the lowest (g, candidate) in row-major order."""
        if self.line_severity is None:
            raise ValueError("line_ranking: the screen ran without lines")
        S, G, c = self.line_severity.shape
        order, sev = _rank(self.line_severity.reshape(S, G * c), top, "line_ranking")
        return torch.stack([order // max(c, 1), self.lines[order % max(c, 1)]], dim=2), sev


@dataclass
class UnitContingencyVerification:
    """`items` [T, 3] int64 (scenario, unit position g, line id k or -1 for the unit alone), the AC `table` [T, n, 4] float64 and
    `status` [T] int32 of `solve_power_flow` on the shifted specification (without line k where k >= 0), `loading` [T, e] float32 =
    I_l / rating_l in the ORIGINAL line numbering (NaN at the outaged line), `severity` / `worst_line` / `overloads` by the screen's
    rules, and `dc_severity` [T] float32, the screen's figure for the item."""
    items: torch.Tensor
    table: torch.Tensor
    status: torch.Tensor
    loading: torch.Tensor
    severity: torch.Tensor
    worst_line: torch.Tensor
    overloads: torch.Tensor
    dc_severity: torch.Tensor


def _host_units(units, n, who):
    """the unit buses as a list of ints, checked on the host: a host sequence or a CPU int64 vector of at least one id, each within
    [0, n) where n is known"""
    if isinstance(units, (int, str, bytes)):                                  # (a bare count means nothing here; bool is an int)
        raise ValueError(f"{who}: units must be a sequence of bus ids; got {units!r}")
    if torch.is_tensor(units):
        if units.device.type != "cpu" or units.dtype != torch.int64 or units.dim() != 1:
            raise ValueError(f"{who}: units as a tensor must be a CPU int64 vector; got {units.dtype} {tuple(units.shape)} on {units.device}")
        got = units.tolist()
    else:
        got = list(units)
        try:
            if any(isinstance(b, bool) for b in got):
                raise TypeError
            got = [operator.index(b) for b in got]                            # (numpy integers too)
        except TypeError:
            raise ValueError(f"{who}: units must be ints, the bus of every unit; got {got!r}") from None
    if len(got) < 1:
        raise ValueError(f"{who}: at least one unit is needed; got none")
    if min(got) < 0 or (n is not None and max(got) >= n):
        raise ValueError(f"{who}: units must lie within [0, {n}); got {min(got)} .. {max(got)}")
    return got


def _device_units(units, dev):
    key = (str(dev), tuple(units))
    got = _UNITS_KEPT.get(key)
    if got is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("contingency_screen_units: the units are uploaded once per list; call it eagerly once before capturing")
        if len(_UNITS_KEPT) >= 16:
            _UNITS_KEPT.pop(next(iter(_UNITS_KEPT)))
        got = _UNITS_KEPT[key] = torch.tensor(units, dtype=torch.int32).to(dev)
    return got


def _per_unit(t, S, G, name, who, dev):
    """a per-unit float64 input, [G] or [S, G] on the inputs' device: (contiguous tensor, per-scenario flag)"""
    L.require_device(t, what=f"{who} {name}")
    if t.dtype != torch.float64 or tuple(t.shape) not in ((G,), (S, G)) or t.device != dev:
        raise RuntimeError(f"{who}: {name} must be float64 ({G},) or ({S}, {G}) on {dev}; got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t.contiguous(), int(t.dim() == 2)


def contingency_screen_units(bus_type, spec, edge_index, rx, ratings=None, *, units=None, unit_p=None, participation=None, lines=None,
                             tol=1e-8, max_iter=10, route="auto", keep_table=False) -> UnitContingencyResult:
    """Screen every generator outage of every scenario under the DC model, alone and -- with `lines` -- followed by a line outage:
    inputs and their checks are `contingency_screen`'s.  `units`: the bus of every unit, a host sequence or a CPU int64 tensor of
    G >= 1 ids within [0, n) (checked on the host; ValueError otherwise); any bus type, the slack included, and a bus may appear more
    than once (several units at one bus); None: the PV buses, ascending (formed on the device).  `unit_p`: float64 [G] or [S, G] on
    the device, the output lost with the unit, generation-positive per-unit; None: max(-spec[s, units, 2], 0), formed on the device.
    `participation`: float64 [G] or [S, G], a_h >= 0: the other units pick the lost output up in proportion a_h / (A - a_g); None (or
    where A - a_g is not > 0): the slack absorbs it.  `lines`: None (units only), "all", or strictly increasing line ids within
    [0, e) (a host sequence or a CPU int64 tensor; `contingency_screen_pairs`' rule): the items (unit g, then line k out of the
    post-unit state).  All e lines are monitored for a unit outage, all but k for (g, k).  `route`: "auto", "lds" (raises where
    B'^-1 does not fit LDS beside the vectors) or "global"; the same bits.  This is the dense route: `route="sparse"` and grids
    beyond `max_unknowns()` raise -- the sparse route is not built.  One launch (two with `lines`: the islands launch first); one
    host read (the bus_type counts, once per tensor); nothing is read back."""
    who = "contingency_screen_units"
    if route == "sparse":
        raise ValueError(f"{who}: route 'sparse' is not built; the unit screen runs on the dense routes {sorted(_ROUTES)} only")
    if route not in _ROUTES:
        raise ValueError(f"{who}: route must be one of {sorted(_ROUTES)}")
    if not isinstance(keep_table, bool):
        raise ValueError(f"{who}: keep_table must be a bool; got {keep_table!r}")
    n_given = int(spec.shape[1]) if torch.is_tensor(spec) and spec.dim() == 3 else None
    e_given = int(edge_index.shape[1]) if torch.is_tensor(edge_index) and edge_index.dim() == 2 else None
    if units is not None:                                                     # on the host, before anything touches the library
        units = _host_units(units, n_given, who)
    every_line = isinstance(lines, str)
    if every_line:
        if lines != "all":
            raise ValueError(f"{who}: lines must be None, 'all' or line ids; got {lines!r}")
    elif lines is not None:
        lines = _candidates(lines, who)
        if len(lines) < 1:
            raise ValueError(f"{who}: lines needs at least one candidate line; got none (None: no unit x line part)")
        if any(b <= a for a, b in zip(lines, lines[1:])):
            raise ValueError(f"{who}: lines must be strictly increasing (sorted, no duplicates)")
        if lines[0] < 0 or (e_given is not None and lines[-1] >= e_given):
            raise ValueError(f"{who}: lines must lie within [0, {e_given}); got {lines[0]} .. {lines[-1]}")

    def dense_only(n, e):
        cap = int(L.load().pfn_powerflow_max_unknowns())
        if n - 1 > cap:
            raise ValueError(f"{who}: {n - 1} unknowns per scenario exceed the dense screen's {cap} (max_unknowns()); the sparse route is not built")
    S, n, e, (n_pv, n_pq, slack), bt, spec, edge_index, rx, ratings = _prepare(who, bus_type, spec, edge_index, rx, ratings, after_check=dense_only)
    dev, lib = spec.device, L.load()
    if units is None:
        if n_pv < 1:
            raise ValueError(f"{who}: units=None means the PV buses, and this grid has none")
        units_d = torch.sort((bt != 1).to(torch.int8), stable=True).indices[:n_pv].to(torch.int32)    # the PV buses, ascending: no read-back
    else:
        units_d = _device_units(units, dev)
    G = int(units_d.shape[0])
    if unit_p is None:
        unit_p, p_each = torch.clamp(-spec[:, units_d.long(), 2], min=0.0).contiguous(), 1
    else:
        unit_p, p_each = _per_unit(unit_p, S, G, "unit_p", who, dev)
    part, a_each = (None, 0) if participation is None else _per_unit(participation, S, G, "participation", who, dev)
    if every_line:
        c, lines_d = e, torch.arange(e, dtype=torch.int32, device=dev)
    elif lines is not None:
        c, lines_d = len(lines), _device_lines(lines, dev)[0]
    else:
        c, lines_d = 0, None
    out = _outputs(S, e, G, dev, keep_table)
    new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device=dev)  # noqa: E731
    line_out = dict(line_severity=None, line_worst_line=None, line_overloads=None, line_post_flow=None)
    islands = None
    if c:
        islands = new(torch.int32, e)
        line_out = dict(line_severity=new(torch.float32, S, G, c), line_worst_line=new(torch.int32, S, G, c),
                        line_overloads=new(torch.int32, S, G, c), line_post_flow=new(torch.float32, S, G, c, e) if keep_table else None)
    need = int(lib.pfn_contingency_units_workspace_bytes(S, n, e, G, _ROUTES[route]))
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    with torch.cuda.device(dev):
        if c:
            _islands(edge_index, e, n, slack, islands)
        L.check(lib.pfn_contingency_units(edge_index.data_ptr(), e, rx.data_ptr(), bt.data_ptr(), spec.data_ptr(), L.ptr(ratings),
                                          int(ratings is not None and ratings.dim() == 2), units_d.data_ptr(), G, unit_p.data_ptr(), p_each,
                                          L.ptr(part), a_each, L.ptr(lines_d), c, L.ptr(islands), S, n, n_pv, n_pq, float(tol), int(max_iter),
                                          _ROUTES[route], out["severity"].data_ptr(), out["worst_line"].data_ptr(), out["overloads"].data_ptr(),
                                          out["base_flow"].data_ptr(), out["status"].data_ptr(), L.ptr(out["post_flow"]),
                                          *[L.ptr(line_out[k]) for k in ("line_severity", "line_worst_line", "line_overloads", "line_post_flow")],
                                          out["flags"].data_ptr(), L.ptr(ws), need, L.stream_ptr()),
                "pfn_contingency_units")
    if c:
        line_out.update(lines=lines_d.long(), islands=islands[lines_d.long()])
    return UnitContingencyResult(units=units_d.long(), unit_p=unit_p if p_each else unit_p.expand(S, G), route="global" if need else "lds",
                                 participation=part, **out, **line_out)


def unit_outage_spec(spec, units, unit_p, participation, g):
    """`spec` [T, n, 4] with the outage of the unit at position g[t] written into the demand-positive P column of row t, by the
    definition of include/pfn_hip.h: P rises by p_g at the unit's bus and, where rest_g = A - a_g > 0, falls by p_g a_h / rest_g at
    the bus of every other unit h (several units of one bus add up, in stored order).  `units` [G] int64, `unit_p` [T, G], `participation` [T, G] or
    None, `g` [T] int64, all on `spec`'s device.  Returns a new tensor."""
    T, G = int(unit_p.shape[0]), int(units.shape[0])
    rows = torch.arange(T, device=spec.device)
    p = unit_p[rows, g]                                                        # [T]
    shift = torch.zeros(T, G, dtype=torch.float64, device=spec.device)
    if participation is not None:
        a = participation.expand(T, G)
        A = torch.zeros(T, dtype=torch.float64, device=spec.device)
        for h in range(G):                                                     # (A in stored order, as the kernel sums it)
            A = A + a[:, h]
        rest = A - a[rows, g]
        share = torch.where((rest > 0)[:, None], -p[:, None] * a / torch.where(rest > 0, rest, torch.ones_like(rest))[:, None], shift)
        share[rows, g] = 0.0
        shift = share
    shift[rows, g] = p
    out = spec.clone()
    for h, b in enumerate(units.tolist()):                                    # stored order, one addition each: the same bits every time
        out[:, b, 2] += shift[:, h]
    return out


def verify_unit_contingencies(result, bus_type, spec, edge_index, rx, ratings=None, *, top=5, items=None,
                              **solver_kw) -> UnitContingencyVerification:
    """AC check of chosen items of a `contingency_screen_units` result (same inputs): `items` -- rows (scenario, unit position g) or
    (scenario, g, line id k), k among the screen's lines (ValueError otherwise) -- or per scenario the `top` unit outages of
    `result.ranking` and, where the screen had lines, the `top` items of `result.line_ranking`; items whose line islands buses are
    skipped.  For every item `spec` is shifted by the outage (`unit_outage_spec`: the screen's `unit_p` and `participation`), line k
    is removed where there is one, the unchanged `solve_power_flow(mode="ac", **solver_kw)` solves, `loss.branch_flows` gives the
    line currents, and the loadings go back to the original line numbering.  THE BUS TYPES STAY AS THEY ARE: a PV bus that loses
    its unit keeps its voltage set point, i.e. its reactive support -- converting a bus that lost its only unit to PQ is not built.
    The rows are chosen on the host (T is small)."""
    who = "verify_unit_contingencies"
    S, n, e = _check(bus_type, spec, edge_index, rx, who)
    ratings = _ratings(ratings, S, e, who)
    dev = spec.device
    G = int(result.units.shape[0])
    held = [] if result.lines is None else result.lines.cpu().tolist()
    isl = [] if result.islands is None else result.islands.cpu().tolist()
    where = {k: j for j, k in enumerate(held)}
    if items is None:
        if isinstance(top, bool) or not isinstance(top, int) or top < 0:
            raise ValueError(f"{who}: top must be an int >= 0; got {top!r}")
        order = result.ranking(min(top, G))[0].cpu().tolist()
        chosen = [(s, g, -1) for s in range(S) for g in order[s]]
        if held:
            pairs = result.line_ranking(G * len(held))[0].cpu().tolist()
            chosen += [(s, g, k) for s in range(S) for g, k in [gk for gk in pairs[s] if isl[where[gk[1]]] == 0][:top]]
    else:
        chosen = []
        for row in (items.tolist() if torch.is_tensor(items) else items):
            row = tuple(int(v) for v in row)
            s, g, k = row if len(row) == 3 else row + (-1,)
            if not (0 <= s < S and 0 <= g < G) or (k != -1 and k not in where):
                raise ValueError(f"{who}: {row} is no (scenario, unit[, line]) of this screen ({S} scenarios, {G} units, lines {held})")
            if k == -1 or isl[where[k]] == 0:
                chosen.append((s, g, k))
    alone = [it for it in chosen if it[2] < 0]
    lined = [it for it in chosen if it[2] >= 0]
    parts = []
    for group, K in [(grp, K) for grp, K in ((alone, 0), (lined, 1)) if grp] or [(alone, 0)]:
        rows = torch.tensor(group, dtype=torch.int64, device=dev).reshape(-1, 3)
        T = int(rows.shape[0])
        sc, g = rows[:, 0], rows[:, 1]
        part = None if result.participation is None else result.participation.expand(S, G)[sc]
        shifted = unit_outage_spec(spec[sc], result.units, result.unit_p[sc], part, g)
        rate = None if ratings is None else (ratings if ratings.dim() == 1 else ratings[sc].contiguous())
        solved, loading, severity, worst, overloads = _verify_removed(bus_type, shifted, edge_index, rx[sc].contiguous(), rate, T, e,
                                                                      torch.arange(T, device=dev), rows[:, 2:2 + K], dict(solver_kw))
        if K:
            pos = torch.tensor([where[k] for _, _, k in group], dtype=torch.int64, device=dev)
            dc = result.line_severity[sc, g, pos]
        else:
            dc = result.severity[sc, g]
        parts.append((rows, solved.table, solved.status, loading, severity, worst, overloads, dc))
    cat = [torch.cat(col, dim=0) for col in zip(*parts)]
    return UnitContingencyVerification(items=cat[0], table=cat[1], status=cat[2], loading=cat[3], severity=cat[4], worst_line=cat[5],
                                       overloads=cat[6], dc_severity=cat[7])
