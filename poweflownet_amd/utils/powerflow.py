"""Batched AC / DC / fast-decoupled power flow on the device: `solve_power_flow` is ONE `pfn_powerflow_solve_init` launch
(csrc/powerflow.hip), one workgroup per sample, from a flat start or from a table the caller gives (a model's prediction).  It stands where the reference calls pandapower -- `pp.runpp` in dataset_generator.py, `pp.rundcpp` in
dc_error.py -- for this project's network model: series admittance only, every stored line in both directions, P and Q
demand-positive per-unit, Va in degrees; no shunts, line charging, taps or unit conversion.  The mismatch it drives to zero
is exactly `PowerImbalance`'s dP_i, dQ_i, so a solved table is what that loss calls balanced.  `solve_power_flow_qlim`
(csrc/powerflow_qlim.hip) is the dense AC solve with per-sample bus types and generator Q-limits, the reference's
`enforce_q_lims=True`; with `route="sparse", plan=qlim_plan(...)` (csrc/powerflow_sparse_qlim.hip) it is the same solve beyond the
dense cap, on the plan of the grid with every non-slack bus PQ.  No CPU path."""
import ctypes as C
import time
from dataclasses import dataclass, replace

import numpy as np
import torch

from .. import _lib as L

# the texts of csrc/powerflow_common.hpp's status enum (PF_NOT_CONVERGED ... PF_QLIM_ROUNDS), which every route's kernel writes
STATUS = {-1: "not converged in max_iter", -2: "singular Jacobian", -3: "non-finite mismatch", -4: "a line names a bus outside the grid",
          -5: "bus_type disagrees with the counts the launch was sized for",
          -6: "the sparse plan was built from another line list or other bus types",
          -7: "Q-limits still violated after max_rounds re-solves"}
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


def sparse_plan(bus_type, edge_index, mode="ac", size_hint=None, device=None) -> SparsePlan:
    """Plan the sparse route for the grid (`bus_type` [n], `edge_index` int64 [2, e]; device or host tensors): one host read of the
    two, a minimum-degree order and the filled pattern built by the library on the host, one upload.  Reuse the plan for every solve
    on that grid and mode ("ac" or "dc").  mode "fd" (also spelled "fdxb" or "fdbx"; the plan's `mode` is "fd" either way): the
    fast-decoupled plan, the symbolic factorisations of B' and B'' in one blob, for `solve_power_flow(mode="fdxb" | "fdbx")`.
    `size_hint`: a guess of the plan's bytes (a plan of nearly the same grid is a good one); the plan is then built straight into a
    buffer of that size, one elimination per matrix where the sizing call and the build call run two, and again only where the
    guess was too small.  The plan is the same, byte for byte.  `device`: where the blob goes (default: where the inputs live)."""
    if mode not in ("ac", "dc") + _FD_PLAN_MODES:
        raise ValueError("sparse_plan: mode must be 'ac', 'dc' or 'fd' ('fdxb' and 'fdbx' are spellings of 'fd')")
    fd = mode in _FD_PLAN_MODES
    if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64 or bus_type.dim() != 1:
        raise RuntimeError(f"sparse_plan: edge_index must be int64 (2, e) and bus_type (n,); got {tuple(edge_index.shape)} and {tuple(bus_type.shape)}")
    dev = torch.device(device) if device is not None else (edge_index.device if edge_index.is_cuda else bus_type.device)
    ei = edge_index.detach().cpu().contiguous()
    bt = bus_type.detach().to(torch.int32).cpu().contiguous()
    lib = L.load()
    e, n = int(ei.shape[1]), int(bt.shape[0])
    t0 = time.perf_counter()
    if size_hint is not None:
        needed, room = C.c_size_t(0), max(int(size_hint), 4 * _PLAN_HEADER_WORDS)
        for _ in range(2):
            host = torch.empty(room, dtype=torch.uint8)
            rc = lib.pfn_powerflow_sparse_plan_into(ei.data_ptr(), e, bt.data_ptr(), n, 2 if fd else _MODES[mode], host.data_ptr(), room, C.byref(needed))
            if rc != -2:                                           # (-2: PFN_ENOSPACE, the guess was too small; `needed` says by how much)
                break
            room = int(needed.value)
        if rc != 0:
            raise RuntimeError(f"sparse_plan failed: {lib.pfn_last_error().decode('utf-8', 'replace')}")
        need = int(needed.value)
        host = host[:need]
    else:
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


@dataclass
class CoverPlan:
    """ONE sparse plan for a chunk of samples with their own line lists (`cover_plan`): `plan` the `SparsePlan` of the COVER list,
    `cover` that list on the device (int64 [2, e_cover]: the base lines in base order, then the extra lines any sample needs),
    `keys` / `slot` the table `pfn_powerflow_cover_map` searches (the cover's keys sorted ascending, equal keys in cover order, and
    the cover line at each sorted position), `n`, `mode` as the plan's, `e_base` the base lines in front, `e_cover` all of them."""
    plan: SparsePlan
    cover: torch.Tensor
    keys: torch.Tensor
    slot: torch.Tensor
    n: int
    mode: str
    e_base: int
    e_cover: int

    @property
    def extras(self) -> int:
        return self.e_cover - self.e_base

    def to(self, device) -> "CoverPlan":
        """The same plan with its blob, cover list and search table on `device`."""
        plan = replace(self.plan, blob=self.plan.blob.to(device))
        return replace(self, plan=plan, cover=self.cover.to(device), keys=self.keys.to(device), slot=self.slot.to(device))


def _line_keys(ei, n):
    """numpy int64 [..., 2, e] -> the lines' keys [..., e]: the unordered bus pair as min * n + max"""
    return np.minimum(ei[..., 0, :], ei[..., 1, :]) * np.int64(n) + np.maximum(ei[..., 0, :], ei[..., 1, :])


def _key_ranks(keys):
    """numpy [S, e] -> the rank of every line among the lines of its row with its key, in stored order"""
    S, e = keys.shape
    order = np.argsort(keys, axis=1, kind="stable")
    sk = np.take_along_axis(keys, order, 1)
    idx = np.broadcast_to(np.arange(e, dtype=np.int64), (S, e))
    first = np.ones((S, e), dtype=bool)
    first[:, 1:] = sk[:, 1:] != sk[:, :-1]
    rank = np.empty((S, e), dtype=np.int64)
    np.put_along_axis(rank, order, idx - np.maximum.accumulate(np.where(first, idx, 0), axis=1), 1)
    return rank


def cover_list(edge_index, n, base=None):
    """The COVER list of the samples' line lists (host numpy int64: `edge_index` [S, 2, e], `base` [2, e0] or None) on `n` buses:
    `base` as it stands, then the missing copies ascending by key -- a line's key is its unordered bus pair, min * n + max --,
    oriented (min, max).  A pair's multiplicity in the cover is the larger of its count in `base` and its count in any ONE sample;
    base lines no sample uses stay.  Returns int64 [2, e_cover]."""
    ei = np.asarray(edge_index, dtype=np.int64)
    base = np.zeros((2, 0), dtype=np.int64) if base is None else np.asarray(base, dtype=np.int64)
    if ei.ndim != 3 or ei.shape[1] != 2 or base.ndim != 2 or base.shape[0] != 2:
        raise RuntimeError(f"cover_list: edge_index must be (S, 2, e) and base (2, e0); got {ei.shape} and {base.shape}")
    span = max(ei.shape[2], base.shape[1]) + 1                      # (key, rank) as one word: rank < span
    have = _line_keys(base, n) * span + _key_ranks(_line_keys(base, n)[None])[0]
    keys = _line_keys(ei, n)
    want = np.unique(keys * span + _key_ranks(keys))
    extra = np.setdiff1d(want, have) // span                         # ascending by (key, rank): by key
    return np.concatenate([base, np.stack([extra // n, extra % n])], axis=1)


def cover_plan(bus_type, edge_index, mode="ac", base=None, size_hint=None, device=None) -> CoverPlan:
    """Plan the sparse route for S samples with their own line lists (`edge_index` int64 [S, 2, e], `bus_type` [n]; device or host):
    ONE `sparse_plan` (mode "ac", "dc" or "fd") on their cover list (`cover_list`; `base` [2, e0]: the grid the samples are
    perturbations of, kept in front so that most lines keep their place).  A factorisation under a static order without pivoting
    stays valid on a superset of a sample's pattern, so the one plan serves every sample of the chunk; `solve_power_flow(...,
    route="sparse", plan=<CoverPlan>)` tells the kernels per sample which cover lines exist.  One host read of the lists, one host
    elimination (`size_hint`: `sparse_plan`'s; without one the builder runs its sizing pass first), one upload -- on `device` where
    given ("cpu": no upload yet; `CoverPlan.to` moves it), else where the inputs live.  A sample line that names a bus outside the
    grid or one bus twice is refused HERE (RuntimeError "cover_plan failed"), before the builder runs: min * n + max would alias
    another pair's key otherwise.  The builder's own PFN_EINVAL still answers a base line outside the grid."""
    if edge_index.dim() != 3 or edge_index.shape[1] != 2 or edge_index.dtype != torch.int64 or bus_type.dim() != 1:
        raise RuntimeError(f"cover_plan: edge_index must be int64 (S, 2, e) and bus_type (n,); got {tuple(edge_index.shape)} and {tuple(bus_type.shape)}")
    if base is not None and (base.dim() != 2 or base.shape[0] != 2 or base.dtype != torch.int64):
        raise RuntimeError(f"cover_plan: base must be int64 (2, e0); got {base.dtype} {tuple(base.shape)}")
    dev = torch.device(device) if device is not None else (edge_index.device if edge_index.is_cuda else bus_type.device)
    n = int(bus_type.shape[0])
    ei = edge_index.detach().cpu().numpy()
    b = None if base is None else base.detach().cpu().numpy()
    lo, hi = np.minimum(ei[:, 0], ei[:, 1]), np.maximum(ei[:, 0], ei[:, 1])
    wrong = (lo < 0) | (hi >= n) | (lo == hi)
    if wrong.any():
        s, k = (int(v[0]) for v in np.nonzero(wrong))
        raise RuntimeError(f"cover_plan failed: line {k} of sample {s} joins buses {int(ei[s, 0, k])} and {int(ei[s, 1, k])}: "
                           f"a line names two different buses inside [0, {n})")
    cover = torch.from_numpy(cover_list(ei, n, b))
    plan = sparse_plan(bus_type, cover, mode, size_hint, device=dev)   # (a base line outside the grid is the builder's refusal)
    order = np.argsort(_line_keys(cover.numpy(), n), kind="stable")
    return CoverPlan(plan=plan, cover=cover.to(dev), keys=torch.from_numpy(_line_keys(cover.numpy(), n)[order]).to(dev),
                     slot=torch.from_numpy(order.astype(np.int32)).to(dev), n=n, mode=plan.mode,
                     e_base=0 if b is None else int(b.shape[1]), e_cover=int(cover.shape[1]))


def cover_map(plan: CoverPlan, edge_index, rx, fill=None):
    """ONE `pfn_powerflow_cover_map` launch (csrc/powerflow_cover.hip): (`line_mask` uint8 [S, e_cover], `rx_cover` float64
    [S, e_cover, 2], `unplaced` int32 [S]) of the samples' lists `edge_index` [S, 2, e] and parameters `rx` [S, e, 2] under the
    plan's cover list, by the slot rule: a sample's k-th line with a key, in stored order, takes the k-th cover line with that key,
    in cover order.  `rx_cover` is written where the mask is 1 only; `fill` (a float, e.g. NaN) is what the rest holds, None leaves
    it unset.  Nothing is read back."""
    dev = L.require_device(edge_index, rx, plan.cover, what="cover_map input")
    if edge_index.dtype != torch.int64 or edge_index.dim() != 3 or edge_index.shape[1] != 2:
        raise RuntimeError(f"cover_map: edge_index must be int64 (S, 2, e); got {edge_index.dtype} {tuple(edge_index.shape)}")
    S, e = int(edge_index.shape[0]), int(edge_index.shape[2])
    if rx.dtype != torch.float64 or tuple(rx.shape) != (S, e, 2):
        raise RuntimeError(f"cover_map: rx must be float64 ({S}, {e}, 2); got {rx.dtype} {tuple(rx.shape)}")
    edge_index, rx = edge_index.contiguous(), rx.contiguous()
    ec = plan.e_cover
    mask = torch.empty(S, ec, dtype=torch.uint8, device=dev)
    rx_cover = torch.empty(S, ec, 2, dtype=torch.float64, device=dev) if fill is None else torch.full((S, ec, 2), float(fill), dtype=torch.float64, device=dev)
    unplaced = torch.empty(S, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().pfn_powerflow_cover_map(edge_index.data_ptr(), e, rx.data_ptr(), S, plan.n, plan.keys.data_ptr(), plan.slot.data_ptr(),
                                                 ec, mask.data_ptr(), rx_cover.data_ptr(), unplaced.data_ptr(), L.stream_ptr()),
                "pfn_powerflow_cover_map")
    return mask, rx_cover, unplaced


class CoverChunker:
    """Splits batches of per-sample line lists into chunks that share one cover plan each.  Every extra line of a cover adds fill,
    so a chunk is as large as keeps its plan's multiply-adds per factor within `max_growth` times those of the plan of `base` alone
    (`base_plan`, built here once): more samples per chunk save host eliminations, fewer save factor work on the device.  The first
    batch finds the size -- from `start`, doubled while the cover fits, halved while it does not, one plan build per trial -- and
    the following chunks and batches reuse it, halving again only where a cover does not fit.  A chunk of one sample is taken as
    it is.  `trials` counts the plans built, `sizes` the chunks handed out."""

    def __init__(self, bus_type, base, mode="ac", max_growth=None, start=64):
        self.bus_type, self.base, self.mode = bus_type, base, mode
        self.max_growth = COVER_MAX_GROWTH if max_growth is None else float(max_growth)
        if not self.max_growth >= 1.0 or start < 1:
            raise ValueError(f"CoverChunker: max_growth must be at least 1 and start at least 1; got {max_growth!r}, {start!r}")
        self.base_plan = sparse_plan(bus_type, base, mode)
        self.device = self.base_plan.blob.device
        self.size, self.settled, self.trials, self.sizes = int(start), False, 0, []
        self.hint = self.base_plan.bytes + self.base_plan.bytes // 5

    def growth(self, plan: CoverPlan) -> float:
        return plan.plan.madds / max(self.base_plan.madds, 1)

    def _try(self, edge_index, at, size):
        self.trials += 1
        # (the base plan's size and a fifth is the guess: a cover adds a few lines and their fill; a miss costs one more elimination)
        # (a trial is judged by the header's multiply-adds alone: it stays on the host, and only an accepted plan is uploaded)
        plan = cover_plan(self.bus_type, edge_index[at:at + size], self.mode, self.base, size_hint=self.hint, device="cpu")
        self.hint = max(self.hint, plan.plan.bytes + plan.plan.bytes // 16)
        return plan, size == 1 or self.growth(plan) <= self.max_growth

    def plans(self, edge_index):
        """Yields (rows, CoverPlan) over `edge_index` [S, 2, e]: `rows` a slice of consecutive samples, the plan their cover's."""
        S, at = int(edge_index.shape[0]), 0
        while at < S:
            size = min(self.size, S - at)
            plan, fits = self._try(edge_index, at, size)
            while not fits:
                size = max(1, size // 2)
                self.size = size
                self.settled = True
                plan, fits = self._try(edge_index, at, size)
            while not self.settled and size == self.size and at + 2 * size <= S:
                wider, fits = self._try(edge_index, at, 2 * size)
                if not fits:
                    break
                plan, size = wider, 2 * size
                self.size = size
            self.settled = True
            self.sizes.append(size)
            yield slice(at, at + size), plan.to(self.device)
            at += size


def solve_power_flow_covered(chunker: CoverChunker, spec, edge_index, rx, *, plans=None, **kw):
    """`solve_power_flow(route="sparse")` for S samples with their own line lists `[S, 2, e]`, in chunks that share a cover plan
    each: (`PowerFlowResult` over all samples, `plans`).  `plans`: the list of (rows, CoverPlan) of an earlier call on the same
    lists, to solve them again (another start, a timing) without planning again; None asks `chunker` (its mode: "fd" serves
    mode="fdxb" and "fdbx").  `kw` goes to `solve_power_flow`."""
    plans = list(chunker.plans(edge_index)) if plans is None else plans
    init = kw.pop("init", None)
    parts = [solve_power_flow(chunker.bus_type, spec[rows], edge_index[rows], rx[rows], route="sparse", plan=plan,
                              init=None if init is None else init[rows], **kw) for rows, plan in plans]
    if not parts:
        raise RuntimeError("solve_power_flow_covered: no samples")
    whole = PowerFlowResult(*(torch.cat([getattr(r, f) for r in parts]) for f in ("table", "status", "iterations", "residual")),
                            flags=torch.stack([r.flags for r in parts]).amax(0), route="sparse")
    return whole, plans


# what a cover may cost: its plan's multiply-adds per factor over the base plan's.  At (6470, 9005), one line removed and one added
# per sample, chunks of 16 / 64 / 256 samples grew the factor work 0.99 / 1.03 / 1.28 times and took 133 / 37.9 / 15.1 ms per sample,
# plan and solve together: the largest chunk won, so the bound admits it (DESIGN 7p has the rows; nothing larger was measured)
COVER_MAX_GROWTH = 1.3


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

    Per-sample line lists `[S, 2, e]` on route "sparse": pass `plan=cover_plan(bus_type, edge_index, mode, base)` (mode "fd" for
    fdxb / fdbx), ONE plan on a cover list that holds every line of every sample.  Two launches, no read-back: the map
    (csrc/powerflow_cover.hip: which cover lines a sample has, its rx in cover order) and the masked solve, in which a line the
    sample lacks is a structural zero.  A sample with a line the cover lacks gets status -6, one whose lists leave a bus without a
    line -2.  `CoverChunker` splits a batch into chunks whose cover keeps the factor work within a growth bound.  A sample's bits
    are a function of (sample, cover plan): independent of the other samples of the batch and of the workgroup size, but under
    another cover the elimination order and fill differ, so the results agree to rounding only.  Without a plan, or with a
    one-topology `SparsePlan`, per-sample lists raise as before.

    One host read (the counts of `bus_type`, which size the launch); no read-back of the results."""
    return _solve(bus_type, spec, edge_index, rx, mode, tol, max_iter, route, init, plan, 0)


@dataclass
class QLimResult(PowerFlowResult):
    """`PowerFlowResult` of `solve_power_flow_qlim` with `bus_type` [S, n] int32, the types the samples ended with (a PV bus that hit
    a limit is 2; a failed sample's are the ones it came with), and `rounds` [S] int32, the re-solves (0: no limit was hit).
    `status` >= 0 counts the Jacobian solves of all rounds."""
    bus_type: torch.Tensor = None
    rounds: torch.Tensor = None


def qlim_plan(bus_type, edge_index, base=None, size_hint=None, device=None):
    """The plan `solve_power_flow_qlim(route="sparse", plan=...)` takes: the AC plan of the grid for the type row in which EVERY
    non-slack bus is PQ, m = 2 (n - 1) unknowns, so that one plan serves whatever PV set a sample has and whichever of its PV buses
    switch (csrc/powerflow_sparse_qlim.hip: the Vm of a bus that is PV is a dead unknown, an identity row and column).  `bus_type`
    [n] or [S, n] integer: only the slack's place is read, and all rows must have their one slack at the same bus (RuntimeError
    otherwise; the plan is built on the host anyway, so the read costs nothing more).  `edge_index` int64 [2, e]: `sparse_plan(all_pq,
    edge_index, "ac", size_hint, device)`, a `SparsePlan`; [S, 2, e]: `cover_plan(all_pq, edge_index, "ac", base, size_hint, device)`,
    a `CoverPlan` on the samples' cover list.  No new blob format.  To chunk a batch of per-sample lists, `CoverChunker(all_pq_row,
    base, "ac")` works as it stands: its plans are these plans."""
    if bus_type.dim() not in (1, 2) or bus_type.dtype not in (torch.int32, torch.int64) or bus_type.shape[-1] < 1:
        raise RuntimeError(f"qlim_plan: bus_type must be an integer tensor (n,) or (S, n); got {bus_type.dtype} {tuple(bus_type.shape)}")
    if edge_index.dtype != torch.int64 or edge_index.dim() not in (2, 3) or edge_index.shape[-2] != 2:
        raise RuntimeError(f"qlim_plan: edge_index must be int64 (2, e) or (S, 2, e); got {edge_index.dtype} {tuple(edge_index.shape)}")
    dev = torch.device(device) if device is not None else (edge_index.device if edge_index.is_cuda else bus_type.device)
    rows = bus_type.detach().cpu().reshape(-1, bus_type.shape[-1])
    slack = rows == 0
    if rows.shape[0] == 0 or bool((slack.sum(1) != 1).any()) or bool((slack != slack[0]).any()):
        raise RuntimeError("qlim_plan: every row of bus_type needs exactly one slack (0), all at the same bus: the plan is built around it")
    all_pq = torch.where(slack[0], 0, 2).to(torch.int32)
    if edge_index.dim() == 2:
        return sparse_plan(all_pq, edge_index, "ac", size_hint, device=dev)
    return cover_plan(all_pq, edge_index, "ac", base, size_hint, device=dev)


def solve_power_flow_qlim(bus_type, spec, edge_index, rx, q_limits=None, *, tol=1e-8, max_iter=10, max_rounds=8, q_tol=None,
                          route="auto", init=None, plan=None) -> QLimResult:
    """`solve_power_flow(mode="ac")` with the bus types the SAMPLE's and generator Q-limits enforced, as the reference's
    `pp.runpp(..., enforce_q_lims=True)` does: ONE `pfn_powerflow_solve_qlim` launch (csrc/powerflow_qlim.hip), one workgroup per
    sample, the rounds inside the kernel.  `bus_type` [n] or [S, n] integer (0 slack, 1 PV, 2 PQ; a row without exactly one slack or
    with another type fails that sample alone, status -5), `spec`, `edge_index` ([2, e] or [S, 2, e]), `rx`, `init` as in
    `solve_power_flow`.  `q_limits` float64 [n, 2] or [S, n, 2] = (lo, hi) on the TABLE's Q column -- demand-positive per-unit, so a
    generator's [Qmin, Qmax] arrives as [-Qmax, -Qmin] --, read at PV buses only, NaN or +-inf meaning no limit on that side; None:
    no limits, the plain Newton solve with per-sample types.

    After an inner Newton loop converges, every PV bus whose Q line sum exceeds `hi + q_tol` becomes a PQ bus with Q fixed at `hi`,
    one below `lo - q_tol` a PQ bus at `lo`; all violators of a round switch together, none switches back, the slack is never
    limited; Newton then continues from the current state.  `max_iter` bounds the solves of each inner loop, `max_rounds` the
    re-solves (status -7 where limits are still violated after them).  `q_tol` None means `tol`: Q is only known to the mismatch
    tolerance, so a violation smaller than that is not one.

    Routes "auto", "lds" and "global"; storage is sized for every non-slack bus ending PQ, m_max = 2 (n - 1) unknowns, so 118 buses
    take the global route.  No host read at all: nothing is sized by the type counts.

    route "sparse", beyond `max_unknowns()` (csrc/powerflow_sparse_qlim.hip, ONE `pfn_powerflow_solve_sparse_qlim` launch): the same
    rounds on the sparse route's fp32 factor, static order, no pivoting.  It needs `plan=qlim_plan(bus_type, edge_index)`, the
    grid's plan with every non-slack bus PQ, built once per grid (without one: ValueError); "auto" never takes this route.  Per-sample
    line lists `[S, 2, e]` take the `CoverPlan` `qlim_plan(bus_type, edge_index, base)` gives: the map launch of `cover_map` first,
    then the masked solve -- two launches, no read-back.  A plan with m != 2 (n - 1), for another n, e or mode, on another device,
    a `CoverPlan` with one `[2, e]` list or a `SparsePlan` with per-sample lists raise before a device is touched.  A sample whose
    slack is not the plan's, or with a line the cover lacks, gets status -6; a sample's bits are a function of (sample, plan)."""
    return _solve_qlim(bus_type, spec, edge_index, rx, q_limits, tol, max_iter, max_rounds, q_tol, route, init, plan, 0)


def _solve_qlim(bus_type, spec, edge_index, rx, q_limits, tol, max_iter, max_rounds, q_tol, route, init, plan, threads) -> QLimResult:
    """`solve_power_flow_qlim` with the sparse route's workgroup size exposed (`threads`: 0 the library's choice, 64 or 256)."""
    if route == "sparse" and plan is None:
        raise ValueError("solve_power_flow_qlim: the sparse route with Q-limits or per-sample bus types needs the grid's plan with every "
                         "non-slack bus PQ: pass plan=qlim_plan(bus_type, edge_index)")
    if route not in ("auto", "lds", "global", "sparse"):
        raise ValueError("solve_power_flow_qlim: route must be one of 'auto', 'lds', 'global', 'sparse'")
    if plan is not None and route != "sparse":
        raise ValueError("solve_power_flow_qlim: a plan goes with route='sparse' only")
    if spec.dtype != torch.float64 or spec.dim() != 3 or spec.shape[2] != 4:
        raise RuntimeError(f"solve_power_flow_qlim: spec must be float64 (S, n, 4); got {spec.dtype} {tuple(spec.shape)}")
    S, n = int(spec.shape[0]), int(spec.shape[1])
    if bus_type.dtype not in (torch.int32, torch.int64) or tuple(bus_type.shape) not in ((n,), (S, n)):
        raise RuntimeError(f"solve_power_flow_qlim: bus_type must be an integer tensor ({n},) or ({S}, {n}); got {bus_type.dtype} {tuple(bus_type.shape)}")
    if edge_index.dtype != torch.int64 or edge_index.dim() not in (2, 3) or edge_index.shape[-2] != 2:
        raise RuntimeError(f"solve_power_flow_qlim: edge_index must be int64 (2, e) or (S, 2, e); got {edge_index.dtype} {tuple(edge_index.shape)}")
    e = int(edge_index.shape[-1])
    if edge_index.dim() == 3 and edge_index.shape[0] != S:
        raise RuntimeError(f"solve_power_flow_qlim: per-sample edge_index of {edge_index.shape[0]} samples against {S}")
    if rx.dtype != torch.float64 or tuple(rx.shape) != (S, e, 2):
        raise RuntimeError(f"solve_power_flow_qlim: rx must be float64 ({S}, {e}, 2); got {rx.dtype} {tuple(rx.shape)}")
    if q_limits is not None and (q_limits.dtype != torch.float64 or tuple(q_limits.shape) not in ((n, 2), (S, n, 2))):
        raise RuntimeError(f"solve_power_flow_qlim: q_limits must be float64 ({n}, 2) or ({S}, {n}, 2); got {q_limits.dtype} {tuple(q_limits.shape)}")
    if init is not None and (not init.is_floating_point() or init.dim() != 3 or tuple(init.shape[:2]) != (S, n) or init.shape[2] < 2):
        raise RuntimeError(f"solve_power_flow_qlim: init must be a float table ({S}, {n}, >= 2); got {init.dtype} {tuple(init.shape)}")
    q_tol = tol if q_tol is None else q_tol
    if max_rounds < 0 or not 0.0 <= q_tol < float("inf"):
        raise ValueError(f"solve_power_flow_qlim: max_rounds must be at least 0 and q_tol finite and at least 0; got {max_rounds!r}, {q_tol!r}")
    if route != "sparse" and 2 * (n - 1) > max_unknowns():
        raise RuntimeError(f"solve_power_flow_qlim: {2 * (n - 1)} unknowns per sample (every non-slack bus of {n} may end PQ) exceed the "
                           f"dense solver's {max_unknowns()}; a sparse factorisation is needed: route='sparse' with "
                           "plan=qlim_plan(bus_type, edge_index)")
    if route == "sparse":
        # what the kind of plan decides, said before anything touches a device
        covered = isinstance(plan, CoverPlan)
        if covered != (edge_index.dim() == 3):
            raise RuntimeError("solve_power_flow_qlim: a CoverPlan goes with per-sample (S, 2, e) line lists and a SparsePlan with one (2, e) "
                               f"list; got {type(plan).__name__} and edge_index {tuple(edge_index.shape)}")
        inner = plan.plan if covered else plan
        if not isinstance(inner, SparsePlan):
            raise RuntimeError(f"solve_power_flow_qlim: plan must be what qlim_plan returns, a SparsePlan or a CoverPlan; got {plan!r}")
        if (inner.n, inner.mode, inner.m) != (n, "ac", 2 * (n - 1)) or (not covered and inner.e != e):
            raise RuntimeError(f"solve_power_flow_qlim: the plan is for (n, e, mode) = {(inner.n, inner.e, inner.mode)} with {inner.m} unknowns; "
                               f"the call has {(n, e, 'ac')} and needs the plan with every non-slack bus PQ, {2 * (n - 1)} unknowns "
                               "(qlim_plan(bus_type, edge_index))")
        where = {t.device for t in (bus_type, spec, edge_index, rx)}
        if where != {inner.blob.device} or (covered and plan.cover.device != inner.blob.device):
            raise RuntimeError(f"solve_power_flow_qlim: the plan lives on {inner.blob.device}, the inputs on {sorted(map(str, where))}")
    dev = L.require_device(bus_type, spec, edge_index, rx, q_limits, init, what="solve_power_flow_qlim input")
    if init is not None:
        init = init[:, :, :2].to(torch.float64).contiguous()
    bt = bus_type.to(torch.int32).contiguous()
    spec, rx, edge_index = spec.contiguous(), rx.contiguous(), edge_index.contiguous()
    q_limits = None if q_limits is None else q_limits.contiguous()
    lib = L.load()
    table = torch.empty(S, n, 4, dtype=torch.float64, device=dev)
    status = torch.empty(S, dtype=torch.int32, device=dev)
    residual = torch.empty(S, dtype=torch.float64, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    types = torch.empty(S, n, dtype=torch.int32, device=dev)
    rounds = torch.empty(S, dtype=torch.int32, device=dev)
    if route == "sparse":
        line_mask = unplaced = None
        if isinstance(plan, CoverPlan):
            # per-sample lists under one cover plan: the map launch lays the samples out in cover order, then the masked solve
            line_mask, rx, unplaced = cover_map(plan, edge_index, rx)
            edge_index, e, plan = plan.cover, plan.e_cover, plan.plan
        need = int(lib.pfn_powerflow_sparse_qlim_workspace_bytes(S, C.addressof(plan.header))) if S else 0
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            L.check(lib.pfn_powerflow_solve_sparse_qlim(edge_index.data_ptr(), e, rx.data_ptr(), L.ptr(line_mask), L.ptr(unplaced), bt.data_ptr(),
                                                        int(bt.dim() == 2), spec.data_ptr(), L.ptr(init), L.ptr(q_limits),
                                                        int(q_limits is not None and q_limits.dim() == 3), S, n, float(tol), float(q_tol),
                                                        int(max_iter), int(max_rounds), C.addressof(plan.header), plan.blob.data_ptr(),
                                                        int(threads), table.data_ptr(), status.data_ptr(), residual.data_ptr(),
                                                        flags.data_ptr(), types.data_ptr(), rounds.data_ptr(), ws.data_ptr(), need,
                                                        L.stream_ptr()),
                    "pfn_powerflow_solve_sparse_qlim")
        return QLimResult(table=table, status=status, iterations=torch.where(status >= 0, status, torch.full_like(status, -1)),
                          residual=residual, flags=flags, route="sparse", bus_type=types, rounds=rounds)
    code = {"auto": 0, "lds": 1, "global": 2}[route]
    need = int(lib.pfn_powerflow_qlim_workspace_bytes(S, n, code))
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    with torch.cuda.device(dev):
        L.check(lib.pfn_powerflow_solve_qlim(edge_index.data_ptr(), int(edge_index.dim() == 3), e, rx.data_ptr(), bt.data_ptr(),
                                             int(bt.dim() == 2), spec.data_ptr(), L.ptr(init), L.ptr(q_limits),
                                             int(q_limits is not None and q_limits.dim() == 3), S, n, float(tol), float(q_tol),
                                             int(max_iter), int(max_rounds), code, table.data_ptr(), status.data_ptr(),
                                             residual.data_ptr(), flags.data_ptr(), types.data_ptr(), rounds.data_ptr(), L.ptr(ws), need,
                                             L.stream_ptr()),
                "pfn_powerflow_solve_qlim")
    return QLimResult(table=table, status=status, iterations=torch.where(status >= 0, status, torch.full_like(status, -1)),
                      residual=residual, flags=flags, route="global" if need else "lds", bus_type=types, rounds=rounds)


def _check_plan_takes_the_lists(spec, edge_index, mode, route, plan):
    """What the kind of plan decides about per-sample line lists on the sparse route, said before anything touches a device.  (So
    CPU tensors with a per-sample list and no cover plan on route "sparse" now raise "one topology" where they used to raise "no CPU
    fallback" first: that call was refused either way, only the order of its two refusals moved.)"""
    if route != "sparse" or mode not in _MODES or not isinstance(edge_index, torch.Tensor) or edge_index.dim() != 3:
        return
    fd = mode in ("fdxb", "fdbx")
    if fd and plan is None:
        return                                                     # (the fast-decoupled modes' own refusal follows)
    if not isinstance(plan, CoverPlan):
        raise RuntimeError("solve_power_flow: route 'sparse' takes one (2, e) line list for all samples: a plan belongs to one topology "
                           "(per-sample lists: plan=cover_plan(bus_type, edge_index, mode))")
    if isinstance(spec, torch.Tensor) and spec.dim() == 3 and (plan.n, plan.mode) != (int(spec.shape[1]), "fd" if fd else mode):
        raise RuntimeError(f"solve_power_flow: the plan is for (n, mode) = {(plan.n, plan.mode)} and per-sample lists; "
                           f"the call has {(int(spec.shape[1]), mode)}")


def _solve(bus_type, spec, edge_index, rx, mode, tol, max_iter, route, init, plan, threads) -> PowerFlowResult:
    """`solve_power_flow` with the sparse route's workgroup size exposed (`threads`: 0 the library's choice, 64 or 256): what
    tools/powerflow_bench.py and the tests measure the two sizes with."""
    _check_plan_takes_the_lists(spec, edge_index, mode, route, plan)
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
        line_mask = unplaced = None
        if isinstance(plan, CoverPlan):
            # per-sample lists under one cover plan: the map launch lays the samples out in cover order, then the masked solve
            if edge_index.dim() != 3:
                raise RuntimeError("solve_power_flow: a CoverPlan goes with per-sample (S, 2, e) line lists; one (2, e) list takes a sparse_plan")
            if plan.cover.device != dev:
                raise RuntimeError(f"solve_power_flow: the plan lives on {plan.cover.device}, the inputs on {dev}")
            line_mask, rx, unplaced = cover_map(plan, edge_index, rx)
            edge_index, e, plan = plan.cover, plan.e_cover, plan.plan
        if plan is None:
            plan = sparse_plan(bt, edge_index, mode)
        if not isinstance(plan, SparsePlan) or (plan.n, plan.e, plan.mode) != (n, e, "fd" if fd else mode):
            raise RuntimeError(f"solve_power_flow: the plan is for (n, e, mode) = {(plan.n, plan.e, plan.mode) if isinstance(plan, SparsePlan) else plan!r}; "
                               f"the call has {(n, e, mode)}")
        if plan.blob.device != dev:
            raise RuntimeError(f"solve_power_flow: the plan lives on {plan.blob.device}, the inputs on {dev}")
        sizer, what = ((lib.pfn_powerflow_sparse_fd_workspace_bytes, "pfn_powerflow_solve_sparse_fd") if fd
                       else (lib.pfn_powerflow_sparse_workspace_bytes, "pfn_powerflow_solve_sparse"))
        masked = () if line_mask is None else (line_mask.data_ptr(), L.ptr(unplaced))
        if masked:
            what += "_masked"
        need = int(sizer(S, C.addressof(plan.header))) if S else 0
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            L.check(getattr(lib, what)(edge_index.data_ptr(), e, rx.data_ptr(), *masked, bt.data_ptr(), spec.data_ptr(), L.ptr(init), S, n,
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
