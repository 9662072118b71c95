"""numpy interpreter of the fast-decoupled sparse plan (csrc/powerflow_plan.cpp pfn_powerflow_sparse_fd_plan, layout in
csrc/powerflow_plan.hpp), written for the tests in the style of tests/powerflow_sparse_ref.py: it parses the outer header and the two
embedded sub-plans, assembles B' and B'' from tests/powerflow_fd_ref.py's weights AT THE PLANNED POSITIONS in the kernel's order (bus
by bus, line ends in stored order, the fp64 diagonal sum last), factors each once with powerflow_sparse_ref.factor -- the factor's
precision a parameter: float32 is the kernel's split (csrc/powerflow_sparse_fd.hip), float64 the plan's arithmetic alone -- and runs
the half-iteration loop of powerflow_fd_ref.fast_decoupled around fp64 substitutions through the two factors.  One sample at a time.
`build_plan` goes through the library's host entry points and needs no GPU."""
import numpy as np

from tests import powerflow_fd_ref as FD
from tests import powerflow_ref as P
from tests import powerflow_sparse_ref as SP

MAGIC = 0x44465350
MODE = 2
H_M_Q, H_OFF_P, H_OFF_Q = 15, 16, 17


def build_plan(bus_type, edge_index):
    """(rc, blob bytes or None, error text) from pfn_powerflow_sparse_fd_plan on host arrays."""
    from poweflownet_amd import _lib as L
    lib = L.load()
    ei = np.ascontiguousarray(edge_index, dtype=np.int64)
    bt = np.ascontiguousarray(bus_type, dtype=np.int32)
    e, n = int(ei.shape[1]), int(bt.shape[0])
    need = int(lib.pfn_powerflow_sparse_fd_plan_bytes(ei.ctypes.data, e, bt.ctypes.data, n))
    if need == 0:
        return -1, None, lib.pfn_last_error().decode()
    buf = np.zeros(need, dtype=np.uint8)
    rc = int(lib.pfn_powerflow_sparse_fd_plan(ei.ctypes.data, e, bt.ctypes.data, n, buf.ctypes.data, need))
    return rc, (buf.tobytes() if rc == 0 else None), (lib.pfn_last_error().decode() if rc else "")


class Half:
    """One embedded sub-plan: a plan of one unknown per bus; `order` has m entries (powerflow_sparse_ref.Plan reads n - 1)."""

    def __init__(self, blob):
        raw = np.frombuffer(blob, dtype=np.uint8)
        h = raw[:4 * SP.HEADER_WORDS].view(np.int32)
        assert h[SP.H_MAGIC] == SP.MAGIC and h[SP.H_VERSION] == 1 and h[SP.H_MODE] == 1 and h[SP.H_BYTES] == len(blob)
        self.header = h
        self.n, self.e, self.m, self.mode = int(h[SP.H_N]), int(h[SP.H_E]), int(h[SP.H_M]), 1
        self.nnz, self.nnz_l, self.max_col, self.slack = int(h[SP.H_NNZ]), int(h[SP.H_NNZ_L]), int(h[SP.H_MAX_COL]), int(h[SP.H_SLACK])
        self.madds = (int(h[SP.H_MADDS_HI]) << 32) | (int(h[SP.H_MADDS_LO]) & 0xffffffff)
        n_adj = int(h[SP.H_N_ADJ])

        def words(off, count, dtype=np.int32):
            return raw[int(h[off]):int(h[off]) + count * np.dtype(dtype).itemsize].view(dtype)
        self.order = words(SP.H_OFF_ORDER, self.m)
        self.ua, self.uv = words(SP.H_OFF_UA, self.n), words(SP.H_OFF_UV, self.n)
        self.colptr, self.diag = words(SP.H_OFF_COLPTR, self.m + 1), words(SP.H_OFF_DIAG, self.m)
        self.rowidx = words(SP.H_OFF_ROWIDX, self.nnz, np.uint16 if h[SP.H_IDX16] else np.int32).astype(np.int64)
        self.adjptr = words(SP.H_OFF_ADJPTR, self.n + 1)
        self.adj = words(SP.H_OFF_ADJ, 2 * n_adj).reshape(n_adj, 2)
        self.adjpos = words(SP.H_OFF_ADJPOS, 4 * n_adj).reshape(n_adj, 4)
        self.buspos = words(SP.H_OFF_BUSPOS, 4 * self.n).reshape(self.n, 4)
        self.col_of = np.repeat(np.arange(self.m), np.diff(self.colptr))

    def pattern(self):
        return set(zip(self.rowidx.tolist(), self.col_of.tolist()))


class Plan:
    """The outer header and the two halves of a blob."""

    def __init__(self, blob):
        h = np.frombuffer(blob, dtype=np.uint8)[:4 * SP.HEADER_WORDS].view(np.int32)
        assert h[SP.H_MAGIC] == MAGIC and h[SP.H_VERSION] == 1 and h[SP.H_MODE] == MODE and h[SP.H_BYTES] == len(blob)
        self.header = h
        self.n, self.e, self.m_p, self.m_q = int(h[SP.H_N]), int(h[SP.H_E]), int(h[SP.H_M]), int(h[H_M_Q])
        self.nnz, self.nnz_l, self.max_col, self.slack = int(h[SP.H_NNZ]), int(h[SP.H_NNZ_L]), int(h[SP.H_MAX_COL]), int(h[SP.H_SLACK])
        self.madds = (int(h[SP.H_MADDS_HI]) << 32) | (int(h[SP.H_MADDS_LO]) & 0xffffffff)
        off_p, off_q = int(h[H_OFF_P]), int(h[H_OFF_Q])
        assert off_p == 4 * SP.HEADER_WORDS and off_p < off_q < len(blob) and off_p % 16 == 0 and off_q % 16 == 0
        bytes_p = int(np.frombuffer(blob, dtype=np.int32, count=SP.HEADER_WORDS, offset=off_p)[SP.H_BYTES])
        bytes_q = int(np.frombuffer(blob, dtype=np.int32, count=SP.HEADER_WORDS, offset=off_q)[SP.H_BYTES])
        assert off_p + bytes_p <= off_q and off_q + bytes_q == len(blob)
        self.blob_p, self.blob_q = blob[off_p:off_p + bytes_p], blob[off_q:off_q + bytes_q]
        self.P, self.Q = Half(self.blob_p), Half(self.blob_q)


def weights(rx, variant):
    """(w', w'') per line: powerflow_fd_ref.fd_matrices' weights."""
    assert variant in ("xb", "bx")
    rx = np.asarray(rx, dtype=np.float64)
    r, x = rx[:, 0], rx[:, 1]
    w_x, w_b = 1.0 / x, x / (r * r + x * x)
    return (w_x, w_b) if variant == "xb" else (w_b, w_x)


def assemble(half, w, dtype=np.float32):
    """The slab of the Laplacian of line weights `w` restricted to the half's unknowns: bus i's owner adds -w at the planned
    off-diagonal position of every line end (rounded to `dtype`, stored order), then the fp64 sum of its weights at its diagonal."""
    slab = np.zeros(half.nnz, dtype=dtype)
    for i in range(half.n):
        d = 0.0
        for q in range(half.adjptr[i], half.adjptr[i + 1]):
            k = int(half.adj[q, 0]) >> 1
            d += w[k]
            if half.adjpos[q, 0] >= 0:
                slab[half.adjpos[q, 0]] += dtype(-w[k])
        if half.buspos[i, 0] >= 0:
            slab[half.buspos[i, 0]] += dtype(d)
    return slab


def dense(half, slab):
    """The assembled slab as a dense matrix in the half's unknown order (before `factor`)."""
    A = np.zeros((half.m, half.m))
    A[half.rowidx, half.col_of] = slab
    return A


def fast_decoupled(plan, bus_type, spec, edge_index, rx, variant="xb", init=None, tol=1e-10, max_iter=60, dtype=np.float32):
    """The kernel's loop on the host: (table or None, status, residual), status as powerflow_fd_ref.fast_decoupled's."""
    bt, sp = np.asarray(bus_type), np.asarray(spec, dtype=np.float64)
    vm, th = FD.start(bt, sp, init)
    wp, wq = weights(rx, variant)
    slab_p, slab_q = assemble(plan.P, wp, dtype), assemble(plan.Q, wq, dtype)
    if not (SP.factor(plan.P, slab_p) and SP.factor(plan.Q, slab_q)):
        return None, -2, np.nan
    on_p, on_q = plan.P.ua >= 0, plan.Q.ua >= 0
    half = 0
    for it in range(max_iter + 1):
        dp, dq, F = FD._mismatch(vm, th, bt, sp, edge_index, rx)
        if not np.isfinite(F).all():
            return None, -3, np.nan
        res = float(np.abs(F).max()) if F.size else 0.0
        if res < tol:
            return P.finish_table(vm, th, bt, sp, edge_index, rx), it, res
        if it == max_iter:
            return None, -1, res
        if half == 0:
            rhs = np.zeros(plan.m_p)
            rhs[plan.P.ua[on_p]] = dp[on_p] / vm[on_p]
            th[on_p] -= SP.substitute(plan.P, slab_p, rhs)[plan.P.ua[on_p]]
        else:
            rhs = np.zeros(plan.m_q)
            rhs[plan.Q.ua[on_q]] = dq[on_q] / vm[on_q]
            vm[on_q] -= SP.substitute(plan.Q, slab_q, rhs)[plan.Q.ua[on_q]]
        half = (1 - half) if plan.m_q else 0
    raise AssertionError


def variant_grid(ei, bt, rx, spec, kind):
    """The degenerate grids the host and the device tests share, from one sample of `make_physical_inputs` (numpy; rx [e, 2] or
    [S, e, 2], spec [n, 4] or [S, n, 4]): "no_pv" every PV bus made PQ; "no_pq" every PQ bus made PV at Vm 1.02 (B'' is empty);
    "parallel" three lines stored twice and two more stored again backwards; "lone_pq" the neighbours of the PQ bus of lowest degree
    made PV at Vm 1.0, so that its only neighbours are the slack and PV buses: a 1 x 1 column of B'' with no L part."""
    ei, bt, rx, spec = np.array(ei), np.array(bt), np.array(rx), np.array(spec)
    if kind == "no_pv":
        bt[bt == 1] = 2
    elif kind == "no_pq":
        spec[..., bt == 2, 0] = 1.02
        bt[bt == 2] = 1
    elif kind == "parallel":
        ei = np.concatenate([ei, ei[:, :3], ei[::-1, 3:5]], axis=1)
        rx = np.concatenate([rx, rx[..., :3, :], rx[..., 3:5, :]], axis=-2)
    elif kind == "lone_pq":
        degree = np.bincount(ei.ravel(), minlength=len(bt))
        pq = np.flatnonzero(bt == 2)
        lone = int(pq[np.argmin(degree[pq])])
        near = np.unique(np.concatenate([ei[1, ei[0] == lone], ei[0, ei[1] == lone]]))
        near = near[(bt[near] == 2) & (near != lone)]
        spec[..., near, 0] = 1.0
        bt[near] = 1
    else:
        assert kind is None, kind
    return ei, bt, rx, spec
