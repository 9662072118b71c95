"""numpy interpreter of the sparse power-flow plan (csrc/powerflow_plan.cpp, layout in csrc/powerflow_plan.hpp), written for the tests:
it parses the blob, assembles the Jacobian from tests/powerflow_ref.py's formulas AT THE PLANNED POSITIONS, and runs the elimination
and the substitutions the kernel runs (csrc/powerflow_sparse.hip) -- left-looking by columns without pivoting, forward and backward
substitution by columns -- with the factor's precision a parameter (float32: the kernel's split; float64: the plan's arithmetic alone).
One sample at a time.  `build_plan` goes through the library's host entry points and needs no GPU."""
import ctypes as C

import numpy as np

from tests import powerflow_ref as P

HEADER_WORDS = 32
MAGIC = 0x50465350
(H_MAGIC, H_VERSION, H_N, H_E, H_M, H_MODE, H_NNZ, H_NNZ_L, H_MADDS_LO, H_MADDS_HI, H_IDX16, H_MAX_COL, H_N_ADJ, H_BYTES,
 H_SLACK) = range(15)
(H_OFF_ORDER, H_OFF_UA, H_OFF_UV, H_OFF_COLPTR, H_OFF_DIAG, H_OFF_ROWIDX, H_OFF_ADJPTR, H_OFF_ADJ, H_OFF_ADJPOS,
 H_OFF_BUSPOS) = range(16, 26)
TINY_PIVOT = 1e-30


def build_plan(bus_type, edge_index, mode=0):
    """(rc, blob bytes or None, error text) from pfn_powerflow_sparse_plan on host arrays."""
    from poweflownet_amd import _lib as L
    lib = L.load()
    ei = np.ascontiguousarray(edge_index, dtype=np.int64)
    bt = np.ascontiguousarray(bus_type, dtype=np.int32)
    e, n = int(ei.shape[1]), int(bt.shape[0])
    need = int(lib.pfn_powerflow_sparse_plan_bytes(ei.ctypes.data, e, bt.ctypes.data, n, mode))
    if need == 0:
        return -1, None, lib.pfn_last_error().decode()
    buf = np.zeros(need, dtype=np.uint8)
    rc = int(lib.pfn_powerflow_sparse_plan(ei.ctypes.data, e, bt.ctypes.data, n, mode, buf.ctypes.data, need))
    return rc, (buf.tobytes() if rc == 0 else None), (lib.pfn_last_error().decode() if rc else "")


class Plan:
    """The sections of a blob as numpy arrays."""

    def __init__(self, blob):
        raw = np.frombuffer(blob, dtype=np.uint8)
        h = raw[:4 * HEADER_WORDS].view(np.int32)
        assert h[H_MAGIC] == MAGIC and h[H_VERSION] == 1 and h[H_BYTES] == len(blob)
        self.header = h
        self.n, self.e, self.m, self.mode = int(h[H_N]), int(h[H_E]), int(h[H_M]), int(h[H_MODE])
        self.nnz, self.nnz_l, self.max_col, self.slack = int(h[H_NNZ]), int(h[H_NNZ_L]), int(h[H_MAX_COL]), int(h[H_SLACK])
        self.madds = (int(h[H_MADDS_HI]) << 32) | (int(h[H_MADDS_LO]) & 0xffffffff)
        n_adj = int(h[H_N_ADJ])

        def words(off, count, dtype=np.int32):
            return raw[int(h[off]):int(h[off]) + count * np.dtype(dtype).itemsize].view(dtype)
        self.order = words(H_OFF_ORDER, self.n - 1)
        self.ua, self.uv = words(H_OFF_UA, self.n), words(H_OFF_UV, self.n)
        self.colptr, self.diag = words(H_OFF_COLPTR, self.m + 1), words(H_OFF_DIAG, self.m)
        self.rowidx = words(H_OFF_ROWIDX, self.nnz, np.uint16 if h[H_IDX16] else np.int32).astype(np.int64)
        self.adjptr = words(H_OFF_ADJPTR, self.n + 1)
        self.adj = words(H_OFF_ADJ, 2 * n_adj).reshape(n_adj, 2)
        self.adjpos = words(H_OFF_ADJPOS, 4 * n_adj).reshape(n_adj, 4)
        self.buspos = words(H_OFF_BUSPOS, 4 * self.n).reshape(self.n, 4)
        self.col_of = np.repeat(np.arange(self.m), np.diff(self.colptr))       # column of every slab position

    def pattern(self):
        """The set of (row, column) pairs of the filled pattern."""
        return set(zip(self.rowidx.tolist(), self.col_of.tolist()))

    def to_solver_order(self, bus_type):
        """perm with x_solver = x_plan[perm]: tests/powerflow_ref.py's unknown order (thetas in bus order, then Vm in bus order)."""
        ang, mag = P.unknowns(bus_type)
        return np.concatenate([self.ua[ang], self.uv[mag]]) if self.mode == 0 else self.ua[ang]


def assemble(plan, vm, th, edge_index, rx, dtype=np.float32):
    """(slab [nnz] of `dtype`, F [m] float64 in plan order, line sums sp, sq): each Jacobian entry rounded to `dtype` and added at
    its planned position in the kernel's order -- bus by bus, line ends in stored order, the diagonal block (fp64 sums) last."""
    ei = np.asarray(edge_index)
    g, b = P.admittance(rx)
    x = np.asarray(rx, dtype=np.float64)[:, 1]
    slab = np.zeros(plan.nnz, dtype=dtype)
    sp, sq = np.zeros(plan.n), np.zeros(plan.n)
    dc = plan.mode == 1

    def add(pos, val):
        if pos >= 0:
            slab[pos] += dtype(val)
    for i in range(plan.n):
        vi, ti = vm[i], th[i]
        dPt = dPv = dQt = dQv = 0.0
        for q in range(plan.adjptr[i], plan.adjptr[i + 1]):
            k, j = int(plan.adj[q, 0]) >> 1, int(plan.adj[q, 1])
            side = int(plan.adj[q, 0]) & 1
            assert ei[side, k] == i and ei[1 - side, k] == j
            pos = plan.adjpos[q]
            if dc:
                bb = -1.0 / x[k]
                sp[i] += bb * (ti - th[j])
                dPt += bb
                add(pos[0], -bb)
                continue
            vj = vm[j]
            vv, c, s = vi * vj, np.cos(ti - th[j]), np.sin(ti - th[j])
            t1, t2 = vv * c - vi * vi, vv * s
            sp[i] += g[k] * t1 + b[k] * t2
            sq[i] += g[k] * t2 - b[k] * t1
            pti, qti = vv * (b[k] * c - g[k] * s), vv * (g[k] * c + b[k] * s)
            dPt += pti
            dPv += g[k] * (vj * c - 2 * vi) + b[k] * vj * s
            dQt += qti
            dQv += g[k] * vj * s - b[k] * (vj * c - 2 * vi)
            add(pos[0], -pti)
            add(pos[1], vi * (g[k] * c + b[k] * s))
            add(pos[2], -qti)
            add(pos[3], vi * (g[k] * s - b[k] * c))
        bp = plan.buspos[i]
        add(bp[0], dPt)
        add(bp[1], dPv)
        add(bp[2], dQt)
        add(bp[3], dQv)
    return slab, sp, sq


def factor(plan, slab):
    """In place: column j scattered into a dense work vector, U_kj final for k ascending, w[rows of L(:, k)] -= L(:, k) U_kj, the pivot
    test, the L part times 1 / pivot.  False at a pivot that is tiny or NaN."""
    dtype = slab.dtype.type
    w = np.zeros(plan.m, dtype=slab.dtype)
    cp, dg, rows = plan.colptr, plan.diag, plan.rowidx
    for j in range(plan.m):
        c0, d, c1 = cp[j], dg[j], cp[j + 1]
        w[rows[c0:c1]] = slab[c0:c1]
        for p in range(c0, d):
            k = rows[p]
            lb, le = dg[k] + 1, cp[k + 1]
            w[rows[lb:le]] -= slab[lb:le] * w[k]
        piv = w[j]
        if not abs(piv) > TINY_PIVOT:
            return False
        col = w[rows[c0:c1]]
        col[d - c0 + 1:] *= dtype(1) / piv
        slab[c0:c1] = col
    return True


def substitute(plan, slab, F):
    """dx (plan order) from the factor and the float64 right-hand side, by columns."""
    F = np.array(F, dtype=np.float64)
    cp, dg, rows = plan.colptr, plan.diag, plan.rowidx
    for j in range(plan.m):
        lb, le = dg[j] + 1, cp[j + 1]
        F[rows[lb:le]] -= slab[lb:le].astype(np.float64) * F[j]
    for j in range(plan.m - 1, -1, -1):
        ub, ue = cp[j], dg[j]
        if ub < ue:
            F[rows[ub:ue]] -= slab[ub:ue].astype(np.float64) * (F[j] / np.float64(slab[ue]))
    return F / slab[dg].astype(np.float64)


def newton(plan, bus_type, spec, edge_index, rx, tol=1e-10, max_iter=10, dtype=np.float32, steps=None):
    """The kernel's loop on the host.  (table or None, status, residual); `steps`: a list that receives (vm, th, F, dx) per solve, F and dx in
    tests/powerflow_ref.py's unknown order."""
    bt, sp_ = np.asarray(bus_type), np.asarray(spec, dtype=np.float64)
    vm, th, _ = P.flat_start(bt, sp_)
    dc = plan.mode == 1
    perm = plan.to_solver_order(bt)
    for it in range(max_iter + 1):
        slab, lp, lq = assemble(plan, vm, th, edge_index, rx, dtype)
        F = np.zeros(plan.m)
        on = plan.ua >= 0
        F[plan.ua[on]] = sp_[on, 2] - lp[on]
        on = plan.uv >= 0
        F[plan.uv[on]] = sp_[on, 3] - lq[on]
        if not np.isfinite(F).all():
            return None, -3, np.nan
        res = float(np.abs(F).max()) if F.size else 0.0
        if res < tol:
            t = np.stack([vm, th / P.RAD, sp_[:, 2], sp_[:, 3]], axis=1)
            t[bt == 0, 1] = sp_[bt == 0, 1]
            t[bt == 0, 2] = lp[bt == 0]
            if dc:
                t[:, 3] = np.nan
            else:
                t[bt != 2, 3] = lq[bt != 2]
            return t, it, res
        if it == max_iter:
            return None, -1, res
        if not factor(plan, slab):
            return None, -2, res
        dx = substitute(plan, slab, F)
        if steps is not None:
            steps.append((vm.copy(), th.copy(), F[perm], dx[perm]))
        on = plan.ua >= 0
        th[on] += dx[plan.ua[on]]
        on = plan.uv >= 0
        vm[on] += dx[plan.uv[on]]
    raise AssertionError
