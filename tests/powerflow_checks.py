"""What the GPU power-flow tests (test_gpu_powerflow*.py) share: the upload, the bounds of DESIGN 7h on a written table -- each against
the float64 yardstick of tests/powerflow_ref.py -- and the capture of a command-line tool's output.  A `case` is any object with the
host arrays `ei` [2, e], `bt` [n], `rx` [S, e, 2] and `spec` [S, n, 4]; the `_Case` classes stay with their tests (they differ in
yardstick, plans and grid variants)."""
import contextlib
import io

import numpy as np
import torch

from tests import branch_ref as R
from tests import powerflow_ref as P

DEV = "cuda:0"
TOL = 1e-10


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _residual_ratio(case, table, tol=TOL):
    """worst over samples and buses of the yardstick's mismatch of the WRITTEN table over tol + 64 * 2^-52 * scale_i: the kernel
    stopped under tol in its own fp64, the rest is the rounding of evaluating the sums again"""
    worst = 0.0
    for s in range(table.shape[0]):
        dp, dq = P.mismatch(table[s], case.ei, case.rx[s])
        bound = tol + 64 * P.EPS64 * P.scale(table[s], case.ei, case.rx[s])
        worst = max(worst, float((np.maximum(np.abs(dp), np.abs(dq)) / bound).max()))
    return worst


def _distance(a, b):
    """max over buses of |dVm| and |dVa| in radians"""
    return max(np.abs(a[:, 0] - b[:, 0]).max(), np.abs(a[:, 1] - b[:, 1]).max() * P.RAD)


def _check_given(case, table):
    """what is given comes back as given, bit for bit"""
    for s in range(table.shape[0]):
        assert np.array_equal(table[s][case.bt != 2, 0], case.spec[s][case.bt != 2, 0]) and np.array_equal(table[s][case.bt != 0, 2], case.spec[s][case.bt != 0, 2])
        assert np.array_equal(table[s][case.bt == 2, 3], case.spec[s][case.bt == 2, 3]) and np.array_equal(table[s][case.bt == 0, 1], case.spec[s][case.bt == 0, 1])


def _imbalance_bound(table32, ei, rx):
    """mean over (sample, bus) of 2 (C_BOUND EPS sum of the per-line scales at the bus + EPS (|P_i| + |Q_i|))^2: every line message
    the physics kernel forms in fp32 is within C_BOUND EPS scale of its exact value (tests/branch_ref.py: the bound the branch-flow
    kernel is held to for the same expressions), P_i and Q_i carry their own fp32 rounding, and dP^2 + dQ^2 has two such terms."""
    S, n = table32.shape[:2]
    _, scales = R.flows(table32, ei, rx)                                       # [S, e, 4]; column 1 = the P / Q scale of the line
    at_bus = np.zeros((S, n))
    for s in range(S):
        np.add.at(at_bus[s], ei[0], scales[s, :, 1])
        np.add.at(at_bus[s], ei[1], scales[s, :, 1])
    t = table32.astype(np.float64)
    return float(np.mean(2 * (R.C_BOUND * R.EPS * at_bus + R.EPS * (np.abs(t[:, :, 2]) + np.abs(t[:, :, 3]))) ** 2))


def _run(main, argv):
    """main(argv) must return 0; what it printed"""
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert main(list(argv)) == 0
    return out.getvalue()
