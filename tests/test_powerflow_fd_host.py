"""The float64 yardstick of the warm start and the fast-decoupled modes (tests/powerflow_fd_ref.py), without a GPU, on
`synth.make_physical_inputs`: both variants converge to Newton's solution in the half-iteration counts measured when this was
written (so a later change of the yardstick shows), the opposite update sign diverges, and a warm start at the solution takes no
iteration.  tests/test_gpu_powerflow_fd.py holds the kernel to this yardstick."""
import numpy as np
import pytest

from poweflownet_amd.synth import make_physical_inputs
from tests import powerflow_fd_ref as FD
from tests import powerflow_ref as P


def _inputs(n, e, S, seed=1, load=0.2):
    ei, bt, rx, spec = make_physical_inputs(n, e, S, seed, load)
    return ei.numpy(), bt.numpy(), rx.numpy(), spec.numpy()


# (n, e, S) -> variant -> (fewest, most) half-iterations over the samples: seed 1, tol 1e-8, fp32 solves of the two constant matrices
COUNTS = {(5, 6, 3): {"xb": (12, 13), "bx": (11, 16)},
          (14, 20, 16): {"xb": (12, 23), "bx": (11, 16)},
          (70, 100, 8): {"xb": (18, 25), "bx": (17, 19)},
          (118, 186, 8): {"xb": (17, 29), "bx": (15, 21)}}


@pytest.mark.parametrize("n,e,S", sorted(COUNTS))
def test_both_variants_converge_to_newtons_solution(n, e, S):
    ei, bt, rx, spec = _inputs(n, e, S)
    tol = 1e-8
    for variant in ("xb", "bx"):
        counts = []
        for s in range(S):
            want, st, _ = P.newton(bt, spec[s], ei, rx[s], tol=tol)
            assert 1 <= st <= 10
            got, status, res = FD.fast_decoupled(bt, spec[s], ei, rx[s], variant, tol=tol, max_iter=60, solve=FD.F32)
            assert status > 0 and res < tol, (variant, s, status, res)
            counts.append(status)
            # two points whose mismatch is under tol each are within 2 tol ||J^-1|| of each other, to first order
            bound = 2 * tol * P.jacobian_inverse_norm(want, bt, ei, rx[s])
            assert np.abs(got[:, 0] - want[:, 0]).max() <= bound and np.abs(got[:, 1] - want[:, 1]).max() * P.RAD <= bound
            dp, dq = P.mismatch(got, ei, rx[s])
            lim = tol + 64 * P.EPS64 * P.scale(got, ei, rx[s])
            assert (np.abs(dp) <= lim).all() and (np.abs(dq) <= lim).all()
            assert np.array_equal(got[bt != 2, 0], spec[s][bt != 2, 0]) and np.array_equal(got[bt == 2, 3], spec[s][bt == 2, 3])
        assert (min(counts), max(counts)) == COUNTS[(n, e, S)][variant], (variant, counts)


def test_the_matrices_are_the_two_laplacians():
    ei, bt, rx, _ = _inputs(14, 20, 1)
    ang, mag = P.unknowns(bt)
    bp_xb, bq_xb = FD.fd_matrices(bt, ei, rx[0], "xb")
    bp_bx, bq_bx = FD.fd_matrices(bt, ei, rx[0], "bx")
    assert bp_xb.shape == (13, 13) and bq_xb.shape == (len(mag),) * 2
    assert np.array_equal(bp_xb, P.dc_matrix(bt, ei, rx[0])[np.ix_(ang, ang)])          # XB's B' is the DC model's matrix
    sub = np.searchsorted(ang, mag)
    assert np.array_equal(bq_bx, bp_xb[np.ix_(sub, sub)])                                # BX's B'' is the same Laplacian on the PQ buses
    assert np.array_equal(bq_xb, bp_bx[np.ix_(sub, sub)])
    for B in (bp_xb, bq_xb, bp_bx, bq_bx):                                               # symmetric, diagonally dominant, positive
        assert np.array_equal(B, B.T) and (np.linalg.eigvalsh(B) > 0).all()
        assert (2 * np.diag(B) >= np.abs(B).sum(axis=1) * (1 - 1e-12)).all()
    # at the flat start B'' is minus d(sum Q) / d(Vm) with r = 0: b = -1 / x there
    rx0 = rx[0].copy()
    rx0[:, 0] = 0
    A = P.flow_jacobian(np.ones(14), np.zeros(14), bt, ei, rx0)
    assert np.allclose(-A[13:, 13:], FD.fd_matrices(bt, ei, rx0, "xb")[1], rtol=1e-12, atol=0)


def test_the_opposite_sign_diverges():
    for n, e in ((5, 6), (14, 20), (118, 186)):
        ei, bt, rx, spec = _inputs(n, e, 2)
        for variant in ("xb", "bx"):
            for s in range(2):
                table, status, res = FD.fast_decoupled(bt, spec[s], ei, rx[s], variant, tol=1e-8, max_iter=60, sign=+1.0)
                assert table is None and status in (-1, -3) and not res < 1e3, (n, variant, s, status, res)


def test_no_pq_bus_runs_the_p_half_only():
    ei, bt, rx, spec = _inputs(14, 20, 4, seed=2)
    spec, bt = spec.copy(), bt.copy()
    spec[:, bt == 2, 0] = 1.02
    bt[bt == 2] = 1
    for s in range(4):
        want, _, _ = P.newton(bt, spec[s], ei, rx[s], tol=1e-10)
        got, status, _ = FD.fast_decoupled(bt, spec[s], ei, rx[s], "xb", tol=1e-10, max_iter=60)
        assert 1 <= status <= 60
        assert np.abs(got[:, 1] - want[:, 1]).max() * P.RAD <= 2e-10 * P.jacobian_inverse_norm(want, bt, ei, rx[s])


def test_a_warm_start_at_the_solution_takes_no_iteration():
    ei, bt, rx, spec = _inputs(14, 20, 4)
    rng = np.random.default_rng(0)
    for s in range(4):
        want, cold, _ = P.newton(bt, spec[s], ei, rx[s], tol=1e-10)
        init = want[:, :2].copy()
        for fn in (FD.newton_from, lambda *a, **k: FD.fast_decoupled(*a, variant="xb", **k), lambda *a, **k: FD.fast_decoupled(*a, variant="bx", **k)):
            got, status, res = fn(bt, spec[s], ei, rx[s], init=init, tol=1e-9)
            assert status == 0 and res < 1e-9
            # finished from the start: what Newton wrote, up to the degree <-> radian round trip of Va
            assert np.array_equal(got[:, 0], want[:, 0]) and np.abs(got - want).max() <= 1e-12 * (1 + np.abs(want).max())
        # what is never read may hold anything
        junk = init.copy()
        junk[bt == 0] = np.nan
        junk[bt == 1, 0] = -7.0
        assert np.array_equal(FD.newton_from(bt, spec[s], ei, rx[s], init=junk, tol=1e-9)[0], FD.newton_from(bt, spec[s], ei, rx[s], init=init, tol=1e-9)[0])
        # a start near the solution needs no more solves than the flat start, and init = None IS the flat start
        near = init + rng.normal(size=init.shape) * np.array([1e-3, 1e-3 / P.RAD])
        assert 1 <= FD.newton_from(bt, spec[s], ei, rx[s], init=near, tol=1e-10)[1] <= cold
        flat, st, _ = FD.newton_from(bt, spec[s], ei, rx[s], tol=1e-10)
        assert st == cold and np.array_equal(flat, want)
