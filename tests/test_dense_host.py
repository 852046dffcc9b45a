"""Dense output on the host: the n x n bridge algebra (`pnmol.base.iwp.bridge_coefficients`) by itself, and the bridge
formulas of DESIGN.md section 14 against the textbook route (tests/dense_reference.py: insert t as a grid point, predict,
one more RTS step) on the oracle's trajectories.  No GPU."""

import numpy as np
import pytest
import scipy.linalg

from dense_reference import augment, bridge_on_oracle, rts_over, smoothed_dense
from helpers import make_pair
from pnmol.base.iwp import _partial_interval, bridge_coefficients
from smooth_reference import rts_on_oracle

THETAS = (0.03, 0.25, 0.5, 0.8, 0.97)


@pytest.mark.parametrize("nu", [1, 2, 3])
def test_chapman_kolmogorov_in_the_frame_of_the_whole_step(nu):
    Q1 = np.flip(scipy.linalg.hilbert(nu + 1))
    A1 = np.flip(scipy.linalg.pascal(nu + 1, kind="lower", exact=False))
    for th in THETAS + (1e-3, 1 - 1e-3):
        A_th, Q_th = _partial_interval(th, nu)
        A_c, Q_c = _partial_interval(1.0 - th, nu)
        np.testing.assert_allclose(A_c @ A_th, A1, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(A_c @ Q_th @ A_c.T + Q_c, Q1, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("nu", [1, 2, 3])
def test_bridge_coefficients_limits_and_shape(nu):
    n, I = nu + 1, np.eye(nu + 1)
    for th in THETAS:
        Bm, Bp, Qb = bridge_coefficients(th, nu)
        assert Bm.shape == Bp.shape == Qb.shape == (n, n)
        assert np.array_equal(Qb, Qb.T)
        assert np.linalg.eigvalsh(Qb).min() >= -1e-15 * np.abs(Qb).max()
        # the bridge reproduces the prior: E[x_t | x_l] = A_th x_l when x_r = A1 x_l (no information from the right)
        A1 = np.flip(scipy.linalg.pascal(n, kind="lower", exact=False))
        np.testing.assert_allclose(Bm + Bp @ A1, _partial_interval(th, nu)[0], rtol=1e-10, atol=1e-12)
    Bm, Bp, Qb = bridge_coefficients(1e-12, nu)
    assert all(np.all(np.isfinite(X)) for X in (Bm, Bp, Qb))
    np.testing.assert_allclose(Bm, I, atol=1e-9)
    np.testing.assert_allclose(Bp, 0 * I, atol=1e-9)
    np.testing.assert_allclose(Qb, 0 * I, atol=1e-9)
    Bm, Bp, Qb = bridge_coefficients(1 - 1e-12, nu)
    assert all(np.all(np.isfinite(X)) for X in (Bm, Bp, Qb))
    np.testing.assert_allclose(Bm, 0 * I, atol=1e-9)
    np.testing.assert_allclose(Bp, I, atol=1e-9)
    np.testing.assert_allclose(Qb, 0 * I, atol=1e-9)
    for bad in (0.0, 1.0, -0.1, 1.5, np.nan):
        with pytest.raises(ValueError):
            bridge_coefficients(bad, nu)


def test_bridge_variance_vanishes_like_the_prior_at_both_ends():
    """The highest derivative is a Brownian motion: given both neighbouring STATES it is known at least as well as a Brownian
    bridge between its two end values, theta (1 - theta), and no variance is ever negative."""
    for nu in (1, 2, 3):
        for th in (1e-6, 1e-3, 1 - 1e-3, 1 - 1e-6):
            Qb = bridge_coefficients(th, nu)[2]
            assert np.all(np.diag(Qb) >= 0.0)
            assert 0.0 < Qb[nu, nu] <= th * (1 - th) * (1 + 1e-9)


@pytest.mark.parametrize("N", [16, 32])
@pytest.mark.parametrize("nu", [1, 2, 3])
@pytest.mark.parametrize("bcond", ["dirichlet", "neumann"])
def test_bridge_formulas_equal_inserting_the_time_as_a_grid_point(N, nu, bcond):
    """Bounds: ten times the figures by which the two NumPy routes differ on these cases, the accuracy table of DESIGN.md section 14
    (solution itself: mean <= 3.4e-13, std <= 2.5e-10 at nu <= 2, 1e-5 at the two noise-free Dirichlet nodes at nu = 3 and 1.6e-9
    with Neumann conditions; covariance <= 6.5e-12 at nu <= 2 and 3.7e-6 at nu = 3, where the raw-coordinate insertion loses
    digits).  The means of the higher derivatives are held to 1e-6 of their largest entry, a tenth of the package's mean tolerance
    (1e-5); the two routes differ by 5.6e-11 there at nu = 2 and 7.8e-8 at nu = 3."""
    K = 12
    _, _, opde, osolver = make_pair(N, nu, 2.0 ** -7, K, bcond)
    osol = osolver.solve(opde)
    for k in (0, K // 2, K - 1):
        h = osol.t[k + 1] - osol.t[k]
        ts = [osol.t[k] + th * h for th in THETAS]
        rm, rs, rP = smoothed_dense(osolver, osol, ts)
        for i, th in enumerate(THETAS):
            m, P = bridge_on_oracle(osolver, osol, k, th, bridge_coefficients)
            s = np.sqrt(np.maximum(np.diag(P), 0.0)).reshape(m.shape, order="F")
            np.testing.assert_allclose(m[0], rm[i][0], rtol=0, atol=4e-12 * np.abs(rm[i][0]).max())
            for a in range(1, nu + 1):      # (the insertion in raw coordinates loses digits in the high derivatives: 8e-8 seen)
                np.testing.assert_allclose(m[a], rm[i][a], rtol=0, atol=1e-6 * np.abs(rm[i][a]).max())
            np.testing.assert_allclose(P, rP[i], rtol=0, atol=(4e-5 if nu == 3 else 6e-11) * np.abs(rP[i]).max())
            tol_s = 3e-9 if nu < 3 else (1e-4 if bcond == "dirichlet" else 2e-8)
            np.testing.assert_allclose(s[0], rs[i][0], rtol=0, atol=tol_s * rs[i][0].max())


def test_reference_inserts_every_query_and_leaves_the_grid_alone():
    """The augmented grid: grid points keep their smoothed values whatever is inserted; two times inside one interval and a time
    past tmax are handled; a grid time maps to the grid point."""
    _, _, opde, osolver = make_pair(12, 2, 2.0 ** -6, 4, "neumann")
    osol = osolver.solve(opde)
    t = osol.t
    ts = [t[1] + 0.7 * (t[2] - t[1]), t[1] + 0.2 * (t[2] - t[1]), t[3], t[-1] + 0.01, t[0] + 1e-3]
    aug = augment(osolver, osol, ts)
    assert np.all(np.diff(aug.t) > 0) and len(aug.t) == len(t) + 4
    assert [aug.t[i] for i in aug.where] == ts
    ms, Ps = rts_over(osolver, aug)
    gm, gP = rts_on_oracle(osolver, osol)
    # (the terminal state of the augmented pass is the prediction past tmax; its information about earlier times is nil)
    for k in range(len(t)):
        i = int(np.flatnonzero(aug.t == t[k])[0])
        np.testing.assert_allclose(ms[i].reshape(gm[k].shape, order="F"), gm[k], rtol=1e-8, atol=1e-10 * np.abs(gm).max())
        np.testing.assert_allclose(Ps[i], gP[k], rtol=1e-6, atol=1e-9 * np.abs(gP[k]).max())
    with pytest.raises(ValueError):
        augment(osolver, osol, [t[0] - 1e-3])
    # one query at a time, the pass over the augmented grid is what `smoothed_dense` computes
    for tq in ts:
        one = augment(osolver, osol, [tq])
        ms, Ps = rts_over(osolver, one)
        rm, rs, rP = smoothed_dense(osolver, osol, [tq])
        i = one.where[0]
        np.testing.assert_allclose(ms[i].reshape(rm[0].shape, order="F"), rm[0], rtol=1e-10, atol=1e-12 * np.abs(rm[0]).max())
        np.testing.assert_allclose(Ps[i], rP[0], rtol=1e-8, atol=1e-11 * np.abs(rP[0]).max())
