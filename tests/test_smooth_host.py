"""The NumPy RTS smoother the GPU smoother is checked against (tests/smooth_reference.py), pinned on the CPU: against the
reference's square-root smoother step (kalman.py:48-66, restated with a NumPy QR) and against joint Gaussian conditioning
of a whole short trajectory.  Also the import surface of `pnmol.base.kalman`."""

import numpy as np
import pytest
import scipy.linalg

import pnmol_oracle as oracle
from helpers import make_pair
from smooth_reference import rts_on_oracle, rts_step


def _qr_form_step(m, sc, m_fut, sc_fut, A, Ql):
    """kalman.py:48-66 restated: gain from the covariance form, covariance factor from the QR of the (3D, 2D) block."""
    P = sc @ sc.T
    P_pred = A @ P @ A.T + Ql @ Ql.T
    sgain = scipy.linalg.cho_solve(scipy.linalg.cho_factor(P_pred, lower=True), A @ P).T
    new_mean = m - sgain @ (A @ m - m_fut)
    D = m.shape[0]
    Z = np.zeros((D, D))
    M = np.block([[(A @ sc).T, sc.T], [Ql.T, Z], [Z, sc_fut.T @ sgain.T]])
    R = scipy.linalg.qr(M, mode="r")[0]
    C = R[D:2 * D, D:].T
    return new_mean, C @ C.T


def test_numpy_rts_step_equals_the_qr_form_on_random_inputs():
    rng = np.random.default_rng(3)
    for D in (3, 8, 13):
        A = rng.standard_normal((D, D))
        Ql = np.tril(rng.standard_normal((D, D))) + 2 * np.eye(D)
        sc, sc_fut = np.tril(rng.standard_normal((D, D))), np.tril(rng.standard_normal((D, D)))
        m, m_fut = rng.standard_normal(D), rng.standard_normal(D)
        I = np.eye(D)
        ms, Ps = rts_step(m, sc @ sc.T, m_fut, sc_fut @ sc_fut.T, A, Ql @ Ql.T, I, I)
        mq, Pq = _qr_form_step(m, sc, m_fut, sc_fut, A, Ql)
        np.testing.assert_allclose(ms, mq, rtol=1e-10, atol=1e-10 * np.abs(mq).max())
        np.testing.assert_allclose(Ps, Pq, rtol=1e-9, atol=1e-10 * np.abs(Pq).max())


@pytest.mark.parametrize("bcond", ["dirichlet", "neumann"])
def test_numpy_rts_step_equals_the_qr_form_on_filter_states(bcond):
    """Filter-derived inputs (oracle trajectory, Nordsieck frame of the step; a noise-free Dirichlet node makes P_k singular)."""
    _, _, opde, osolver = make_pair(10, 2, 2.0 ** -6, 3, bcond)
    osol = osolver.solve(opde)
    A, Ql = osolver.iwp.preconditioned_discretize
    for k in range(len(osol.t) - 1):
        Pc, Pcinv = osolver.iwp.nordsieck_preconditioner(osol.t[k + 1] - osol.t[k])
        m, sc = Pcinv @ osol.mean[k].reshape(-1, order="F"), Pcinv @ osol.cov_sqrtm[k]
        m_fut, sc_fut = Pcinv @ osol.mean[k + 1].reshape(-1, order="F"), Pcinv @ osol.cov_sqrtm[k + 1]
        I = np.eye(m.shape[0])
        ms, Ps = rts_step(m, sc @ sc.T, m_fut, sc_fut @ sc_fut.T, A, Ql @ Ql.T, I, I)
        mq, Pq = _qr_form_step(m, sc, m_fut, sc_fut, A, Ql)
        np.testing.assert_allclose(ms, mq, rtol=1e-9, atol=1e-11 * np.abs(mq).max())
        np.testing.assert_allclose(Ps, Pq, rtol=1e-7, atol=1e-11 * np.abs(Pq).max())


def test_numpy_rts_equals_joint_gaussian_conditioning():
    """x_0 ~ the filter's initial posterior, x_{k+1} = Phi x_k + w_k, observations H x_k = 0 (noise R) at k = 1..T:
    the posterior marginals of the joint Gaussian equal the RTS pass over the filter's trajectory."""
    _, _, opde, osolver = make_pair(6, 1, 0.05, 3, "neumann")
    osol = osolver.solve(opde)
    ms, Ps = rts_on_oracle(osolver, osol)
    n, d = osol.mean.shape[1:]
    D, T = n * d, len(osol.t) - 1
    E0, E1 = osolver.E0, osolver.E1
    H = np.vstack((E1 - opde.L @ E0, opde.B @ E0))
    E = scipy.linalg.block_diag(opde.E_sqrtm, opde.R_sqrtm)
    R = E @ E.T
    # joint prior of (x_0 .. x_T)
    mu = np.zeros((T + 1) * D)
    Sig = np.zeros(((T + 1) * D, (T + 1) * D))
    mu[:D] = osol.mean[0].reshape(-1, order="F")
    Sig[:D, :D] = osol.cov_sqrtm[0] @ osol.cov_sqrtm[0].T
    for k in range(T):
        Phi, Ql = osolver.iwp.non_preconditioned_discretize(osol.t[k + 1] - osol.t[k])
        a, b = slice(k * D, (k + 1) * D), slice((k + 1) * D, (k + 2) * D)
        mu[b] = Phi @ mu[a]
        Sig[b, :(k + 1) * D] = Phi @ Sig[a, :(k + 1) * D]
        Sig[:(k + 1) * D, b] = Sig[b, :(k + 1) * D].T
        Sig[b, b] = Phi @ Sig[a, a] @ Phi.T + Ql @ Ql.T
    m = H.shape[0]
    HH = np.zeros((T * m, (T + 1) * D))
    for k in range(1, T + 1):
        HH[(k - 1) * m:k * m, k * D:(k + 1) * D] = H
    S = HH @ Sig @ HH.T + np.kron(np.eye(T), R)
    assert np.linalg.cond(S) < 1e12
    K = scipy.linalg.solve(S, HH @ Sig, assume_a="pos").T
    mu_post = mu - K @ (HH @ mu)
    Sig_post = Sig - K @ HH @ Sig
    for k in range(T + 1):
        sl = slice(k * D, (k + 1) * D)
        np.testing.assert_allclose(ms[k].reshape(-1, order="F"), mu_post[sl], rtol=1e-6, atol=1e-8 * np.abs(mu_post).max())
        np.testing.assert_allclose(Ps[k], Sig_post[sl, sl], rtol=1e-5, atol=1e-8 * np.abs(np.diag(Sig_post)).max())


def test_kalman_module_exposes_the_reference_names():
    from pnmol.base import kalman

    for name in ("filter_step", "smoother_step_traditional", "smoother_step_sqrt"):
        assert callable(getattr(kalman, name))
    import pnmol.base

    assert pnmol.base.kalman is kalman


def test_smooth_is_part_of_the_white_noise_solvers():
    import pnmol

    assert callable(pnmol.white.LinearWhiteNoiseEK1.smooth) and callable(pnmol.white.SemiLinearWhiteNoiseEK1.smooth)
    assert "pnmol_smoother_step" in __import__("pnmol._hip", fromlist=["SYMBOLS"]).SYMBOLS
    assert oracle is not None
