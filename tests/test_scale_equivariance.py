"""Equivariance of the filter step under a power-of-two scaling c of all square-root factors: Gamma, E_sqrtm, R_sqrtm and
the starting covariance factor times c, the mean unchanged.  Then every step gives the same means, covariance factors
times c, diffusion_squared_local (sigma^2) times 1/c^2 and the same error estimates -- exactly in exact arithmetic, and in
floating point too as long as no step hides an absolute threshold (a power of two scales without rounding).

The law is pinned on the oracle first (CPU).  The device paths follow: the covariance form and the square-root (QR) form
in fp64 (against their own unscaled run), the fp32 QR form and the fp32 covariance form (against the fp64 oracle of the
unscaled problem, at the modes' own tolerances), and the latent-force model in the fp64 QR form.  Every run starts from a
state set directly: `initialize()` adds a fixed 1e-10 nugget, which is deliberately not scale-equivariant."""

import copy

import numpy as np
import pytest
import scipy.linalg

import pnmol
import pnmol_oracle as oracle
from helpers import assert_mean_std_parity, make_pair

DT, NU = 2.0 ** -7, 2


# ---- the law, on the oracle (no GPU) ---------------------------------------------------------------------------------
def _oracle_run(osolver, opde, state, K):
    out = []
    for _ in range(K):
        state, _ = osolver.attempt_step(state, DT, opde)
        out.append(state)
    return out


@pytest.mark.parametrize("c", [2.0 ** -40, 2.0 ** 40])
def test_oracle_step_is_scale_equivariant(c):
    N, K = 24, 6
    _, _, opde, osolver = make_pair(N, NU, DT, K)
    state0 = osolver.initialize(opde)
    gamma = osolver.initialize_iwp(opde)[3]
    ref = _oracle_run(osolver, opde, state0, K)

    spde = copy.copy(opde)
    spde.E_sqrtm, spde.R_sqrtm = c * opde.E_sqrtm, c * opde.R_sqrtm
    osolver.iwp = oracle.IWP(N, NU, c * gamma)
    s0 = state0._replace(y=oracle.MVN(state0.y.mean, c * state0.y.cov_sqrtm))
    got = _oracle_run(osolver, spde, s0, K)
    for a, b in zip(got, ref):
        np.testing.assert_allclose(a.y.mean, b.y.mean, rtol=1e-13, atol=1e-13 * np.abs(b.y.mean).max())
        np.testing.assert_allclose(a.y.cov_sqrtm / c, b.y.cov_sqrtm, rtol=1e-13, atol=1e-13 * np.abs(b.y.cov_sqrtm).max())
        np.testing.assert_allclose(a.diffusion_squared_local * c * c, b.diffusion_squared_local, rtol=1e-13)
        np.testing.assert_allclose(a.error_estimate, b.error_estimate, rtol=1e-13, atol=1e-13 * np.abs(b.error_estimate).max())


# ---- the device paths ------------------------------------------------------------------------------------------------
def _problem(N, K):
    """1-d Dirichlet heat problem and a starting state after initialize() (mean (n, d), cov_sqrtm (D, D), reference order)."""
    pde, solver, opde, osolver = make_pair(N, NU, DT, K)
    state0 = osolver.initialize(opde)
    gamma = osolver.initialize_iwp(opde)[3]
    return pde, opde, osolver, gamma, state0


def _oracle_marginals(osolver, opde, state0, K):
    states = _oracle_run(osolver, opde, state0, K)
    om = np.array([s.y.mean[0] for s in states])
    ovar = np.array([np.einsum("ij,ij->i", s.y.cov_sqrtm, s.y.cov_sqrtm) for s in states])
    return om, np.sqrt(ovar @ osolver.E0.T)


def _covariance_form(ctx, pde, gamma, state0, c, K, dtype="f64"):
    """K steps of `pnmol_filter_step` with every square-root factor times c: means, stds / c, sigma^2 c^2, errors."""
    from pnmol import _hip

    f = _hip.Filter(ctx, L=pde.L, B=pde.B, E_sqrtm=c * pde.E_sqrtm, R_sqrtm=c * pde.R_sqrtm, Gamma=c * gamma,
                    num_derivatives=NU, dtype=dtype)
    s = f.new_state()
    s.set_sqrtm(state0.t, state0.y.mean, c * state0.y.cov_sqrtm)
    f.prepare_error_model(DT)
    means, stds, sig, err = [], [], [], []
    for _ in range(K):
        s, info, e = f.step(s, DT)
        means.append(s.mean()[0])
        stds.append(np.sqrt(np.maximum(s.marginal_var()[0], 0.0)) / c)
        sig.append(info.diffusion_squared_local * c * c)
        err.append(e)
    return [np.array(x) for x in (means, stds, sig, err)]


def _sqrt_form(ctx, c, K, dtype="f64", L=None, B=None, E_sqrtm=None, R_sqrtm=None, Gamma=None, state0=None, want_error=True):
    """K steps of `pnmol_sqrt_filter_step` with every square-root factor times c: means, stds / c, sigma^2 c^2, errors."""
    from pnmol import _hip

    f = _hip.SqrtFilter(ctx, L=L, B=B, E_sqrtm=c * E_sqrtm, R_sqrtm=c * R_sqrtm, Gamma=c * Gamma, num_derivatives=NU,
                        dtype=dtype)
    f.set_state(state0.t, state0.y.mean, c * state0.y.cov_sqrtm)
    if want_error:
        f.prepare_error_model(DT)
    means, stds, sig, err = [], [], [], []
    for _ in range(K):
        if want_error:
            info, e = f.step(DT, want_error=True)
            err.append(e)
        else:
            info = f.step(DT)
        _, mean, C = f.get_state()
        var = np.einsum("ij,ij->i", C, C).reshape(mean.shape, order="F")
        means.append(mean[0])
        stds.append(np.sqrt(var[0]) / c)
        sig.append(info.diffusion_squared_local * c * c)
    return [np.array(x) for x in (means, stds, sig, err)]


def _assert_equivariant(got, ref, tol):
    """means, stds, sigma^2 and errors of the scaled run against the unscaled one; True if bit for bit."""
    for a, b in zip(got, ref):
        if b.size:
            np.testing.assert_allclose(a, b, rtol=tol, atol=tol * np.abs(b).max())
    return all(np.array_equal(a, b) for a, b in zip(got, ref))


@pytest.mark.gpu
@pytest.mark.parametrize("c", [2.0 ** -100, 2.0 ** 100])
def test_covariance_form_fp64_is_scale_equivariant(hip_ctx, c):
    N, K = 128, 10
    pde, _, _, gamma, state0 = _problem(N, K)
    ref = _covariance_form(hip_ctx, pde, gamma, state0, 1.0, K)
    got = _covariance_form(hip_ctx, pde, gamma, state0, c, K)
    bitwise = _assert_equivariant(got, ref, 1e-12)
    print(f"covariance form fp64, c = 2^{np.log2(c):+.0f}: bit for bit = {bitwise}")


def _sqrt_args(pde, gamma, state0):
    return dict(L=pde.L, B=pde.B, E_sqrtm=pde.E_sqrtm, R_sqrtm=pde.R_sqrtm, Gamma=gamma, state0=state0)


@pytest.mark.gpu
@pytest.mark.parametrize("c", [2.0 ** -100, 2.0 ** 100])
def test_qr_form_fp64_is_scale_equivariant(hip_ctx, c):
    N, K = 128, 10
    pde, _, _, gamma, state0 = _problem(N, K)
    ref = _sqrt_form(hip_ctx, 1.0, K, **_sqrt_args(pde, gamma, state0))
    got = _sqrt_form(hip_ctx, c, K, **_sqrt_args(pde, gamma, state0))
    bitwise = _assert_equivariant(got, ref, 1e-12)
    print(f"QR form fp64, c = 2^{np.log2(c):+.0f}: bit for bit = {bitwise}")


@pytest.mark.gpu
@pytest.mark.parametrize("c", [2.0 ** -20, 2.0 ** -40, 2.0 ** 40])
def test_qr_form_fp32_is_scale_equivariant(hip_ctx, c):
    """The fp32 QR form at its tolerances (mean 1e-5, std 1e-4) against the fp64 oracle of the unscaled problem.  At
    c = 2^-40 the entries of the stacked matrices are 1e-22 .. 1e-9: the sums of squares below a panel's diagonal fall
    under FLT_MIN, where `dlarfg` has to rescale instead of dropping the column."""
    N, K = 64, 10
    pde, opde, osolver, gamma, state0 = _problem(N, K)
    om, ostd = _oracle_marginals(osolver, opde, state0, K)
    means, stds, sig, err = _sqrt_form(hip_ctx, c, K, dtype="f32", **_sqrt_args(pde, gamma, state0))
    assert np.isfinite(means).all() and np.isfinite(stds).all()
    assert_mean_std_parity(means, stds, om, ostd)


@pytest.mark.gpu
def test_covariance_form_fp32_is_scale_equivariant(hip_ctx):
    """The fp32 covariance form where it is validated (2-d Dirichlet heat, nu = 1, tests/test_gpu_fp32.py) at c = 2^-20
    (c^2 = 2^-40 sets the covariance's range), at its tolerances against the fp64 oracle of the unscaled problem:
    mean rtol 1e-5, std rtol 1e-4 on the entries of at least 1 % of the largest."""
    from pnmol import _hip

    n, K, dt, c = 12, 6, 2.0 ** -8, 2.0 ** -20
    opde = oracle.heat_2d_dirichlet_discretized(nums=(n, n), tmax=K * dt, diffusion_rate=0.05, kernel=oracle.SquareExponential())
    pde = pnmol.pde.examples.heat_2d_dirichlet_discretized(nums=(n, n), tmax=K * dt, diffusion_rate=0.05,
                                                           kernel=pnmol.kernels.SquareExponential())
    osolver = oracle.WhiteNoiseEK1(num_derivatives=1, steprule=oracle.Constant(dt), canonical_factor_signs=True,
                                   spatial_kernel=oracle.Matern52() + oracle.WhiteNoise())
    state0 = osolver.initialize(opde)
    gamma = osolver.initialize_iwp(opde)[3]
    states = []
    s = state0
    for _ in range(K):
        s, _ = osolver.attempt_step(s, dt, opde)
        states.append(s)
    om = np.array([x.y.mean[0] for x in states])
    os_ = np.sqrt(np.array([np.einsum("ij,ij->i", x.y.cov_sqrtm, x.y.cov_sqrtm) for x in states]) @ osolver.E0.T)
    f = _hip.Filter(hip_ctx, L=pde.L, B=pde.B, E_sqrtm=c * pde.E_sqrtm, R_sqrtm=c * pde.R_sqrtm, Gamma=c * gamma,
                    num_derivatives=1, dtype="f32")
    st = f.new_state()
    st.set_sqrtm(state0.t, state0.y.mean, c * state0.y.cov_sqrtm)
    f.prepare_error_model(dt)
    means, stds = [], []
    for _ in range(K):
        st, info, _ = f.step(st, dt)
        means.append(st.mean()[0])
        stds.append(np.sqrt(np.maximum(st.marginal_var()[0], 0.0)) / c)
    means, stds = np.array(means), np.array(stds)
    np.testing.assert_allclose(means, om, rtol=1e-5, atol=1e-9 * np.abs(om).max())
    big = os_ >= 1e-2 * os_.max()
    np.testing.assert_allclose(stds[big], os_[big], rtol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("c", [2.0 ** -100, 2.0 ** 100])
def test_latent_force_qr_form_fp64_is_scale_equivariant(hip_ctx, c):
    """The latent-force model (state [u; eps], d_state = 2d, noise-free update) in the fp64 QR form."""
    N, K = 64, 8
    pde, _, _, _ = make_pair(N, NU, DT, K)
    solver = pnmol.sqrtform.LinearLatentForceEK1(num_derivatives=NU, steprule=pnmol.odetools.step.Constant(DT),
                                                 spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
    state0 = solver.initialize(pde)
    gamma = solver.initialize_iwp_latent(pde)[4]
    d, nB = N, pde.B.shape[0]
    args = dict(L=np.hstack((pde.L, np.eye(d))), B=np.hstack((pde.B, np.zeros((nB, d)))), E_sqrtm=np.zeros((d, d)),
                R_sqrtm=np.zeros((nB, nB)), Gamma=scipy.linalg.block_diag(gamma, np.asarray(pde.E_sqrtm)), state0=state0,
                want_error=False)
    ref = _sqrt_form(hip_ctx, 1.0, K, **args)
    got = _sqrt_form(hip_ctx, c, K, **args)
    bitwise = _assert_equivariant(got, ref, 1e-12)
    print(f"latent-force QR form fp64, c = 2^{np.log2(c):+.0f}: bit for bit = {bitwise}")
