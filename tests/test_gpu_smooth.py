"""RTS smoothing on the GPU (`solver.smooth`, `pnmol_smoother_step`) against a dense NumPy RTS pass over the oracle's
filtered trajectory (tests/smooth_reference.py).  North-star tolerances (helpers.assert_mean_std_parity).  Run with -m gpu."""

import ctypes

import numpy as np
import pytest

import pnmol
import pnmol_oracle as oracle
from helpers import assert_mean_std_parity, make_pair
from smooth_reference import marginal_std, rts_on_oracle

pytestmark = pytest.mark.gpu


def _check(sol, ssol, opde, osolver, osol):
    ms, Ps = rts_on_oracle(osolver, osol)
    n, d = osol.mean.shape[1:]
    ostd = marginal_std(Ps, n, d)
    assert np.array_equal(ssol.t, sol.t) and ssol.info == sol.info
    assert ssol.diffusion_squared_calibrated == sol.diffusion_squared_calibrated
    assert_mean_std_parity(ssol.mean[:, 0], ssol.marginal_std[:, 0], ms[:, 0], ostd[:, 0])
    return ms, ostd


@pytest.mark.parametrize("N", [32, 128])
@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("bcond", ["dirichlet", "neumann"])
def test_smooth_heat(hip_ctx, N, nu, bcond):
    pde, solver, opde, osolver = make_pair(N, nu, 2.0 ** -7, 24, bcond)
    sol = solver.solve(pde)
    osol = osolver.solve(opde)
    ssol = solver.smooth(sol)
    _check(sol, ssol, opde, osolver, osol)
    # smoothing matters here: interior stds shrink against the filter's
    assert (ssol.marginal_std[1:-1, 0].sum() < sol.marginal_std[1:-1, 0].sum())


def test_smooth_heat_nu3(hip_ctx):
    """nu = 3: the interior nodes at the north-star tolerances.  The two noise-free Dirichlet nodes (exact std 0; the NumPy RTS
    gives 1e-23) come out at up to 8.6e-13 = 4.5e-4 of the largest std, above the 1e-5 floor: in the Nordsieck frame of
    nu = 3 their variance is a difference of O(1) entries, resolved to eps (the covariance form's limit at nu = 3, as
    for the filter).  They are checked against 1e-3 of the largest std."""
    pde, solver, opde, osolver = make_pair(32, 3, 2.0 ** -7, 20, "dirichlet")
    sol = solver.solve(pde)
    osol = osolver.solve(opde)
    ssol = solver.smooth(sol)
    ms, Ps = rts_on_oracle(osolver, osol)
    ostd = marginal_std(Ps, *osol.mean.shape[1:])
    assert_mean_std_parity(ssol.mean[:, 0, 1:-1], ssol.marginal_std[:, 0, 1:-1], ms[:, 0, 1:-1], ostd[:, 0, 1:-1])
    np.testing.assert_allclose(ssol.mean[:, 0], ms[:, 0], rtol=1e-5, atol=1e-5 * np.abs(ms[:, 0]).max())
    np.testing.assert_allclose(ssol.marginal_std[:, 0, [0, -1]], ostd[:, 0, [0, -1]], rtol=0, atol=1e-3 * ostd[:, 0].max())


def test_smooth_adaptive_steps(hip_ctx):
    kw = dict(abstol=1e-4, reltol=1e-3)
    pde, solver, opde, osolver = make_pair(64, 2, 2.0 ** -7, 24, "neumann")
    solver.steprule = pnmol.odetools.step.Adaptive(**kw)
    osolver.steprule = oracle.Adaptive(**kw)
    sol = solver.solve(pde)
    osol = osolver.solve(opde)
    assert sol.info == osol.info and sol.info["num_attempted_steps"] > sol.info["num_steps"] > 3
    assert len(set(np.round(np.diff(sol.t), 14))) > 2
    np.testing.assert_allclose(sol.t, osol.t, rtol=1e-9)
    osol.t = sol.t
    _check(sol, solver.smooth(sol), opde, osolver, osol)


def test_smooth_semilinear_diagonal_jacobian(hip_ctx):
    """Spruce budworm (`df_diagonal` path of the forward step)."""
    kw = dict(tmax=24 * 2.0 ** -6, dx=1.0 / 47, diffusion_rate=0.05, bcond="dirichlet", stencil_size_interior=3,
              stencil_size_boundary=3)
    pde = pnmol.pde.examples.spruce_budworm_1d_discretized(kernel=pnmol.kernels.SquareExponential(),
                                                           nugget_gram_matrix_fd=0.0, **kw)
    opde = oracle.spruce_budworm_1d_discretized(kernel=oracle.SquareExponential(), **kw)
    solver = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=2, steprule=pnmol.odetools.step.Constant(2.0 ** -6),
                                                 spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
    osolver = oracle.WhiteNoiseEK1(num_derivatives=2, steprule=oracle.Constant(2.0 ** -6), semilinear=True,
                                   canonical_factor_signs=True, spatial_kernel=oracle.Matern52() + oracle.WhiteNoise())
    assert pde.df_diagonal is not None
    sol = solver.solve(pde)
    _check(sol, solver.smooth(sol), opde, osolver, osolver.solve(opde))


def test_smooth_semilinear_dense_jacobian(hip_ctx):
    """Lotka-Volterra (a system: dense Jacobian through `pnmol_filter_set_operator`), the recipe of
    tests/test_systems.py; north-star tolerances per component."""
    dt, K = 2.0 ** -6, 20
    kw = dict(dx=1.0 / 23, tmax=K * dt)
    pde = pnmol.pde.examples.lotka_volterra_1d_discretized(**kw)
    opde = oracle.lotka_volterra_1d_discretized(**kw)
    solver = pnmol.white.SemiLinearWhiteNoiseEK1(
        num_derivatives=2, steprule=pnmol.odetools.step.Constant(dt),
        spatial_kernel=pnmol.kernels.duplicate(pnmol.kernels.SquareExponential() + pnmol.kernels.WhiteNoise(), num=2))
    osolver = oracle.WhiteNoiseEK1(num_derivatives=2, steprule=oracle.Constant(dt), semilinear=True,
                                   canonical_factor_signs=True,
                                   spatial_kernel=oracle.duplicate(oracle.SquareExponential() + oracle.WhiteNoise(), 2))
    sol = solver.solve(pde)
    osol = osolver.solve(opde)
    ssol = solver.smooth(sol)
    ms, Ps = rts_on_oracle(osolver, osol)
    ostd = marginal_std(Ps, *osol.mean.shape[1:])
    d = pde.y0.shape[0]
    for sl in (slice(0, d // 2), slice(d // 2, d)):
        assert_mean_std_parity(ssol.mean[:, 0, sl], ssol.marginal_std[:, 0, sl], ms[:, 0, sl], ostd[:, 0, sl])


@pytest.mark.parametrize("N,K", [(256, 100), (512, 20)])
def test_smooth_large(hip_ctx, N, K):
    pde, solver, opde, osolver = make_pair(N, 2, 2.0 ** -7, K, "dirichlet")
    sol = solver.solve(pde)
    _check(sol, solver.smooth(sol), opde, osolver, osolver.solve(opde))


def test_smooth_invariants(hip_ctx):
    pde, solver, _, _ = make_pair(48, 2, 2.0 ** -7, 12, "dirichlet")
    sol = solver.solve(pde)
    before = [(y.mean.copy(), y.marginal_var.copy()) for y in sol._ys]
    s1, s2 = solver.smooth(sol), solver.smooth(sol)
    after = [(y.mean.copy(), y.marginal_var.copy()) for y in sol._ys]
    for (m0, v0), (m1, v1) in zip(before, after):                       # input unchanged
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
    assert np.array_equal(s1.mean, s2.mean) and np.array_equal(s1.marginal_std, s2.marginal_std)   # deterministic
    # terminal state = the filtered one, bit for bit
    assert np.array_equal(s1.mean[-1], sol.mean[-1]) and np.array_equal(s1._ys[-1].cov, sol._ys[-1].cov)
    assert np.array_equal(s1._ys[-1].marginal_var, sol._ys[-1].marginal_var)
    # smoothing never widens a marginal
    for ys, yf in zip(s1._ys, sol._ys):
        vs, vf = ys.marginal_var, yf.marginal_var
        assert np.all(vs <= vf + 1e-10 * vf.max())
    # the smoothed states are ordinary states: covariance factor and full covariance agree, symmetric
    C = s1._ys[3].cov_sqrtm
    P = s1._ys[3].cov
    assert np.array_equal(P, P.T)
    np.testing.assert_allclose(C @ C.T, P, atol=1e-9 * np.abs(P).max())
    # a later solve() re-binds the solver: the old solution still smooths with its own filter
    solver.solve(pde)
    s3 = solver.smooth(sol)
    assert np.array_equal(s3.mean, s1.mean)


def test_smooth_rejects_unsupported_solvers(hip_ctx):
    pde, solver, _, _ = make_pair(24, 1, 2.0 ** -7, 3, "dirichlet")
    sol = solver.solve(pde)
    for cls in (pnmol.sqrtform.LinearWhiteNoiseEK1, pnmol.latent.LinearLatentForceEK1):
        other = cls(num_derivatives=1, steprule=pnmol.odetools.step.Constant(2.0 ** -7))
        with pytest.raises(TypeError, match="white-noise"):
            other.smooth(sol)
    f32 = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(2.0 ** -7))
    f32.dtype = "f32"
    with pytest.raises(TypeError, match="fp64"):
        f32.smooth(sol)


def test_smoother_step_argument_checks(hip_ctx):
    pde, solver, _, _ = make_pair(24, 2, 2.0 ** -7, 2, "dirichlet")
    sol = solver.solve(pde)
    flt = sol._ys[-1].device_state.filter
    lib = flt.lib
    a, b = sol._ys[0].device_state, sol._ys[1].device_state
    out = flt.new_state()
    dt = 2.0 ** -7
    assert lib.pnmol_smoother_step(None, a.handle, b.handle, dt, out.handle) == -1
    assert lib.pnmol_smoother_step(flt.handle, None, b.handle, dt, out.handle) == -1
    assert lib.pnmol_smoother_step(flt.handle, a.handle, None, dt, out.handle) == -1
    assert lib.pnmol_smoother_step(flt.handle, a.handle, b.handle, dt, None) == -1
    assert lib.pnmol_smoother_step(flt.handle, a.handle, b.handle, 0.0, out.handle) == -1
    assert lib.pnmol_smoother_step(flt.handle, a.handle, b.handle, -dt, out.handle) == -1
    assert lib.pnmol_smoother_step(flt.handle, a.handle, b.handle, dt, a.handle) == -1
    assert lib.pnmol_smoother_step(flt.handle, a.handle, b.handle, dt, b.handle) == -1
    pde2, solver2, _, _ = make_pair(24, 2, 2.0 ** -7, 1, "dirichlet")
    foreign = solver2.solve(pde2)._ys[0].device_state
    assert lib.pnmol_smoother_step(flt.handle, foreign.handle, b.handle, dt, out.handle) == -1
    assert lib.pnmol_smoother_step(flt.handle, a.handle, b.handle, dt, out.handle) == 0
    with pytest.raises(pnmol._hip.PnmolHipError, match="pnmol_smoother_step"):
        flt.smoother_step(a, b, 0.0)
    assert isinstance(ctypes.c_int(0), ctypes.c_int)


def test_kalman_on_the_device_reference_fixture(hip_ctx):
    """tests/test_base/test_kalman.py:11-49,131-135 of the reference, restated: n = 4, m = 1..4, sc = sq = I,
    phi = triu of 1..16 (column order), h = first two unit rows, b = 1..2, data = 10..11."""
    from pnmol.base import kalman

    n = 4
    m, sc, sq = np.arange(1.0, 1 + n), np.eye(n), np.eye(n)
    phi = np.triu(np.arange(1.0, 1 + n ** 2).reshape((n, n)).T)
    h, b, data = np.eye(n // 2, n), np.arange(1.0, 1 + n // 2), np.arange(10.0, 10 + n // 2)
    out = kalman.filter_step(m=m, sc=sc, phi=phi, sq=sq, h=h, b=b, data=data)
    assert [x.shape for x in out] == [(n,), (n, n), (n, n), (n,), (n, n), (n, n)]
    m_fut, sc_fut, sgain, mp, scp, x = out
    m1, sc1 = kalman.smoother_step_sqrt(m=m, sc=sc, m_fut=m_fut, sc_fut=sc_fut, sgain=sgain, mp=mp, sq=sq, x=x)
    m2, sc2 = kalman.smoother_step_traditional(m=m, sc=sc, m_fut=m_fut, sc_fut=sc_fut, sgain=sgain, mp=mp, scp=scp)
    assert m1.shape == m2.shape == (n,) and sc1.shape == sc2.shape == (n, n)
    np.testing.assert_allclose(m1, m2, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(sc1, sc2, rtol=1e-7, atol=1e-9)
    # and against the covariance form in NumPy
    P = sc @ sc.T + sgain @ (sc_fut @ sc_fut.T - scp @ scp.T) @ sgain.T
    np.testing.assert_allclose(sc2 @ sc2.T, P, rtol=1e-9, atol=1e-10)
