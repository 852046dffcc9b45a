"""Dense output on the GPU (`PDESolution.__call__`, `.state_at`, `solver.smooth(dense=...)`, `solver.sample_dense`, and the C entry
points behind them) against the textbook route in dense NumPy over the ORACLE's trajectory (tests/dense_reference.py: the query
time inserted as a grid point, prediction, one more RTS step).  North-star tolerances (helpers.assert_mean_std_parity) unless a
bound is derived where it is used.  Run with -m gpu."""

import ctypes

import numpy as np
import pytest

import pnmol
import pnmol_oracle as oracle
from dense_reference import as_solution, augment, filtered_dense, predict, rts_over, smoothed_dense
from helpers import assert_mean_std_parity, make_pair
from sample_reference import increment_std, maps_on_oracle
from smooth_reference import rts_on_oracle

pytestmark = pytest.mark.gpu

THETAS = (0.03, 0.37, 0.5, 0.97)


def _assert_means_close_in_the_frame(solver, h, mean, ref, tol=1e-5):
    """All derivatives of a mean at once, in the Nordsieck frame of h, where the filter works and the derivatives are commensurable:
    errors relative to the largest entry of the whole state there (a derivative whose exact mean is zero -- the highest one of
    the initial state -- holds rounding noise only, and has no scale of its own to be compared on)."""
    s = solver.iwp.nordsieck_preconditioner_1d_raw(h)[0][:, None]
    np.testing.assert_allclose(mean / s, ref / s, rtol=tol, atol=tol * np.abs(ref / s).max())


def _queries(t, intervals, thetas=THETAS, seed=0):
    """theta-points of the given intervals, shuffled (queries come unsorted and spread over many intervals)."""
    ts = np.array([t[k] + th * (t[k + 1] - t[k]) for k in intervals for th in thetas])
    return np.random.default_rng(seed).permutation(ts)


def _check_smoothed(ssol, osolver, osol, ts, blocks=None, derivatives=(0,)):
    out = ssol(ts)
    assert np.array_equal(out.t, ts)
    rm, rs, _ = smoothed_dense(osolver, osol, ts)
    assert out.mean.shape == rm.shape and out.marginal_std.shape == rs.shape
    for a in derivatives:
        for sl in (blocks or [slice(None)]):
            print(f"derivative {a}: mean error {np.abs(out.mean[:, a, sl] - rm[:, a, sl]).max() / np.abs(rm[:, a, sl]).max():.2e}, "
                  f"std error {np.abs(out.marginal_std[:, a, sl] - rs[:, a, sl]).max() / rs[:, a, sl].max():.2e} of the largest")
            assert_mean_std_parity(out.mean[:, a, sl], out.marginal_std[:, a, sl], rm[:, a, sl], rs[:, a, sl])
    return out, rm, rs


def _adaptive_pair():
    """The adaptive-step case of test_gpu_smooth.py."""
    kw = dict(abstol=1e-4, reltol=1e-3)
    pde, solver, opde, osolver = make_pair(64, 2, 2.0 ** -7, 24, "neumann")
    solver.steprule = pnmol.odetools.step.Adaptive(**kw)
    osolver.steprule = oracle.Adaptive(**kw)
    sol = solver.solve(pde)
    osol = osolver.solve(opde)
    assert sol.info == osol.info and sol.info["num_steps"] > 3
    np.testing.assert_allclose(sol.t, osol.t, rtol=1e-9)
    osol.t = sol.t
    return solver, sol, osolver, osol


# ---------------------------------------------------------------------------------------------- smoothed dense output
@pytest.mark.parametrize("N", [32, 128])
@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("bcond", ["dirichlet", "neumann"])
def test_dense_smoothed_heat(hip_ctx, N, nu, bcond):
    pde, solver, opde, osolver = make_pair(N, nu, 2.0 ** -7, 24, bcond)
    sol, osol = solver.solve(pde), osolver.solve(opde)
    ssol = solver.smooth(sol)
    assert ssol.smoothed and len(ssol.bridges) == len(sol.t) - 1 and not ssol.bridges[0].full
    _check_smoothed(ssol, osolver, osol, _queries(sol.t, (0, 1, 5, 11, 12, 17, 23)))


def test_dense_smoothed_all_derivatives(hip_ctx):
    pde, solver, opde, osolver = make_pair(32, 2, 2.0 ** -7, 24, "neumann")
    sol, osol = solver.solve(pde), osolver.solve(opde)
    _check_smoothed(solver.smooth(sol), osolver, osol, _queries(sol.t, (0, 6, 13, 23)), derivatives=(0, 1, 2))


def test_dense_smoothed_heat_nu3(hip_ctx):
    """nu = 3, N = 32: the interior at the north-star tolerances, the two noise-free Dirichlet nodes at 1e-3 of the largest std --
    the allowance and the reason of test_gpu_smooth.py::test_smooth_heat_nu3 (their variance is a difference of O(1) entries in
    the Nordsieck frame; the NumPy reference's insertion in raw coordinates loses digits there as well)."""
    pde, solver, opde, osolver = make_pair(32, 3, 2.0 ** -7, 20, "dirichlet")
    sol, osol = solver.solve(pde), osolver.solve(opde)
    ts = _queries(sol.t, (0, 4, 10, 19))
    out = solver.smooth(sol)(ts)
    rm, rs, _ = smoothed_dense(osolver, osol, ts)
    assert_mean_std_parity(out.mean[:, 0, 1:-1], out.marginal_std[:, 0, 1:-1], rm[:, 0, 1:-1], rs[:, 0, 1:-1])
    np.testing.assert_allclose(out.mean[:, 0], rm[:, 0], rtol=1e-5, atol=1e-5 * np.abs(rm[:, 0]).max())
    np.testing.assert_allclose(out.marginal_std[:, 0, [0, -1]], rs[:, 0, [0, -1]], rtol=0, atol=1e-3 * rs[:, 0].max())


def test_dense_smoothed_adaptive_steps(hip_ctx):
    solver, sol, osolver, osol = _adaptive_pair()
    assert len(set(np.round(np.diff(sol.t), 14))) > 2
    T = len(sol.t) - 1
    _check_smoothed(solver.smooth(sol), osolver, osol, _queries(sol.t, sorted({0, 1, T // 3, T // 2, T - 2, T - 1})))


def test_dense_smoothed_semilinear_diagonal_jacobian(hip_ctx):
    """Spruce budworm (the case of test_gpu_smooth.py)."""
    kw = dict(tmax=24 * 2.0 ** -6, dx=1.0 / 47, diffusion_rate=0.05, bcond="dirichlet", stencil_size_interior=3,
              stencil_size_boundary=3)
    pde = pnmol.pde.examples.spruce_budworm_1d_discretized(kernel=pnmol.kernels.SquareExponential(),
                                                           nugget_gram_matrix_fd=0.0, **kw)
    opde = oracle.spruce_budworm_1d_discretized(kernel=oracle.SquareExponential(), **kw)
    solver = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=2, steprule=pnmol.odetools.step.Constant(2.0 ** -6),
                                                 spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
    osolver = oracle.WhiteNoiseEK1(num_derivatives=2, steprule=oracle.Constant(2.0 ** -6), semilinear=True,
                                   canonical_factor_signs=True, spatial_kernel=oracle.Matern52() + oracle.WhiteNoise())
    sol, osol = solver.solve(pde), osolver.solve(opde)
    _check_smoothed(solver.smooth(sol), osolver, osol, _queries(sol.t, (0, 7, 12, 23)))


def test_dense_smoothed_semilinear_dense_jacobian(hip_ctx):
    """Lotka-Volterra (the case of test_gpu_smooth.py), north-star tolerances per component."""
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
    sol, osol = solver.solve(pde), osolver.solve(opde)
    d = pde.y0.shape[0]
    _check_smoothed(solver.smooth(sol), osolver, osol, _queries(sol.t, (0, 9, 19)),
                    blocks=(slice(0, d // 2), slice(d // 2, d)))


@pytest.mark.parametrize("N,K,intervals", [(256, 100, (0, 50, 99)), (512, 20, (0, 10, 19))])
def test_dense_smoothed_large(hip_ctx, N, K, intervals):
    pde, solver, opde, osolver = make_pair(N, 2, 2.0 ** -7, K, "dirichlet")
    sol, osol = solver.solve(pde), osolver.solve(opde)
    _check_smoothed(solver.smooth(sol), osolver, osol, _queries(sol.t, intervals, thetas=(0.03, 0.5, 0.97)))


# ---------------------------------------------------------------------------------------------- filter solutions, extrapolation
def test_dense_filter_solution_and_extrapolation(hip_ctx):
    """A filtering solution answers by prediction from the grid state on the left; so does any solution past its last grid time."""
    pde, solver, opde, osolver = make_pair(32, 2, 2.0 ** -7, 12, "dirichlet")
    sol, osol = solver.solve(pde), osolver.solve(opde)
    h = 2.0 ** -7
    ts = np.concatenate((_queries(sol.t, (0, 5, 11)), sol.t[-1] + h * np.array([0.1, 1.0, 3.5])))
    out = sol(ts)
    rm, rs, _ = filtered_dense(osolver, osol, ts)
    for a in range(3):
        assert_mean_std_parity(out.mean[:, a], out.marginal_std[:, a], rm[:, a], rs[:, a])
    # the smoothed solution beyond tmax: prediction from its terminal state, which is the filtered one
    past = ts[-3:]
    sout = solver.smooth(sol)(past)
    assert np.array_equal(sout.mean, out.mean[-3:]) and np.array_equal(sout.marginal_std, out.marginal_std[-3:])


@pytest.mark.parametrize("nu", [1, 2, 3])
def test_state_predict_against_the_oracle_prediction(hip_ctx, nu):
    pde, solver, opde, osolver = make_pair(32, nu, 2.0 ** -7, 6, "neumann")
    sol, osol = solver.solve(pde), osolver.solve(opde)
    flt = sol._ys[0].device_state.filter
    n, d = osol.mean.shape[1:]
    for k, dt in ((0, 0.3 * 2.0 ** -7), (3, 2.0 ** -7), (6, 2.5 * 2.0 ** -7)):
        st = flt.predict(sol._ys[k].device_state, dt)
        assert st.t == sol.t[k] + dt
        m, P = predict(osolver, osol.mean[k].reshape(-1, order="F"), osol.cov_sqrtm[k] @ osol.cov_sqrtm[k].T, dt)
        rstd = np.sqrt(np.diag(P)).reshape((n, d), order="F")
        rmean = m.reshape((n, d), order="F")
        assert_mean_std_parity(st.mean()[0], np.sqrt(st.marginal_var()[0]), rmean[0], rstd[0])
        _assert_means_close_in_the_frame(solver, dt, st.mean(), rmean)
        for a in range(n):
            np.testing.assert_allclose(np.sqrt(st.marginal_var()[a]), rstd[a], rtol=1e-4, atol=1e-5 * rstd[a].max())
        cov = st.cov()
        assert np.array_equal(np.diag(cov).reshape((n, d), order="F"), st.marginal_var())
        sc = np.sqrt(np.diag(P))
        # covariance entries relative to the two stds they belong to (north-star std tolerance, squared scale)
        np.testing.assert_allclose(cov / np.outer(sc, sc), P / np.outer(sc, sc), rtol=0, atol=2e-4)
        # `sol.state_at` of a filtering solution is this prediction
        y = sol.state_at(sol.t[k] + dt) if k < 6 and dt < 2.0 ** -7 else None
        if y is not None:
            assert np.array_equal(y.cov, cov)
        # and the marginal read-out agrees with the full prediction
        pm, ps = flt.predict_marginals(sol._ys[k].device_state, [dt, 0.0])
        np.testing.assert_allclose(pm[0], st.mean(), rtol=1e-12, atol=1e-13 * np.abs(st.mean()).max())
        np.testing.assert_allclose(ps[0] ** 2, st.marginal_var(), rtol=1e-9, atol=1e-12 * st.marginal_var().max())
        assert np.array_equal(pm[1], sol._ys[k].device_state.mean())
        assert np.array_equal(ps[1], np.sqrt(np.maximum(sol._ys[k].device_state.marginal_var(), 0.0)))


# ---------------------------------------------------------------------------------------------- full covariance
@pytest.mark.parametrize("nu", [2, 3])
def test_state_at_full_covariance_and_the_two_device_routes(hip_ctx, nu):
    """`state_at` with dense="full": std parity with the reference, a symmetric covariance whose diagonal is `marginal_var`, and a
    factor that reproduces it (as test_smooth_invariants).  Then the two DEVICE routes on the same states: `pnmol_bridge_state`
    against the textbook `pnmol_state_predict` + `pnmol_smoother_step` over (1 - theta) h.

    Tolerance of the route comparison, relative to the largest covariance entry: ten times the largest difference of the same
    two routes in dense NumPy on these cases (heat N = 32, Dirichlet, 12 steps, intervals 0 / 5 / 11, theta in {0.03, 0.25, 0.5,
    0.8, 0.97}; `bridge_on_oracle` against `smoothed_dense` of tests/dense_reference.py), which was measured as 6.5e-12 at nu = 2
    and 3.7e-6 at nu = 3, where the textbook route's insertion in raw coordinates is the lossy side.  So the bounds are 6.5e-11
    and 3.7e-5; the two device routes were seen to differ by 2.0e-11 and 7.8e-6."""
    measured = {2: 6.5e-12, 3: 3.7e-6}[nu]
    pde, solver, opde, osolver = make_pair(32, nu, 2.0 ** -7, 12, "dirichlet")
    sol, osol = solver.solve(pde), osolver.solve(opde)
    ssol = solver.smooth(sol, dense="full")
    assert all(b.full for b in ssol.bridges)
    flt = sol._ys[0].device_state.filter
    n, d = osol.mean.shape[1:]
    worst = 0.0
    for k in (0, 5, 11):
        h = sol.t[k + 1] - sol.t[k]
        for th in (0.03, 0.25, 0.5, 0.8, 0.97):
            t = sol.t[k] + th * h
            y = ssol.state_at(t)
            rm, rs, rP = smoothed_dense(osolver, osol, [t])
            std = np.sqrt(np.maximum(y.marginal_var, 0.0))
            inner = slice(1, -1) if nu == 3 else slice(None)
            assert_mean_std_parity(y.mean[0, inner], std[0, inner], rm[0][0, inner], rs[0][0, inner])
            if nu == 3:   # the two noise-free nodes: the allowance of test_dense_smoothed_heat_nu3
                np.testing.assert_allclose(std[0, [0, -1]], rs[0][0, [0, -1]], rtol=0, atol=1e-3 * rs[0][0].max())
            P = y.cov
            assert np.array_equal(P, P.T)
            assert np.array_equal(np.diag(P).reshape((n, d), order="F"), y.marginal_var)
            # the marginal read-out and the full state are the same posterior
            out = ssol(t)
            # (two kernels, two orders of summation: held to a tenth of the mean tolerance and a hundredth of the variance
            # tolerance that the north-star std tolerance implies, floors as there)
            _assert_means_close_in_the_frame(solver, h, out.mean[0], y.mean, tol=1e-6)
            for a in range(n):
                np.testing.assert_allclose(out.marginal_std[0][a] ** 2, y.marginal_var[a], rtol=2e-6,
                                           atol=1e-10 * y.marginal_var[a].max())
            # textbook route on the device, same states
            pred = flt.predict(sol._ys[k].device_state, th * h)
            tb = flt.smoother_step(pred, ssol._ys[k + 1].device_state, (1 - th) * h)
            Pt = tb.cov()
            diff = np.abs(P - Pt).max() / np.abs(Pt).max()
            worst = max(worst, diff)
            _assert_means_close_in_the_frame(solver, h, y.mean, tb.mean())
    print(f"nu = {nu}: largest relative covariance difference of the two device routes {worst:.2e} (NumPy: {measured:.1e})")
    assert worst <= 10 * measured
    # the factor reproduces the covariance, to the bound of test_gpu_smooth.py::test_smooth_invariants
    y = ssol.state_at(sol.t[5] + 0.37 * (sol.t[6] - sol.t[5]))
    C, P = y.cov_sqrtm, y.cov
    np.testing.assert_allclose(C @ C.T, P, atol=1e-9 * np.abs(P).max())
    with pytest.raises(RuntimeError, match='dense="full"'):
        solver.smooth(sol).state_at(sol.t[3] + 0.5 * h)


# ---------------------------------------------------------------------------------------------- invariants
def test_dense_invariants(hip_ctx):
    pde, solver, _, _ = make_pair(48, 2, 2.0 ** -7, 12, "dirichlet")
    sol = solver.solve(pde)
    before = [(y.mean.copy(), y.marginal_var.copy()) for y in sol._ys]
    s_none, s_marg, s_full = solver.smooth(sol, dense=None), solver.smooth(sol), solver.smooth(sol, dense="full")
    # keeping bridges changes no bit of the smoothed solution
    for s in (s_marg, s_full):
        assert np.array_equal(s.mean, s_none.mean) and np.array_equal(s.marginal_std, s_none.marginal_std)
        assert np.array_equal(s._ys[4].cov, s_none._ys[4].cov)
    assert s_none.bridges is None and s_none.smoothed
    # a grid time returns the smoothed knot bit for bit (alone, and mixed with other queries)
    g = s_marg(sol.t)
    assert np.array_equal(g.mean, s_marg.mean) and np.array_equal(g.marginal_std, s_marg.marginal_std)
    ts = np.random.default_rng(5).uniform(sol.t[0], sol.t[-1], 50)
    ts[7], ts[31] = sol.t[3], sol.t[-1]
    a = s_marg(ts)
    assert np.array_equal(a.mean[7], s_marg.mean[3]) and np.array_equal(a.marginal_std[31], s_marg.marginal_std[-1])
    assert s_marg.state_at(sol.t[3]) is s_marg._ys[3]
    # deterministic, and independent of how queries are batched: one call of 50 times == 50 calls
    b = s_marg(ts)
    assert np.array_equal(a.mean, b.mean) and np.array_equal(a.marginal_std, b.marginal_std)
    for i, tq in enumerate(ts):
        one = s_marg(tq)
        assert one.mean.shape == (1,) + a.mean.shape[1:]
        assert np.array_equal(one.mean[0], a.mean[i]) and np.array_equal(one.marginal_std[0], a.marginal_std[i])
    # "full" bridges answer marginal queries with the same bits
    c = s_full(ts)
    assert np.array_equal(a.mean, c.mean) and np.array_equal(a.marginal_std, c.marginal_std)
    # the C level returns the knots' stored values at the two ends of an interval
    br = s_marg.bridges[3]
    m, s = br.eval([br.t, br.t + br.dt])
    np.testing.assert_allclose(m[0], s_marg.mean[3], rtol=1e-15, atol=0)
    np.testing.assert_allclose(m[1], s_marg.mean[4], rtol=1e-13, atol=1e-15 * np.abs(s_marg.mean[4]).max())
    np.testing.assert_allclose(s[0], s_marg.marginal_std[3], rtol=1e-15, atol=0)
    np.testing.assert_allclose(s[1], s_marg.marginal_std[4], rtol=1e-12, atol=1e-14 * s_marg.marginal_std[4].max())
    # smoothing never widens: dense std <= the filter's predicted std at the same time
    f = sol(ts)
    assert np.all(a.marginal_std <= f.marginal_std + 1e-10 * f.marginal_std.max())
    # continuity towards the knots (the formula just inside an interval against the stored values at its ends)
    eps = 1e-9 * (sol.t[4] - sol.t[3])
    near = s_marg([sol.t[3] + eps, sol.t[4] - eps])
    np.testing.assert_allclose(near.mean[:, 0], s_marg.mean[3:5, 0], rtol=1e-6, atol=1e-7 * np.abs(s_marg.mean[:, 0]).max())
    np.testing.assert_allclose(near.marginal_std[:, 0], s_marg.marginal_std[3:5, 0], rtol=1e-3,
                               atol=1e-4 * s_marg.marginal_std[:, 0].max())
    # inputs unchanged
    after = [(y.mean.copy(), y.marginal_var.copy()) for y in sol._ys]
    for (m0, v0), (m1, v1) in zip(before, after):
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
    # a later solve() re-binds the solver: the old solution's bridges answer as before
    solver.solve(pde)
    again = s_marg(ts)
    assert np.array_equal(again.mean, a.mean) and np.array_equal(again.marginal_std, a.marginal_std)


def test_dense_refusals(hip_ctx):
    pde, solver, _, _ = make_pair(24, 1, 2.0 ** -7, 3, "dirichlet")
    sol = solver.solve(pde)
    ssol = solver.smooth(sol)
    mid = 0.5 * (sol.t[1] + sol.t[2])
    for s in (sol, ssol):
        with pytest.raises(ValueError, match=r"t\[0\]"):
            s(sol.t[0] - 1e-3)
        with pytest.raises(ValueError):
            s(np.nan)
        with pytest.raises(ValueError):
            s(np.zeros((2, 2)))
        with pytest.raises(ValueError):
            s.state_at([mid, mid])
    with pytest.raises(RuntimeError, match='dense="marginal"'):
        solver.smooth(sol, dense=None)(mid)
    assert solver.smooth(sol, dense=None)(sol.t[1]).mean.shape == (1, 2, 24)        # grid times need no bridge
    with pytest.raises(ValueError, match="dense"):
        solver.smooth(sol, dense="everything")
    host = pnmol.pdefilter.PDESolution(t=sol.t, mean=sol.mean, ys=[pnmol.base.rv.MultivariateNormal(y.mean, y.cov_sqrtm)
                                                                   for y in sol._ys],
                                       info=sol.info, diffusion_squared_calibrated=1.0)
    with pytest.raises(TypeError, match="device-resident"):
        host(mid)
    for cls in (pnmol.sqrtform.LinearWhiteNoiseEK1, pnmol.latent.LinearLatentForceEK1):
        other = cls(num_derivatives=1, steprule=pnmol.odetools.step.Constant(2.0 ** -7))
        with pytest.raises(TypeError, match="white-noise"):
            other.smooth(sol, dense="full")
        with pytest.raises(TypeError, match="white-noise"):
            other.sample_dense(sol, 4, [mid])
    f32 = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(2.0 ** -7))
    f32.dtype = "f32"
    with pytest.raises(TypeError, match="fp64"):
        f32.sample_dense(sol, 4, [mid])
    with pytest.raises(ValueError, match="noise_dense"):
        solver.sample_dense(sol, 2, [mid], noise_dense=[np.zeros((2, 48))])
    with pytest.raises(ValueError, match=">= solution.t"):
        solver.sample_dense(sol, 2, [sol.t[0] - 1.0])


def test_dense_argument_checks(hip_ctx):
    pde, solver, _, _ = make_pair(24, 2, 2.0 ** -7, 3, "dirichlet")
    sol = solver.solve(pde)
    flt = sol._ys[-1].device_state.filter
    lib = flt.lib
    s0, s1, s2, s3 = (y.device_state for y in sol._ys)
    dt = 2.0 ** -7
    out = flt.new_state()
    dp = ctypes.POINTER(ctypes.c_double)
    buf = np.empty((4, flt.n, flt.d))
    bp = buf.ctypes.data_as(dp)
    q = np.array([0.5 * dt, 0.0, dt, 2 * dt])
    qp = q.ctypes.data_as(dp)
    pde2, solver2, _, _ = make_pair(24, 2, 2.0 ** -7, 1, "dirichlet")
    foreign = solver2.solve(pde2)._ys[0].device_state
    f32 = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(dt))
    f32.dtype = "f32"
    lat = pnmol.latent.LinearLatentForceEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(dt),
                                            spatial_kernel=pnmol.kernels.SquareExponential() + pnmol.kernels.WhiteNoise())
    # pnmol_state_predict
    assert lib.pnmol_state_predict(None, s0.handle, dt, out.handle) == -1
    assert lib.pnmol_state_predict(flt.handle, None, dt, out.handle) == -1
    assert lib.pnmol_state_predict(flt.handle, s0.handle, dt, None) == -1
    assert lib.pnmol_state_predict(flt.handle, s0.handle, dt, s0.handle) == -1
    assert lib.pnmol_state_predict(flt.handle, s0.handle, 0.0, out.handle) == -1
    assert lib.pnmol_state_predict(flt.handle, s0.handle, -dt, out.handle) == -1
    assert lib.pnmol_state_predict(flt.handle, s0.handle, float("nan"), out.handle) == -1
    assert lib.pnmol_state_predict(flt.handle, foreign.handle, dt, out.handle) == -1
    assert b"pnmol_state_predict" in lib.pnmol_last_error(flt.ctx.handle)
    assert lib.pnmol_state_predict(flt.handle, s0.handle, dt, out.handle) == 0
    for other in (f32, lat):
        osol = other.solve(pde)
        oflt = osol._ys[-1].device_state.filter
        o_in, o_out = osol._ys[0].device_state, oflt.new_state()
        assert lib.pnmol_state_predict(oflt.handle, o_in.handle, dt, o_out.handle) == -1
        assert lib.pnmol_state_predict_marginals(oflt.handle, o_in.handle, 1, qp, bp, bp) == -1
        h = ctypes.c_void_p()
        assert lib.pnmol_smoother_step_bridge(oflt.handle, o_in.handle, osol._ys[1].device_state.handle, dt, o_out.handle, 0,
                                              ctypes.byref(h)) == -1
        assert not h.value
    # pnmol_state_predict_marginals
    assert lib.pnmol_state_predict_marginals(None, s0.handle, 4, qp, bp, bp) == -1
    assert lib.pnmol_state_predict_marginals(flt.handle, None, 4, qp, bp, bp) == -1
    assert lib.pnmol_state_predict_marginals(flt.handle, foreign.handle, 4, qp, bp, bp) == -1
    assert lib.pnmol_state_predict_marginals(flt.handle, s0.handle, 0, qp, bp, bp) == -1
    assert lib.pnmol_state_predict_marginals(flt.handle, s0.handle, 4, None, bp, bp) == -1
    assert lib.pnmol_state_predict_marginals(flt.handle, s0.handle, 4, qp, None, None) == -1
    bad = np.array([dt, -dt, float("nan")])
    assert lib.pnmol_state_predict_marginals(flt.handle, s0.handle, 2, bad.ctypes.data_as(dp), bp, bp) == -1
    assert lib.pnmol_state_predict_marginals(flt.handle, s0.handle, 1, bad[2:].ctypes.data_as(dp), bp, bp) == -1
    assert b"pnmol_state_predict_marginals" in lib.pnmol_last_error(flt.ctx.handle)
    assert lib.pnmol_state_predict_marginals(flt.handle, s0.handle, 4, qp, bp, None) == 0 and np.all(np.isfinite(buf))
    # pnmol_smoother_step_bridge: the checks of pnmol_smoother_step, and the bridge pointer
    h = ctypes.c_void_p()
    assert lib.pnmol_smoother_step_bridge(flt.handle, s2.handle, s3.handle, dt, out.handle, 0, None) == -1
    assert lib.pnmol_smoother_step_bridge(None, s2.handle, s3.handle, dt, out.handle, 0, ctypes.byref(h)) == -1
    assert lib.pnmol_smoother_step_bridge(flt.handle, None, s3.handle, dt, out.handle, 0, ctypes.byref(h)) == -1
    assert lib.pnmol_smoother_step_bridge(flt.handle, s2.handle, None, dt, out.handle, 0, ctypes.byref(h)) == -1
    assert lib.pnmol_smoother_step_bridge(flt.handle, s2.handle, s3.handle, dt, None, 0, ctypes.byref(h)) == -1
    assert lib.pnmol_smoother_step_bridge(flt.handle, s2.handle, s3.handle, 0.0, out.handle, 0, ctypes.byref(h)) == -1
    assert lib.pnmol_smoother_step_bridge(flt.handle, s2.handle, s3.handle, dt, s2.handle, 0, ctypes.byref(h)) == -1
    assert lib.pnmol_smoother_step_bridge(flt.handle, foreign.handle, s3.handle, dt, out.handle, 0, ctypes.byref(h)) == -1
    assert not h.value
    assert lib.pnmol_bridge_destroy(None) == -1
    assert lib.pnmol_bridge_get_interval(None, None, None, None) == -1
    sm2, marg = flt.smoother_step(s2, s3, dt, bridge="marginal")
    sm2b, full = flt.smoother_step(s2, s3, dt, bridge="full")
    plain = flt.smoother_step(s2, s3, dt)
    assert np.array_equal(sm2.cov(), plain.cov()) and np.array_equal(sm2b.cov(), plain.cov())
    assert np.array_equal(sm2.mean(), plain.mean()) and np.array_equal(sm2.marginal_var(), plain.marginal_var())
    assert (marg.t, marg.dt, marg.full) == (s2.t, dt, False) and full.full
    assert lib.pnmol_bridge_get_interval(marg.handle, None, None, None) == 0           # every output is optional
    only_dt = ctypes.c_double(0.0)
    assert lib.pnmol_bridge_get_interval(full.handle, None, ctypes.byref(only_dt), None) == 0 and only_dt.value == dt
    with pytest.raises(ValueError, match="bridge"):
        flt.smoother_step(s2, s3, dt, bridge="some")
    # pnmol_bridge_eval
    tq = np.array([s2.t + 0.25 * dt, s2.t, s2.t + dt, s2.t + 0.9 * dt])
    tp = tq.ctypes.data_as(dp)
    assert lib.pnmol_bridge_eval(None, 4, tp, bp, bp) == -1
    assert lib.pnmol_bridge_eval(marg.handle, 0, tp, bp, bp) == -1
    assert lib.pnmol_bridge_eval(marg.handle, -1, tp, bp, bp) == -1
    assert lib.pnmol_bridge_eval(marg.handle, 4, None, bp, bp) == -1
    assert lib.pnmol_bridge_eval(marg.handle, 4, tp, None, None) == -1
    for badt in (s2.t - 0.01 * dt, s2.t + 1.01 * dt, float("nan"), float("inf")):
        b1 = np.array([tq[0], badt])
        assert lib.pnmol_bridge_eval(marg.handle, 2, b1.ctypes.data_as(dp), bp, bp) == -1
    assert b"pnmol_bridge_eval" in lib.pnmol_last_error(flt.ctx.handle)
    assert lib.pnmol_bridge_eval(marg.handle, 4, tp, bp, None) == 0 and np.all(np.isfinite(buf))
    # pnmol_bridge_state
    t_in = s2.t + 0.4 * dt
    assert lib.pnmol_bridge_state(None, sm2.handle, s3.handle, t_in, out.handle) == -1
    assert lib.pnmol_bridge_state(full.handle, None, s3.handle, t_in, out.handle) == -1
    assert lib.pnmol_bridge_state(full.handle, sm2.handle, None, t_in, out.handle) == -1
    assert lib.pnmol_bridge_state(full.handle, sm2.handle, s3.handle, t_in, None) == -1
    assert lib.pnmol_bridge_state(full.handle, sm2.handle, s3.handle, t_in, sm2.handle) == -1
    assert lib.pnmol_bridge_state(full.handle, sm2.handle, s3.handle, t_in, s3.handle) == -1
    assert lib.pnmol_bridge_state(full.handle, foreign.handle, s3.handle, t_in, out.handle) == -1
    assert lib.pnmol_bridge_state(marg.handle, sm2.handle, s3.handle, t_in, out.handle) == -1       # made without keep_full
    assert b"keep_full" in lib.pnmol_last_error(flt.ctx.handle)
    assert lib.pnmol_bridge_state(full.handle, s1.handle, s3.handle, t_in, out.handle) == -1         # not the bridge's times
    assert lib.pnmol_bridge_state(full.handle, sm2.handle, s2.handle, t_in, out.handle) == -1
    for badt in (s2.t, s2.t + dt, s2.t - 0.1 * dt, s2.t + 1.1 * dt, float("nan")):
        assert lib.pnmol_bridge_state(full.handle, sm2.handle, s3.handle, badt, out.handle) == -1
    assert b"pnmol_bridge_state" in lib.pnmol_last_error(flt.ctx.handle)
    assert lib.pnmol_bridge_state(full.handle, sm2.handle, s3.handle, t_in, out.handle) == 0 and out.t == t_in
    # pnmol_samples_clone / pnmol_samples_interpolate
    S = 4
    left, right, mid, other = (flt.new_samples(S) for _ in range(4))
    big = flt.new_samples(8)
    h = ctypes.c_void_p()
    assert lib.pnmol_samples_clone(None, ctypes.byref(h)) == -1
    assert lib.pnmol_samples_clone(left.handle, None) == -1
    args = (None, 0, 9, 1.0)
    assert lib.pnmol_samples_interpolate(mid.handle, left.handle, right.handle, t_in, *args) == -1    # nothing drawn yet
    right.draw(s3)
    left.draw(s3)
    left.step_back(s2, dt)
    assert lib.pnmol_samples_interpolate(None, left.handle, right.handle, t_in, *args) == -1
    assert lib.pnmol_samples_interpolate(mid.handle, None, right.handle, t_in, *args) == -1
    assert lib.pnmol_samples_interpolate(left.handle, left.handle, right.handle, t_in, *args) == -1
    assert lib.pnmol_samples_interpolate(right.handle, left.handle, right.handle, t_in, *args) == -1
    assert lib.pnmol_samples_interpolate(big.handle, left.handle, right.handle, t_in, *args) == -1
    assert lib.pnmol_samples_interpolate(mid.handle, left.handle, other.handle, t_in, *args) == -1     # `other` holds no draw
    for badt in (s2.t, s3.t, s2.t - dt, s3.t + dt, float("nan")):
        assert lib.pnmol_samples_interpolate(mid.handle, left.handle, right.handle, badt, *args) == -1
    assert lib.pnmol_samples_interpolate(mid.handle, left.handle, None, s2.t, *args) == -1
    assert lib.pnmol_samples_interpolate(mid.handle, left.handle, right.handle, t_in, None, 0, 9, float("nan")) == -1
    fb = solver2.solve(pde2)._ys[-1].device_state.filter.new_samples(S)
    assert lib.pnmol_samples_interpolate(fb.handle, left.handle, right.handle, t_in, *args) == -1
    assert b"pnmol_samples_interpolate" in lib.pnmol_last_error(flt.ctx.handle)
    assert lib.pnmol_samples_interpolate(mid.handle, left.handle, right.handle, t_in, *args) == 0 and mid.t == t_in
    assert lib.pnmol_samples_interpolate(other.handle, right.handle, None, s3.t + dt, *args) == 0 and other.t == s3.t + dt
    cp = left.clone()
    assert cp.t == left.t and np.array_equal(cp.get(), left.get())
    with pytest.raises(pnmol._hip.PnmolHipError, match="pnmol_samples_interpolate"):
        mid.interpolate(left, right, s3.t)
    with pytest.raises(pnmol._hip.PnmolHipError, match="pnmol_bridge_eval"):
        marg.eval([s2.t + 2 * dt])


def test_bridges_keep_their_filter_alive(hip_ctx):
    """`pnmol_filter_destroy` returns -1 and frees nothing while a pnmol_bridge lives, 0 once it is destroyed; a bridge references
    no state (the states it was made from may go first)."""
    pde, solver, _, _ = make_pair(24, 1, 2.0 ** -7, 2, "dirichlet")
    sol = solver.solve(pde)
    src = sol._ys[-1].device_state.filter
    flt = pnmol._hip.Filter(hip_ctx, L=src._keep[0], B=src._keep[1], E_sqrtm=src._keep[2], R_sqrtm=src._keep[3],
                            Gamma=src._keep[4], num_derivatives=1)
    lib = flt.lib
    D = flt.n * flt.d
    a, b, out = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    for s in (a, b, out):
        assert lib.pnmol_state_create(flt.handle, ctypes.byref(s)) == 0
    mean, cov = np.zeros((flt.n, flt.d)), np.eye(D)
    mp, cp = (x.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for x in (mean, cov))
    assert lib.pnmol_state_set(a, 0.0, mp, cp) == 0 and lib.pnmol_state_set(b, 0.25, mp, cp) == 0
    h = ctypes.c_void_p()
    assert lib.pnmol_smoother_step_bridge(flt.handle, a, b, 0.25, out, 1, ctypes.byref(h)) == 0 and h.value
    for s in (a, b, out):
        assert lib.pnmol_state_destroy(s) == 0
    fh, flt.handle = flt.handle, None                                     # (this test destroys the filter by hand)
    assert lib.pnmol_filter_destroy(fh) == -1
    assert b"1 bridge(s)" in lib.pnmol_last_error(hip_ctx.handle)
    buf = np.empty((2, flt.n, flt.d))
    tq = np.array([0.1, 0.2])
    dp = ctypes.POINTER(ctypes.c_double)
    assert lib.pnmol_bridge_eval(h, 2, tq.ctypes.data_as(dp), buf.ctypes.data_as(dp), None) == 0   # the bridge still answers
    assert lib.pnmol_bridge_destroy(h) == 0
    assert lib.pnmol_filter_destroy(fh) == 0


# ---------------------------------------------------------------------------------------------- draws
def _dense_times(t, T):
    """Two times inside one interval, one each in two others (first and last), unsorted."""
    return np.array([t[T // 2] + 0.7 * (t[T // 2 + 1] - t[T // 2]), t[0] + 0.4 * (t[1] - t[0]),
                     t[T // 2] + 0.25 * (t[T // 2 + 1] - t[T // 2]), t[T - 1] + 0.6 * (t[T] - t[T - 1])])


def _check_dense_zero_noise(solver, sol, osolver, osol, blocks=None):
    """Tolerances of test_gpu_sample.py::_check_zero_noise."""
    n, d = osol.mean.shape[1:]
    T = len(sol.t) - 1
    ts = np.concatenate((_dense_times(sol.t, T), [sol.t[-1] + 0.5 * (sol.t[-1] - sol.t[-2]), sol.t[2]]))
    noise = [np.zeros((3, 2 * n * d)) for _ in range(T)] + [np.zeros((3, n * d))]
    grid, dense = solver.sample_dense(sol, 3, ts, noise=noise, noise_dense=[np.zeros((3, n * d)) for _ in ts])
    assert grid.shape == (3, T + 1, n, d) and dense.shape == (3, len(ts), n, d)
    assert np.array_equal(grid, solver.sample(sol, 3, noise=noise))
    assert np.array_equal(dense[0], dense[1]) and np.array_equal(dense[:, -1], grid[:, 2])
    ref, _, _ = smoothed_dense(osolver, osol, ts)
    print(f"zero-noise dense path: largest error {np.abs(dense[0][:, 0] - ref[:, 0]).max() / np.abs(ref[:, 0]).max():.2e}")
    for sl in (blocks or [slice(None)]):
        np.testing.assert_allclose(dense[0][:, 0, sl], ref[:, 0, sl], rtol=1e-5, atol=1e-5 * np.abs(ref[:, 0, sl]).max())


@pytest.mark.parametrize("nu,bcond", [(1, "dirichlet"), (2, "neumann"), (3, "dirichlet")])
def test_dense_zero_noise_is_the_dense_smoothed_mean(hip_ctx, nu, bcond):
    pde, solver, opde, osolver = make_pair(32, nu, 2.0 ** -7, 12, bcond)
    _check_dense_zero_noise(solver, solver.solve(pde), osolver, osolver.solve(opde))


def test_dense_zero_noise_is_the_dense_smoothed_mean_adaptive(hip_ctx):
    _check_dense_zero_noise(*_adaptive_pair())


def _check_dense_law(solver, sol, osolver, osol, dirichlet_allowance=False):
    """test_gpu_sample.py::_check_law over ALL inputs, grid and inserted: column s gets one unit input and zero noise elsewhere,
    plus one all-zero column.  The reference is the chain over the grid with the times inserted (tests/dense_reference.py,
    tests/sample_reference.py): the stds at every point of it and the stds of the increments between neighbours of it -- an
    inserted time and both its neighbours, two inserted times inside one interval.  Tolerances and the nu = 3 allowance of
    `_check_law`."""
    n, d = osol.mean.shape[1:]
    D, T = n * d, len(sol.t) - 1
    ts = _dense_times(sol.t, T)
    aug = augment(osolver, osol, ts)
    fake = as_solution(aug, (n, d))
    _, _, steps = maps_on_oracle(osolver, fake)
    ms, Ps = rts_over(osolver, aug)
    ostd = np.stack([np.sqrt(np.maximum(np.diag(P), 0.0)).reshape((n, d), order="F") for P in Ps])[:, 0]
    omean = np.stack([m.reshape((n, d), order="F") for m in ms])[:, 0]
    oinc = increment_std(Ps, steps, n, d)[:, 0]
    nq = len(ts)
    S = D + 2 * D * T + nq * D + 1
    noise = [np.zeros((S, 2 * D)) for _ in range(T)] + [np.zeros((S, D))]
    for k in range(T):
        noise[k][2 * D * k:2 * D * (k + 1)] = np.eye(2 * D)
    noise[T][2 * D * T:2 * D * T + D] = np.eye(D)
    off = 2 * D * T + D
    noise_dense = [np.zeros((S, D)) for _ in range(nq)]
    for q in range(nq):
        noise_dense[q][off + q * D:off + (q + 1) * D] = np.eye(D)
    grid, dense = solver.sample_dense(sol, S, ts, noise=noise, noise_dense=noise_dense)
    x = np.empty((S, len(aug.t), d))                                    # the draws along the augmented grid
    for k in range(T + 1):
        x[:, int(np.flatnonzero(aug.t == sol.t[k])[0])] = grid[:, k, 0]
    for q in range(nq):
        x[:, aug.where[q]] = dense[:, q, 0]
    dev = x[:-1] - x[-1]
    std = np.sqrt((dev ** 2).sum(axis=0))
    inc = np.sqrt(((dev[:, 1:] - dev[:, :-1]) ** 2).sum(axis=0))
    ins = sorted(aug.where)
    print(f"inserted times: std error {np.abs(std[ins] - ostd[ins]).max() / ostd.max():.2e} of the largest; increment std error "
          f"{np.abs(inc - oinc).max() / oinc.max():.2e} of the largest")
    np.testing.assert_allclose(x[-1], omean, rtol=1e-5, atol=1e-5 * np.abs(omean).max())
    inner = slice(1, -1) if dirichlet_allowance else slice(None)
    np.testing.assert_allclose(std[:, inner], ostd[:, inner], rtol=1e-4, atol=1e-5 * ostd.max())
    np.testing.assert_allclose(inc[:, inner], oinc[:, inner], rtol=1e-4, atol=1e-5 * oinc.max())
    if dirichlet_allowance:
        np.testing.assert_allclose(std[:, [0, -1]], ostd[:, [0, -1]], rtol=0, atol=1e-3 * ostd.max())
        np.testing.assert_allclose(inc[:, [0, -1]], oinc[:, [0, -1]], rtol=0, atol=1e-3 * oinc.max())


@pytest.mark.parametrize("nu", [1, 2, 3])
def test_dense_one_hot_noise_gives_the_joint_law(hip_ctx, nu):
    pde, solver, opde, osolver = make_pair(32, nu, 2.0 ** -7, 12, "dirichlet")
    _check_dense_law(solver, solver.solve(pde), osolver, osolver.solve(opde), dirichlet_allowance=(nu == 3))


def test_dense_one_hot_noise_gives_the_joint_law_adaptive(hip_ctx):
    _check_dense_law(*_adaptive_pair())


def test_dense_draws_device_noise_and_grid_bits(hip_ctx):
    pde, solver, _, _ = make_pair(32, 2, 2.0 ** -7, 6, "dirichlet")
    sol = solver.solve(pde)
    flt = sol._ys[-1].device_state.filter
    D, T, S = flt.n * flt.d, len(sol.t) - 1, 64
    ts = np.concatenate((_dense_times(sol.t, T), [sol.t[-1] + 0.01, sol.t[-1] + 0.03]))
    g, x = solver.sample_dense(sol, S, ts, seed=7)
    assert np.array_equal(g, solver.sample(sol, S, seed=7))                # the grid draws are `sample`'s, bit for bit
    noise = [hip_ctx.sample_noise(7, k, S, 2 * D if k < T else D) for k in range(T + 1)]
    nd = [hip_ctx.sample_noise(7, T + 1 + q, S, D) for q in range(len(ts))]
    g2, x2 = solver.sample_dense(sol, S, ts, noise=noise, noise_dense=nd)
    np.testing.assert_allclose(x, x2, rtol=1e-12, atol=1e-12 * np.abs(x).max())
    g3, x3 = solver.sample_dense(sol, S, ts, seed=7)
    assert np.array_equal(x, x3) and np.array_equal(g, g3)                  # same call twice
    assert not np.array_equal(x, solver.sample_dense(sol, S, ts, seed=8)[1])
    # the same times in another order: the draw at a time depends on its position in ts (step_index), not on the walk
    p = np.array([3, 0, 2, 1, 5, 4])
    nd_p = [nd[i] for i in p]
    _, xp = solver.sample_dense(sol, S, ts[p], noise=noise, noise_dense=nd_p)
    np.testing.assert_allclose(xp, x2[:, p], rtol=0, atol=1e-12 * np.abs(x).max())
    # calibrated draws: deviations from the zero-noise path scale with sqrt(sigma^2)
    zero = solver.sample_dense(sol, S, ts, noise=[0 * a for a in noise], noise_dense=[0 * a for a in nd])[1]
    cal = solver.sample_dense(sol, S, ts, noise=noise, noise_dense=nd, calibrated=True)[1]
    sig = float(np.sqrt(sol.diffusion_squared_calibrated))
    np.testing.assert_allclose(cal - zero, sig * (x2 - zero), rtol=0, atol=1e-10 * max(sig, 1.0) * np.abs(x2 - zero).max())
    assert solver.sample_dense(sol, 2, [])[1].shape == (2, 0, flt.n, flt.d)
    # a time given twice, followed by later times in the same interval (inside the grid and past it): the repeats get the
    # same draws, the others what they get without the repeats (their step_index is their position in ts)
    a, b, c = sol.t[2] + 0.2 * 2.0 ** -7, sol.t[2] + 0.6 * 2.0 ** -7, sol.t[2] + 0.9 * 2.0 ** -7
    e, f = sol.t[-1] + 0.01, sol.t[-1] + 0.02
    rep = np.array([a, a, b, a, c, e, e, f])
    nr = [hip_ctx.sample_noise(7, T + 1 + q, S, D) for q in range(len(rep))]
    _, xr = solver.sample_dense(sol, S, rep, noise=noise, noise_dense=nr)
    assert np.array_equal(xr[:, 0], xr[:, 1]) and np.array_equal(xr[:, 0], xr[:, 3]) and np.array_equal(xr[:, 5], xr[:, 6])
    uniq = [0, 2, 4, 5, 7]
    _, xu = solver.sample_dense(sol, S, rep[uniq], noise=noise, noise_dense=[nr[i] for i in uniq])
    np.testing.assert_allclose(xr[:, uniq], xu, rtol=0, atol=1e-12 * np.abs(xu).max())
    _, xd = solver.sample_dense(sol, S, rep, seed=7)                           # the same through the device generator
    np.testing.assert_allclose(xd, xr, rtol=1e-12, atol=1e-12 * np.abs(xr).max())


def test_dense_monte_carlo_moments_with_the_device_generator(hip_ctx):
    """S = 4096 draws at two inserted times (and one past tmax): sample mean and std of every entry within 5 standard errors of
    the dense smoothed mean and std, plus the north-star floor: the bounds of
    test_gpu_sample.py::test_monte_carlo_moments_with_the_device_generator."""
    pde, solver, opde, osolver = make_pair(32, 2, 2.0 ** -7, 12, "dirichlet")
    sol, osol = solver.solve(pde), osolver.solve(opde)
    ts = np.array([sol.t[6] + 0.3 * 2.0 ** -7, sol.t[2] + 0.8 * 2.0 ** -7, sol.t[-1] + 0.5 * 2.0 ** -7])
    rm, rs, _ = smoothed_dense(osolver, osol, ts)
    S = 4096
    x = solver.sample_dense(sol, S, ts, seed=0)[1][:, :, 0]
    sig, mu = rs[:, 0], rm[:, 0]
    floor = 1e-5 * sig.max()
    em = np.abs(x.mean(axis=0) - mu)
    es = np.abs(x.std(axis=0, ddof=1) - sig)
    pos = sig > floor
    print(f"largest mean error {np.max(em[pos] / (sig[pos] / np.sqrt(S))):.2f} standard errors, largest std error "
          f"{np.max(es[pos] / (sig[pos] / np.sqrt(2 * (S - 1)))):.2f}")
    assert np.all(em <= 5 * sig / np.sqrt(S) + floor)
    assert np.all(es <= 5 * sig / np.sqrt(2 * (S - 1)) + floor)
