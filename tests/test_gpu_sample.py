"""Joint posterior draws on the GPU (`solver.sample`, `pnmol_samples_*`, `pnmol_sample_noise`) against the dense NumPy chain
(tests/sample_reference.py) and the NumPy RTS pass (tests/smooth_reference.py) over the ORACLE's filtered trajectory.
North-star tolerances (helpers.assert_mean_std_parity) unless a bound is derived where it is used.  Run with -m gpu.

The tests do not depend on which noise component drives which direction of the state (that is the library's business):
they use zero noise, complete sets of one-hot noise (sums of squares over all columns), and the device generator."""

import ctypes

import numpy as np
import pytest

import pnmol
import pnmol_oracle as oracle
from helpers import assert_mean_std_parity, make_pair
from sample_reference import device_noise, increment_std, maps_on_oracle
from smooth_reference import marginal_std, rts_on_oracle

pytestmark = pytest.mark.gpu


def _zero_noise(S, T, D):
    return [np.zeros((S, 2 * D)) for _ in range(T)] + [np.zeros((S, D))]


def _random_noise(rng, S, T, D):
    return [rng.standard_normal((S, 2 * D)) for _ in range(T)] + [rng.standard_normal((S, D))]


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


def _spruce_budworm():
    kw = dict(tmax=24 * 2.0 ** -6, dx=1.0 / 47, diffusion_rate=0.05, bcond="dirichlet", stencil_size_interior=3,
              stencil_size_boundary=3)
    pde = pnmol.pde.examples.spruce_budworm_1d_discretized(kernel=pnmol.kernels.SquareExponential(),
                                                           nugget_gram_matrix_fd=0.0, **kw)
    opde = oracle.spruce_budworm_1d_discretized(kernel=oracle.SquareExponential(), **kw)
    solver = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=2, steprule=pnmol.odetools.step.Constant(2.0 ** -6),
                                                 spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
    osolver = oracle.WhiteNoiseEK1(num_derivatives=2, steprule=oracle.Constant(2.0 ** -6), semilinear=True,
                                   canonical_factor_signs=True, spatial_kernel=oracle.Matern52() + oracle.WhiteNoise())
    return solver, solver.solve(pde), osolver, osolver.solve(opde)


def _lotka_volterra():
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
    return solver, solver.solve(pde), osolver, osolver.solve(opde)


# ---------------------------------------------------------------------------------------------- zero noise = smoothed means
def _check_zero_noise(solver, sol, osolver, osol, blocks=None):
    ms, _ = rts_on_oracle(osolver, osol)
    n, d = osol.mean.shape[1:]
    T = len(sol.t) - 1
    x = solver.sample(sol, 3, noise=_zero_noise(3, T, n * d))
    assert x.shape == (3, T + 1, n, d)
    assert np.array_equal(x[0], x[1]) and np.array_equal(x[0], x[2])
    ref = ms[:, 0]
    print(f"zero-noise path: largest error {np.abs(x[0][:, 0] - ref).max() / np.abs(ref).max():.2e} of the largest mean")
    for sl in (blocks or [slice(None)]):
        np.testing.assert_allclose(x[0][:, 0, sl], ref[:, sl], rtol=1e-5, atol=1e-5 * np.abs(ref[:, sl]).max())


@pytest.mark.parametrize("N", [32, 128])
@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("bcond", ["dirichlet", "neumann"])
def test_zero_noise_is_the_smoothed_mean_heat(hip_ctx, N, nu, bcond):
    pde, solver, opde, osolver = make_pair(N, nu, 2.0 ** -7, 24, bcond)
    _check_zero_noise(solver, solver.solve(pde), osolver, osolver.solve(opde))


def test_zero_noise_is_the_smoothed_mean_nu3(hip_ctx):
    pde, solver, opde, osolver = make_pair(32, 3, 2.0 ** -7, 20, "dirichlet")
    _check_zero_noise(solver, solver.solve(pde), osolver, osolver.solve(opde))


def test_zero_noise_is_the_smoothed_mean_adaptive(hip_ctx):
    _check_zero_noise(*_adaptive_pair())


def test_zero_noise_is_the_smoothed_mean_spruce_budworm(hip_ctx):
    _check_zero_noise(*_spruce_budworm())


def test_zero_noise_is_the_smoothed_mean_lotka_volterra(hip_ctx):
    solver, sol, osolver, osol = _lotka_volterra()
    d = osol.mean.shape[2]
    _check_zero_noise(solver, sol, osolver, osol, blocks=(slice(0, d // 2), slice(d // 2, d)))   # per component, as for smooth


@pytest.mark.parametrize("N,K", [(256, 100), (512, 20)])
def test_zero_noise_is_the_smoothed_mean_large(hip_ctx, N, K):
    pde, solver, opde, osolver = make_pair(N, 2, 2.0 ** -7, K, "dirichlet")
    _check_zero_noise(solver, solver.solve(pde), osolver, osolver.solve(opde))


# ---------------------------------------------------------------------------------------------- the law, by one-hot noise
def _check_law(solver, sol, osolver, osol, dirichlet_allowance=False):
    """Column s <-> (k, i) gets xi_k = e_i and zero noise elsewhere, plus one all-zero column: the deviations from the
    zero column are the columns of the linear map noise -> trajectory, so their sums of squares are the variances of the
    chain -- of the states (RTS stds) and of the increments x_{j+1} - x_j (what joint draws have and independent draws of
    the marginals have not)."""
    ms, Ps = rts_on_oracle(osolver, osol)
    n, d = osol.mean.shape[1:]
    D, T = n * d, len(sol.t) - 1
    _, _, steps = maps_on_oracle(osolver, osol)
    ostd = marginal_std(Ps, n, d)[:, 0]
    oinc = increment_std(Ps, steps, n, d)[:, 0]
    S = D + 2 * D * T + 1
    noise = _zero_noise(S, T, D)
    for k in range(T):
        noise[k][2 * D * k:2 * D * (k + 1)] = np.eye(2 * D)
    noise[T][2 * D * T:2 * D * T + D] = np.eye(D)
    x = solver.sample(sol, S, noise=noise)[:, :, 0]                   # (S, T+1, d)
    dev = x[:-1] - x[-1]
    std = np.sqrt((dev ** 2).sum(axis=0))
    inc = np.sqrt(((dev[:, 1:] - dev[:, :-1]) ** 2).sum(axis=0))
    indep = np.sqrt(ostd[1:] ** 2 + ostd[:-1] ** 2)
    print(f"std: largest error {np.abs(std - ostd).max() / ostd.max():.2e} of the largest; increment std: "
          f"{np.abs(inc - oinc).max() / oinc.max():.2e} of the largest; increment std / independent-draw value: "
          f"{(oinc.sum(axis=1) / indep.sum(axis=1)).min():.2f} .. {(oinc.sum(axis=1) / indep.sum(axis=1)).max():.2f}")
    np.testing.assert_allclose(x[-1], ms[:, 0], rtol=1e-5, atol=1e-5 * np.abs(ms[:, 0]).max())
    inner = slice(1, -1) if dirichlet_allowance else slice(None)
    np.testing.assert_allclose(std[:, inner], ostd[:, inner], rtol=1e-4, atol=1e-5 * ostd.max())
    np.testing.assert_allclose(inc[:, inner], oinc[:, inner], rtol=1e-4, atol=1e-5 * oinc.max())
    if dirichlet_allowance:   # the two noise-free nodes at nu = 3: the allowance and the reason of test_smooth_heat_nu3
        np.testing.assert_allclose(std[:, [0, -1]], ostd[:, [0, -1]], rtol=0, atol=1e-3 * ostd.max())
        np.testing.assert_allclose(inc[:, [0, -1]], oinc[:, [0, -1]], rtol=0, atol=1e-3 * oinc.max())


@pytest.mark.parametrize("nu,bcond", [(1, "dirichlet"), (2, "dirichlet"), (3, "dirichlet"), (2, "neumann")])
def test_one_hot_noise_gives_the_joint_law(hip_ctx, nu, bcond):
    pde, solver, opde, osolver = make_pair(32, nu, 2.0 ** -7, 12, bcond)
    _check_law(solver, solver.solve(pde), osolver, osolver.solve(opde), dirichlet_allowance=(nu == 3))


def test_one_hot_noise_gives_the_joint_law_adaptive(hip_ctx):
    _check_law(*_adaptive_pair())


# ---------------------------------------------------------------------------------------------- scale and linearity
def test_scale_and_linearity(hip_ctx):
    pde, solver, _, _ = make_pair(32, 2, 2.0 ** -7, 8, "dirichlet")
    sol = solver.solve(pde)
    flt = sol._ys[-1].device_state.filter
    D, T, S, c = flt.n * flt.d, len(sol.t) - 1, 5, 3.7
    noise = _random_noise(np.random.default_rng(1), S, T, D)
    zero = solver.sample(sol, S, noise=_zero_noise(S, T, D))
    base = solver.sample(sol, S, noise=noise)
    big = max(np.abs(base - zero).max(), 1e-300)
    # scale = c with xi  ==  scale = 1 with c xi   (C level: `sample` has no scale argument)
    t = np.asarray(sol.t)
    blk = flt.new_samples(S)
    scaled = np.empty_like(base)
    blk.draw(sol._ys[-1].device_state, noise[T], scale=c)
    scaled[:, T] = blk.get()
    for k in range(T - 1, -1, -1):
        blk.step_back(sol._ys[k].device_state, t[k + 1] - t[k], noise[k], scale=c)
        scaled[:, k] = blk.get()
        assert blk.t == sol._ys[k].device_state.t
    by_noise = solver.sample(sol, S, noise=[c * x for x in noise])
    np.testing.assert_allclose(scaled, by_noise, rtol=0, atol=1e-12 * c * big)
    np.testing.assert_allclose(scaled - zero, c * (base - zero), rtol=0, atol=1e-10 * c * big)
    # calibrated = mean path + sqrt(sigma^2) x deviations
    sig = float(np.sqrt(sol.diffusion_squared_calibrated))
    assert np.isfinite(sig) and sig > 0
    cal = solver.sample(sol, S, noise=noise, calibrated=True)
    np.testing.assert_allclose(cal - zero, sig * (base - zero), rtol=0, atol=1e-10 * sig * big)


# ---------------------------------------------------------------------------------------------- generator
def _corr(a, b):
    return float(np.mean(a * b))


def test_generator_moments_and_independence(hip_ctx):
    """2^20 values; bounds are 5 standard errors of the estimators under N(0, 1): mean 1/sqrt(M), variance sqrt(2/M),
    fourth moment sqrt(96/M), a product of independent normals 1/sqrt(M)."""
    R = C = 1024
    M = R * C
    z = hip_ctx.sample_noise(0, 0, R, C)
    assert z.shape == (R, C) and np.all(np.isfinite(z))
    se = 1 / np.sqrt(M)
    assert abs(z.mean()) <= 5 * se
    assert abs(z.var() - 1) <= 5 * np.sqrt(2 / M)
    assert abs(np.mean(z ** 4) - 3) <= 5 * np.sqrt(96 / M)
    assert abs(_corr(z[:, :-1], z[:, 1:])) <= 5 / np.sqrt(R * (C - 1))     # neighbouring components
    assert abs(_corr(z[:-1], z[1:])) <= 5 / np.sqrt((R - 1) * C)           # neighbouring samples
    assert abs(_corr(z, hip_ctx.sample_noise(0, 1, R, C))) <= 5 * se       # step_index k and k + 1
    assert abs(_corr(z, hip_ctx.sample_noise(1, 0, R, C))) <= 5 * se       # seeds 0 and 1
    assert np.array_equal(z, hip_ctx.sample_noise(0, 0, R, C))             # same arguments, same bits
    assert np.array_equal(z[:8, :33], hip_ctx.sample_noise(0, 0, 8, 33))   # a value depends on (seed, index, i, column) only
    # the documented map, restated in NumPy (log / cos of the two libraries differ by rounding only)
    np.testing.assert_allclose(hip_ctx.sample_noise(7, 2 ** 40 + 3, 64, 33), device_noise(7, 2 ** 40 + 3, 64, 33),
                               rtol=1e-12, atol=1e-14)


def test_device_noise_equals_host_supplied_noise_and_prefix_property(hip_ctx):
    pde, solver, _, _ = make_pair(32, 2, 2.0 ** -7, 6, "dirichlet")
    sol = solver.solve(pde)
    flt = sol._ys[-1].device_state.filter
    D, T, S = flt.n * flt.d, len(sol.t) - 1, 64
    a = solver.sample(sol, S, seed=7)
    noise = [hip_ctx.sample_noise(7, k, S, 2 * D if k < T else D) for k in range(T + 1)]
    b = solver.sample(sol, S, noise=noise)
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12 * np.abs(a).max())
    assert np.array_equal(a, solver.sample(sol, S, seed=7))                # same call twice
    assert not np.array_equal(a, solver.sample(sol, S, seed=8))
    p = solver.sample(sol, 8, seed=7)
    np.testing.assert_allclose(a[:8], p, rtol=0, atol=1e-12 * np.abs(a).max())
    assert np.array_equal(a[:8], p)                                        # (each column's arithmetic is independent)


# ---------------------------------------------------------------------------------------------- end to end (Monte Carlo)
def test_monte_carlo_moments_with_the_device_generator(hip_ctx):
    """S = 4096 draws: sample mean and std of every entry within 5 standard errors (sigma / sqrt(S), sigma / sqrt(2 (S - 1)))
    of the RTS mean and std, plus the north-star floor."""
    pde, solver, opde, osolver = make_pair(32, 2, 2.0 ** -7, 12, "dirichlet")
    sol, osol = solver.solve(pde), osolver.solve(opde)
    ms, Ps = rts_on_oracle(osolver, osol)
    n, d = osol.mean.shape[1:]
    sig = marginal_std(Ps, n, d)[:, 0]
    S = 4096
    x = solver.sample(sol, S, seed=0)[:, :, 0]
    floor = 1e-5 * sig.max()
    em = np.abs(x.mean(axis=0) - ms[:, 0])
    es = np.abs(x.std(axis=0, ddof=1) - sig)
    pos = sig > floor
    print(f"largest mean error {np.max(em[pos] / (sig[pos] / np.sqrt(S))):.2f} standard errors, largest std error "
          f"{np.max(es[pos] / (sig[pos] / np.sqrt(2 * (S - 1)))):.2f}")
    assert np.all(em <= 5 * sig / np.sqrt(S) + floor)
    assert np.all(es <= 5 * sig / np.sqrt(2 * (S - 1)) + floor)


# ---------------------------------------------------------------------------------------------- invariants and refusals
def test_sample_invariants(hip_ctx):
    pde, solver, _, _ = make_pair(48, 2, 2.0 ** -7, 10, "dirichlet")
    sol = solver.solve(pde)
    before = [(y.mean.copy(), y.marginal_var.copy()) for y in sol._ys]
    x1 = solver.sample(sol, 16, seed=3)
    after = [(y.mean.copy(), y.marginal_var.copy()) for y in sol._ys]
    for (m0, v0), (m1, v1) in zip(before, after):                       # input unchanged
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
    # sample and smooth interleaved (shared workspace) give what each gives alone
    s1 = solver.smooth(sol)
    x2 = solver.sample(sol, 16, seed=3)
    s2 = solver.smooth(sol)
    assert np.array_equal(x1, x2)
    assert np.array_equal(s1.mean, s2.mean) and np.array_equal(s1.marginal_std, s2.marginal_std)
    # one cross-check with the library's own smoother: zero noise walks its means
    flt = sol._ys[-1].device_state.filter
    z = solver.sample(sol, 1, noise=_zero_noise(1, len(sol.t) - 1, flt.n * flt.d))
    np.testing.assert_allclose(z[0], s1.mean, rtol=1e-5, atol=1e-5 * np.abs(s1.mean[:, 0]).max())
    # a later solve() re-binds the solver: the old solution still samples with its own filter
    solver.solve(pde)
    assert np.array_equal(solver.sample(sol, 16, seed=3), x1)


def test_sample_rejects_unsupported_solvers(hip_ctx):
    pde, solver, _, _ = make_pair(24, 1, 2.0 ** -7, 3, "dirichlet")
    sol = solver.solve(pde)
    for cls in (pnmol.sqrtform.LinearWhiteNoiseEK1, pnmol.latent.LinearLatentForceEK1):
        other = cls(num_derivatives=1, steprule=pnmol.odetools.step.Constant(2.0 ** -7))
        with pytest.raises(TypeError, match="white-noise"):
            other.sample(sol, 4)
    f32 = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(2.0 ** -7))
    f32.dtype = "f32"
    with pytest.raises(TypeError, match="fp64"):
        f32.sample(sol, 4)
    with pytest.raises(ValueError, match="num_samples"):
        solver.sample(sol, 0)
    with pytest.raises(ValueError, match="noise"):
        solver.sample(sol, 2, noise=[np.zeros((2, 4))])


def test_samples_argument_checks(hip_ctx):
    pde, solver, _, _ = make_pair(24, 2, 2.0 ** -7, 3, "dirichlet")
    sol = solver.solve(pde)
    flt = sol._ys[-1].device_state.filter
    lib = flt.lib
    s0, s1, s2, s3 = (y.device_state for y in sol._ys)
    dt = 2.0 ** -7
    h = ctypes.c_void_p()
    assert lib.pnmol_samples_create(None, 4, ctypes.byref(h)) == -1
    assert lib.pnmol_samples_create(flt.handle, 0, ctypes.byref(h)) == -1
    assert lib.pnmol_samples_create(flt.handle, -3, ctypes.byref(h)) == -1
    assert lib.pnmol_samples_create(flt.handle, 4, None) == -1
    assert lib.pnmol_samples_destroy(None) == -1
    # fp32 and latent-force filters
    f32 = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(dt))
    f32.dtype = "f32"
    lat = pnmol.latent.LinearLatentForceEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(dt),
                                            spatial_kernel=pnmol.kernels.SquareExponential() + pnmol.kernels.WhiteNoise())
    for other in (f32, lat):
        oflt = other.solve(pde)._ys[-1].device_state.filter
        assert lib.pnmol_samples_create(oflt.handle, 4, ctypes.byref(h)) == -1
        assert b"pnmol_samples_create" in lib.pnmol_last_error(oflt.ctx.handle)

    blk = flt.new_samples(4)
    x = blk.handle
    out = np.empty((4, flt.n, flt.d))
    tt = ctypes.c_double(0)
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    # no draw yet
    assert lib.pnmol_samples_step_back(x, s2.handle, dt, None, 0, 0, 1.0) == -1
    assert b"pnmol_samples_step_back" in lib.pnmol_last_error(flt.ctx.handle)
    assert lib.pnmol_samples_get(x, op) == -1
    assert lib.pnmol_samples_get_time(x, ctypes.byref(tt)) == -1
    # draw
    pde2, solver2, _, _ = make_pair(24, 2, 2.0 ** -7, 1, "dirichlet")
    foreign = solver2.solve(pde2)._ys[0].device_state
    assert lib.pnmol_samples_draw(None, s3.handle, None, 0, 0, 1.0) == -1
    assert lib.pnmol_samples_draw(x, None, None, 0, 0, 1.0) == -1
    assert lib.pnmol_samples_draw(x, foreign.handle, None, 0, 0, 1.0) == -1
    assert lib.pnmol_samples_draw(x, s3.handle, None, 0, 0, float("nan")) == -1
    assert lib.pnmol_samples_draw(x, s3.handle, None, 0, 0, float("inf")) == -1
    assert b"pnmol_samples_draw" in lib.pnmol_last_error(flt.ctx.handle)
    assert lib.pnmol_samples_draw(x, s3.handle, None, 0, 3, 1.0) == 0
    assert lib.pnmol_samples_get_time(x, ctypes.byref(tt)) == 0 and tt.value == s3.t
    # step_back
    assert lib.pnmol_samples_step_back(None, s2.handle, dt, None, 0, 2, 1.0) == -1
    assert lib.pnmol_samples_step_back(x, None, dt, None, 0, 2, 1.0) == -1
    assert lib.pnmol_samples_step_back(x, foreign.handle, dt, None, 0, 2, 1.0) == -1
    assert lib.pnmol_samples_step_back(x, s2.handle, 0.0, None, 0, 2, 1.0) == -1
    assert lib.pnmol_samples_step_back(x, s2.handle, -dt, None, 0, 2, 1.0) == -1
    assert lib.pnmol_samples_step_back(x, s2.handle, dt, None, 0, 2, float("nan")) == -1
    assert lib.pnmol_samples_step_back(x, s1.handle, dt, None, 0, 2, 1.0) == -1          # a step in the wrong order
    assert b"order" in lib.pnmol_last_error(flt.ctx.handle)
    assert lib.pnmol_samples_step_back(x, s2.handle, 2 * dt, None, 0, 2, 1.0) == -1      # wrong dt for this state
    assert lib.pnmol_samples_step_back(x, s2.handle, dt, None, 0, 2, 1.0) == 0
    assert lib.pnmol_samples_step_back(x, s2.handle, dt, None, 0, 2, 1.0) == -1          # the block has moved on
    assert lib.pnmol_samples_step_back(x, s1.handle, dt, None, 0, 1, 1.0) == 0
    assert lib.pnmol_samples_get(x, None) == -1
    assert lib.pnmol_samples_get(x, op) == 0 and np.all(np.isfinite(out))
    assert lib.pnmol_samples_get_time(x, ctypes.byref(tt)) == 0 and tt.value == s1.t
    assert lib.pnmol_sample_noise(None, 0, 0, 4, 4, op) == -1
    assert lib.pnmol_sample_noise(flt.ctx.handle, 0, 0, 0, 4, op) == -1
    assert lib.pnmol_sample_noise(flt.ctx.handle, 0, 0, 4, 4, None) == -1
    with pytest.raises(pnmol._hip.PnmolHipError, match="pnmol_samples_step_back"):
        blk.step_back(s0, 0.0)


def test_samples_keep_their_filter_alive(hip_ctx):
    """`pnmol_filter_destroy` returns -1 and frees nothing while a pnmol_samples lives, 0 once it is destroyed."""
    pde, solver, _, _ = make_pair(24, 1, 2.0 ** -7, 2, "dirichlet")
    sol = solver.solve(pde)
    src = sol._ys[-1].device_state.filter
    flt = pnmol._hip.Filter(hip_ctx, L=src._keep[0], B=src._keep[1], E_sqrtm=src._keep[2], R_sqrtm=src._keep[3],
                            Gamma=src._keep[4], num_derivatives=1)
    lib = flt.lib
    h = ctypes.c_void_p()
    assert lib.pnmol_samples_create(flt.handle, 8, ctypes.byref(h)) == 0
    fh, flt.handle = flt.handle, None                                     # (this test destroys the filter by hand)
    assert lib.pnmol_filter_destroy(fh) == -1
    assert b"1 sample block(s)" in lib.pnmol_last_error(hip_ctx.handle)
    st = ctypes.c_void_p()
    assert lib.pnmol_state_create(fh, ctypes.byref(st)) == 0              # the filter is still usable
    assert lib.pnmol_filter_destroy(fh) == -1
    assert lib.pnmol_state_destroy(st) == 0
    assert lib.pnmol_filter_destroy(fh) == -1
    assert lib.pnmol_samples_destroy(h) == 0
    assert lib.pnmol_filter_destroy(fh) == 0
