"""The measurement update on the GPU (`pnmol_state_observe`, `solve(pde, observations=...)`) against the dense NumPy reference of
tests/observe_reference.py: the oracle's steps with `oracle.update_sqrt` at the observation times.  Run with -m gpu."""

import ctypes

import numpy as np
import pytest

import pnmol
import pnmol_oracle as oracle
import observe_reference as ref
from dense_reference import smoothed_dense
from helpers import assert_mean_std_parity, make_pair
from pnmol import _hip, data
from sample_reference import maps_on_oracle, run_chain
from smooth_reference import marginal_std, rts_on_oracle

pytestmark = pytest.mark.gpu

# Stage parity, rounding-level: ten times the largest figure measured on an MI355X over all cases and updates (DESIGN.md section
# 15 has the table).  scalars: relative, measured 1.04e-15; mean: |increment error| / largest |increment|, measured 5.01e-14;
# cov: |error| / largest |P| (a variance resolves to eps |P|), measured 1.78e-15.
TOL_SCALARS = 1.1e-14
TOL_MEAN = 5.1e-13
TOL_COV = 1.8e-14


def stage_figures(flt, u, C):
    """One update on the device from the reference's state before it; the largest relative differences to the reference."""
    n, ds = flt.n, flt.ds
    state = flt.new_state()
    state.set(u.t, ref.unflat_state(u.m, n, ds != C.shape[1]), u.P)
    Cd = C if C.shape[1] == ds else np.hstack((C, np.zeros_like(C)))
    out, res = flt.observe(state, Cd, u.y, u.R)
    assert res.info == -1 and out.t == u.t
    inc_ref = u.m_post - u.m
    inc = ref.flat_mean(out.mean(), ds != C.shape[1]) - u.m
    P = out.cov()
    assert np.array_equal(P, P.T)
    assert np.array_equal(ref.flat_mean(out.marginal_var(), ds != C.shape[1]), np.diag(P))
    return dict(log_likelihood=abs(res.log_likelihood - u.log_likelihood) / abs(u.log_likelihood),
                mahalanobis=abs(res.mahalanobis - u.mahalanobis) / abs(u.mahalanobis),
                logdet=abs(res.logdet - u.logdet) / abs(u.logdet),
                mean=np.abs(inc - inc_ref).max() / np.abs(inc_ref).max(),
                cov=np.abs(P - u.P_post).max() / np.abs(u.P).max())


@pytest.mark.parametrize("N,nu,bcond,q", ref.CASES)
def test_stage_parity(hip_ctx, N, nu, bcond, q):
    """Upload the reference's state before each update, call `observe`, compare everything with the reference's update.
    q = 33 has a second column block and (Dp = 144) edge tiles of the down-date; q = 576 runs the left-looking sweep."""
    run = ref.reference_run(N, nu, bcond, q, 1) if N > 128 else ref.reference_run(N, nu, bcond, q)
    run.solver.initialize(run.pde)
    flt = run.solver._device_filter
    worst = {}
    for u, ob in zip(run.updates, run.observations):
        for key, v in stage_figures(flt, u, ob.C).items():
            worst[key] = max(worst.get(key, 0.0), float(v))
    print("stage parity", (N, nu, bcond, q), {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst["log_likelihood"], worst["mahalanobis"], worst["logdet"]) <= TOL_SCALARS
    assert worst["mean"] <= TOL_MEAN
    assert worst["cov"] <= TOL_COV


def _sensor_std(y, C, n):
    P00 = y.cov[0::n, 0::n]
    return np.sqrt(np.einsum("ij,jk,ik->i", C, P00, C))


@pytest.mark.parametrize("N,nu,bcond,q", ref.CASES[:5])
def test_solve_with_observations(hip_ctx, N, nu, bcond, q):
    run = ref.reference_run(N, nu, bcond, q)
    pde, solver, osol = run.pde, run.solver, run.solution
    sol = solver.solve(pde, observations=run.observations)
    np.testing.assert_allclose(sol.t, osol.t, rtol=0, atol=1e-14)
    om, ostd = oracle.read_mean_and_std(osol, run.osolver.E0)
    assert_mean_std_parity(sol.mean[:, 0], sol.marginal_std[:, 0], om, ostd)
    lls = sol.info["data_log_likelihoods"]
    print("log-likelihoods", lls, osol.info["data_log_likelihoods"])
    assert len(lls) == len(run.observations)
    np.testing.assert_allclose(sol.info["data_log_likelihood"], osol.info["data_log_likelihood"], rtol=1e-4)
    np.testing.assert_allclose(lls, osol.info["data_log_likelihoods"], rtol=1e-4)
    assert sol.info["data_log_likelihood"] == pytest.approx(sum(lls), rel=1e-14)
    for key in ("num_steps", "num_attempted_steps", "num_f_evaluations"):
        assert sol.info[key] == osol.info[key]
    # diffusion_squared_calibrated keeps its meaning: PDE residuals only
    np.testing.assert_allclose(sol.diffusion_squared_calibrated, osol.diffusion_squared_calibrated, rtol=1e-4)
    # the data matters: the means leave the unobserved solve by more than 100 times the parity floor
    plain = solver.solve(pde)
    assert set(plain.info) == {"num_f_evaluations", "num_df_evaluations", "num_df_diagonal_evaluations", "num_steps",
                               "num_attempted_steps"}
    moved = np.abs(sol.mean[:, 0] - plain.mean[:, 0]).max()
    print(f"means moved by {moved:.2e}, floor {1e-5 * np.abs(om).max():.2e}")
    assert moved > 100 * 1e-5 * np.abs(om).max()
    # sensor stds after each update are below those before it (the step from the state before, taken again)
    flt, n = sol._ys[0].device_state.filter, nu + 1
    for ob in run.observations:
        k = int(np.argmin(np.abs(sol.t - ob.t)))
        before, _, _ = flt.step(sol._ys[k - 1].device_state, sol.t[k] - sol.t[k - 1])
        sb = _sensor_std(pnmol.base.rv.DeviceMultivariateNormal(None, before), ob.C, n)
        sa = _sensor_std(sol._ys[k], ob.C, n)
        assert np.all(sa < sb) and np.all(sa < 1.01 * ref.NOISE_STD)


def test_simulate_final_state_and_initial_time_observation(hip_ctx):
    """`simulate_final_state` takes the same keyword; an observation at pde.t0 updates the initial state."""
    run = ref.reference_run(32, 2, "dirichlet", 3)
    state, info = run.solver.simulate_final_state(run.pde, observations=run.observations)
    np.testing.assert_allclose(info["data_log_likelihood"], run.solution.info["data_log_likelihood"], rtol=1e-4)
    om, _ = oracle.read_mean_and_std(run.solution, run.osolver.E0)
    np.testing.assert_allclose(state.y.mean[0], om[-1], rtol=1e-5, atol=1e-5 * np.abs(om).max())
    C = ref.sensor_matrix(32, 3)
    first = data.Observation(run.pde.t0, C, C @ run.pde.y0 + 1e-4, ref.NOISE_STD)
    obs = [first] + list(run.observations)
    osol, updates = ref.drive(run.osolver, run.opde, obs)
    assert len(updates) == 4 and updates[0].t == run.pde.t0
    sol = run.solver.solve(run.pde, observations=obs)
    om, ostd = oracle.read_mean_and_std(osol, run.osolver.E0)
    assert_mean_std_parity(sol.mean[:, 0], sol.marginal_std[:, 0], om, ostd)
    np.testing.assert_allclose(sol.info["data_log_likelihoods"], osol.info["data_log_likelihoods"], rtol=1e-4)


def test_adaptive_steps_land_on_the_observation_times(hip_ctx):
    kw = dict(abstol=1e-4, reltol=1e-3)
    N, nu, dt, K = 64, 2, 2.0 ** -4, 12
    pde, solver, opde, osolver = make_pair(N, nu, dt, K, "neumann", kappa=ref.KAPPA_MODEL)
    _, _, tpde, tsolver = make_pair(N, nu, dt, K, "neumann", kappa=ref.KAPPA_TRUTH)
    truth = tsolver.solve(tpde)
    idx = np.array([3, 7, 11])
    obs = ref.make_observations(truth.t[idx], truth.mean[idx, 0], ref.sensor_matrix(N, 5), seed=5)
    solver.steprule = pnmol.odetools.step.Adaptive(**kw)
    osolver.steprule = oracle.Adaptive(**kw)
    sol = solver.solve(pde, observations=obs)
    osol, updates = ref.drive(osolver, opde, obs, stop_at=[o.t for o in obs])
    assert len(updates) == 3 and sol.info["num_attempted_steps"] > sol.info["num_steps"] > 3
    for key in ("num_steps", "num_attempted_steps"):
        assert sol.info[key] == osol.info[key]
    for o in obs:
        assert np.any(np.abs(sol.t - o.t) <= 16 * np.finfo(float).eps * o.t)
    np.testing.assert_allclose(sol.t, osol.t, rtol=1e-9)
    om, ostd = oracle.read_mean_and_std(osol, osolver.E0)
    assert_mean_std_parity(sol.mean[:, 0], sol.marginal_std[:, 0], om, ostd)
    np.testing.assert_allclose(sol.info["data_log_likelihood"], osol.info["data_log_likelihood"], rtol=1e-4)


def test_latent_force_solver_with_observations(hip_ctx):
    N, nu = 32, 1
    run = ref.latent_reference_run(N, nu, "dirichlet", 3)
    sol = run.solver.solve(run.pde, observations=run.observations)
    osol, n = run.solution, nu + 1
    assert sol.mean.shape == osol.mean.shape == (ref.STEPS + 1, n, 2 * N)
    ovar = np.einsum("tij,tij->ti", osol.cov_sqrtm, osol.cov_sqrtm)
    ostd = np.sqrt(np.stack([ref.unflat_state(v, n, True) for v in ovar]))
    std = sol.marginal_std
    for a in range(n):
        for half in (slice(0, N), slice(N, 2 * N)):
            assert_mean_std_parity(sol.mean[:, a, half], std[:, a, half], osol.mean[:, a, half], ostd[:, a, half])
    np.testing.assert_allclose(sol.info["data_log_likelihoods"], osol.info["data_log_likelihoods"], rtol=1e-4)
    plain = run.solver.solve(run.pde)
    assert np.abs(sol.mean[:, 0, :N] - plain.mean[:, 0, :N]).max() > 100 * 1e-5 * np.abs(osol.mean[:, 0, :N]).max()


@pytest.mark.parametrize("N,nu,bcond,q", [ref.CASES[2], ref.CASES[3]])
def test_downstream_results_on_a_conditioned_solution(hip_ctx, N, nu, bcond, q):
    """`smooth`, `sample` and dense output run unchanged on a solution with observations: no measurement lies inside a step."""
    run = ref.reference_run(N, nu, bcond, q)
    solver, osolver, osol = run.solver, run.osolver, run.solution
    sol = solver.solve(run.pde, observations=run.observations)
    n, d = osol.mean.shape[1:]
    D, T = n * d, len(sol.t) - 1
    # smooth against the dense RTS pass over the reference's conditioned states
    ms, Ps = rts_on_oracle(osolver, osol)
    ostd = marginal_std(Ps, n, d)
    ssol = solver.smooth(sol)
    assert ssol.info == sol.info
    assert_mean_std_parity(ssol.mean[:, 0], ssol.marginal_std[:, 0], ms[:, 0], ostd[:, 0])
    # sample with host-supplied noise against the reference chain: zero noise is the chain's own path, one-hot noise gives the
    # columns of the map noise -> trajectory, whose sums of squares (the law) do not depend on the choice of factors
    mT, CT, steps = maps_on_oracle(osolver, osol)
    zero = [np.zeros((1, 2 * D)) for _ in range(T)] + [np.zeros((1, D))]
    x0 = solver.sample(sol, 1, noise=zero)[0, :, 0]
    r0 = run_chain(mT, CT, steps, zero)[0][:, 0::n]
    np.testing.assert_allclose(x0, r0, rtol=1e-5, atol=1e-5 * np.abs(r0).max())
    S = D + 2 * D * T + 1
    noise = [np.zeros((S, 2 * D)) for _ in range(T)] + [np.zeros((S, D))]
    for k in range(T):
        noise[k][2 * D * k:2 * D * (k + 1)] = np.eye(2 * D)
    noise[T][2 * D * T:2 * D * T + D] = np.eye(D)
    x = solver.sample(sol, S, noise=noise)[:, :, 0]
    r = run_chain(mT, CT, steps, noise)[:, :, 0::n]
    std, rstd = np.sqrt(((x[:-1] - x[-1]) ** 2).sum(axis=0)), np.sqrt(((r[:-1] - r[-1]) ** 2).sum(axis=0))
    np.testing.assert_allclose(std, rstd, rtol=1e-4, atol=1e-5 * rstd.max())
    np.testing.assert_allclose(rstd, ostd[:, 0], rtol=1e-6, atol=1e-7 * ostd[:, 0].max())   # (the chain's law is the RTS law)
    # dense output between two observations and exactly at one
    ts = np.array([0.5 * (sol.t[5] + sol.t[6]), sol.t[ref.EVERY]])
    out = ssol(ts)
    rm, rs, _ = smoothed_dense(osolver, osol, ts, base=(ms, Ps))
    assert_mean_std_parity(out.mean[:, 0], out.marginal_std[:, 0], rm[:, 0], rs[:, 0])
    assert np.array_equal(out.mean[1], ssol.mean[ref.EVERY])


def test_observe_argument_checks(hip_ctx):
    """Every -1 of include/pnmol_hip.h through raw ctypes, the -3 of a singular innovation matrix, an fp32 filter refused; a
    valid call afterwards still works."""
    N = 24
    pde, solver, _, _ = make_pair(N, 2, 2.0 ** -7, 2, "dirichlet")
    sol = solver.solve(pde)
    flt = sol._ys[-1].device_state.filter
    lib, a, out = flt.lib, sol._ys[1].device_state, flt.new_state()
    dp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    C = np.ascontiguousarray(data.select_nodes(N, [5, 9]))
    y, R = np.array([0.1, 0.2]), 1e-3 * np.eye(2)
    res = _hip.ObserveOut()
    call = lambda f, s, q, c, yy, rr, o, rs: lib.pnmol_state_observe(f, s, q, c, yy, rr, o, rs)
    ok = (flt.handle, a.handle, 2, dp(C), dp(y), dp(R), out.handle, ctypes.byref(res))
    for pos in (0, 1, 3, 4, 6, 7):                                            # a null pointer in every required place
        args = list(ok)
        args[pos] = None
        assert call(*args) == -1
    assert call(flt.handle, a.handle, 2, dp(C), dp(y), dp(R), a.handle, ctypes.byref(res)) == -1       # out aliases in
    assert call(flt.handle, a.handle, 0, dp(C), dp(y), dp(R), out.handle, ctypes.byref(res)) == -1     # q < 1
    assert call(flt.handle, a.handle, N + 1, dp(C), dp(y), dp(R), out.handle, ctypes.byref(res)) == -1  # q > d_state
    pde2, solver2, _, _ = make_pair(N, 2, 2.0 ** -7, 1, "dirichlet")
    foreign = solver2.solve(pde2)._ys[0].device_state
    assert call(flt.handle, foreign.handle, 2, dp(C), dp(y), dp(R), out.handle, ctypes.byref(res)) == -1
    assert call(flt.handle, a.handle, 2, dp(C), dp(y), dp(R), foreign.handle, ctypes.byref(res)) == -1
    assert b"pnmol_state_observe" in lib.pnmol_last_error(flt.ctx.handle)
    # an fp32 filter is refused
    f32 = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(2.0 ** -7))
    f32.dtype = "f32"
    pde3, _, _, _ = make_pair(N, 1, 2.0 ** -7, 1, "dirichlet")
    s32 = f32.initialize(pde3).y.device_state
    o32 = s32.filter.new_state()
    assert call(s32.filter.handle, s32.handle, 2, dp(C), dp(y), dp(R), o32.handle, ctypes.byref(res)) == -1
    assert b"fp32" in lib.pnmol_last_error(s32.filter.ctx.handle)
    # duplicate rows of C without noise: S is singular, the second pivot is named
    Cdup = np.ascontiguousarray(np.vstack((C[0], C[0])))
    assert call(flt.handle, a.handle, 2, dp(Cdup), dp(y), None, out.handle, ctypes.byref(res)) == -3
    assert res.info == 1 and b"pivot 1" in lib.pnmol_last_error(flt.ctx.handle)
    with pytest.raises(_hip.PnmolHipError, match="pivot 1"):
        flt.observe(a, Cdup, y)
    # a valid call afterwards: 0, the noise-free update pins the two sensors to the data
    assert call(*ok) == 0 and res.info == -1 and np.isfinite(res.log_likelihood)
    exact, _ = flt.observe(a, C, y)
    np.testing.assert_allclose(C @ exact.mean()[0], y, rtol=0, atol=1e-12)
    assert np.all(C @ exact.marginal_var()[0] <= 1e-6 * (C @ a.marginal_var()[0]))
