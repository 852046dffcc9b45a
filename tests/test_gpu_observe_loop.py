"""Sensor data inside the device-resident constant-step loop (`pnmol_filter_set_observations`, `solve_marginals(pde,
observations=...)`) against the dense NumPy reference of tests/observe_reference.py -- the oracle's steps with
`oracle.update_sqrt` at the observation times -- and against `solve(pde, observations=...)` of the same solver.  Run with -m gpu."""

import ctypes

import numpy as np
import pytest

import pnmol
import pnmol_oracle as oracle
import observe_reference as ref
from helpers import assert_mean_std_parity, assert_parity, make_pair
from observe_loop_cases import SCHEDULES, schedule_run
from pnmol import _hip, data
from pnmol.pde import reactions

pytestmark = pytest.mark.gpu

SINGLE_WG = "PNMOL_HIP_OBSERVE_SINGLE_WG"     # read by `pnmol_filter_set_observations`: plans of q <= 32 take the single-workgroup route

# Stage parity of the single-workgroup route (q <= 32), rounding-level: ten times the largest figure measured on an MI355X over its
# five cases and all their updates (DESIGN.md section 19 has the table).  scalars: relative, measured 1.63e-15; mean: |increment
# error| / largest |increment|, measured 2.20e-14; cov: |error| / largest |P|, measured 1.65e-15.
TOL_SCALARS = 1.7e-14
TOL_MEAN = 2.2e-13
TOL_COV = 1.7e-14
# The sweep route (the default, every q) gives the bits of `pnmol_state_observe` (asserted); against the reference it is held to that call's own
# bounds (tests/test_gpu_observe.py)
SWEEP_TOL_SCALARS, SWEEP_TOL_MEAN, SWEEP_TOL_COV = 1.1e-14, 5.1e-13, 1.8e-14


def _dp(x):
    return x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _widen(C, ds):
    return C if C.shape[1] == ds else np.hstack((C, np.zeros((C.shape[0], ds - C.shape[1]))))


# ------------------------------------------------------------------------------------------------------------------ 1. stage parity
def planned_figures(flt, u, C, sweep=True):
    """One update through `observe_planned` from the reference's state before it (raw frame, a one-entry plan); the largest
    relative differences to the reference.  sweep (the plan takes the sweep route): everything equal to `Filter.observe` on a
    clone, bit for bit."""
    n, ds = flt.n, flt.ds
    latent = ds != C.shape[1]
    state = flt.new_state()
    state.set(u.t, ref.unflat_state(u.m, n, latent), u.P)
    Cd = _widen(C, ds)
    flt.set_observations([u.t], Cd, u.y[None, :], u.R)
    assert flt.observations_pending() == (0, 1)
    twin, twin_res = (flt.observe(state.clone(), Cd, u.y, u.R) if sweep else (None, None))
    res = flt.observe_planned(state, 0)
    assert res.info == -1 and state.t == u.t and flt.observations_pending() == (1, 1)
    kept = flt.observation_results(0, 1)[0]
    assert (kept.log_likelihood, kept.mahalanobis, kept.logdet, kept.info) == (res.log_likelihood, res.mahalanobis, res.logdet, -1)
    P, mean, var = state.cov(), state.mean(), state.marginal_var()
    assert np.array_equal(P, P.T)
    assert np.array_equal(ref.flat_mean(var, latent), np.diag(P))
    if twin is not None:
        assert np.array_equal(mean, twin.mean()) and np.array_equal(P, twin.cov()) and np.array_equal(var, twin.marginal_var())
        assert (res.log_likelihood, res.mahalanobis, res.logdet) == (twin_res.log_likelihood, twin_res.mahalanobis, twin_res.logdet)
    flt.clear_observations()
    inc_ref = u.m_post - u.m
    inc = ref.flat_mean(mean, latent) - u.m
    return dict(log_likelihood=abs(res.log_likelihood - u.log_likelihood) / abs(u.log_likelihood),
                mahalanobis=abs(res.mahalanobis - u.mahalanobis) / abs(u.mahalanobis),
                logdet=abs(res.logdet - u.logdet) / abs(u.logdet),
                mean=np.abs(inc - inc_ref).max() / np.abs(inc_ref).max(),
                cov=np.abs(P - u.P_post).max() / np.abs(u.P).max())


@pytest.mark.parametrize("N,nu,bcond,q,single", [c + (False,) for c in ref.CASES] + [c + (True,) for c in ref.CASES if c[3] <= 32])
def test_stage_parity_of_the_loops_path(hip_ctx, monkeypatch, N, nu, bcond, q, single):
    """The sweep route (the default) on every case: q = 33 with edge tiles (Dp = 144), q = 576 on the left-looking sweep, one
    update.  The single-workgroup route on the cases of q <= 32 (q = 32: no padding, q = 1: a single column)."""
    if single:
        monkeypatch.setenv(SINGLE_WG, "1")
    run = ref.reference_run(N, nu, bcond, q, 1) if N > 128 else ref.reference_run(N, nu, bcond, q)
    run.solver.initialize(run.pde)
    flt = run.solver._device_filter
    worst = {}
    for u, ob in zip(run.updates, run.observations):
        for key, v in planned_figures(flt, u, ob.C, sweep=not single).items():
            worst[key] = max(worst.get(key, 0.0), float(v))
    print("planned stage parity", (N, nu, bcond, q), "single workgroup" if single else "sweep", {k: f"{v:.2e}" for k, v in worst.items()})
    tol = (TOL_SCALARS, TOL_MEAN, TOL_COV) if single else (SWEEP_TOL_SCALARS, SWEEP_TOL_MEAN, SWEEP_TOL_COV)
    assert max(worst["log_likelihood"], worst["mahalanobis"], worst["logdet"]) <= tol[0]
    assert worst["mean"] <= tol[1]
    assert worst["cov"] <= tol[2]


# ------------------------------------------------------------------------------------------------------------------ 2. end to end
@pytest.mark.parametrize("name,single", [(n, False) for n in sorted(SCHEDULES)] +
                         [(n, True) for n in sorted(SCHEDULES) if SCHEDULES[n][3] <= 32])
def test_loop_end_to_end(hip_ctx, monkeypatch, name, single):
    if single:
        monkeypatch.setenv(SINGLE_WG, "1")
    run = schedule_run(name)
    N, nu, bcond, q, K, behind, at_t0 = SCHEDULES[name]
    pde, solver, osol = run.pde, run.solver, run.solution
    t, means, stds, sig, final, info = solver.solve_marginals(pde, observations=run.observations)
    np.testing.assert_allclose(t, osol.t, rtol=0, atol=1e-14)
    om, ostd = oracle.read_mean_and_std(osol, run.osolver.E0)
    assert_parity(means, stds, om, ostd, nu)
    lls = info["data_log_likelihoods"]
    print("log-likelihoods", name, lls, osol.info["data_log_likelihoods"])
    assert len(lls) == len(run.observations) and info["num_steps"] == len(t) - 1 == osol.info["num_steps"]
    np.testing.assert_allclose(lls, osol.info["data_log_likelihoods"], rtol=1e-4)
    np.testing.assert_allclose(info["data_log_likelihood"], osol.info["data_log_likelihood"], rtol=1e-4)
    assert info["data_log_likelihood"] == pytest.approx(sum(lls), rel=1e-14)
    # diffusion_squared_local keeps its meaning: PDE residuals only
    assert sig.shape == (len(t) - 1,)
    np.testing.assert_allclose(np.mean(sig), osol.diffusion_squared_calibrated, rtol=1e-4)
    np.testing.assert_allclose(final.y.mean[0], om[-1], rtol=1e-5, atol=1e-5 * np.abs(om).max())
    assert solver._device_filter.observations_pending() == (0, 0)               # the plan is cleared behind the solve
    # the data matters
    plain = solver.solve_marginals(pde)
    assert len(plain) == 5
    moved = np.abs(means - plain[1]).max()
    print(f"means moved by {moved:.2e}, floor {1e-5 * np.abs(om).max():.2e}")
    assert moved > 100 * 1e-5 * np.abs(om).max()


# ------------------------------------------------------------------------------------------------- 3. against solve(observations=)
def _against_solve(solver, pde, obs, nu, d=None):
    """Loop and `solve(pde, observations=obs)` of one solver, row by row at the end-to-end bounds; prints the largest differences.
    Returns (loop means, solve means)."""
    t, means, stds, sig, final, info = solver.solve_marginals(pde, observations=obs)
    d = means.shape[1] if d is None else d
    st, sm, ss, ssig, sinfo = [], [], [], [], None
    for state, sinfo in solver.solution_generator(pde, observations=obs):
        st.append(state.t), sm.append(state.y.mean[0][:d])
        ss.append(np.sqrt(np.maximum(state.y.marginal_var[0][:d], 0.0)))
        if not isinstance(state.diffusion_squared_local, list):
            ssig.append(state.diffusion_squared_local)
    sm, ss, ssig = np.array(sm), np.array(ss), np.array(ssig)
    np.testing.assert_allclose(t, st, rtol=0, atol=1e-14)
    print(f"loop vs solve: bit-identical means {np.array_equal(means, sm)}; mean {np.abs(means - sm).max():.2e} of "
          f"{np.abs(sm).max():.2e}, std {np.abs(stds - ss).max():.2e} of {ss.max():.2e}, log-likelihoods "
          f"{np.abs(np.array(info['data_log_likelihoods']) - np.array(sinfo['data_log_likelihoods'])).max():.2e}, "
          f"diffusion_squared_local {np.abs(sig / ssig - 1.0).max():.2e} relative")
    assert_parity(means, stds, sm, ss, nu)
    np.testing.assert_allclose(info["data_log_likelihoods"], sinfo["data_log_likelihoods"], rtol=1e-4)
    np.testing.assert_allclose(sig, ssig, rtol=1e-4)              # step by step: an update must not spoil the residual behind it
    return means, sm


def test_loop_against_solve_with_observations(hip_ctx):
    run = schedule_run("lead-consecutive-chunks")
    _against_solve(run.solver, run.pde, run.observations, 2)


def test_sweep_route_in_the_loop_is_bit_identical_to_solve_if_the_steps_are(hip_ctx):
    """q = 33 takes the kernels of `pnmol_state_observe` in their order.  Whether the loop's steps themselves give the bits of
    `attempt_step` is measured with a plan whose only entry lies behind the last step (the loop then runs the same self-contained
    steps, and rows 0 .. 11 see no data); if they do, the means of the full schedule must be equal bit for bit."""
    run = schedule_run("sweep-q33")
    last = [run.observations[-1]]
    _, lm, _, _, _, _ = run.solver.solve_marginals(run.pde, observations=last)
    sm = run.solver.solve(run.pde, observations=last).mean[:, 0]
    steps_identical = np.array_equal(lm[:-1], sm[:-1])
    means, smeans = _against_solve(run.solver, run.pde, run.observations, 2)
    print(f"steps bit-identical: {steps_identical}; full schedule bit-identical: {np.array_equal(means, smeans)}")
    if steps_identical:
        assert np.array_equal(means, smeans)


# ------------------------------------------------------------------------------------------------------------------ 4. split calls
def _bound(run):
    """(filter, initial device state, dt, plan arguments) of a schedule whose data all lie behind steps of one dt."""
    state = run.solver.initialize(run.pde)
    flt = run.solver._device_filter
    dt = run.solver.steprule.first_dt(run.pde)
    flt.prepare_error_model(dt)
    times, C, R, ys = data.shared_sensors(run.observations)
    return flt, state.y.device_state, dt, (times, _widen(C, flt.ds), ys, R)


@pytest.mark.parametrize("name", ["every-q3", "sweep-q33"])
def test_split_calls_give_the_bits_of_one_call(hip_ctx, name):
    run = schedule_run(name)
    flt, s0, dt, plan = _bound(run)
    nobs = len(run.observations)
    first5 = sum(1 for j in SCHEDULES[name][5] if j <= 5)
    a, b = s0.clone(), s0.clone()
    flt.set_observations(*plan)
    assert flt.observations_pending() == (0, nobs)
    m1, s1, i1 = flt.steps(a, 5, dt)
    assert flt.observations_pending() == (first5, nobs)
    m2, s2, i2 = flt.steps(a, 7, dt)
    assert flt.observations_pending() == (nobs, nobs)
    split = [(r.log_likelihood, r.mahalanobis, r.logdet, r.info) for r in flt.observation_results()]
    flt.set_observations(*plan)                                                    # (the cursor goes back to entry 0)
    assert flt.observations_pending() == (0, nobs)
    m, s, i = flt.steps(b, 12, dt)
    whole = [(r.log_likelihood, r.mahalanobis, r.logdet, r.info) for r in flt.observation_results()]
    flt.clear_observations()
    assert np.array_equal(np.vstack((m1, m2)), m) and np.array_equal(np.vstack((s1, s2)), s)
    assert split == whole and len(whole) == nobs and all(w[3] == -1 for w in whole)
    assert [o.diffusion_squared_local for o in list(i1) + list(i2)] == [o.diffusion_squared_local for o in i]
    assert np.array_equal(a.mean(), b.mean()) and np.array_equal(a.cov(), b.cov()) and a.t == b.t


# ------------------------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_through_raw_ctypes(hip_ctx):
    N, dt = 24, 2.0 ** -7
    pde, solver, _, _ = make_pair(N, 2, dt, 8, "dirichlet")
    s = solver.initialize(pde).y.device_state
    flt = solver._device_filter
    flt.prepare_error_model(dt)
    lib, h = flt.lib, flt.handle
    err = lambda: lib.pnmol_last_error(flt.ctx.handle).decode()
    C = np.ascontiguousarray(data.select_nodes(N, [5, 9]))
    R = 1e-3 * np.eye(2)
    t = np.array([2 * dt, 4 * dt])
    y = np.array([[0.1, 0.2], [0.1, 0.2]])
    nan = float("nan")

    def set_obs(f=h, t=t, q=2, C=C, R=R, y=y):
        t, C, y = (np.ascontiguousarray(x, dtype=np.float64) for x in (t, C, y))
        R = None if R is None else np.ascontiguousarray(R, dtype=np.float64)
        return lib.pnmol_filter_set_observations(f, len(t), _dp(t), q, _dp(C), None if R is None else _dp(R), _dp(y))

    assert set_obs(f=None) == -1
    for kw, why in ((dict(q=0), "q = 0"), (dict(q=N + 1), "d_state"), (dict(t=[4 * dt, 2 * dt]), "strictly increasing"),
                    (dict(t=[2 * dt, 2 * dt]), "strictly increasing"), (dict(t=[2 * dt, nan]), "not finite"),
                    (dict(t=[2 * dt, float("inf")]), "not finite"), (dict(C=np.where(C > 0, nan, C)), "C has"),
                    (dict(y=[[0.1, 0.2], [nan, 0.2]]), "y has"), (dict(R=[[1e-3, 0.0], [nan, 1e-3]]), "R has"),
                    (dict(R=[[1e-3, 1e-4], [0.0, 1e-3]]), "not lower triangular")):
        assert set_obs(**kw) == -1, kw
        assert "pnmol_filter_set_observations" in err() and why in err(), (kw, err())
        assert flt.observations_pending() == (0, 0)
    # an fp32 filter
    f32 = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(dt))
    f32.dtype = "f32"
    pde3, _, _, _ = make_pair(N, 1, dt, 1, "dirichlet")
    s32 = f32.initialize(pde3).y.device_state
    assert set_obs(f=s32.filter.handle) == -1 and "fp32" in lib.pnmol_last_error(s32.filter.ctx.handle).decode()
    # _begin: an entry inside a step, before s->t, at s->t -- -1, nothing enqueued, the state untouched bit for bit
    mean0, cov0, t0 = s.mean(), s.cov(), s.t
    for times, why in (([2.5 * dt, 4 * dt], "strictly between"), ([t0 - dt, 4 * dt], "before"), ([t0, 4 * dt], "never applied")):
        assert set_obs(t=times) == 0
        assert lib.pnmol_filter_steps_begin(h, s.handle, 6, dt) == -1
        assert "pnmol_filter_steps_begin" in err() and "entry 0" in err() and why in err(), err()
        with pytest.raises(_hip.PnmolHipError, match="entry 0"):
            flt.steps(s, 6, dt)
        assert s.t == t0 and np.array_equal(s.mean(), mean0) and np.array_equal(s.cov(), cov0)
        assert flt.observations_pending() == (0, 2)
    # observe_planned: index out of range
    res = _hip.ObserveOut()
    for index in (-1, 2):
        assert lib.pnmol_state_observe_planned(h, s.handle, index, ctypes.byref(res)) == -1
        assert "pnmol_state_observe_planned" in err()
    assert lib.pnmol_state_observe_planned(h, None, 0, ctypes.byref(res)) == -1
    assert lib.pnmol_filter_observation_results(h, 0, 1, ctypes.byref(res)) == -1 and "has not been applied" in err()
    assert np.array_equal(s.mean(), mean0) and np.array_equal(s.cov(), cov0)
    # the entry at s->t applied by hand, then the loop takes the rest; then a fixed plan from scratch
    r0 = flt.observe_planned(s, 0)
    assert r0.info == -1 and np.isfinite(r0.log_likelihood) and flt.observations_pending() == (1, 2)
    means, stds, infos = flt.steps(s, 6, dt)
    assert flt.observations_pending() == (2, 2) and np.all(np.isfinite(means)) and all(o.info == -1 for o in infos)
    assert set_obs(t=[s.t + 2 * dt, s.t + 4 * dt]) == 0
    means, stds, infos = flt.steps(s, 6, dt)
    assert flt.observations_pending() == (2, 2) and np.all(np.isfinite(means)) and all(o.info == -1 for o in infos)
    assert all(r.info == -1 and np.isfinite(r.log_likelihood) for r in flt.observation_results())
    flt.clear_observations()


# ------------------------------------------------------------------------------------------------------------------ 6. not PD
@pytest.mark.parametrize("q,single", [(2, True), (2, False), (34, False)])
def test_not_positive_definite_innovation_is_reported(hip_ctx, monkeypatch, q, single):
    """Two identical noise-free sensor rows (q = 2, on the single-workgroup route and on the sweep route; padded with 32 more
    noise-free distinct nodes to q = 34), behind the last step of a call: a numerical return code on a well-formed launch -- `steps` returns
    -3, the error names entry and pivot, `info` of the entry's result is the pivot."""
    if single:
        monkeypatch.setenv(SINGLE_WG, "1")
    N, dt = 48, 2.0 ** -4
    pde, solver, _, _ = make_pair(N, 2, dt, 4, "neumann")
    s = solver.initialize(pde).y.device_state
    flt = solver._device_filter
    flt.prepare_error_model(dt)
    nodes = [5, 5] + list(range(8, 8 + q - 2))
    C = np.ascontiguousarray(data.select_nodes(N, nodes))
    t = np.array([2 * dt])
    y = np.full((1, q), 0.1)
    flt.set_observations(t, C, y, None)
    means = np.empty((2, N))
    stds = np.empty((2, N))
    infos = (_hip.StepOut * 2)()
    rc = flt.lib.pnmol_filter_steps(flt.handle, s.handle, 2, dt, _dp(means), _dp(stds), infos)
    msg = flt.lib.pnmol_last_error(flt.ctx.handle).decode()
    print(rc, msg)
    assert rc == -3 and "entry 0" in msg and "pivot 1" in msg and "not positive definite" in msg
    assert all(o.info == -1 for o in infos)                                        # (the PDE residuals' own factorisations are fine)
    assert flt.observations_pending() == (1, 1)
    res = flt.observation_results(0, 1)[0]
    assert res.info == 1 and np.isnan(res.log_likelihood)
    flt.clear_observations()


# ------------------------------------------------------------------------------------------------------------------ 7. cleared plan
def test_cleared_plan_gives_the_bits_of_a_filter_that_never_had_one(hip_ctx):
    run = schedule_run("sweep-q33")
    flt, s0, dt, plan = _bound(run)
    a, b, c = s0.clone(), s0.clone(), s0.clone()
    fresh = flt.steps(a, 12, dt)
    probe = a.clone()
    ob = run.observations[0]
    out0, res0 = flt.observe(probe, ob.C, ob.y, ob.R_sqrtm)
    flt.set_observations(*plan)
    out1, res1 = flt.observe(probe, ob.C, ob.y, ob.R_sqrtm)                        # `Filter.observe` on a filter that has a plan
    assert np.array_equal(out0.mean(), out1.mean()) and np.array_equal(out0.cov(), out1.cov())
    assert (res0.log_likelihood, res0.mahalanobis, res0.logdet) == (res1.log_likelihood, res1.mahalanobis, res1.logdet)
    with_data = flt.steps(b, 12, dt)
    assert not np.array_equal(with_data[0], fresh[0])
    out2, _ = flt.observe(probe, ob.C, ob.y, ob.R_sqrtm)                           # ... and after the loop used the workspace
    assert np.array_equal(out0.mean(), out2.mean()) and np.array_equal(out0.cov(), out2.cov())
    flt.clear_observations()
    assert flt.observations_pending() == (0, 0)
    cleared = flt.steps(c, 12, dt)
    assert np.array_equal(cleared[0], fresh[0]) and np.array_equal(cleared[1], fresh[1])
    assert [o.diffusion_squared_local for o in cleared[2]] == [o.diffusion_squared_local for o in fresh[2]]
    assert np.array_equal(a.mean(), c.mean()) and np.array_equal(a.cov(), c.cov())


# ------------------------------------------------------------------------------------------------------------------ 8. composition
def test_reaction_term_composes_with_a_plan(hip_ctx):
    N, nu, dt, K = 33, 2, 2.0 ** -6, 12
    kw = dict(tmax=K * dt, dx=1.0 / (N - 1), diffusion_rate=0.05, bcond="dirichlet", stencil_size_interior=3, stencil_size_boundary=3)
    pde = pnmol.pde.examples.reaction_diffusion_1d_discretized(reactions.logistic(1.0), kernel=pnmol.kernels.SquareExponential(),
                                                               nugget_gram_matrix_fd=0.0, **kw)
    solver = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=nu, steprule=pnmol.odetools.step.Constant(dt),
                                                 spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
    plain = solver.solve_marginals(pde)
    assert solver._device_filter.reaction is pde.reaction
    # (dt = 2^-6 leaves a prior std of 5e-6 at the sensors: the noise std is chosen beside it, so that the data moves the means)
    C, noise = ref.sensor_matrix(N, 3), 3e-6
    rng = np.random.default_rng(33)
    obs = [data.Observation(plain[0][j], C, 1.02 * (C @ plain[1][j]) + noise * rng.standard_normal(3), noise) for j in (4, 8, 12)]
    means, _ = _against_solve(solver, pde, obs, nu)
    assert np.abs(means - plain[1]).max() > 100 * 1e-5 * np.abs(plain[1]).max()


def test_latent_force_solver_takes_observations_in_the_loop(hip_ctx):
    N, nu = 32, 1
    run = ref.latent_reference_run(N, nu, "dirichlet", 3)
    _against_solve(run.solver, run.pde, run.observations, nu, d=N)
    t, means, stds, sig, final, info = run.solver.solve_marginals(run.pde, observations=run.observations)
    osol, n = run.solution, nu + 1
    ovar = np.einsum("tij,tij->ti", osol.cov_sqrtm, osol.cov_sqrtm)
    ostd = np.sqrt(np.stack([ref.unflat_state(v, n, True) for v in ovar]))
    assert means.shape == (ref.STEPS + 1, N)
    assert_mean_std_parity(means, stds, osol.mean[:, 0, :N], ostd[:, 0, :N])
    np.testing.assert_allclose(info["data_log_likelihoods"], osol.info["data_log_likelihoods"], rtol=1e-4)
    assert_mean_std_parity(final.y.mean[0][:N], np.sqrt(np.maximum(final.y.marginal_var[0][:N], 0.0)), osol.mean[-1, 0, :N], ostd[-1, 0, :N])
