"""Posterior of linear functionals of the whole trajectory on the GPU (`solver.functionals`, `pnmol_functionals`).  Run with
-m gpu.

Stage parity on synthetic inputs follows DESIGN.md section 21: the device is held to 16 max(e64, 2^-52) against the
extended-precision truth of tests/functional_reference.py, e64 being the error of the fp64 restatement of the device's order
against the same truth, computed here from the reference alone.  Functionals are independent rows of the weights, so truth and
restatement are evaluated once per case for 64 functionals and the tests with fewer compare the leading ones."""

import ctypes
import functools

import numpy as np
import pytest

import functional_reference as fr
import pnmol
import pnmol_oracle as oracle
import stage_reference as sr
from helpers import assert_mean_std_parity, make_pair
from pnmol import functionals as fn
from smooth_reference import marginal_std, rts_on_oracle

pytestmark = pytest.mark.gpu

CASES = [(20, 1, "dirichlet"), (33, 2, "dirichlet"), (40, 3, "dirichlet"), (96, 2, "neumann"), (150, 1, "neumann"),
         (170, 2, "dirichlet")]
STAGE = [(c, Q) for c in CASES for Q in (1, 3, 33)] + [(CASES[1], 64)]
QMAX = 64


@functools.lru_cache(maxsize=None)
def _stage(case, T=3):
    """Trajectory, 64 random functionals, their truth and restatement (read-only, shared)."""
    tc = fr.trajectory_case(*case, T=T)
    c = tc.c
    W = fr.random_weights(tc, QMAX)
    return tc, W, fr.truth(c, tc.states, tc.dts, W), fr.restate(c.A, c.Q, c.nu, c.d, tc.states, tc.dts, W)


def _filter(c):
    if getattr(c, "flt", None) is None:
        c.solver.initialize(c.pde)
        c.flt = c.solver._device_filter
    return c.flt


def _upload(flt, tc):
    out = []
    for t, st in zip(tc.t, tc.states):
        s = flt.new_state()
        s.set(t, *st)
        out.append(s)
    return out


def _hold(head, dev, true, e64):
    """device <= 16 max(e64, 2^-52) in the metric max|X - X_true| / max|X_true|, figures printed first."""
    for name, x, x_true, x64 in (("mean", dev[0], true[0], e64[0]), ("cov", dev[1], true[1], e64[1])):
        e, ed = fr.error(x64, x_true), fr.error(x, x_true)
        print(f"STAGE functionals {head} | {name} | e64 {e:.2e} | device {ed:.2e} | ratio {ed / max(e, sr.EPS):.2f}")
        assert ed <= sr.bound(e), f"{head}: {name}: device {ed:.3e} > 16 max(e64 = {e:.3e}, 2^-52)"


# ---- stage parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,Q", STAGE, ids=[f"{sr.case_id(c)}-Q{Q}" for c, Q in STAGE])
def test_stage_parity(hip_ctx, case, Q):
    tc, W, (mt, ct), (m64, c64, _) = _stage(case)
    flt = _filter(tc.c)
    states = _upload(flt, tc)
    mean, cov = flt.functionals(states, tc.dts, W[:Q])
    assert np.array_equal(cov, cov.T)
    _hold(f"{sr.case_id(case)} Q={Q}", (mean, cov), (mt[:Q], ct[:Q, :Q]), (m64[:Q], c64[:Q, :Q]))
    for s, (m0, P0) in zip(states, tc.states):                                  # the inputs are unchanged, bit for bit
        assert np.array_equal(s.mean(), m0) and np.array_equal(s.cov(), P0)
    mean2, cov2 = flt.functionals(states, tc.dts, W[:Q])                        # two calls give the same bits
    assert np.array_equal(mean, mean2) and np.array_equal(cov, cov2)


@pytest.mark.parametrize("T", [0, 1])
def test_short_trajectories_and_zero_rows(hip_ctx, T):
    """T = 0 (W_0 m_0, W_0 P_0 W_0^T) and T = 1, weights that are zero at all times but one, and functionals that are zero
    altogether: their rows and columns of cov, and their means, are exact zeros."""
    case = CASES[1]
    tc = fr.trajectory_case(*case, T=T)
    c = tc.c
    W = fr.random_weights(tc, 5)
    W[0, 1:] = 0.0                                                              # only the first time
    W[1, :-1] = 0.0                                                             # only the last time
    W[2] = 0.0
    W[4] = 0.0
    flt = _filter(c)
    mean, cov = flt.functionals(_upload(flt, tc), tc.dts, W)
    assert np.array_equal(cov, cov.T)
    for q in (2, 4):
        assert mean[q] == 0.0 and not cov[q].any() and not cov[:, q].any()
    _hold(f"{sr.case_id(case)} T={T}", (mean, cov), fr.truth(c, tc.states, tc.dts, W), fr.restate(c.A, c.Q, c.nu, c.d, tc.states, tc.dts, W)[:2])
    if T == 0:
        m0, P0 = sr.flat(tc.states[0][0]), tc.states[0][1]
        Wf = fr.flat_weights(W)[:, 0]
        np.testing.assert_allclose(mean, Wf @ m0, rtol=1e-12, atol=1e-14 * np.abs(Wf @ m0).max())
        np.testing.assert_allclose(cov, Wf @ P0 @ Wf.T, rtol=1e-12, atol=1e-14 * np.abs(cov).max())


# ---- against the device's own smoother and the oracle's trajectory --------------------------------------------------------------
def _oracle_reference(osolver, osol, W):
    """(mean, cov) of the dense reference (1) on the oracle's trajectory; asserts, from the restatement's `gross`, that none of the
    functionals cancels (cov_qq >= 1e-3 of the positive terms it is accumulated from): they are held at a relative tolerance."""
    A, Ql = osolver.iwp.preconditioned_discretize
    states = [(mu, C @ C.T) for mu, C in zip(osol.mean, osol.cov_sqrtm)]
    dts = list(np.diff(osol.t))
    n, d = osol.mean.shape[1:]
    _, c2, gross = fr.restate(A, Ql @ Ql.T, n - 1, d, states, dts, W)
    assert np.all(np.diag(c2) >= 1e-3 * gross), np.diag(c2) / gross
    return fr.dense_reference(A, Ql @ Ql.T, osolver.iwp.nordsieck_preconditioner, states, dts, W)[:2]


@pytest.mark.parametrize("N", [32, 33])
@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("bcond", ["dirichlet", "neumann"])
def test_against_smoother_and_oracle(hip_ctx, N, nu, bcond):
    K = 6
    pde, solver, opde, osolver = make_pair(N, nu, 2.0 ** -7, K, bcond)
    sol = solver.solve(pde)
    ssol = solver.smooth(sol)
    where = [(k, j) for k in (0, 3, K) for j in (1, N // 2, N - 2)]
    post = solver.functionals(sol, np.stack([fn.point(K, N, k, j) for k, j in where]))
    sm = np.array([ssol.mean[k, 0, j] for k, j in where])
    sd = np.array([ssol.marginal_std[k, 0, j] for k, j in where])
    assert_mean_std_parity(post.mean, post.std, sm, sd)
    # integrals and means, against the dense reference on the oracle's trajectory
    osol = osolver.solve(opde)
    W = np.stack([fn.space_time_mean(sol.t, N), fn.trapezoid_in_time(sol.t, np.eye(N)[N // 2])])
    post = solver.functionals(sol, W)
    assert np.array_equal(post.cov, post.cov.T)
    om, oc = _oracle_reference(osolver, osol, fn.checked_weights(W, K, nu + 1, N))
    assert_mean_std_parity(post.mean, post.std, om, np.sqrt(np.diag(oc)))


# ---- composition: whatever made the filtered states ------------------------------------------------------------------------------
def _against_own_states(solver, sol, N, nu, bcond):
    """`functionals(sol)` against the dense reference (1) evaluated on the device's own filtered states, read back raw; the prior is
    the oracle's of the same mesh, kernel and nu.  North-star tolerances; the restatement's `gross` shows, from the reference
    alone, that none of the functionals used cancels (cov_qq >= 1e-3 of the positive terms it is accumulated from)."""
    _, _, opde, osolver = make_pair(N, nu, 2.0 ** -7, 1, bcond)
    osolver.iwp, osolver.E0, osolver.E1, _ = osolver.initialize_iwp(opde)
    A, Ql = osolver.iwp.preconditioned_discretize
    T = len(sol.t) - 1
    states = [(y.device_state.mean(), y.device_state.cov()) for y in sol._ys]
    W = np.stack([fn.space_time_mean(sol.t, N), fn.trapezoid_in_time(sol.t, np.eye(N)[N // 2]), fn.point(T, N, T // 2, N // 3)])
    full = fn.checked_weights(W, T, nu + 1, N)
    dts = list(np.diff(sol.t))
    m1, c1, _, _ = fr.dense_reference(A, Ql @ Ql.T, osolver.iwp.nordsieck_preconditioner, states, dts, full)
    _, c2, gross = fr.restate(A, Ql @ Ql.T, nu, N, states, dts, full)
    assert np.all(np.diag(c2) >= 1e-3 * gross)
    post = solver.functionals(sol, W)
    assert np.array_equal(post.cov, post.cov.T)
    assert_mean_std_parity(post.mean, post.std, m1, np.sqrt(np.diag(c1)))
    for y, (m0, P0) in zip(sol._ys, states):                                    # the solution is unchanged
        assert np.array_equal(y.device_state.mean(), m0) and np.array_equal(y.device_state.cov(), P0)


def test_adaptive_steps(hip_ctx):
    N, nu, bcond = 33, 2, "neumann"
    pde, solver, _, _ = make_pair(N, nu, 2.0 ** -7, 12, bcond)
    solver.steprule = pnmol.odetools.step.Adaptive(abstol=1e-4, reltol=1e-3)
    sol = solver.solve(pde)
    assert len(set(np.round(np.diff(sol.t), 14))) > 2
    _against_own_states(solver, sol, N, nu, bcond)


def test_with_observations(hip_ctx):
    N, nu, bcond, K = 33, 2, "dirichlet", 6
    pde, solver, _, _ = make_pair(N, nu, 2.0 ** -7, K, bcond)
    t, means, stds, _, _ = solver.solve_marginals(pde)
    C = np.eye(N)[[5, 16, 27]]
    noise = float(np.median(stds[1:, 1:-1]))
    obs = [pnmol.data.Observation(t[j], C, 1.02 * (C @ means[j]), noise) for j in (2, 4)]
    sol = solver.solve(pde, observations=obs)
    assert np.abs(sol.mean[-1, 0] - means[-1]).max() > 0.0                       # (the data moved the solution)
    _against_own_states(solver, sol, N, nu, bcond)


def test_solve_on_device_with_a_reaction(hip_ctx):
    from pnmol.pde import reactions

    N, nu, bcond, dt, K = 33, 2, "dirichlet", 2.0 ** -6, 8
    kw = dict(tmax=K * dt, dx=1.0 / (N - 1), diffusion_rate=0.05, bcond=bcond, stencil_size_interior=3, stencil_size_boundary=3)
    pde = pnmol.pde.examples.reaction_diffusion_1d_discretized(reactions.logistic(1.0), kernel=pnmol.kernels.SquareExponential(),
                                                               nugget_gram_matrix_fd=0.0, **kw)
    solver = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=nu, steprule=pnmol.odetools.step.Constant(dt),
                                                 spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
    sol = solver.solve_on_device(pde)
    assert len(sol.t) == K + 1
    _against_own_states(solver, sol, N, nu, bcond)


# ---- against the device's sampler ------------------------------------------------------------------------------------------------
def _unit_noise(T, D):
    """Host noise for S = 1 + 2 D T + D draws: draw 0 has none, every other draw one unit entry in one coordinate of one time."""
    S = 1 + 2 * D * T + D
    noise = [np.zeros((S, 2 * D)) for _ in range(T)] + [np.zeros((S, D))]
    i = 1
    for k in range(T + 1):
        for col in range(noise[k].shape[1]):
            noise[k][i, col] = 1.0
            i += 1
    assert i == S
    return noise


def _cov_from_draws(X, Wf):
    """W M M^T W^T from draws (S, T+1, D): the deviations from the noise-free draw 0 are the columns of the factor M."""
    B = np.einsum("qkd,skd->qs", Wf, X[1:] - X[:1])
    return B @ B.T


@pytest.mark.parametrize("case", [CASES[0], CASES[1]], ids=[sr.case_id(CASES[0]), sr.case_id(CASES[1])])
def test_against_the_sampler(hip_ctx, case):
    """`sample(sol, S, noise=unit vectors)` recovers the columns of the factor M of the joint covariance of the trajectory as the
    device's sampler draws it (the stage tests recover factor columns the same way), and W M M^T W^T is held against `cov` of
    `functionals` on the same states: two device routes that share the filtered states and the sweep's launch, nothing else.

    Bound, from the reference alone: the sampler's chain is restated in fp64 (`sample_reference.sample_step`, run on the same
    noise, deviations taken from its own noise-free draw), and e64 is the error of ITS W M M^T W^T against the longdouble truth
    of the functionals' covariance, in the metric max|X - X_true| / max|X_true|.  M M^T accumulates one term per time point,
    T + 1 of them, each a stage of the sampler held to `stage_reference.bound`; so |W M M^T W^T - cov| / max|cov_true| is held to
    (T + 1) * 16 max(e64, 2^-52)."""
    import sample_reference
    from pnmol import pdefilter
    from pnmol.base import rv

    tc, W, (_, ct), _ = _stage(case)
    c, T = tc.c, tc.T
    flt = _filter(c)
    states = _upload(flt, tc)
    ys = [rv.DeviceMultivariateNormal(m0, s) for (m0, _), s in zip(tc.states, states)]
    sol = pdefilter.PDESolution(t=tc.t, mean=np.stack([y.mean for y in ys]), ys=ys, info={}, diffusion_squared_calibrated=1.0)
    Wf = fr.flat_weights(W)
    noise = _unit_noise(T, c.D)
    X = c.solver.sample(sol, noise[0].shape[0], noise=noise)                    # (S, T+1, n, d), raw
    X = np.stack([[sr.flat(x) for x in draw] for draw in X])
    cov_s = _cov_from_draws(X, Wf)
    post = c.solver.functionals(sol, W)
    # the restated chain
    steps = []
    for (m0, P0), h in zip(tc.states, tc.dts):
        Pc, Pcinv = c.osolver.iwp.nordsieck_preconditioner(h)
        steps.append(sample_reference.sample_step(sr.flat(m0), P0, c.A, c.Q, c.Ql, Pc, Pcinv))
    mT, PT = sr.flat(tc.states[T][0]), tc.states[T][1]
    X64 = sample_reference.run_chain(mT, sample_reference.psd_factor(PT), steps, noise)
    e64 = fr.error(_cov_from_draws(X64, Wf), ct)
    allowed = (T + 1) * sr.bound(e64)
    scale = float(np.abs(ct).max())
    figures = {"sampler vs truth": fr.error(cov_s, ct), "sampler vs functionals": float(np.abs(cov_s - post.cov).max() / scale)}
    for name, v in figures.items():
        print(f"STAGE functionals {sr.case_id(case)} | {name} | e64 {e64:.2e} | device {v:.2e} | allowed {allowed:.2e}")
    for name, v in figures.items():
        assert v <= allowed, f"{name}: {v:.3e} > (T + 1) 16 max(e64 = {e64:.3e}, 2^-52)"
    np.testing.assert_array_equal(X[0, T], mT)                                  # the noise-free terminal draw is the mean


# ---- hygiene -----------------------------------------------------------------------------------------------------------------
def test_python_layer(hip_ctx):
    dt, K, N = 2.0 ** -7, 3, 24
    pde, solver, _, _ = make_pair(N, 1, dt, K, "dirichlet")
    sol = solver.solve(pde)
    W = np.stack([fn.space_time_mean(sol.t, N), fn.point(K, N, 2, 5)])
    post = solver.functionals(sol, W)
    assert post.mean.shape == (2,) and post.cov.shape == (2, 2) and post.std.shape == (2,)
    assert np.array_equal(post.std, np.sqrt(np.diag(post.cov)))
    cal = solver.functionals(sol, W, calibrated=True)
    assert np.array_equal(cal.cov, post.cov * sol.diffusion_squared_calibrated) and np.array_equal(cal.mean, post.mean)
    full = fn.checked_weights(W, K, 2, N)
    again = solver.functionals(sol, full)
    assert np.array_equal(again.mean, post.mean) and np.array_equal(again.cov, post.cov)
    for bad in (np.zeros((2, K, N)), np.zeros((2, K + 1, N + 1)), np.zeros((K + 1, N)), np.zeros((0, K + 1, N)),
                np.zeros((2, K + 1, 3, N))):
        with pytest.raises(ValueError, match="weights must have shape"):
            solver.functionals(sol, bad)
    W[1, 0, 0] = np.inf
    with pytest.raises(ValueError, match="finite"):
        solver.functionals(sol, W)
    for cls in (pnmol.sqrtform.LinearWhiteNoiseEK1, pnmol.latent.LinearLatentForceEK1):
        other = cls(num_derivatives=1, steprule=pnmol.odetools.step.Constant(dt))
        with pytest.raises(TypeError, match="white-noise"):
            other.functionals(sol, full)
    f32 = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(dt))
    f32.dtype = "f32"
    with pytest.raises(TypeError, match="fp64"):
        f32.functionals(sol, full)


def test_c_refusals(hip_ctx):
    dt, K, N = 2.0 ** -7, 3, 24
    pde, solver, _, _ = make_pair(N, 1, dt, K, "dirichlet")
    sol = solver.solve(pde)
    flt = sol._ys[-1].device_state.filter
    lib, n, d = flt.lib, flt.n, flt.d
    dp = ctypes.POINTER(ctypes.c_double)
    handles = [y.device_state.handle for y in sol._ys]
    dts = np.full(K, dt)
    w = np.ones((2, K + 1, n, d))
    mean, cov = np.full(2, 7.0), np.full((2, 2), 7.0)

    def call(f=flt.handle, T=K, filt=handles, dts=dts, Q=2, w=w, mean=mean, cov=cov):
        arr = None if filt is None else (ctypes.c_void_p * len(filt))(*filt)
        ptr = [None if a is None else a.ctypes.data_as(dp) for a in (dts, w, mean, cov)]
        rc = lib.pnmol_functionals(f, T, arr, ptr[0], Q, ptr[1], ptr[2], ptr[3])
        return rc, (lib.pnmol_last_error(flt.ctx.handle) or b"").decode()

    assert call(f=None)[0] == -1
    for kw, msg in ((dict(filt=None), "null pointer"), (dict(dts=None), "null pointer"), (dict(w=None), "null pointer"),
                    (dict(mean=None), "null pointer"), (dict(cov=None), "null pointer"),
                    (dict(Q=0), "Q < 1"), (dict(Q=65, w=np.ones((65, K + 1, n, d))), "above PNMOL_FUNCTIONALS_MAX_Q = 64"),
                    (dict(T=-1), "T < 0"),
                    (dict(dts=np.array([dt, 0.0, dt])), "dt <= 0 or not finite at step 1"),
                    (dict(dts=np.array([dt, dt, -dt])), "dt <= 0 or not finite at step 2"),
                    (dict(dts=np.array([np.inf, dt, dt])), "dt <= 0 or not finite at step 0"),
                    (dict(dts=np.array([dt, np.nan, dt])), "dt <= 0 or not finite at step 1"),
                    (dict(w=np.where(np.arange(w.size).reshape(w.shape) == 11, np.nan, w)), "weights not finite"),
                    (dict(w=np.where(np.arange(w.size).reshape(w.shape) == w.size - 1, -np.inf, w)), "weights not finite"),
                    (dict(filt=handles[:2] + [None] + handles[3:]), "null state at index 2")):
        rc, err = call(**kw)
        assert rc == -1 and err.startswith("pnmol_functionals: bad argument") and msg in err, (kw.keys(), rc, err)
    pde2, solver2, _, _ = make_pair(N, 1, dt, 1, "dirichlet")
    foreign = solver2.solve(pde2)._ys[0].device_state
    rc, err = call(filt=handles[:1] + [foreign.handle] + handles[2:])
    assert rc == -1 and "foreign state at index 1" in err
    assert np.all(mean == 7.0) and np.all(cov == 7.0)                          # nothing was written
    # fp32 and latent-force filters
    f32 = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(dt))
    f32.dtype = "f32"
    lat = pnmol.latent.LinearLatentForceEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(dt),
                                            spatial_kernel=pnmol.kernels.SquareExponential() + pnmol.kernels.WhiteNoise())
    for other in (f32, lat):
        osol = other.solve(pde)
        oflt = osol._ys[-1].device_state.filter
        rc, _ = call(f=oflt.handle, filt=[y.device_state.handle for y in osol._ys])
        assert rc == -1 and b"latent-force or fp32 filter" in lib.pnmol_last_error(oflt.ctx.handle)
    # between pnmol_filter_steps_begin and _end
    scratch = sol._ys[-1].device_state.clone()
    flt.steps_begin(scratch, 2, dt)
    rc, err = call()
    flt.steps_end(scratch)
    assert rc == -1 and "unfinished pnmol_filter_steps_begin" in err
    rc, err = call()
    assert rc == 0 and np.all(np.isfinite(mean)) and np.array_equal(cov, cov.T)
    # T = 0 needs no step sizes
    rc, err = call(T=0, filt=handles[:1], dts=None, w=np.ones((2, 1, n, d)))
    assert rc == 0, err


def test_recorder_and_observation_plan_survive(hip_ctx):
    """A call between two calls of the constant-step loop leaves a recorder and an observation plan of the filter as they were."""
    dt, N = 2.0 ** -7, 24
    pde, solver, _, _ = make_pair(N, 1, dt, 4, "dirichlet")
    sol = solver.solve(pde)
    flt = sol._ys[-1].device_state.filter
    slots = [flt.new_state() for _ in range(4)]
    flt.set_recorder(slots)
    H = np.zeros((1, N))
    H[0, N // 2] = 1.0
    flt.set_observations([sol.t[0] + 3 * dt], H, [[0.1]], [[1e-2]])

    def pending():
        return [flt.recorder_pending(), flt.observations_pending()]

    s = sol._ys[0].device_state.clone()
    flt.steps(s, 2, dt)
    before = pending()
    rec = [slots[i].cov() for i in range(2)]
    W = np.stack([fn.space_time_mean(sol.t, N)])
    post = solver.functionals(sol, W)
    assert pending() == before == [(2, 4), (0, 1)]
    assert all(np.array_equal(slots[i].cov(), rec[i]) for i in range(2))
    flt.steps(s, 2, dt)
    assert pending() == [(4, 4), (1, 1)]
    again = solver.functionals(sol, W)
    assert np.array_equal(again.mean, post.mean) and np.array_equal(again.cov, post.cov)
    flt.clear_recorder()
    flt.clear_observations()
