"""The filtered trajectory out of the device-resident loop and the backward pass in one call (`pnmol_filter_set_recorder`,
`pnmol_smoother_steps`, `solve_on_device`, `smooth_marginals`; csrc/pnmol_record.hip): recorded states against
`solve()`'s states, `solve_on_device` against the oracle, with sensor data, on the latent-force solver, cursor and lifetimes,
clearing, the post-filter features on the result, and the one-call backward pass against `smooth`.
Heat: dt = 2^-7, the recipe of tests/helpers.py; logistic: dt = 2^-6, the recipe of tests/test_gpu_reaction.py; Burgers: the recipe
of tests/convection_reference.py.  Run with -m gpu."""

import ctypes

import numpy as np
import pytest

import pnmol
import pnmol_oracle as oracle
import convection_reference as cref
import observe_reference as ref
from helpers import assert_mean_std_parity, assert_parity, make_pair, rel
from pnmol import _hip, data
from pnmol.pde import reactions
from smooth_reference import marginal_std, rts_on_oracle

pytestmark = pytest.mark.gpu

DT_HEAT = 2.0 ** -7
DT_REACTION = 2.0 ** -6

# Recorded states against the states of `solve()`, and the one-call backward pass against `smooth`: the same kernels on the same
# inputs in the same order, and k_record copies bits.  Measured on an MI355X over every case of this file that asserts it (means,
# marginal variances, full covariances, per grid time): 0.  Ten times the measured figure (the STAGE_BOUND convention of
# tests/test_gpu_reaction.py) is 0: the tests assert equality.
RECORD_BOUND = 0.0
# The std rows of `smooth_marginals` against `PDESolution.marginal_std` of `smooth`: the same variances read out by two
# arithmetics -- s0 sqrt(var) on the device (k_sm_readout, the loop's read-out) against sqrt(s0 s0 var) on the host -- so a last-place
# difference is what is expected (the one-ulp difference of DESIGN.md section 16; the variances themselves are equal bit for bit,
# which the kept states assert).  Largest |difference| / largest std measured on an MI355X: 1.49e-16 (N = 24), 1.80e-16 (N = 264),
# 1.38e-16 (adaptive steps); the bound is ten times the largest.
READOUT_STD_BOUND = 1.8e-15

# (kind, N, nu, boundary, steps): heat N = 24, nu = 2 has Dp = 96 (one tile of the 64 x 64 kernels, the tail of the copy); N = 33,
# nu = 1 has Dp = 128; 13 steps at N = 264 take the lead step eagerly, the ten-step graph and the pair graph; 8.3: a runt last step
CASES = [("heat", 24, 2, "dirichlet", 6), ("heat", 24, 2, "neumann", 6), ("heat", 33, 1, "dirichlet", 8.3), ("heat", 33, 1, "neumann", 8.3),
         ("heat", 40, 3, "dirichlet", 5), ("heat", 40, 3, "neumann", 5), ("heat", 264, 2, "dirichlet", 13), ("heat", 264, 2, "neumann", 13),
         ("logistic", 33, 2, "dirichlet", 8.3), ("logistic", 264, 2, "dirichlet", 13),
         ("burgers", 33, 2, "dirichlet", 8), ("burgers", 264, 2, "dirichlet", 13)]


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


def _reaction_kw(N, bcond, tmax):
    return dict(tmax=tmax, dx=1.0 / (N - 1), diffusion_rate=0.05, bcond=bcond, stencil_size_interior=3, stencil_size_boundary=3)


def product(kind, N, nu, bcond, K):
    """(pde, solver, dt) of the product."""
    if kind == "heat":
        pde, solver, _, _ = make_pair(N, nu, DT_HEAT, K, bcond)
        return pde, solver, DT_HEAT
    if kind == "burgers":
        return cref.product("burgers", N, nu, bcond, K * cref.DT) + (cref.DT,)
    pde = pnmol.pde.examples.reaction_diffusion_1d_discretized(reactions.logistic(1.0), kernel=pnmol.kernels.SquareExponential(),
                                                               nugget_gram_matrix_fd=0.0, **_reaction_kw(N, bcond, K * DT_REACTION))
    solver = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=nu, steprule=pnmol.odetools.step.Constant(DT_REACTION),
                                                 spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
    return pde, solver, DT_REACTION


_ORACLE = {}


def oracle_side(kind, N, nu, bcond, K):
    """(osolver, opde) of a case; `oracle_solve` adds the solution, computed once and shared (nothing modifies it)."""
    if kind == "heat":
        _, _, opde, osolver = make_pair(N, nu, DT_HEAT, K, bcond)
        return osolver, opde
    if kind == "burgers":
        osolver = oracle.WhiteNoiseEK1(num_derivatives=nu, steprule=oracle.Constant(cref.DT), semilinear=True,
                                       canonical_factor_signs=True, spatial_kernel=oracle.Matern52() + oracle.WhiteNoise())
        return osolver, cref.oracle_problem("burgers", N, bcond, K * cref.DT)
    opde = oracle.spruce_budworm_1d_discretized(kernel=oracle.SquareExponential(), **_reaction_kw(N, bcond, K * DT_REACTION))
    opde.f = lambda _t, x: x * (1.0 - x)
    opde.df = lambda _t, x: np.diag(1.0 - 2.0 * x)
    osolver = oracle.WhiteNoiseEK1(num_derivatives=nu, steprule=oracle.Constant(DT_REACTION), semilinear=True,
                                   canonical_factor_signs=True, spatial_kernel=oracle.Matern52() + oracle.WhiteNoise())
    return osolver, opde


def oracle_solve(*case):
    if case not in _ORACLE:
        osolver, opde = oracle_side(*case)
        osol = osolver.solve(opde)
        _ORACLE[case] = (osolver, osol) + tuple(oracle.read_mean_and_std(osol, osolver.E0))
    return _ORACLE[case]


def poison_new_states(monkeypatch):
    """Every state `Filter.new_state` hands out is full of NaN, so that an element the record copy misses shows."""
    plain = _hip.Filter.new_state

    def poisoned(self):
        s = plain(self)
        D = self.n * self.ds
        s.set(0.0, np.full((self.n, self.ds), np.nan), np.full((D, D), np.nan))
        return s

    monkeypatch.setattr(_hip.Filter, "new_state", poisoned)


def state_differences(ys, ys_ref, label):
    """Largest relative differences of mean, marginal variances and full covariance over the grid times; printed, returned."""
    assert len(ys) == len(ys_ref)
    worst = dict(mean=0.0, var=0.0, cov=0.0)
    for a, b in zip(ys, ys_ref):
        got = dict(mean=rel(a.device_state.mean(), b.device_state.mean()), var=rel(a.marginal_var, b.marginal_var),
                   cov=rel(a.cov, b.cov))
        for key, v in got.items():
            if np.isnan(v) or v > worst[key]:                   # (a NaN stays: nothing compares greater than it)
                worst[key] = v
    print(f"recorded vs solve, {label}: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    return worst


def assert_states_equal(sol, sol_ref, label):
    assert np.array_equal(sol.t, sol_ref.t)
    worst = state_differences(sol._ys, sol_ref._ys, label)
    for kind, v in worst.items():
        assert v <= RECORD_BOUND, (label, kind, v)
    # the host means of the result are those of the states (one read-back for all of them)
    for y in sol._ys:
        assert np.array_equal(y.mean, y.device_state.mean())
    assert np.array_equal(sol.mean, np.stack([y.mean for y in sol._ys]))


# --------------------------------------------------------------------------------------------- 1. + 2. recorded states, oracle
@pytest.mark.parametrize("kind,N,nu,bcond,K", CASES, ids=_ids(CASES))
def test_recorded_states_equal_solves_and_meet_the_oracle(hip_ctx, monkeypatch, kind, N, nu, bcond, K):
    pde, solver, dt = product(kind, N, nu, bcond, K)
    sol = solver.solve(pde)
    poison_new_states(monkeypatch)
    rec = solver.solve_on_device(pde)
    flt = solver._device_filter
    assert flt.recorder_pending() == (0, 0)
    if kind == "heat" and N in (24, 33):
        assert flt.dims()["dp"] * flt.n == {24: 96, 33: 128}[N]
    steps = int(np.ceil(K))
    assert rec.t.shape == (steps + 1,) and rec.mean.shape == sol.mean.shape and rec.info["num_steps"] == steps
    if steps != K:
        assert abs((rec.t[-1] - rec.t[-2]) - (K - steps + 1) * dt) < 1e-12
    assert_states_equal(rec, sol, f"{kind} N={N} nu={nu} {bcond} K={K}")
    assert rec.diffusion_squared_calibrated == sol.diffusion_squared_calibrated
    # 2. against the oracle
    osolver, osol, om, os_ = oracle_solve(kind, N, nu, bcond, K)
    assert np.allclose(rec.t, osol.t, rtol=0, atol=1e-15)
    assert_parity(rec.mean[:, 0], rec.marginal_std[:, 0], om, os_, nu)
    np.testing.assert_allclose(rec.diffusion_squared_calibrated, osol.diffusion_squared_calibrated, rtol=1e-5)


# ------------------------------------------------------------------------------------------------------------ 3. with data
def sensor_data(solver, pde, N, q, behind, at_t0):
    """Readings of q sensors behind the steps `behind` (and at t0): 1.02 x the model's own filtering mean plus noise of the size of
    its interior std there, so that the data moves the means and the innovation matrices stay well conditioned."""
    t, means, stds, _, _ = solver.solve_marginals(pde)
    C = ref.sensor_matrix(N, q)
    noise = float(np.median(stds[1:, 1:-1]))
    rng = np.random.default_rng(N + q)
    idx = ([0] if at_t0 else []) + [j for j in behind if j < len(t)]
    return [data.Observation(t[j], C, 1.02 * (C @ means[j]) + noise * rng.standard_normal(q), noise) for j in idx], means


DATA_CASES = [("heat", 33, 2, "dirichlet", 12.3, 1, True), ("heat", 33, 2, "dirichlet", 12.3, 4, False),
              ("burgers", 33, 2, "dirichlet", 12.3, 1, False), ("burgers", 33, 2, "dirichlet", 12.3, 4, True),
              ("heat", 264, 2, "dirichlet", 13, 4, False)]


@pytest.mark.parametrize("kind,N,nu,bcond,K,every,at_t0", DATA_CASES, ids=_ids(DATA_CASES))
def test_with_sensor_data_the_recorded_states_equal_solves(hip_ctx, monkeypatch, kind, N, nu, bcond, K, every, at_t0):
    """q = 8 sensors reporting behind every step / every 4th step, a reading at t0, a runt last step (12.3: the 13th step is short
    and, with data behind every step, carries a reading of its own); N = 264: updates behind steps that end a captured graph."""
    pde, solver, dt = product(kind, N, nu, bcond, K)
    steps = int(np.ceil(K))
    obs, plain = sensor_data(solver, pde, N, 8, range(every, steps + 1, every), at_t0)
    sol = solver.solve(pde, observations=obs)
    poison_new_states(monkeypatch)
    rec = solver.solve_on_device(pde, observations=obs)
    flt = solver._device_filter
    assert flt.recorder_pending() == (0, 0) and flt.observations_pending() == (0, 0)
    assert_states_equal(rec, sol, f"data {kind} N={N} every {every} t0 {at_t0}")
    lls, slls = rec.info["data_log_likelihoods"], sol.info["data_log_likelihoods"]
    print("log-likelihoods: largest relative difference", np.abs(np.array(lls) / np.array(slls) - 1.0).max())
    assert len(lls) == len(obs) == len(slls) and rec.info["num_steps"] == steps == sol.info["num_steps"]
    np.testing.assert_allclose(lls, slls, rtol=1e-4)              # (the bound of DESIGN.md section 19 for the loop against solve)
    np.testing.assert_allclose(rec.info["data_log_likelihood"], sol.info["data_log_likelihood"], rtol=1e-4)
    assert np.abs(rec.mean[:, 0] - plain).max() > 100 * 1e-5 * np.abs(plain).max()       # the data matters


# ------------------------------------------------------------------------------------------------------------ 4. latent force
def test_latent_force_solver_records_and_stays_refused_by_the_smoother(hip_ctx, monkeypatch):
    N, nu = 32, 1
    pde, solver, opde, osolver = ref.latent_pair(N, nu, ref.case_dt(nu), 9, "dirichlet", ref.KAPPA_MODEL)
    sol = solver.solve(pde)
    poison_new_states(monkeypatch)
    rec = solver.solve_on_device(pde)
    assert rec.mean.shape == (10, nu + 1, 2 * N)                                          # [u; eps]
    assert_states_equal(rec, sol, "latent force")
    assert np.abs(rec.mean[:, :, N:]).max() > 0.0
    with pytest.raises(TypeError, match="white-noise"):
        solver.smooth(rec)
    with pytest.raises(TypeError, match="white-noise"):
        solver.smooth_marginals(rec)
    semi = pnmol.latent.SemiLinearLatentForceEK1(num_derivatives=nu, steprule=pnmol.odetools.step.Constant(ref.case_dt(nu)))
    with pytest.raises(TypeError, match="linear PDE"):
        semi.solve_on_device(pde)


# ------------------------------------------------------------------------------------------------------------ 5. cursor, lifetimes
def _bound(N=24, nu=2, K=12):
    pde, solver, _, _ = make_pair(N, nu, DT_HEAT, K, "dirichlet")
    s0 = solver.initialize(pde).y.device_state
    flt = solver._device_filter
    flt.prepare_error_model(DT_HEAT)
    return flt, s0


def _snapshot(states):
    return [(s.mean(), s.marginal_var(), s.cov(), s.t) for s in states]


def _equal(a, b):
    return all(np.array_equal(x, y) for sa, sb in zip(a, b) for x, y in zip(sa, sb)) and len(a) == len(b)


def test_two_calls_that_fill_one_slot_list_equal_one_call(hip_ctx):
    flt, s0 = _bound()
    a, b = s0.clone(), s0.clone()
    slots = [flt.new_state() for _ in range(12)]
    flt.set_recorder(slots)
    assert flt.recorder_pending() == (0, 12)
    m1, s1, _ = flt.steps(a, 5, DT_HEAT)
    assert flt.recorder_pending() == (5, 12)
    m2, s2, _ = flt.steps(a, 7, DT_HEAT)
    assert flt.recorder_pending() == (12, 12)
    split = _snapshot(slots)
    split_means = flt.recorder_means()
    flt.set_recorder(slots)                                                       # (the cursor goes back to slot 0)
    mean_b, cov_b = b.mean(), b.cov()
    flt.prepare_steps(b, 12, DT_HEAT)                                             # a rehearsal: the state and the cursor come back
    assert flt.recorder_pending() == (0, 12) and np.array_equal(b.mean(), mean_b) and np.array_equal(b.cov(), cov_b)
    m, s, _ = flt.steps(b, 12, DT_HEAT)
    whole = _snapshot(slots)
    assert np.array_equal(np.vstack((m1, m2)), m) and np.array_equal(np.vstack((s1, s2)), s)
    assert _equal(split, whole)
    assert np.array_equal(split_means, np.stack([w[0] for w in whole])) and np.array_equal(flt.recorder_means(3, 4), split_means[3:7])
    np.testing.assert_allclose([w[3] for w in whole], s0.t + DT_HEAT * np.arange(1, 13), rtol=0, atol=1e-15)
    # the last slot is the state the loop ends in; the read-out rows are those of the slots
    assert np.array_equal(whole[-1][0], b.mean()) and np.array_equal(whole[-1][2], b.cov()) and whole[-1][3] == b.t
    assert np.array_equal(np.stack([w[0][0] for w in whole]), m)
    flt.clear_recorder()
    assert flt.recorder_pending() == (0, 0)


def test_recorder_refusals_and_lifetimes(hip_ctx):
    flt, s0 = _bound()
    lib, h = flt.lib, flt.handle
    err = lambda: lib.pnmol_last_error(flt.ctx.handle).decode()
    slots = [flt.new_state() for _ in range(4)]

    def set_raw(handles, f=h):
        arr = (ctypes.c_void_p * len(handles))(*handles)
        return lib.pnmol_filter_set_recorder(f, len(handles), arr)

    hs = [s.handle for s in slots]
    assert set_raw(hs, f=None) == -1
    assert set_raw([hs[0], None, hs[2]]) == -1 and "slot 1 is null" in err()
    assert set_raw([hs[0], hs[1], hs[0]]) == -1 and "slot 2 is the state of slot 0 again" in err()
    flt2, foreign = _bound()
    assert set_raw([hs[0], foreign.handle]) == -1 and "slot 1 is a state of another filter" in err()
    assert flt.recorder_pending() == (0, 0)
    # an fp32 filter
    f32 = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(DT_HEAT))
    f32.dtype = "f32"
    pde3, _, _, _ = make_pair(24, 1, DT_HEAT, 1, "dirichlet")
    s32 = f32.initialize(pde3).y.device_state
    slot32 = s32.filter.new_state()
    assert set_raw([slot32.handle], f=s32.filter.handle) == -1
    assert "fp32" in lib.pnmol_last_error(s32.filter.ctx.handle).decode()
    with pytest.raises(TypeError, match="fp64"):
        f32.solve_on_device(pde3)
    # between _begin and _end
    work = s0.clone()
    flt.steps_begin(work, 2, DT_HEAT)
    assert set_raw(hs) == -1 and "between pnmol_filter_steps_begin" in err()
    flt.steps_end(work)
    assert flt.recorder_pending() == (0, 0)
    # a set recorder: k beyond the slots left, the stepping state among the slots -- -1, nothing enqueued, the state untouched
    flt.set_recorder(slots)
    mean0, cov0, t0 = work.mean(), work.cov(), work.t
    assert lib.pnmol_filter_steps_begin(h, work.handle, 5, DT_HEAT) == -1
    assert "pnmol_filter_steps_begin" in err() and "5 step(s) asked for, 4 of 4" in err()
    with pytest.raises(_hip.PnmolHipError, match="recorder slot"):
        flt.steps(work, 5, DT_HEAT)
    assert lib.pnmol_filter_steps_begin(h, slots[3].handle, 1, DT_HEAT) == -1 and "one of the recorder's slots" in err()
    assert work.t == t0 and np.array_equal(work.mean(), mean0) and np.array_equal(work.cov(), cov0)
    assert flt.recorder_pending() == (0, 4)
    with pytest.raises(_hip.PnmolHipError, match="not been filled"):
        flt.recorder_means(0, 1)
    flt.steps(work, 3, DT_HEAT)
    assert flt.recorder_pending() == (3, 4)
    assert lib.pnmol_filter_steps_begin(h, work.handle, 2, DT_HEAT) == -1 and "2 step(s) asked for, 1 of 4" in err()
    assert np.array_equal(slots[2].mean(), work.mean()) and np.array_equal(slots[2].cov(), work.cov())
    # a live slot is not destroyed; after clearing it is
    raw = ctypes.c_void_p()
    assert lib.pnmol_state_create(h, ctypes.byref(raw)) == 0
    flt.set_recorder(slots + [_hip.State(flt, raw)])
    assert lib.pnmol_state_destroy(raw) == -1 and "recorder" in err()
    extra = flt._recorder[-1]
    flt.clear_recorder()
    assert flt.recorder_pending() == (0, 0)
    flt._live.pop(id(extra))
    extra.handle = None
    assert lib.pnmol_state_destroy(raw) == 0


# ------------------------------------------------------------------------------------------------------------ 6. clearing
@pytest.mark.parametrize("N", [24, 264])
def test_cleared_recorder_gives_the_bits_of_a_filter_that_never_had_one(hip_ctx, N):
    """The fused path again: means, stds and the final covariance of 12 steps."""
    flt, s0 = _bound(N=N)
    a, b, c = s0.clone(), s0.clone(), s0.clone()
    fresh = flt.steps(a, 12, DT_HEAT)
    slots = [flt.new_state() for _ in range(12)]
    flt.set_recorder(slots)
    recorded = flt.steps(b, 12, DT_HEAT)
    print(f"recorded (non-fused) against fused loop, N={N}: means {rel(recorded[0], fresh[0]):.2e}, stds {rel(recorded[1], fresh[1]):.2e}")
    flt.clear_recorder()
    del slots
    cleared = flt.steps(c, 12, DT_HEAT)
    assert np.array_equal(cleared[0], fresh[0]) and np.array_equal(cleared[1], fresh[1])
    assert [o.diffusion_squared_local for o in cleared[2]] == [o.diffusion_squared_local for o in fresh[2]]
    assert np.array_equal(a.mean(), c.mean()) and np.array_equal(a.cov(), c.cov()) and np.array_equal(a.marginal_var(), c.marginal_var())


# ------------------------------------------------------------------------------------------------------------ 7. post-filter features
def _heat_with_sensors():
    N, nu, K = 33, 2, 12
    pde, solver, opde, osolver = make_pair(N, nu, DT_HEAT, K, "dirichlet")
    obs, _ = sensor_data(solver, pde, N, 8, range(4, K + 1, 4), False)
    osol, _ = ref.drive(osolver, opde, obs)
    return pde, solver, obs, osolver, osol


def _logistic():
    case = ("logistic", 33, 2, "dirichlet", 12)
    pde, solver, _ = product(*case)
    osolver, osol = oracle_solve(*case)[:2]
    return pde, solver, None, osolver, osol


@pytest.mark.parametrize("make", [_heat_with_sensors, _logistic], ids=["heat-sensors", "logistic"])
def test_post_filter_features_work_on_the_result(hip_ctx, make):
    pde, solver, obs, osolver, osol = make()
    kw = {} if obs is None else dict(observations=obs)
    rec = solver.solve_on_device(pde, **kw)
    sol = solver.solve(pde, **kw)
    # smooth: the tolerances of tests/test_gpu_smooth.py against the NumPy RTS pass over the oracle's filtered trajectory
    ms, Ps = rts_on_oracle(osolver, osol)
    ostd = marginal_std(Ps, *osol.mean.shape[1:])
    srec = solver.smooth(rec)
    assert np.array_equal(srec.t, rec.t) and srec.info == rec.info and srec.smoothed
    assert_mean_std_parity(srec.mean[:, 0], srec.marginal_std[:, 0], ms[:, 0], ostd[:, 0])
    # sample: the draws of the solve() solution
    a, b = solver.sample(rec, 4, seed=1), solver.sample(sol, 4, seed=1)
    print(f"sample on solve_on_device vs solve: {rel(a, b):.3e}")
    assert a.shape == (4, len(rec.t), 3, 33) and rel(a, b) <= RECORD_BOUND
    # dense output between grid times: the filtering solution by prediction, the smoothed one from its bridges
    tq = np.array([rec.t[2] + 0.3 * (rec.t[3] - rec.t[2]), rec.t[5], rec.t[-1] + 0.5 * DT_HEAT])
    da, db = rec(tq), sol(tq)
    assert np.array_equal(da.mean, db.mean) and np.array_equal(da.marginal_std, db.marginal_std)
    assert np.array_equal(da.mean[1], rec.mean[5])
    ds, dr = srec(tq[:1]), solver.smooth(sol)(tq[:1])
    assert np.all(np.isfinite(ds.mean)) and np.array_equal(ds.mean, dr.mean) and np.array_equal(ds.marginal_std, dr.marginal_std)
    st = rec.state_at(float(tq[0]))
    assert np.array_equal(st.mean, sol.state_at(float(tq[0])).mean)


# ------------------------------------------------------------------------------------------------------------ 8. backward pass
def _smooth_inputs(which):
    if which == "adaptive":
        pde, solver, _, _ = make_pair(64, 2, DT_HEAT, 24, "neumann")
        solver.steprule = pnmol.odetools.step.Adaptive(abstol=1e-4, reltol=1e-3)
        sol = solver.solve(pde)
        assert len(set(np.round(np.diff(sol.t), 14))) > 2
        return solver, sol
    pde, solver, _, _ = make_pair(which, 2, DT_HEAT, 6, "dirichlet")
    return solver, solver.solve_on_device(pde)


@pytest.mark.parametrize("which", [24, 264, "adaptive"])
def test_backward_pass_in_one_call_equals_smooth(hip_ctx, which):
    solver, sol = _smooth_inputs(which)
    ssol = solver.smooth(sol, dense=None)
    means, stds = solver.smooth_marginals(sol)
    T = len(sol.t) - 1
    assert means.shape == stds.shape == (T + 1, sol.mean.shape[2])
    worst = dict(mean=rel(means, ssol.mean[:, 0]), std=rel(stds, ssol.marginal_std[:, 0]))
    flt = sol._ys[0].device_state.filter
    m2, s2, kept = flt.smoother_steps([y.device_state for y in sol._ys], np.diff(sol.t), keep=True)
    assert np.array_equal(m2, means) and np.array_equal(s2, stds) and len(kept) == T + 1
    for k, (a, b) in enumerate(zip(kept, ssol._ys)):
        assert a.t == sol.t[k]
        worst["state mean"] = max(worst.get("state mean", 0.0), rel(a.mean(), b.device_state.mean()))
        worst["state var"] = max(worst.get("state var", 0.0), rel(a.marginal_var(), b.marginal_var))
        worst["state cov"] = max(worst.get("state cov", 0.0), rel(a.cov(), b.cov))
    print(f"one-call backward pass vs smooth ({which}): " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for kind, v in worst.items():
        assert v <= (READOUT_STD_BOUND if kind == "std" else RECORD_BOUND), (kind, v)
    # the terminal row is the filtered state's, and a second pass gives the same bits (the rotating states carry nothing over)
    assert np.array_equal(means[-1], sol.mean[-1, 0]) and np.array_equal(kept[-1].cov(), sol._ys[-1].cov)
    again = solver.smooth_marginals(sol)
    assert np.array_equal(again[0], means) and np.array_equal(again[1], stds)
    # the input is unchanged
    assert np.array_equal(sol._ys[2].device_state.mean(), sol.mean[2])


def test_smoother_steps_argument_checks(hip_ctx):
    pde, solver, _, _ = make_pair(24, 2, DT_HEAT, 3, "dirichlet")
    sol = solver.solve_on_device(pde)
    states = [y.device_state for y in sol._ys]
    flt = states[0].filter
    lib, h = flt.lib, flt.handle
    err = lambda: lib.pnmol_last_error(flt.ctx.handle).decode()
    T = 3
    means, stds = np.empty((T + 1, 24)), np.empty((T + 1, 24))
    dp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    outs = [flt.new_state() for _ in range(T + 1)]
    before = [s.cov() for s in states]

    def call(f=h, T=T, filt=states, dts=(DT_HEAT,) * 3, out=None, null_filt=False, null_dt=False):
        fa = (ctypes.c_void_p * len(filt))(*[None if s is None else s.handle for s in filt])
        oa = None if out is None else (ctypes.c_void_p * len(out))(*[None if s is None else s.handle for s in out])
        d = np.array(dts, dtype=np.float64)
        return lib.pnmol_smoother_steps(f, T, None if null_filt else fa, None if null_dt else dp(d), oa, dp(means), dp(stds), None)

    assert call(f=None) == -1
    for kw, why in ((dict(T=0), "T < 1"), (dict(null_filt=True), "no filtered states"), (dict(null_dt=True), "no step sizes"),
                    (dict(filt=states[:2] + [None] + states[3:]), "null state at index 2"),
                    (dict(out=outs[:1] + [None] + outs[2:]), "null state at index 1"),
                    (dict(dts=(DT_HEAT, 0.0, DT_HEAT)), "dt <= 0 at step 1"), (dict(dts=(DT_HEAT, DT_HEAT, -DT_HEAT)), "dt <= 0 at step 2"),
                    (dict(dts=(DT_HEAT, float("nan"), DT_HEAT)), "dt <= 0 at step 1"),
                    (dict(out=outs[:3] + [states[0]]), "a state of out is one of filt"),
                    (dict(out=[states[1]] + outs[1:]), "a state of out is one of filt"),
                    (dict(out=outs[:3] + [outs[0]]), "listed twice in out")):
        assert call(**kw) == -1, kw
        assert "pnmol_smoother_steps" in err() and why in err(), (kw, err())
    pde2, solver2, _, _ = make_pair(24, 2, DT_HEAT, 1, "dirichlet")
    foreign = solver2.solve(pde2)._ys[0].device_state
    assert call(filt=[foreign] + states[1:]) == -1 and "foreign state at index 0" in err()
    assert call(out=outs[:2] + [foreign] + outs[3:]) == -1 and "foreign state at index 2" in err()
    # a latent-force and an fp32 filter
    lpde, lsolver, _, _ = ref.latent_pair(24, 1, DT_HEAT, 2, "dirichlet", ref.KAPPA_MODEL)
    lstates = [y.device_state for y in lsolver.solve(lpde)._ys]
    lmeans = np.empty((3, 24))
    la = (ctypes.c_void_p * 3)(*[s.handle for s in lstates])
    ld = np.array([DT_HEAT, DT_HEAT])
    assert lib.pnmol_smoother_steps(lstates[0].filter.handle, 2, la, dp(ld), None, dp(lmeans), None, None) == -1
    assert "latent-force or fp32" in lib.pnmol_last_error(lstates[0].filter.ctx.handle).decode()
    f32 = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(DT_HEAT))
    f32.dtype = "f32"
    pde3, _, _, _ = make_pair(24, 1, DT_HEAT, 2, "dirichlet")
    fstates = [y.device_state for y in f32.solve(pde3)._ys]
    fa = (ctypes.c_void_p * 3)(*[s.handle for s in fstates])
    assert lib.pnmol_smoother_steps(fstates[0].filter.handle, 2, fa, dp(ld), None, dp(lmeans), None, None) == -1
    with pytest.raises(TypeError, match="fp64"):
        f32.smooth_marginals(f32.solve(pde3))
    # nothing was enqueued by any of the refused calls; the call itself works, with and without out and outputs
    assert all(np.array_equal(s.cov(), b) for s, b in zip(states, before))
    assert call() == 0 and call(out=outs) == 0
    info = (ctypes.c_int * T)()
    fa = (ctypes.c_void_p * (T + 1))(*[s.handle for s in states])
    d = np.full(T, DT_HEAT)
    assert lib.pnmol_smoother_steps(h, T, fa, dp(d), None, None, None, info) == 0 and list(info) == [0, 0, 0]
    assert np.array_equal(outs[-1].cov(), states[-1].cov()) and outs[0].t == states[0].t
    with pytest.raises(ValueError):
        flt.smoother_steps(states[:1], [])
