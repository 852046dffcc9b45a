"""Driven problems on the device (`pnmol.pde.forcing`, `pnmol_filter_set_forcing`, `pnmol_filter_force_at`; csrc/pnmol_forcing.hip,
DESIGN.md section 25): the forced innovation against the unforced one row by row, `solve()`, `solve_marginals` and `solve_on_device`
against the forced oracle (tests/forcing_reference.py, which fixes the cases) and against each other bit for bit, composition with
the terms the device linearises, sensor data, linearisation points and the iterated smoother, the backward pass on forced
solutions, and the refusals of the C ABI.  Shapes: (20, 1) m = 22 in mp = 32; (33, 2) m = 35 in mp = 64; (32, 2, neumann) flux data
with R_sqrtm; (260, 1) mp = 288, the second workgroup of the 256-thread launch.  Run with -m gpu."""

import ctypes

import numpy as np
import pytest

import forcing_reference as fr
import iterated_reference as ir
import pnmol
import pnmol_oracle as oracle
from helpers import assert_mean_std_parity, per_step, rel
from pnmol import _hip, data
from pnmol import functionals as fn
from pnmol._hip import _dp
from pnmol.pde import reactions
from smooth_reference import marginal_std, rts_on_oracle

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
ALL_SHAPES = fr.SHAPES + [fr.BIG[:3]]


def _steps_of(shape):
    return fr.BIG[3] if shape == fr.BIG[:3] else fr.STEPS


def _bound(shape, mode):
    """(pde, solver, filter, initial device state) of a linear case, the device bound."""
    pde, solver, _, _ = fr.linear_pair(*shape, mode, K=_steps_of(shape))
    s0 = solver.initialize(pde).y.device_state
    return pde, solver, solver._device_filter, s0


def _species_parity(name, means, stds, omeans, ostds):
    """North-star tolerances (helpers.assert_mean_std_parity); per species for the system, whose components differ in size."""
    C = 2 if fr.TERMS[name].kind == "lotka_volterra" else 1
    N = means.shape[-1] // C
    for c in range(C):
        part = slice(c * N, (c + 1) * N)
        assert_mean_std_parity(means[..., part], stds[..., part], omeans[..., part], ostds[..., part])


def _assert_states_bitwise(got, want, label):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a.mean(), b.mean()), (label, k, "mean", rel(a.mean(), b.mean()))
        assert np.array_equal(a.marginal_var(), b.marginal_var()), (label, k, "var")
        assert np.array_equal(a.cov(), b.cov()), (label, k, "cov", rel(a.cov(), b.cov()))


# ------------------------------------------------------------------------------------------------------------------ 1. stage
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_forced_innovation_is_the_unforced_one_minus_rhs(hip_ctx, shape):
    """One `pnmol_filter_step` unforced and one behind `force_at(rhs)` on one linear filter: z_f against z_u - rhs row by row at
    4 eps (|z_u| + |rhs|) -- both sides are at most two roundings from the same dot product --, the padded rows exactly 0, and
    `force_at(NULL)` gives z_u back bit for bit."""
    pde, solver, flt, s0 = _bound(shape, "both")
    dims = flt.dims()
    m, mp = dims["m"], dims["mp"]
    assert m == shape[0] + 2 and mp > m and mp % 32 == 0
    dt = fr.DT
    flt.prepare_error_model(dt)
    rhs = pde.forcing.rhs(dt, pde)
    assert np.abs(rhs[:-2]).max() > 0.1 and np.all(rhs[-2:] != 0.0)
    out_u, info_u, err_u = flt.step(s0, dt)
    z_u = flt.debug_read(4, mp)
    flt.force_at(rhs)
    out_f, info_f, err_f = flt.step(s0, dt)
    z_f = flt.debug_read(4, mp)
    want = z_u[:m] - rhs
    excess = np.abs(z_f[:m] - want) / (4 * EPS * (np.abs(z_u[:m]) + np.abs(rhs)))
    print(f"{shape}: forced innovation off z_u - rhs by at most {excess.max():.2f} of the bound; moved by {np.abs(z_f - z_u).max():.3f}")
    assert np.all(excess <= 1.0)
    assert not z_f[m:].any() and not z_u[m:].any()
    assert np.abs(z_f[:m] - z_u[:m]).max() > 0.1                # the forcing is there
    # forcing enters the means only: the covariance and the error model's diagonal are those of the unforced step
    assert np.array_equal(out_f.cov(), out_u.cov()) and not np.array_equal(out_f.mean(), out_u.mean())
    assert np.isfinite(info_f.error_sigma2) and np.all(np.isfinite(err_f)) and info_f.error_sigma2 != info_u.error_sigma2
    np.testing.assert_allclose(err_f / np.sqrt(info_f.error_sigma2), err_u / np.sqrt(info_u.error_sigma2), rtol=1e-14)
    # the same right-hand side again: the same bits (the forced shift lives in a buffer of its own)
    out_f2, _, _ = flt.step(s0, dt)
    assert np.array_equal(flt.debug_read(4, mp), z_f) and np.array_equal(out_f2.mean(), out_f.mean())
    flt.force_at(None)
    out_b, info_b, err_b = flt.step(s0, dt)
    assert np.array_equal(flt.debug_read(4, mp), z_u)
    assert np.array_equal(out_b.mean(), out_u.mean()) and np.array_equal(out_b.cov(), out_u.cov())
    assert info_b.error_sigma2 == info_u.error_sigma2 and np.array_equal(err_b, err_u)


# ------------------------------------------------------------------------------------------------------------------ 2. oracle
@pytest.mark.parametrize("mode", fr.MODES)
@pytest.mark.parametrize("shape", fr.SHAPES)
def test_solves_meet_the_forced_oracle(hip_ctx, shape, mode):
    pde, solver, _, _ = fr.linear_pair(*shape, mode)
    osol, om, os_ = fr.linear_reference(*shape, mode)
    sol = solver.solve(pde)
    np.testing.assert_allclose(sol.t, osol.t, rtol=0, atol=1e-15)
    assert_mean_std_parity(sol.mean[:, 0], sol.marginal_std[:, 0], om, os_)
    t, means, stds, sig, final = solver.solve_marginals(pde)
    assert solver._device_filter.forcing_pending() == (0, 0)    # (cleared behind the solve)
    assert_mean_std_parity(means, stds, om, os_)
    rec = solver.solve_on_device(pde)
    assert_mean_std_parity(rec.mean[:, 0], rec.marginal_std[:, 0], om, os_)
    if shape[2] == "dirichlet" and mode != "source":            # the boundary nodes follow g
        g = np.stack([pde.forcing.boundary(tk, pde) for tk in t])
        np.testing.assert_allclose(means @ pde.B.T, g, rtol=0, atol=1e-5 * np.abs(om).max())


def test_big_case_meets_the_forced_oracle(hip_ctx):
    N, nu, bcond, K = fr.BIG
    pde, solver, _, _ = fr.linear_pair(N, nu, bcond, "both", K=K)
    osol, om, os_ = fr.linear_reference(N, nu, bcond, "both", K)
    t, means, stds, sig, final = solver.solve_marginals(pde)
    assert solver._device_filter.dims()["mp"] == 288
    assert_mean_std_parity(means, stds, om, os_)
    sm, ss, ssig = per_step(solver, pde)
    assert np.array_equal(means, sm) and np.array_equal(sig, ssig)


def test_adaptive_solve_follows_the_oracles_accept_reject_sequence(hip_ctx):
    kw = dict(abstol=1e-4, reltol=1e-3)
    pde, solver, opde, osolver = fr.linear_pair(33, 2, "dirichlet", "both", K=24)
    solver.steprule = pnmol.odetools.step.Adaptive(**kw)
    osolver.steprule = oracle.Adaptive(**kw)
    # The first step of the rule is |y0| / |f(t0, y0)| where a problem has an `f`, else |y0| / |L y0| (step.py:109-133).  The
    # oracle carries the source as f = s only as its vehicle; the problem is the linear one on both sides, and so is its first step.
    first = solver.steprule.first_dt(pde)
    assert np.isclose(first, 0.01 * np.linalg.norm(opde.y0) / np.linalg.norm(opde.L @ opde.y0), rtol=1e-12, atol=0.0)
    osolver.steprule.first_dt = lambda _pde: first
    sol = solver.solve(pde)
    osol = osolver.solve(opde)
    print(f"adaptive: {sol.info['num_steps']} steps, {sol.info['num_attempted_steps']} attempts")
    assert sol.info == osol.info and sol.info["num_steps"] > 3
    np.testing.assert_allclose(sol.t, osol.t, rtol=1e-9)
    om, os_ = oracle.read_mean_and_std(osol, osolver.E0)
    assert_mean_std_parity(sol.mean[:, 0], sol.marginal_std[:, 0], om, os_)


@pytest.mark.parametrize("mode", ["source", "boundary", "both"])
def test_latent_force_solver_meets_the_forced_oracle(hip_ctx, mode):
    """Both halves of the d_state = 2 d state -- the solution u and the latent force eps, which the source moves from the
    first update on --, every derivative, of `solve()` and of `solve_on_device` against the forced oracle (as
    tests/test_gpu_observe.py reads the oracle's stacked factor); the read-out of `solve_marginals` against its state half."""
    import observe_reference as oref

    N, nu, _ = fr.LATENT
    n = nu + 1
    pde, solver, _, _ = fr.latent_pair(mode)
    osol, om, os_ = fr.latent_reference(mode)
    ovar = np.einsum("tij,tij->ti", osol.cov_sqrtm, osol.cov_sqrtm)
    ostd = np.sqrt(np.stack([oref.unflat_state(v, n, True) for v in ovar]))
    sol = solver.solve(pde)
    rec = solver.solve_on_device(pde)
    assert sol.mean.shape == rec.mean.shape == osol.mean.shape == (fr.STEPS + 1, n, 2 * N)
    for got in (sol, rec):
        std = got.marginal_std
        for a in range(n):
            for half in (slice(0, N), slice(N, 2 * N)):
                assert_mean_std_parity(got.mean[:, a, half], std[:, a, half], osol.mean[:, a, half], ostd[:, a, half])
    assert np.array_equal(rec.mean, sol.mean)
    t, means, stds, sig, final = solver.solve_marginals(pde)
    assert means.shape == (fr.STEPS + 1, N)
    assert_mean_std_parity(means, stds, om, os_)
    assert np.array_equal(means, sol.mean[:, 0, :N])


# ------------------------------------------------------------------------------------------------------------------ 3. bits
@pytest.mark.parametrize("shape,mode", [(fr.SHAPES[0], "both"), (fr.SHAPES[1], "both"), (fr.SHAPES[2], "boundary"),
                                        (fr.SHAPES[1], "source")])
def test_loop_routes_equal_solve_bit_for_bit(hip_ctx, shape, mode):
    """`solve_marginals` and `solve_on_device` against `solve()` on the forced problem, bit for bit: means, sigma^2, the marginal
    variances and stds of every state, the covariance of every state and of the final one.  The std ROWS that `solve_marginals`
    reads out itself have no counterpart of the same arithmetic in `solve()`: the loop forms s0 sqrt(var) on the device, a
    state's std is sqrt(s0 s0 var) on the host -- the last-place difference of DESIGN.md section 16, which an unforced problem
    shows as well (tests/test_gpu_iterated.py holds it to 2 ulp beside the variances' equality; measured here: 2.0 ulp at every
    shape).  So the rows are held to 2 ulp, beside the equality of the variances they are read out from."""
    pde, solver, _, _ = fr.linear_pair(*shape, mode)
    sol = solver.solve(pde)
    sm, ss, ssig = per_step(solver, pde)
    t, means, stds, sig, final = solver.solve_marginals(pde)
    rec = solver.solve_on_device(pde)
    assert np.array_equal(t, sol.t) and np.array_equal(rec.t, sol.t)
    assert np.array_equal(means, sm) and np.array_equal(rec.mean, sol.mean)
    assert np.array_equal(sig, ssig) and rec.diffusion_squared_calibrated == sol.diffusion_squared_calibrated
    _assert_states_bitwise([y.device_state for y in rec._ys], [y.device_state for y in sol._ys], (shape, mode))
    assert np.array_equal(rec.marginal_std, sol.marginal_std)
    assert np.array_equal(final.y.device_state.cov(), sol._ys[-1].device_state.cov())
    assert np.array_equal(final.y.device_state.marginal_var(), sol._ys[-1].device_state.marginal_var())
    ulps = np.abs(stds - ss) / np.spacing(np.maximum(np.abs(stds), np.abs(ss)))
    print(f"{shape} {mode}: the loop's own std rows off sqrt(var) of solve()'s states by at most {ulps.max():.1f} ulp")
    assert ulps.max() <= 2.0


def test_two_calls_equal_one_call_and_the_rehearsal_rewinds(hip_ctx):
    shape = fr.SHAPES[1]
    pde, solver, flt, s0 = _bound(shape, "both")
    ts, dts = solver._constant_schedule(pde, None)
    table = pde.forcing.table(ts, pde)
    flt.prepare_error_model(fr.DT)
    a, b = s0.clone(), s0.clone()
    flt.set_forcing(table)
    assert flt.forcing_pending() == (0, 12)
    flt.prepare_steps(a, 12, fr.DT)                             # the rehearsal consumes no row and leaves the state alone
    assert flt.forcing_pending() == (0, 12) and np.array_equal(a.mean(), s0.mean()) and np.array_equal(a.cov(), s0.cov())
    m, s, i = flt.steps(a, 12, fr.DT)
    assert flt.forcing_pending() == (12, 12)
    flt.set_forcing(table)                                      # the same table again: the cursor goes back to row 0
    assert flt.forcing_pending() == (0, 12)
    m1, s1, i1 = flt.steps(b, 5, fr.DT)
    assert flt.forcing_pending() == (5, 12)
    m2, s2, i2 = flt.steps(b, 7, fr.DT)
    assert flt.forcing_pending() == (12, 12)
    flt.clear_forcing()
    assert np.array_equal(np.vstack((m1, m2)), m) and np.array_equal(np.vstack((s1, s2)), s)
    assert [o.diffusion_squared_local for o in list(i1) + list(i2)] == [o.diffusion_squared_local for o in i]
    assert [o.error_sigma2 for o in list(i1) + list(i2)] == [o.error_sigma2 for o in i]
    assert all(np.isfinite(o.error_sigma2) for o in i)          # without a term the loop keeps the error model
    assert np.array_equal(a.mean(), b.mean()) and np.array_equal(a.cov(), b.cov()) and a.t == b.t


def test_second_table_on_the_same_filter_replays_the_graphs(hip_ctx):
    """A table that fits the one before it is overwritten in place and the captured graphs of the first run serve the second: its
    result equals that of a fresh filter bit for bit."""
    shape = fr.SHAPES[0]
    pde, solver, flt, s0 = _bound(shape, "both")
    ts, _ = solver._constant_schedule(pde, None)
    table = pde.forcing.table(ts, pde)
    second = np.ascontiguousarray(-0.7 * table[::-1])
    flt.prepare_error_model(fr.DT)
    flt.set_forcing(table)
    first = flt.steps(s0.clone(), fr.STEPS, fr.DT)
    flt.set_forcing(second)
    assert flt.forcing_pending() == (0, fr.STEPS)
    w = s0.clone()
    again = flt.steps(w, fr.STEPS, fr.DT)
    assert np.abs(again[0] - first[0]).max() > 1e-3 * np.abs(first[0]).max()
    _, _, oflt, q0 = _bound(shape, "both")
    oflt.prepare_error_model(fr.DT)
    oflt.set_forcing(second)
    fresh = oflt.steps(q0, fr.STEPS, fr.DT)
    assert np.array_equal(again[0], fresh[0]) and np.array_equal(again[1], fresh[1])
    assert [o.diffusion_squared_local for o in again[2]] == [o.diffusion_squared_local for o in fresh[2]]
    assert np.array_equal(w.mean(), q0.mean()) and np.array_equal(w.cov(), q0.cov())


def test_zero_table_and_cleared_table_give_the_unforced_bits(hip_ctx):
    """On the filter of the unforced problem: an all-zero table gives the unforced `solve()` result bit for bit (0 - 0 = +0 is the
    shift a linear filter has anyway), and a filter whose table was cleared gives the bits of a filter that never had one."""
    shape = fr.SHAPES[1]
    forced_pde, forced_solver, _, _ = fr.linear_pair(*shape, "both")
    pde, solver, _, _ = fr.linear_pair(*shape, None)
    sm, ss, ssig = per_step(solver, pde)                        # the unforced solve()
    p0 = solver.initialize(pde).y.device_state
    flt = solver._device_filter
    flt.prepare_error_model(fr.DT)
    flt.set_forcing(np.zeros((12, flt.m)))
    zstate = p0.clone()
    zero = flt.steps(zstate, 12, fr.DT)
    assert flt.forcing_pending() == (12, 12)
    assert np.array_equal(zero[0], sm[1:]) and [o.diffusion_squared_local for o in zero[2]] == list(ssig)
    last = solver.solve(pde)._ys[-1].device_state               # (binds a new filter; `flt` keeps its own)
    assert np.array_equal(zstate.mean(), last.mean()) and np.array_equal(zstate.cov(), last.cov())
    assert np.array_equal(zstate.marginal_var(), last.marginal_var())
    # a table that matters, then cleared
    ts, _ = forced_solver._constant_schedule(forced_pde, None)
    flt.set_forcing(forced_pde.forcing.table(ts, forced_pde))
    forced = flt.steps(p0.clone(), 12, fr.DT)
    assert np.abs(forced[0] - zero[0]).max() > 1e-2
    flt.clear_forcing()
    assert flt.forcing_pending() == (0, 0)
    state = p0.clone()
    cleared = flt.steps(state, 12, fr.DT)
    # ... against a filter that never had one
    other = fr.linear_pair(*shape, None)[1]
    q0 = other.initialize(pde).y.device_state
    other._device_filter.prepare_error_model(fr.DT)
    fresh = other._device_filter.steps(q0, 12, fr.DT)
    assert np.array_equal(cleared[0], fresh[0]) and np.array_equal(cleared[1], fresh[1])
    assert [o.diffusion_squared_local for o in cleared[2]] == [o.diffusion_squared_local for o in fresh[2]]
    assert [o.error_sigma2 for o in cleared[2]] == [o.error_sigma2 for o in fresh[2]]
    assert np.array_equal(state.mean(), q0.mean()) and np.array_equal(state.cov(), q0.cov())


def test_host_callable_route_meets_the_forced_oracle(hip_ctx):
    """The route such a problem had to take before: `SemiLinearWhiteNoiseEK1` on host callables with f(t, u) = s(t), no
    `pde.forcing`.  Not a bit test: it keeps the old route honest against the same oracle."""
    shape = fr.SHAPES[1]
    pde, solver, _, _ = fr.host_route_pair(*shape)
    assert getattr(pde, "forcing", None) is None
    osol, om, os_ = fr.linear_reference(*shape, "source")
    sol = solver.solve(pde)
    assert solver._device_filter.reaction is None and solver._device_filter.forcing_pending() == (0, 0)
    assert_mean_std_parity(sol.mean[:, 0], sol.marginal_std[:, 0], om, os_)


# ------------------------------------------------------------------------------------------------------------------ 4. composition
@pytest.mark.parametrize("name", list(fr.TERMS))
def test_terms_compose_with_forcing(hip_ctx, name):
    """A term the device linearises plus forcing, through `solve_marginals` against the forced oracle; `solve()` of the same
    solver gives the same means bit for bit."""
    pde, solver, _, _ = fr.term_pair(name)
    osol, om, os_ = fr.term_reference(name)
    t, means, stds, sig, final = solver.solve_marginals(pde)
    assert solver._device_filter.reaction is pde.reaction and len(t) == fr.TERM_STEPS + 1
    _species_parity(name, means, stds, om, os_)
    sm, ss, ssig = per_step(solver, pde)
    assert np.array_equal(means, sm) and np.array_equal(sig, ssig)
    _, plain, _ = fr.term_reference(name, False)
    assert np.abs(means - plain).max() > 100 * 1e-5 * np.abs(plain).max()


@pytest.mark.parametrize("name", list(fr.TERMS))
def test_terms_compose_with_forcing_sensor_data_and_linearisation_points(hip_ctx, name):
    """... with `observations=` of a shared sensor array, and with `linearize_at` (the forced oracle's own filtering means as the
    points, injected into the oracle too)."""
    import observe_reference as oref

    pde, solver, opde, osolver = fr.term_pair(name)
    obs = fr.term_observations(name)
    osol, _ = oref.drive(osolver, opde, obs)
    om, os_ = oracle.read_mean_and_std(osol, osolver.E0)
    t, means, stds, sig, final, info = solver.solve_marginals(pde, observations=obs)
    _species_parity(name, means, stds, om, os_)
    np.testing.assert_allclose(info["data_log_likelihoods"], osol.info["data_log_likelihoods"], rtol=1e-4)
    _, forced, _ = fr.term_reference(name)
    assert np.abs(means - forced).max() > 10 * 1e-5 * np.abs(forced).max()      # the data matters
    # linearisation points: the filtering means of the plain forced run, shifted a little, in product and oracle alike
    points = 1.01 * forced[1:]
    osolver.set_points(points)
    try:
        psol = osolver.solve(opde)
    finally:
        osolver.set_points(None)
    pm, ps = oracle.read_mean_and_std(psol, osolver.E0)
    t, means, stds, sig, final = solver.solve_marginals(pde, linearize_at=points)
    _species_parity(name, means, stds, pm, ps)
    assert solver._device_filter.forcing_pending() == (0, 0) and solver._device_filter.linearization_pending() == (0, 0)


def test_iterated_smoother_on_the_forced_logistic_case(hip_ctx):
    name = "logistic-source"
    pde, solver, opde, osolver = fr.term_pair(name)
    it = ir.iterate(osolver, opde)
    got = solver.solve_iterated(pde, iterations=ir.ITERATIONS, tol=ir.TOL)
    print(f"forced logistic: reference increments {it.increments}, device {got.increments}")
    assert it.converged and got.converged and abs(got.num_iterations - it.num_iterations) <= 1
    assert_mean_std_parity(got.means, got.stds, it.means, it.stds)
    assert solver._device_filter.forcing_pending() == (0, 0)


# ------------------------------------------------------------------------------------------------------------------ 5. backward pass
@pytest.mark.parametrize("shape", fr.SHAPES)
def test_backward_pass_on_a_forced_solution(hip_ctx, shape):
    """`smooth`, `smooth_marginals` and `functionals` on a forced `solve_on_device` result against the dense NumPy RTS over the
    forced oracle trajectory, at the tolerances of tests/test_gpu_smooth.py (north star): the backward pass uses the prior alone."""
    N, nu, bcond = shape
    pde, solver, opde, osolver = fr.linear_pair(*shape, "both")
    osol, _, _ = fr.linear_reference(*shape, "both")
    osolver.initialize(opde)                                    # (E0 and the prior of this instance)
    sol = solver.solve_on_device(pde)
    ms, Ps = rts_on_oracle(osolver, osol)
    n, d = osol.mean.shape[1:]
    ostd = marginal_std(Ps, n, d)
    ssol = solver.smooth(sol)
    assert_mean_std_parity(ssol.mean[:, 0], ssol.marginal_std[:, 0], ms[:, 0], ostd[:, 0])
    means, stds = solver.smooth_marginals(sol)
    assert_mean_std_parity(means, stds, ms[:, 0], ostd[:, 0])
    K = len(sol.t) - 1
    where = [(k, j) for k in (0, K // 2, K) for j in (1, N // 2, N - 2)]
    post = solver.functionals(sol, np.stack([fn.point(K, N, k, j) for k, j in where]))
    sm = np.array([ms[k, 0, j] for k, j in where])
    sd = np.array([ostd[k, 0, j] for k, j in where])
    assert_mean_std_parity(post.mean, post.std, sm, sd)


# ------------------------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_through_raw_ctypes(hip_ctx):
    shape = fr.SHAPES[0]
    pde, solver, flt, s = _bound(shape, "both")
    dt = fr.DT
    flt.prepare_error_model(dt)
    lib, h = flt.lib, flt.handle
    err = lambda: lib.pnmol_last_error(flt.ctx.handle).decode()                 # noqa: E731
    m, d = flt.m, flt.d
    ts, _ = solver._constant_schedule(pde, None)
    table = np.ascontiguousarray(pde.forcing.table(ts, pde))
    nxt, cnt = ctypes.c_int(7), ctypes.c_int(7)

    def pending():
        assert lib.pnmol_filter_forcing_pending(h, ctypes.byref(nxt), ctypes.byref(cnt)) == 0
        return nxt.value, cnt.value

    assert pending() == (0, 0)
    assert lib.pnmol_filter_forcing_pending(None, ctypes.byref(nxt), ctypes.byref(cnt)) == -1
    assert lib.pnmol_filter_set_forcing(None, 12, _dp(table)) == -1
    assert lib.pnmol_filter_force_at(None, _dp(table[0])) == -1
    assert lib.pnmol_filter_set_forcing(h, -1, _dp(table)) == -1
    assert "pnmol_filter_set_forcing" in err() and "count < 0" in err()
    for bad in (np.nan, np.inf):
        broken = table.copy()
        broken[7, 3] = bad
        assert lib.pnmol_filter_set_forcing(h, 12, _dp(broken)) == -1
        assert "row 7" in err() and "column 3" in err() and "not finite" in err(), err()
        broken = table[0].copy()
        broken[m - 1] = bad
        assert lib.pnmol_filter_force_at(h, _dp(broken)) == -1
        assert "pnmol_filter_force_at" in err() and f"column {m - 1}" in err(), err()
    assert pending() == (0, 0)
    # an fp32 filter
    f32 = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(dt))
    f32.dtype = "f32"
    pde32, _, _, _ = fr.linear_pair(*shape, None)
    s32 = f32.initialize(pde32).y.device_state
    h32, ctx32 = s32.filter.handle, s32.filter.ctx.handle
    assert lib.pnmol_filter_set_forcing(h32, 12, _dp(table)) == -1 and "fp32" in lib.pnmol_last_error(ctx32).decode()
    assert lib.pnmol_filter_force_at(h32, _dp(table[0])) == -1 and "fp32" in lib.pnmol_last_error(ctx32).decode()
    # between steps_begin and steps_end
    w = s.clone()
    flt.steps_begin(w, 2, dt)
    assert lib.pnmol_filter_set_forcing(h, 12, _dp(table)) == -1 and "between pnmol_filter_steps_begin" in err()
    assert lib.pnmol_filter_set_forcing(h, 0, None) == -1 and "between" in err()
    assert lib.pnmol_filter_force_at(h, _dp(table[0])) == -1 and "pnmol_filter_force_at" in err() and "between" in err()
    assert lib.pnmol_filter_force_at(h, None) == -1 and "between" in err()
    flt.steps_end(w)
    # k steps with k - 1 rows left: -1, the counts in the text, nothing enqueued, the state untouched bit for bit
    assert lib.pnmol_filter_set_forcing(h, 5, _dp(table)) == 0 and pending() == (0, 5)
    w = s.clone()
    mean0, cov0, t0 = w.mean(), w.cov(), w.t
    assert lib.pnmol_filter_steps_begin(h, w.handle, 6, dt) == -1
    assert "pnmol_filter_steps_begin" in err() and "6 step(s) asked for, 5 of 5" in err(), err()
    with pytest.raises(_hip.PnmolHipError, match="right-hand side"):
        flt.steps(w, 6, dt)
    assert w.t == t0 and np.array_equal(w.mean(), mean0) and np.array_equal(w.cov(), cov0) and pending() == (0, 5)
    flt.steps(w, 3, dt)
    assert pending() == (3, 5)
    mean3, cov3 = w.mean(), w.cov()
    assert lib.pnmol_filter_steps_begin(h, w.handle, 3, dt) == -1 and "3 step(s) asked for, 2 of 5" in err()
    assert np.array_equal(w.mean(), mean3) and np.array_equal(w.cov(), cov3) and pending() == (3, 5)
    flt.steps(w, 2, dt)
    assert pending() == (5, 5)
    # the operator setters refuse while forcing is set: a table, or a single right-hand side
    M = np.ascontiguousarray(pde.L)
    jd = np.zeros(d)
    assert lib.pnmol_filter_set_operator(h, _dp(M), None) == -1 and "clear the forcing first" in err()
    assert lib.pnmol_filter_set_operator_diagonal(h, _dp(jd), None) == -1 and "clear the forcing first" in err()
    flt.clear_forcing()
    assert pending() == (0, 0)
    flt.force_at(table[0])
    assert lib.pnmol_filter_set_operator(h, _dp(M), None) == -1 and "clear the forcing first" in err()
    flt.force_at(None)
    assert lib.pnmol_filter_set_operator_diagonal(h, _dp(jd), None) == 0
    assert lib.pnmol_filter_set_operator(h, _dp(M), None) == 0


def test_term_setters_keep_the_table_and_a_failed_call_keeps_the_cursor(hip_ctx):
    name = "logistic-source"
    pde, solver, _, _ = fr.term_pair(name)
    s0 = solver.initialize(pde).y.device_state
    flt = solver._device_filter
    ts, dts = solver._constant_schedule(pde, None)
    table = pde.forcing.table(ts, pde)
    dt = dts[0]
    flt.set_forcing(table)
    flt.set_linearization_points(np.tile(pde.y0, (len(dts), 1)))
    flt.set_reaction(None)                                      # clearing the term drops its points, not the problem's forcing
    assert flt.forcing_pending() == (0, len(dts)) and flt.linearization_pending() == (0, 0)
    flt.set_reaction(reactions.logistic(2.0))                   # pnmol_filter_set_reaction
    assert flt.forcing_pending() == (0, len(dts))
    flt.steps(s0.clone(), 2, dt)                                # (the cursor inside the table: the setters leave it there too)
    assert flt.forcing_pending() == (2, len(dts))
    burgers = reactions.burgers()                               # pnmol_filter_set_convection, with an operator G of its own
    d = pde.L.shape[0]
    burgers.set_operator(0.5 * (np.eye(d, k=1) - np.eye(d, k=-1)))
    flt.set_reaction(burgers)
    assert flt.forcing_pending() == (2, len(dts))
    # pnmol_filter_set_reaction_system: three species of 11 points on the d = 33 rows
    flt.set_reaction(reactions.SystemReaction(3, p=[[(1.0, (1, 0, 0)), (-1.0, (1, 1, 0))], [(0.5, (1, 1, 0))], [(-0.2, (0, 0, 1))]]))
    assert flt.forcing_pending() == (2, len(dts))
    flt.set_reaction(None)
    assert flt.forcing_pending() == (2, len(dts))
    flt.set_reaction(pde.reaction)
    assert flt.forcing_pending() == (2, len(dts))
    flt.set_forcing(table)                                      # (the cursor back to row 0 for the run below)
    a = s0.clone()
    m, s, i = flt.steps(a, len(dts), dt)
    flt.clear_forcing()
    sm, ss, ssig = per_step(solver, pde)                        # (binds a new filter; `flt` keeps its own)
    assert np.array_equal(m, sm[1:])
    # a call that fails numerically consumes no row: two identical noise-free sensor rows behind step 2 of 2 (rc = -3)
    N = pde.L.shape[0]
    flt.set_forcing(table)
    C = np.ascontiguousarray(data.select_nodes(N, [5, 5]))
    flt.set_observations(np.array([s0.t + 2 * dt]), C, np.full((1, 2), 0.1), None)
    b = s0.clone()
    means, stds = np.empty((2, N)), np.empty((2, N))
    infos = (_hip.StepOut * 2)()
    rc = flt.lib.pnmol_filter_steps(flt.handle, b.handle, 2, dt, _dp(means), _dp(stds), infos)
    assert rc == -3 and "not positive definite" in flt.lib.pnmol_last_error(flt.ctx.handle).decode()
    assert flt.forcing_pending() == (0, len(dts))
    flt.clear_observations()
    flt.clear_forcing()
