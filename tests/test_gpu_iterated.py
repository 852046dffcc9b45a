"""The iterated EK1 smoother on the device (`pnmol_filter_set_linearization_points`, `pnmol_filter_linearize_at`, `solve_iterated`;
csrc/pnmol_reaction.hip): the loop over a table of points against single steps linearised at the same points
and against the NumPy reference pass, a table of the loop's own predicted means against the plain loop, `solve_iterated` against
the reference iteration (tests/iterated_reference.py, which fixes the cases and their step sizes), start independence, sensor
data, split calls, cleaning up, and the refusals of the C ABI.  13 steps: the first one eagerly, a 10-step graph, a 2-step graph;
the runt case adds a 14th, shorter step, which is a call of its own.  Run with -m gpu."""

import ctypes

import numpy as np
import pytest

import iterated_reference as ir
from helpers import assert_mean_std_parity, make_pair, rel
from pnmol import _hip

pytestmark = pytest.mark.gpu


def _parity(name, means, stds, omeans, ostds):
    """North-star tolerances (helpers.assert_mean_std_parity); per species for the system, whose components differ in size."""
    C = 2 if ir.CASES[name].kind == "lotka_volterra" else 1
    N = means.shape[-1] // C
    for c in range(C):
        part = slice(c * N, (c + 1) * N)
        assert_mean_std_parity(means[..., part], stds[..., part], omeans[..., part], ostds[..., part])


def _bound(name):
    """(pde, solver, filter, initial device state, the steps of the constant schedule) of a case."""
    pde, solver = ir.product(name)
    s0 = solver.initialize(pde).y.device_state
    _, dts = solver._constant_schedule(pde, None)
    return pde, solver, solver._device_filter, s0, dts


def _single_steps(flt, s0, dts, points):
    """`linearize_at(points[k])` + `step` per step: the states behind the steps."""
    s, out = s0, []
    for k, dt in enumerate(dts):
        flt.linearize_at(points[k])
        s, info, _ = flt.step(s, dt, want_error=False)
        assert info.info == -1
        out.append(s)
    return out


def _loop(flt, s0, dts, points=None):
    """The device loop over `dts` (runs of equal dt: one call each) with a recorder: (read-out means, stds, recorded states)."""
    slots = [flt.new_state() for _ in dts]
    work = s0.clone()
    means, stds = [], []
    try:
        flt.set_recorder(slots)
        if points is not None:
            flt.set_linearization_points(points)
        i = 0
        while i < len(dts):
            j = i
            while j < len(dts) and dts[j] == dts[i]:
                j += 1
            if points is not None:
                assert flt.linearization_pending() == (i, len(dts))
            m, s, _ = flt.steps(work, j - i, dts[i])
            means.extend(m), stds.extend(s)
            i = j
        if points is not None:
            assert flt.linearization_pending() == (len(dts), len(dts))
    finally:
        flt.clear_recorder()
        flt.clear_linearization_points()
    return np.array(means), np.array(stds), slots


def _assert_states_bitwise(got, want, label):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a.mean(), b.mean()), (label, k, "mean", rel(a.mean(), b.mean()))
        assert np.array_equal(a.marginal_var(), b.marginal_var()), (label, k, "var", rel(a.marginal_var(), b.marginal_var()))
        assert np.array_equal(a.cov(), b.cov()), (label, k, "cov", rel(a.cov(), b.cov()))


# ------------------------------------------------------------------------------------------------ 1. the table, one pass
@pytest.mark.parametrize("name", ["fisher-neumann", "fisher-264", "lotka-volterra", "burgers"])
def test_loop_over_a_table_equals_single_steps_and_meets_the_reference_pass(hip_ctx, name):
    """Points: the table of the reference's pass 1 (its smoothed EK1 trajectory).  The loop with the table against
    `pnmol_filter_linearize_at` + `pnmol_filter_step` per step, bit for bit: the states behind the steps (the recorder copies
    them) in mean, marginal variances -- what a std is read out from -- and full covariance, and the rows of means the loop reads
    out.  The loop's own std rows come out of another launch than a state's variances (s0 sqrt(var) on the device against
    sqrt(s0 s0 var) on the host: the one-ulp difference of DESIGN.md section 16), so they are held to 2 ulp beside the variances'
    equality.  Then the north-star tolerances against the reference pass.  N = 33: d is padded; N = 264: the linearise kernels run
    two blocks; Lotka-Volterra 2 x 33: same-point slots; Burgers: the neighbours come from the same row of the table."""
    it = ir.reference(name)
    points, ref_pass = it.points[1], it.passes[1]
    pde, solver, flt, s0, dts = _bound(name)
    assert len(dts) == 13 and points.shape == (13, flt.d)
    assert flt.dims()["dp"] > flt.d and flt.dims()["dp"] % 32 == 0      # (padded rows and components in every case)
    means, stds, recorded = _loop(flt, s0, dts, points)
    singles = _single_steps(flt, s0, dts, points)
    _assert_states_bitwise(recorded, singles, name)
    step_means = np.stack([s.mean()[0] for s in singles])
    step_stds = np.stack([np.sqrt(np.maximum(s.marginal_var()[0], 0.0)) for s in singles])
    assert np.array_equal(means, step_means)
    ulps = np.abs(stds - step_stds) / np.spacing(np.maximum(np.abs(stds), np.abs(step_stds)))
    print(f"{name}: loop std rows off the states' by at most {ulps.max():.1f} ulp")
    assert ulps.max() <= 2.0
    _parity(name, means, stds, ref_pass.means[1:], ref_pass.stds[1:])
    # the table matters: the plain loop gives another trajectory, the one of the reference's EK1 pass
    plain_means, plain_stds, _ = _loop(flt, s0, dts)
    _parity(name, plain_means, plain_stds, it.passes[0].means[1:], it.passes[0].stds[1:])
    assert np.abs(plain_means - means).max() > 10 * 1e-5 * np.abs(means).max()


# ------------------------------------------------------------------------------------------------ 2. the loop's own points
def test_table_of_the_loops_own_predicted_means_reproduces_the_plain_loop(hip_ctx):
    """`pnmol_filter_predict_mean` per step of a plain run (the runt case: the 14th step changes the frame) as the table: the
    states of `solve_on_device` bit for bit."""
    name = "fisher-dirichlet-runt"
    pde, solver, flt, s0, dts = _bound(name)
    assert len(dts) == 14 and dts[-1] < dts[0]
    s, predicted = s0, []
    for dt in dts:
        predicted.append(flt.predict_mean(s, dt))
        flt.linearize(s, dt)
        s, _, _ = flt.step(s, dt, want_error=False)
    plain = solver.solve_on_device(pde)
    tabled = solver.solve_on_device(pde, linearize_at=np.stack(predicted))
    assert solver._device_filter.linearization_pending() == (0, 0)
    assert np.array_equal(plain.t, tabled.t) and np.array_equal(plain.mean, tabled.mean)
    _assert_states_bitwise([y.device_state for y in tabled._ys], [y.device_state for y in plain._ys], name)
    assert tabled.diffusion_squared_calibrated == plain.diffusion_squared_calibrated
    a, b = solver.solve_marginals(pde), solver.solve_marginals(pde, linearize_at=np.stack(predicted))
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))


@pytest.mark.parametrize("name", ["fisher-neumann", "burgers"])
def test_linearize_keeps_the_predicted_mean_while_a_table_is_set(hip_ctx, name):
    """`pnmol_filter_linearize` + `pnmol_filter_step` on a filter with a table set give the bits of a filter that has none, and
    consume no row: with the cursor at row 0, behind a `steps` call that left the cursor inside the table, and behind one that
    used it up (cursor + step counter then point past the last row)."""
    points = ir.reference(name).points[1][:5] + 0.25             # (far from the predicted means: a row taken by mistake shows)
    _, _, plain_flt, plain_s0, dts = _bound(name)
    _, _, flt, s0, _ = _bound(name)
    dt = dts[0]

    def one_step(f, s):
        f.linearize(s, dt)
        out, info, _ = f.step(s, dt, want_error=False)
        assert info.info == -1
        return out

    flt.set_linearization_points(points)
    _assert_states_bitwise([one_step(flt, s0)], [one_step(plain_flt, plain_s0)], name + ", cursor 0")
    assert flt.linearization_pending() == (0, 5)
    work, plain_work = s0.clone(), plain_s0.clone()
    for k, label in ((3, "cursor inside"), (2, "table used up")):
        flt.steps(work, k, dt)
        plain_flt.steps(plain_work, k, dt)
        assert not np.array_equal(work.mean(), plain_work.mean())                  # (the loop did take the table)
        _assert_states_bitwise([one_step(flt, s0)], [one_step(plain_flt, plain_s0)], f"{name}, {label}")
    assert flt.linearization_pending() == (5, 5)
    # and the loop goes on from its cursor whatever `linearize` did in between: the rows 3, 4 against single steps at them
    again = s0.clone()
    flt.set_linearization_points(points)
    flt.steps(again, 3, dt)
    one_step(flt, s0)
    flt.steps(again, 2, dt)
    singles = _single_steps(flt, s0, [dt] * 5, points)
    _assert_states_bitwise([again], [singles[-1]], name + ", rows across a linearize call")
    flt.clear_linearization_points()


# ------------------------------------------------------------------------------------------------ 3. the iteration
@pytest.mark.parametrize("name", list(ir.CASES))
def test_solve_iterated_against_the_reference_iteration(hip_ctx, name):
    it = ir.reference(name)
    pde, solver = ir.product(name)
    res = solver.solve_iterated(pde, iterations=ir.ITERATIONS, tol=ir.TOL)
    print(f"{name}: increments device " + ", ".join(f"{x:.1e}" for x in res.increments) + " | reference "
          + ", ".join(f"{x:.1e}" for x in it.increments))
    assert res.converged and res.num_iterations == len(res.increments) and abs(res.num_iterations - it.num_iterations) <= 1
    T = int(np.ceil(ir.CASES[name].K))
    assert res.means.shape == res.stds.shape == (T + 1, pde.L.shape[0])
    assert np.allclose(res.filtered.t, it.last.solution.t, rtol=0, atol=1e-15)
    _parity(name, res.means, res.stds, it.means, it.stds)
    _parity(name, res.filtered.mean[:, 0], res.filtered.marginal_std[:, 0], it.last.means, it.last.stds)
    assert res.smoothed is not None and res.smoothed.smoothed and np.array_equal(res.smoothed.mean[:, 0], res.means)
    assert res.data_log_likelihood is None and res.data_log_likelihoods is None
    assert res.filtered.info["num_steps"] == T


# ------------------------------------------------------------------------------------------------ 4. start independence
def test_fixed_point_does_not_depend_on_the_start(hip_ctx):
    name = "fisher-neumann"
    pde, solver = ir.product(name)
    default = solver.solve_iterated(pde, smooth=None)
    start = np.tile(pde.y0, (13, 1))
    other = solver.solve_iterated(pde, start=start, smooth=None)
    diff = np.abs(other.means - default.means).max() / np.abs(default.means).max()
    print(f"start y0 repeated: {other.num_iterations} iterations (default {default.num_iterations}), means differ by {diff:.1e}")
    assert default.converged and other.converged and default.smoothed is None
    assert other.increments[0] > 100 * default.increments[0]      # (the start was far off)
    assert diff <= 1e-7
    # relaxation < 1 reaches it too, in more iterations
    damped = solver.solve_iterated(pde, relaxation=0.8, iterations=20, smooth=None)
    assert damped.converged and damped.num_iterations > default.num_iterations
    assert np.abs(damped.means - default.means).max() / np.abs(default.means).max() <= 1e-7


# ------------------------------------------------------------------------------------------------ 5. with sensor data
def test_solve_iterated_with_sensor_data(hip_ctx):
    """Three sensor times -- t0, behind step 6, on the last step -- of 8 sensors; the reference iteration takes the oracle's
    `update_sqrt` behind the same steps (observe_reference.drive)."""
    name = "fisher-neumann"
    it = ir.reference(name, observed=True)
    obs = ir.sensor_setup(name)
    pde, solver = ir.product(name)
    res = solver.solve_iterated(pde, observations=obs)
    print("observed: increments device " + ", ".join(f"{x:.1e}" for x in res.increments) + " | reference "
          + ", ".join(f"{x:.1e}" for x in it.increments))
    assert res.converged and abs(res.num_iterations - it.num_iterations) <= 1
    _parity(name, res.means, res.stds, it.means, it.stds)
    olls = it.last.solution.info["data_log_likelihoods"]
    assert len(res.data_log_likelihoods) == 3 == len(olls)
    np.testing.assert_allclose(res.data_log_likelihoods, olls, rtol=1e-4)         # (the bound of DESIGN.md section 19)
    np.testing.assert_allclose(res.data_log_likelihood, it.last.solution.info["data_log_likelihood"], rtol=1e-4)
    draws = solver.sample(res.filtered, 4, seed=1)
    assert draws.shape == (4, 14, 3, 33) and np.all(np.isfinite(draws))
    tq = np.array([res.filtered.t[2] + 0.3 * (res.filtered.t[3] - res.filtered.t[2]), res.filtered.t[5]])
    dense = res.smoothed(tq)
    assert np.all(np.isfinite(dense.mean)) and np.array_equal(dense.mean[1], res.smoothed.mean[5])
    flt = solver._device_filter
    assert flt.linearization_pending() == (0, 0) and flt.recorder_pending() == (0, 0) and flt.observations_pending() == (0, 0)


# ------------------------------------------------------------------------------------------------ 6. split calls, cleaning up
def test_runt_step_consumes_rows_across_two_calls(hip_ctx):
    name = "fisher-dirichlet-runt"
    points = ir.reference(name).points[1]
    pde, solver, flt, s0, dts = _bound(name)
    assert points.shape[0] == 14 == len(dts) and len(set(dts)) == 2
    means, stds, recorded = _loop(flt, s0, dts, points)            # (asserts the cursor (0, 14) -> (13, 14) -> (14, 14))
    _assert_states_bitwise(recorded, _single_steps(flt, s0, dts, points), name)
    # a rehearsal consumes no row; the real call behind it gives the same bits
    flt.set_linearization_points(points)
    work = s0.clone()
    flt.prepare_steps(work, 13, dts[0])
    assert flt.linearization_pending() == (0, 14) and np.array_equal(work.mean(), s0.mean())
    m, _, _ = flt.steps(work, 13, dts[0])
    assert np.array_equal(m, means[:13]) and flt.linearization_pending() == (13, 14)
    flt.clear_linearization_points()


def test_nothing_is_left_set_behind_solve_iterated(hip_ctx, monkeypatch):
    name = "fisher-neumann"
    pde, solver = ir.product(name)
    fresh = ir.product(name)[1].solve_marginals(pde)
    res = solver.solve_iterated(pde, iterations=2, tol=0.0, smooth=None)
    assert res.num_iterations == 2 and not res.converged
    flt = solver._device_filter
    pending = lambda f: (f.linearization_pending(), f.recorder_pending(), f.observations_pending())
    assert pending(flt) == ((0, 0),) * 3
    # an exception in the middle of the iteration: the forward pass before it has cleaned up behind itself
    calls, plain = [], type(solver).smooth_marginals

    def failing(self, solution):
        calls.append(self._device_filter)
        if len(calls) == 2:
            raise RuntimeError("stop here")
        return plain(self, solution)

    monkeypatch.setattr(type(solver), "smooth_marginals", failing)
    with pytest.raises(RuntimeError, match="stop here"):
        solver.solve_iterated(pde)
    monkeypatch.undo()
    assert len(calls) == 2 and pending(calls[1]) == ((0, 0),) * 3
    after = solver.solve_marginals(pde)
    assert pending(solver._device_filter) == ((0, 0),) * 3
    assert all(np.array_equal(x, y) for x, y in zip(after[:4], fresh[:4]))


# ------------------------------------------------------------------------------------------------ 7. refusals of the C ABI
def test_c_abi_refusals(hip_ctx):
    name = "fisher-neumann"
    pde, solver, flt, s0, dts = _bound(name)
    lib, h, d = flt.lib, flt.handle, flt.d
    err = lambda: lib.pnmol_last_error(flt.ctx.handle).decode()
    dp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    table = np.full((5, d), 0.5)
    set_points = lib.pnmol_filter_set_linearization_points
    assert set_points(None, 5, dp(table)) == -1 and lib.pnmol_filter_linearize_at(None, dp(table)) == -1
    assert lib.pnmol_filter_linearization_pending(None, None, None) == -1
    # count < 0, an entry that is not finite
    assert set_points(h, -1, dp(table)) == -1 and "pnmol_filter_set_linearization_points" in err() and "count < 0" in err()
    for bad in (np.nan, np.inf):
        broken = table.copy()
        broken[3, d - 1] = bad
        assert set_points(h, 5, dp(broken)) == -1 and f"row 3 is not finite at component {d - 1}" in err()
    assert flt.linearization_pending() == (0, 0)
    # no term set: a linear problem's filter, and this one after its term is cleared
    hpde, hsolver, _, _ = make_pair(33, 2, dts[0], 13)
    hs0 = hsolver.initialize(hpde).y.device_state
    hflt = hsolver._device_filter
    herr = lambda: lib.pnmol_last_error(hflt.ctx.handle).decode()
    assert set_points(hflt.handle, 5, dp(table)) == -1 and "no term set" in herr()
    assert lib.pnmol_filter_linearize_at(hflt.handle, dp(table)) == -1
    assert "pnmol_filter_linearize_at" in herr() and "no term set" in herr()
    assert lib.pnmol_filter_linearize_at(h, None) == -1 and "null point" in err()
    assert set_points(hflt.handle, 0, None) == 0                                        # (clearing needs no term)
    # more steps than rows left: -1 before anything is enqueued, the state and the cursor untouched
    flt.set_linearization_points(table)
    work = s0.clone()
    mean0, cov0, t0 = work.mean(), work.cov(), work.t
    assert lib.pnmol_filter_steps_begin(h, work.handle, 6, dts[0]) == -1
    assert "pnmol_filter_steps_begin" in err() and "6 step(s) asked for, 5 of 5 linearisation point(s) left" in err()
    with pytest.raises(_hip.PnmolHipError, match="linearisation point"):
        flt.steps(work, 6, dts[0])
    assert work.t == t0 and np.array_equal(work.mean(), mean0) and np.array_equal(work.cov(), cov0)
    assert flt.linearization_pending() == (0, 5)
    flt.steps(work, 3, dts[0])
    assert flt.linearization_pending() == (3, 5)
    assert lib.pnmol_filter_steps_begin(h, work.handle, 3, dts[0]) == -1 and "3 step(s) asked for, 2 of 5" in err()
    # between _begin and _end
    flt.steps_begin(work, 2, dts[0])
    assert set_points(h, 5, dp(table)) == -1 and "between pnmol_filter_steps_begin" in err()
    assert set_points(h, 0, None) == -1 and "between pnmol_filter_steps_begin" in err()
    flt.steps_end(work)
    assert flt.linearization_pending() == (5, 5)
    # a table that is set again starts over; clearing the term clears the table
    flt.set_linearization_points(table[:2])
    assert flt.linearization_pending() == (0, 2)
    flt.set_reaction(None)
    assert flt.linearization_pending() == (0, 0)
    assert set_points(h, 5, dp(table)) == -1 and "no term set" in err()
