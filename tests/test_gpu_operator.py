"""Time-dependent operators on the device (`pnmol.pde.coefficients`, `pnmol_filter_set_operator_family`, `_set_operator_schedule`,
`_operator_at`; csrc/pnmol_operator.hip): `solve()`, `solve_marginals` and `solve_on_device` against the oracle's
semilinear path with M(t) and E(t) (tests/operator_reference.py, which fixes the cases) and against each other bit for bit, unit
coefficients against the time-independent problem bit for bit, the cursor, `operator_at`, adaptive steps, composition with a
reaction, forcing, sensor data, linearisation points and the iterated smoother, the backward pass, and the refusals of the C ABI.
Shapes: (24, 2, neumann) mp = 32, one block; (33, 1) 31 padded points in mp = 64; (255, 1) m = 257 in mp = 288, the second block of the
256-thread launch holds one boundary row and padding; (40, 3) the n = 4 instantiations.  Families: (A) kappa(t) u_xx; (B) 0.05 u_xx -
c(t) u_x with a 5-point gradient, c(t0) = 0, changing sign.  Run with -m gpu."""

import ctypes

import numpy as np
import pytest

import iterated_reference as ir
import observe_reference as oref
import operator_reference as orf
import pnmol
import pnmol_oracle as oracle
from helpers import assert_mean_std_parity, per_step, rel
from pnmol import _hip
from pnmol import functionals as fn
from pnmol._hip import _dp
from pnmol.pde import reactions
from pnmol.pde.forcing import Forcing
from smooth_reference import marginal_std, rts_on_oracle

pytestmark = pytest.mark.gpu

DT = orf.DT
CASES = [("A", s) for s in orf.SHAPES] + [("B", s) for s in orf.SHAPES_B]


def _bound(family, shape, plain=False, **kw):
    """(pde, solver, filter, initial device state), the device bound.  plain: the time-independent problem of t0, no family."""
    N, nu, bcond, K = shape
    pde, solver, _, _ = orf.pair(family, N, nu, bcond, K, **kw)
    if plain:
        pde = orf.plain_copy(pde)
    s0 = solver.initialize(pde).y.device_state
    return pde, solver, solver._device_filter, s0


def _table(pde, solver):
    ts, dts = solver._constant_schedule(pde, None)
    return pde.time_dependent_operator.table(ts)


def _assert_states_bitwise(got, want, label):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a.mean(), b.mean()), (label, k, "mean", rel(a.mean(), b.mean()))
        assert np.array_equal(a.marginal_var(), b.marginal_var()), (label, k, "var")
        assert np.array_equal(a.cov(), b.cov()), (label, k, "cov", rel(a.cov(), b.cov()))


def _north_star(label, means, stds, omeans, ostds):
    """`helpers.assert_mean_std_parity`, the figures printed first: the largest mean and std errors in units of the largest reference
    entry, over all nodes and over the two end nodes (exactly 0 under Dirichlet conditions: the floor 1e-5 applies there)."""
    me, se = np.abs(means - omeans) / np.abs(omeans).max(), np.abs(stds - ostds) / np.abs(ostds).max()
    print(f"{label}: mean error {me.max():.2e}, std error {se.max():.2e} (end nodes {se[:, [0, -1]].max():.2e}) of the largest entry")
    assert_mean_std_parity(means, stds, omeans, ostds)


def _sig(infos):
    return [o.diffusion_squared_local for o in infos]


# ------------------------------------------------------------------------------------------------------------------ 1. oracle
@pytest.mark.parametrize("family, shape", CASES)
def test_solves_meet_the_reference(hip_ctx, family, shape):
    N, nu, bcond, K = shape
    pde, solver, _, _ = orf.pair(family, *shape)
    osol, om, os_ = orf.reference(family, *shape)
    sol = solver.solve(pde)
    flt = solver._device_filter
    dims = flt.dims()
    assert dims["m"] == N + 2 and dims["mp"] == {24: 32, 33: 64, 255: 288, 40: 64}[N] and flt.operator_family == (2 if family == "B" else 1)
    np.testing.assert_allclose(sol.t, osol.t, rtol=0, atol=1e-15)
    _north_star(f"({family}) {shape} solve", sol.mean[:, 0], sol.marginal_std[:, 0], om, os_)
    t, means, stds, sig, final = solver.solve_marginals(pde)
    assert solver._device_filter.operator_schedule_pending() == (0, 0)          # (cleared behind the solve)
    _north_star(f"({family}) {shape} solve_marginals", means, stds, om, os_)
    rec = solver.solve_on_device(pde)
    _north_star(f"({family}) {shape} solve_on_device", rec.mean[:, 0], rec.marginal_std[:, 0], om, os_)
    # sigma^2 of every step against the oracle's, at the relative tolerance the loop tests use for it
    osig = orf.reference_sigmas(family, *shape)
    print(f"({family}) {shape}: sigma^2 off the reference by {rel(sig, osig):.2e}")
    np.testing.assert_allclose(sig, osig, rtol=1e-4)
    np.testing.assert_allclose(rec.diffusion_squared_calibrated, osol.diffusion_squared_calibrated, rtol=1e-4)
    # against constant coefficients the case moves by 100 tolerances (tests/test_operator_host.py): an ignored schedule fails above
    _, om0, _ = orf.reference(family, *shape, constant=True)
    assert np.abs(means - om0).max() > 100 * 1e-5 * np.abs(om0).max()


# ------------------------------------------------------------------------------------------------------------------ 2. bits
@pytest.mark.parametrize("family, shape", [("A", orf.SHAPES[0]), ("A", orf.SHAPES[1]), ("A", orf.SHAPES[3]), ("B", orf.SHAPES[0]),
                                           ("B", orf.SHAPES[1])])
def test_loop_routes_equal_solve_bit_for_bit(hip_ctx, family, shape):
    """`solve_marginals` and `solve_on_device` against `solve()`, bit for bit: t, means, sigma^2, the marginal variances, stds and
    covariance of every recorded state and of the final one.  The std ROWS `solve_marginals` reads out itself are held to 2 ulp
    beside the equality of the variances they come from, as in tests/test_gpu_forcing.py."""
    pde, solver, _, _ = orf.pair(family, *shape)
    sol = solver.solve(pde)
    sm, ss, ssig = per_step(solver, pde)
    t, means, stds, sig, final = solver.solve_marginals(pde)
    rec = solver.solve_on_device(pde)
    assert np.array_equal(t, sol.t) and np.array_equal(rec.t, sol.t)
    assert np.array_equal(means, sm) and np.array_equal(rec.mean, sol.mean)
    assert np.array_equal(sig, ssig) and rec.diffusion_squared_calibrated == sol.diffusion_squared_calibrated
    _assert_states_bitwise([y.device_state for y in rec._ys], [y.device_state for y in sol._ys], (family, shape))
    assert np.array_equal(rec.marginal_std, sol.marginal_std)
    assert np.array_equal(final.y.device_state.cov(), sol._ys[-1].device_state.cov())
    assert np.array_equal(final.y.device_state.marginal_var(), sol._ys[-1].device_state.marginal_var())
    ulps = np.abs(stds - ss) / np.spacing(np.maximum(np.abs(stds), np.abs(ss)))
    assert ulps.max() <= 2.0


# ------------------------------------------------------------------------------------------------------------------ 3. unit coefficients
@pytest.mark.parametrize("shape", [orf.SHAPES[0], orf.SHAPES[1]])
def test_unit_coefficients_give_the_bits_of_the_time_independent_problem(hip_ctx, shape):
    """a = (1,) on the family (pde.L,), and a = (1, 0) on (pde.L, G) with a 3-point gradient G, against plain `solve()` on the
    time-independent problem: states and sigma^2 bit for bit -- 1 * v, v + 0 * g and (1 e)^2 + (0 e')^2 are exact.  (The 5-point
    family of (B) takes the wide-stencil launches of the step, whose sums run in another order than the narrow ones of the
    3-point problem: its exact case is the loop-against-solve() test above.)  Then the family and the schedule are cleared: the
    filter gives the bits of a fresh one, through `steps` on the fused loop again."""
    N, nu, bcond, K = shape
    pde, solver, flt, s0 = _bound("A", shape, plain=True, constant=True)
    assert getattr(pde, "time_dependent_operator", None) is None and flt.operator_family == 0
    sm, ss, ssig = per_step(solver, pde)                        # plain solve(); binds a filter of its own
    last = solver.solve(pde)._ys[-1].device_state
    s0 = solver.initialize(pde).y.device_state
    flt = solver._device_filter
    e = np.diag(pde.E_sqrtm)
    G, Ge = pnmol.discretize.fd_probabilistic(pnmol.diffops.gradient(), mesh_spatial=pde.mesh_spatial,
                                              kernel=pnmol.kernels.SquareExponential(), stencil_size_interior=3,
                                              stencil_size_boundary=3, nugget_gram_matrix=0.0)
    for ops, noise, row in (([pde.L], [e], (1.0,)), ([pde.L, G], [e, np.diag(Ge)], (1.0, 0.0))):
        flt.set_operator_family(np.stack(ops), np.stack(noise))
        flt.set_operator_schedule(np.tile(row, (K, 1)))
        w = s0.clone()
        m, s, infos = flt.steps(w, K, DT)
        assert flt.operator_schedule_pending() == (K, K)
        assert np.array_equal(m, sm[1:]) and _sig(infos) == list(ssig), row
        assert np.array_equal(w.mean(), last.mean()) and np.array_equal(w.cov(), last.cov())
        assert np.array_equal(w.marginal_var(), last.marginal_var())
    # a schedule that matters, then everything cleared
    flt.set_operator_schedule(np.tile((1.5, 0.3), (K, 1)))
    moved = flt.steps(s0.clone(), K, DT)
    assert np.abs(moved[0] - sm[1:]).max() > 1e-3 * np.abs(sm).max()
    flt.clear_operator_schedule()
    flt.clear_operator_family()
    assert flt.operator_schedule_pending() == (0, 0)
    flt.prepare_error_model(DT)
    state = s0.clone()
    cleared = flt.steps(state, K, DT)
    _, other, oflt, q0 = _bound("A", shape, plain=True, constant=True)
    oflt.prepare_error_model(DT)
    fresh = oflt.steps(q0, K, DT)
    assert np.array_equal(cleared[0], fresh[0]) and np.array_equal(cleared[1], fresh[1])
    assert _sig(cleared[2]) == _sig(fresh[2]) and [o.error_sigma2 for o in cleared[2]] == [o.error_sigma2 for o in fresh[2]]
    assert np.array_equal(state.mean(), q0.mean()) and np.array_equal(state.cov(), q0.cov())
    # ... and through solve_marginals on the plain problem (the fused loop), which a solver's fresh filter runs
    t, means, stds, sig, final = other.solve_marginals(pde)
    assert np.array_equal(means[1:], cleared[0]) and np.array_equal(stds[1:], cleared[1]) and list(sig) == _sig(cleared[2])


# ------------------------------------------------------------------------------------------------------------------ 4. cursor
@pytest.mark.parametrize("family", ["A", "B"])
def test_two_calls_equal_one_call_and_the_rehearsal_rewinds(hip_ctx, family):
    shape = orf.SHAPES[1]
    K = shape[3]
    pde, solver, flt, s0 = _bound(family, shape)
    table = _table(pde, solver)
    a, b = s0.clone(), s0.clone()
    flt.set_operator_schedule(table)
    assert flt.operator_schedule_pending() == (0, K)
    flt.prepare_steps(a, K, DT)                                 # the rehearsal consumes no row and leaves the state alone
    assert flt.operator_schedule_pending() == (0, K) and np.array_equal(a.mean(), s0.mean()) and np.array_equal(a.cov(), s0.cov())
    m, s, i = flt.steps(a, K, DT)
    assert flt.operator_schedule_pending() == (K, K)
    assert all(np.isnan(o.error_sigma2) for o in i)             # the loop carries no error model while a schedule is set
    flt.set_operator_schedule(table)                            # the same table again: the cursor goes back to row 0
    m1, s1, i1 = flt.steps(b, 5, DT)
    assert flt.operator_schedule_pending() == (5, K)
    m2, s2, i2 = flt.steps(b, K - 5, DT)
    assert flt.operator_schedule_pending() == (K, K)
    assert np.array_equal(np.vstack((m1, m2)), m) and np.array_equal(np.vstack((s1, s2)), s)
    assert _sig(list(i1) + list(i2)) == _sig(i)
    assert np.array_equal(a.mean(), b.mean()) and np.array_equal(a.cov(), b.cov()) and a.t == b.t
    # too few rows: -1, the state and the cursor untouched
    flt.set_operator_schedule(table[:5])
    w = s0.clone()
    with pytest.raises(_hip.PnmolHipError, match=r"6 step\(s\) asked for, 5 of 5 row\(s\) of coefficients left"):
        flt.steps(w, 6, DT)
    assert w.t == s0.t and np.array_equal(w.mean(), s0.mean()) and np.array_equal(w.cov(), s0.cov())
    assert flt.operator_schedule_pending() == (0, 5)
    flt.clear_operator_schedule()


def test_runt_last_step_takes_its_own_row(hip_ctx):
    N, nu, bcond, _ = orf.SHAPES[0]
    pde, solver, _, _ = orf.pair("A", N, nu, bcond, 12.5)
    ts, dts = solver._constant_schedule(pde, None)
    assert len(dts) == 13 and dts[-1] == 0.5 * DT
    sm, ss, ssig = per_step(solver, pde)
    t, means, stds, sig, final = solver.solve_marginals(pde)
    assert np.array_equal(t, ts) and np.array_equal(means, sm) and np.array_equal(sig, ssig)
    # the last row is the one of tmax: a schedule whose last row is another moves the last mean alone
    s0 = solver.initialize(pde).y.device_state
    flt = solver._device_filter
    table = pde.time_dependent_operator.table(ts)
    other = table.copy()
    other[-1] *= 1.5
    flt.set_operator_schedule(other)
    w = s0.clone()
    m12, _, _ = flt.steps(w, 12, DT)
    m13, _, _ = flt.steps(w, 1, dts[-1])
    assert flt.operator_schedule_pending() == (13, 13)
    assert np.array_equal(m12, sm[1:13]) and not np.array_equal(m13[0], sm[13])
    flt.clear_operator_schedule()


def test_second_table_on_the_same_filter_replays_the_graphs(hip_ctx):
    """A table that fits the one before it is overwritten in place and the captured graphs of the first run serve the second: its
    result equals that of a fresh filter bit for bit."""
    shape = orf.SHAPES[1]
    K = shape[3]
    pde, solver, flt, s0 = _bound("B", shape)
    table = _table(pde, solver)
    second = np.ascontiguousarray(table[::-1] * np.array([1.2, -0.7]))
    flt.set_operator_schedule(table)
    first = flt.steps(s0.clone(), K, DT)
    flt.set_operator_schedule(second)
    assert flt.operator_schedule_pending() == (0, K)
    w = s0.clone()
    again = flt.steps(w, K, DT)
    assert np.abs(again[0] - first[0]).max() > 1e-3 * np.abs(first[0]).max()
    _, _, oflt, q0 = _bound("B", shape)
    oflt.set_operator_schedule(second)
    fresh = oflt.steps(q0, K, DT)
    assert np.array_equal(again[0], fresh[0]) and np.array_equal(again[1], fresh[1]) and _sig(again[2]) == _sig(fresh[2])
    assert np.array_equal(w.mean(), q0.mean()) and np.array_equal(w.cov(), q0.cov())


# ------------------------------------------------------------------------------------------------------------------ 5. operator_at
@pytest.mark.parametrize("family", ["A", "B"])
def test_operator_at_persists_and_equals_the_loops_rows(hip_ctx, family):
    shape = orf.SHAPES[0]
    pde, solver, flt, s0 = _bound(family, shape)
    table = _table(pde, solver)
    rows = np.ascontiguousarray(table[[2, 2, 7]])               # the second step runs on the operator the first call left
    flt.set_operator_schedule(rows)
    w = s0.clone()
    m, s, infos = flt.steps(w, 3, DT)
    flt.clear_operator_schedule()
    flt.operator_at(rows[0])
    a1, i1, _ = flt.step(s0, DT, want_error=False)
    a2, i2, _ = flt.step(a1, DT, want_error=False)              # no call in between: the operator persists
    flt.operator_at(rows[2])
    flt.prepare_error_model(DT)
    a3, i3, err = flt.step(a2, DT)
    assert np.isfinite(i3.error_sigma2) and np.all(np.isfinite(err))
    for k, a in enumerate((a1, a2, a3)):
        assert np.array_equal(a.mean()[0], m[k]), k
    assert [i1.diffusion_squared_local, i2.diffusion_squared_local, i3.diffusion_squared_local] == _sig(infos)
    assert np.array_equal(a3.mean(), w.mean()) and np.array_equal(a3.cov(), w.cov())


# ------------------------------------------------------------------------------------------------------------------ 6. adaptive
@pytest.mark.parametrize("family", ["A", "B"])
def test_adaptive_solve_follows_the_references_accept_reject_sequence(hip_ctx, family):
    kw = dict(abstol=1e-4, reltol=1e-3)
    N, nu, bcond, K = 33, 2, "dirichlet", 24
    pde, solver, opde, osolver = orf.pair(family, N, nu, bcond, K)
    solver.steprule = pnmol.odetools.step.Adaptive(**kw)
    osolver.steprule = oracle.Adaptive(**kw)
    # the first step of the rule is |y0| / |L y0| on the product's linear problem; the oracle carries M(t) - L0 as f only as its
    # vehicle, so it takes the product's first step
    first = solver.steprule.first_dt(pde)
    assert np.isclose(first, 0.01 * np.linalg.norm(pde.y0) / np.linalg.norm(pde.L @ pde.y0), rtol=1e-12, atol=0.0)
    osolver.steprule.first_dt = lambda _pde: first
    sol = solver.solve(pde)
    osol = osolver.solve(opde)
    print(f"adaptive ({family}): {sol.info['num_steps']} steps, {sol.info['num_attempted_steps']} attempts")
    assert sol.info == osol.info and sol.info["num_steps"] > 3
    np.testing.assert_allclose(sol.t, osol.t, rtol=1e-9)
    om, os_ = oracle.read_mean_and_std(osol, osolver.E0)
    assert_mean_std_parity(sol.mean[:, 0], sol.marginal_std[:, 0], om, os_)


# ------------------------------------------------------------------------------------------------------------------ 7. composition
def _source(t, X):
    return 0.5 * np.sin(np.pi * np.asarray(X).reshape(-1)) * np.cos(8.0 * t)


def test_reaction_composes_with_the_operator(hip_ctx):
    pde, solver, _, _ = orf.logistic_pair()
    osol, om, os_ = orf.logistic_reference()
    t, means, stds, sig, final = solver.solve_marginals(pde)
    assert solver._device_filter.reaction is pde.reaction and solver._device_filter.operator_family == 1
    assert_mean_std_parity(means, stds, om, os_)
    sm, ss, ssig = per_step(solver, pde)
    assert np.array_equal(means, sm) and np.array_equal(sig, ssig)
    rec = solver.solve_on_device(pde)
    assert np.array_equal(rec.mean[:, 0], sm)


def test_reaction_forcing_and_sensor_data_compose_with_the_operator(hip_ctx):
    forcing = Forcing(source=_source)
    pde, solver, opde, osolver = orf.logistic_pair(forcing=forcing, source=_source)
    osol = osolver.solve(opde)
    om, os_ = oracle.read_mean_and_std(osol, osolver.E0)
    t, means, stds, sig, final = solver.solve_marginals(pde)
    assert_mean_std_parity(means, stds, om, os_)
    _, plain, _ = orf.logistic_reference()
    assert np.abs(means - plain).max() > 100 * 1e-5 * np.abs(plain).max()      # the source is there
    # one sensor array: three readings, 1.05 x the reference's own filtering mean plus noise of its median interior std
    q = 6
    C = oref.sensor_matrix(means.shape[1], q)
    noise = float(np.median(os_[1:, 1:-1]))
    rng = np.random.default_rng(means.shape[1] + q)
    obs = [pnmol.data.Observation(osol.t[j], C, 1.05 * (C @ om[j]) + noise * rng.standard_normal(q), noise)
           for j in (0, 6, len(osol.t) - 1)]
    dsol, _ = oref.drive(osolver, opde, obs)
    dm, ds = oracle.read_mean_and_std(dsol, osolver.E0)
    t, means, stds, sig, final, info = solver.solve_marginals(pde, observations=obs)
    assert_mean_std_parity(means, stds, dm, ds)
    np.testing.assert_allclose(info["data_log_likelihoods"], dsol.info["data_log_likelihoods"], rtol=1e-4)
    assert np.abs(means - om).max() > 10 * 1e-5 * np.abs(om).max()             # the data matters
    flt = solver._device_filter
    assert flt.operator_schedule_pending() == (0, 0) and flt.forcing_pending() == (0, 0)


def test_linearisation_points_and_the_iterated_smoother_compose_with_the_operator(hip_ctx):
    pde, solver, opde, osolver = orf.logistic_pair(osolver_cls=ir.PointwiseEK1)
    _, om, _ = orf.logistic_reference()
    points = 1.01 * om[1:]
    osolver.set_points(points)
    try:
        psol = osolver.solve(opde)
    finally:
        osolver.set_points(None)
    pm, ps = oracle.read_mean_and_std(psol, osolver.E0)
    t, means, stds, sig, final = solver.solve_marginals(pde, linearize_at=points)
    assert_mean_std_parity(means, stds, pm, ps)
    flt = solver._device_filter
    assert flt.operator_schedule_pending() == (0, 0) and flt.linearization_pending() == (0, 0)
    it = ir.iterate(osolver, opde)
    got = solver.solve_iterated(pde, iterations=ir.ITERATIONS, tol=ir.TOL)
    print(f"logistic on kappa(t): reference increments {it.increments}, device {got.increments}")
    assert it.converged and got.converged and abs(got.num_iterations - it.num_iterations) <= 1
    assert_mean_std_parity(got.means, got.stds, it.means, it.stds)


def _bound_with_three_tables():
    """(filter, initial device state, K, (schedule, right-hand sides, points)): the forced logistic problem on kappa(t), the device
    bound, and the K rows of each per-step table of its loop -- not yet set."""
    pde, solver, _, _ = orf.logistic_pair(forcing=Forcing(source=_source), source=_source)
    s0 = solver.initialize(pde).y.device_state
    ts, _ = solver._constant_schedule(pde, None)
    _, om, _ = orf.logistic_reference()
    tables = (pde.time_dependent_operator.table(ts), pde.forcing.table(ts, pde), np.ascontiguousarray(1.01 * om[1:]))
    assert all(len(rows) == orf.LOGISTIC[3] for rows in tables)
    return solver._device_filter, s0, orf.LOGISTIC[3], tables


def _set_three(flt, tables):
    flt.set_operator_schedule(tables[0])
    flt.set_forcing(tables[1])
    flt.set_linearization_points(tables[2])


def _cursors(flt):
    return flt.linearization_pending(), flt.forcing_pending(), flt.operator_schedule_pending()


def test_three_tables_in_one_loop(hip_ctx):
    """Operator schedule, right-hand sides and linearisation points together: the rehearsal rewinds all three cursors, and one call
    of K steps equals calls of 5 and K - 5 on a second filter bit for bit."""
    flt, s0, K, tables = _bound_with_three_tables()
    _set_three(flt, tables)
    assert _cursors(flt) == ((0, K),) * 3
    a = s0.clone()
    flt.prepare_steps(a, K, DT)
    assert _cursors(flt) == ((0, K),) * 3 and np.array_equal(a.mean(), s0.mean()) and np.array_equal(a.cov(), s0.cov())
    m, s, i = flt.steps(a, K, DT)
    assert _cursors(flt) == ((K, K),) * 3
    oflt, b, _, _ = _bound_with_three_tables()
    _set_three(oflt, tables)
    m1, s1, i1 = oflt.steps(b, 5, DT)
    assert _cursors(oflt) == ((5, K),) * 3
    m2, s2, i2 = oflt.steps(b, K - 5, DT)
    assert _cursors(oflt) == ((K, K),) * 3
    assert np.array_equal(np.vstack((m1, m2)), m) and np.array_equal(np.vstack((s1, s2)), s)
    assert _sig(list(i1) + list(i2)) == _sig(i)
    assert np.array_equal(a.mean(), b.mean()) and np.array_equal(a.cov(), b.cov()) and a.t == b.t


def test_refusal_with_three_tables_names_the_short_one(hip_ctx):
    flt, s0, K, tables = _bound_with_three_tables()
    _set_three(flt, (tables[0], tables[1][:K - 1], tables[2]))
    w = s0.clone()
    with pytest.raises(_hip.PnmolHipError,
                       match=rf"forcing: {K} step\(s\) asked for, {K - 1} of {K - 1} right-hand side\(s\) left"):
        flt.steps(w, K, DT)
    assert _cursors(flt) == ((0, K), (0, K - 1), (0, K))
    assert w.t == s0.t and np.array_equal(w.mean(), s0.mean()) and np.array_equal(w.cov(), s0.cov())


# ------------------------------------------------------------------------------------------------------------------ 8. backward pass
@pytest.mark.parametrize("family, shape", [("A", orf.SHAPES[0]), ("A", orf.SHAPES[1]), ("B", orf.SHAPES[1])])
def test_backward_pass_on_a_recorded_solution(hip_ctx, family, shape):
    """`smooth`, `smooth_marginals` and `functionals` on a `solve_on_device` result against the dense NumPy RTS over the reference
    trajectory, at north-star tolerances: the backward pass uses the prior alone."""
    N, nu, bcond, K = shape
    pde, solver, opde, osolver = orf.pair(family, *shape)
    osol, _, _ = orf.reference(family, *shape)
    osolver.initialize(opde)                                    # (E0 and the prior of this instance)
    sol = solver.solve_on_device(pde)
    ms, Ps = rts_on_oracle(osolver, osol)
    n, d = osol.mean.shape[1:]
    ostd = marginal_std(Ps, n, d)
    ssol = solver.smooth(sol)
    assert_mean_std_parity(ssol.mean[:, 0], ssol.marginal_std[:, 0], ms[:, 0], ostd[:, 0])
    means, stds = solver.smooth_marginals(sol)
    assert_mean_std_parity(means, stds, ms[:, 0], ostd[:, 0])
    where = [(k, j) for k in (0, K // 2, K) for j in (1, N // 2, N - 2)]
    post = solver.functionals(sol, np.stack([fn.point(K, N, k, j) for k, j in where]))
    sm = np.array([ms[k, 0, j] for k, j in where])
    sd = np.array([ostd[k, 0, j] for k, j in where])
    assert_mean_std_parity(post.mean, post.std, sm, sd)


# ------------------------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_through_raw_ctypes(hip_ctx):
    shape = orf.SHAPES[0]
    K = shape[3]
    pde, solver, flt, s = _bound("B", shape, plain=True)
    op = orf.pair("B", *shape)[0].time_dependent_operator
    lib, h = flt.lib, flt.handle
    err = lambda: lib.pnmol_last_error(flt.ctx.handle).decode()                 # noqa: E731
    d = flt.d
    Ls, es = np.ascontiguousarray(op.operators), np.ascontiguousarray(op.noise_diagonals)
    ts, _ = solver._constant_schedule(pde, None)
    table = np.ascontiguousarray(op.table(ts))
    nxt, cnt = ctypes.c_int(7), ctypes.c_int(7)

    def pending():
        assert lib.pnmol_filter_operator_schedule_pending(h, ctypes.byref(nxt), ctypes.byref(cnt)) == 0
        return nxt.value, cnt.value

    def untouched(ref):
        out, _, _ = flt.step(s, DT, want_error=False)
        return np.array_equal(out.mean(), ref.mean()) and np.array_equal(out.cov(), ref.cov())

    ref, _, _ = flt.step(s, DT, want_error=False)              # the step of the plain filter: what every refusal leaves in place
    assert pending() == (0, 0)
    # null filter
    assert lib.pnmol_filter_set_operator_family(None, 2, _dp(Ls), _dp(es)) == -1
    assert lib.pnmol_filter_set_operator_schedule(None, K, _dp(table)) == -1
    assert lib.pnmol_filter_operator_at(None, _dp(table[0])) == -1
    assert lib.pnmol_filter_operator_schedule_pending(None, ctypes.byref(nxt), ctypes.byref(cnt)) == -1
    # a schedule or coefficients without a family
    assert lib.pnmol_filter_set_operator_schedule(h, K, _dp(table)) == -1
    assert "pnmol_filter_set_operator_schedule" in err() and "no operator family set" in err()
    assert lib.pnmol_filter_operator_at(h, _dp(table[0])) == -1 and "pnmol_filter_operator_at" in err() and "no operator family" in err()
    # R outside [1, 4]
    five = np.ascontiguousarray(np.tile(Ls[:1], (5, 1, 1)))
    assert lib.pnmol_filter_set_operator_family(h, 5, _dp(five), _dp(np.ones((5, d)))) == -1
    assert "pnmol_filter_set_operator_family" in err() and "R outside [1, 4]" in err()
    assert lib.pnmol_filter_set_operator_family(h, -1, _dp(Ls), _dp(es)) == -1 and "R outside [1, 4]" in err()
    # entries that are not finite: operator, row and column are named
    for bad in (np.nan, np.inf):
        broken = Ls.copy()
        broken[1, 7, 3] = bad
        assert lib.pnmol_filter_set_operator_family(h, 2, _dp(broken), _dp(es)) == -1
        assert "operator 1" in err() and "row 7" in err() and "column 3" in err() and "not finite" in err(), err()
        broken = es.copy()
        broken[0, 5] = bad
        assert lib.pnmol_filter_set_operator_family(h, 2, _dp(Ls), _dp(broken)) == -1
        assert "noise diagonal of operator 0" in err() and "row 5" in err(), err()
    assert untouched(ref) and flt.dims()["m"] == d + 2
    # a filter whose operator or shift was replaced through the setters: image and clearing start from the creation-time operator
    # and would lose it.  Setting a term restores that operator and lifts the refusal.
    _, _, rflt, rs = _bound("B", shape, plain=True)
    rh, rerr = rflt.handle, (lambda: lib.pnmol_last_error(rflt.ctx.handle).decode())
    rflt.set_operator(1.5 * pde.L, np.full(d, 0.25))
    shifted, _, _ = rflt.step(rs, DT, want_error=False)
    assert lib.pnmol_filter_set_operator_family(rh, 2, _dp(Ls), _dp(es)) == -1 and "operator given at creation was replaced" in rerr()
    again, _, _ = rflt.step(rs, DT, want_error=False)          # nothing was touched: the replaced operator and its shift are there
    assert np.array_equal(again.mean(), shifted.mean()) and np.array_equal(again.cov(), shifted.cov())
    assert not np.array_equal(shifted.mean(), ref.mean())
    rflt.set_reaction(reactions.logistic(2.0))
    rflt.set_reaction(None)
    assert lib.pnmol_filter_set_operator_family(rh, 2, _dp(Ls), _dp(es)) == 0
    assert lib.pnmol_filter_set_operator_family(rh, 0, None, None) == 0
    back, _, _ = rflt.step(rs, DT, want_error=False)
    assert np.array_equal(back.mean(), ref.mean()) and np.array_equal(back.cov(), ref.cov())
    rflt.set_operator_diagonal(np.full(d, -0.5))
    assert lib.pnmol_filter_set_operator_family(rh, 2, _dp(Ls), _dp(es)) == -1 and "was replaced" in rerr()
    # a latent-force and an fp32 filter
    import observe_reference as oref_

    lpde, lsolver, _, _ = oref_.latent_pair(24, 1, DT, K, "dirichlet", 0.05)
    ls = lsolver.initialize(lpde).y.device_state
    lh, lctx = ls.filter.handle, ls.filter.ctx.handle
    assert lib.pnmol_filter_set_operator_family(lh, 2, _dp(Ls), _dp(es)) == -1 and "latent-force" in lib.pnmol_last_error(lctx).decode()
    f32 = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(DT))
    f32.dtype = "f32"
    s32 = f32.initialize(pde).y.device_state
    h32, ctx32 = s32.filter.handle, s32.filter.ctx.handle
    assert lib.pnmol_filter_set_operator_family(h32, 2, _dp(Ls), _dp(es)) == -1 and "fp32" in lib.pnmol_last_error(ctx32).decode()
    assert lib.pnmol_filter_set_operator_schedule(h32, K, _dp(table)) == -1 and "fp32" in lib.pnmol_last_error(ctx32).decode()
    assert lib.pnmol_filter_operator_at(h32, _dp(table[0])) == -1 and "fp32" in lib.pnmol_last_error(ctx32).decode()
    # a reaction system or a convection term and a family: whichever comes second is refused
    burgers = reactions.burgers()
    burgers.set_operator(0.5 * (np.eye(d, k=1) - np.eye(d, k=-1)))
    system = reactions.SystemReaction(2, p=[[(1.0, (1, 0)), (-1.0, (1, 1))], [(0.5, (1, 1))]])
    for term in (burgers, system):
        flt.set_reaction(term)
        assert lib.pnmol_filter_set_operator_family(h, 2, _dp(Ls), _dp(es)) == -1 and "widened image of their own" in err()
        flt.set_reaction(None)
    assert untouched(ref)
    assert lib.pnmol_filter_set_operator_family(h, 2, _dp(Ls), _dp(es)) == 0
    # the family alone changes nothing: the operator and noise given at creation until the first coefficients arrive.  The image
    # is 5 slots wide now and the step takes its wide-stencil launches, whose sums run in another order: the same step to
    # rounding (1e-8 of the largest entry; an operator or a noise that had changed would show at 1e-2), and from here on the
    # refusals are held to the bits of this step
    plain_ref, ref = ref, flt.step(s, DT, want_error=False)[0]
    np.testing.assert_allclose(ref.mean(), plain_ref.mean(), rtol=0, atol=1e-8 * np.abs(plain_ref.mean()).max())
    np.testing.assert_allclose(ref.cov(), plain_ref.cov(), rtol=0, atol=1e-8 * np.abs(plain_ref.cov()).max())
    for term in (burgers, system):
        with pytest.raises(_hip.PnmolHipError, match="a time-dependent operator is set"):
            flt.set_reaction(term)
    flt.set_reaction(reactions.logistic(2.0))                   # a scalar reaction composes
    flt.set_reaction(None)
    assert untouched(ref)
    # the operator setters refuse while a family is set
    M, jd = np.ascontiguousarray(pde.L), np.zeros(d)
    assert lib.pnmol_filter_set_operator(h, _dp(M), None) == -1 and "clear the operator family first" in err()
    assert lib.pnmol_filter_set_operator_diagonal(h, _dp(jd), None) == -1 and "clear the operator family first" in err()
    # the table: count < 0, entries that are not finite
    assert lib.pnmol_filter_set_operator_schedule(h, -1, _dp(table)) == -1 and "count < 0" in err()
    for bad in (np.nan, -np.inf):
        broken = table.copy()
        broken[7, 1] = bad
        assert lib.pnmol_filter_set_operator_schedule(h, K, _dp(broken)) == -1
        assert "row 7" in err() and "column 1" in err() and "not finite" in err(), err()
        broken = table[0].copy()
        broken[1] = bad
        assert lib.pnmol_filter_operator_at(h, _dp(broken)) == -1 and "pnmol_filter_operator_at" in err() and "column 1" in err()
    assert lib.pnmol_filter_operator_at(h, None) == -1 and "null coefficients" in err()
    assert pending() == (0, 0) and untouched(ref)
    # between steps_begin and steps_end
    w = s.clone()
    flt.steps_begin(w, 2, DT)
    assert lib.pnmol_filter_set_operator_family(h, 2, _dp(Ls), _dp(es)) == -1 and "between pnmol_filter_steps_begin" in err()
    assert lib.pnmol_filter_set_operator_family(h, 0, None, None) == -1 and "between" in err()
    assert lib.pnmol_filter_set_operator_schedule(h, K, _dp(table)) == -1 and "between" in err()
    assert lib.pnmol_filter_set_operator_schedule(h, 0, None) == -1 and "between" in err()
    assert lib.pnmol_filter_operator_at(h, _dp(table[0])) == -1 and "between" in err()
    flt.steps_end(w)
    # k steps with k - 1 rows left: -1, the counts in the text, nothing enqueued, state and cursor untouched
    assert lib.pnmol_filter_set_operator_schedule(h, 5, _dp(table)) == 0 and pending() == (0, 5)
    w = s.clone()
    mean0, cov0, t0 = w.mean(), w.cov(), w.t
    assert lib.pnmol_filter_steps_begin(h, w.handle, 6, DT) == -1
    assert "pnmol_filter_steps_begin" in err() and "6 step(s) asked for, 5 of 5" in err(), err()
    assert w.t == t0 and np.array_equal(w.mean(), mean0) and np.array_equal(w.cov(), cov0) and pending() == (0, 5)
    flt.steps(w, 3, DT)
    assert pending() == (3, 5)
    assert lib.pnmol_filter_steps_begin(h, w.handle, 3, DT) == -1 and "3 step(s) asked for, 2 of 5" in err() and pending() == (3, 5)
    # clearing the family drops the schedule and gives the plain filter back
    assert lib.pnmol_filter_set_operator_family(h, 0, None, None) == 0 and pending() == (0, 0)
    flt.operator_family = 0
    assert untouched(plain_ref)
    assert lib.pnmol_filter_set_operator_diagonal(h, _dp(jd), None) == 0
    assert lib.pnmol_filter_set_operator(h, _dp(M), None) == 0
