"""CPU tests of time-dependent operators (`pnmol.pde.coefficients`, `pnmol_filter_set_operator_family`, `_set_operator_schedule`,
`_operator_at`): validation and arithmetic of `TimeDependentOperator`, the host logic of the family's image and
the schedule (csrc/pnmol_operator_plan.hpp, nothing of HIP in it) under AddressSanitizer + UBSan -- tests/operator_plan_check.cpp is a
stand-alone program that includes nothing but that header --, the C ABI's new names, the recipes, the refusal of every solver class
that does not honour the operator, the `"operator"` option of the loop driver on a stub, and the conditions the cases of
tests/test_gpu_operator.py must meet on the NumPy reference alone (tests/operator_reference.py).  No GPU."""

import pathlib
import re
import subprocess

import numpy as np
import pytest

import pnmol
import operator_reference as orf
import test_loop_driver_host as drv
from pnmol import _hip, pdefilter
from pnmol.base import rv
from pnmol.pde import coefficients, examples, reactions
from pnmol.pde.coefficients import TimeDependentOperator

ROOT = pathlib.Path(__file__).resolve().parent.parent
CLANG = pathlib.Path("/opt/rocm/lib/llvm/bin/clang++")
NAMES = ("pnmol_filter_set_operator_family", "pnmol_filter_set_operator_schedule", "pnmol_filter_operator_schedule_pending",
         "pnmol_filter_operator_at")


@pytest.mark.skipif(not CLANG.exists(), reason="the ROCm clang++ is not available")
def test_operator_plan_host_logic_under_asan_ubsan(tmp_path):
    exe = tmp_path / "operator_plan_check"
    subprocess.run([str(CLANG), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'pnmol-experiments_amd' / 'csrc'}", str(ROOT / "tests" / "operator_plan_check.cpp"), "-o", str(exe)],
                   check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "operator plan: ok" and "runtime error" not in run.stderr


def test_operator_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "pnmol_hip.h").read_text()
    lib = _hip.load_library()
    for name in NAMES:
        assert name in _hip.SYMBOLS
        assert re.search(rf"\bint {name}\(", header)
        assert hasattr(lib, name)
    assert lib.pnmol_abi_version() == 3
    assert re.search(r"#define PNMOL_OPERATOR_MAXR 4\b", header) and coefficients.MAX_OPERATORS == 4
    for method in ("set_operator_family", "clear_operator_family", "set_operator_schedule", "clear_operator_schedule",
                   "operator_schedule_pending", "operator_at"):
        assert method in dir(_hip.Filter)
    assert (ROOT / "pnmol-experiments_amd" / "csrc" / "pnmol_operator.hip") in __import__("__graft_entry__").SOURCES


# ------------------------------------------------------------------------------------------------ TimeDependentOperator
def _family(d=5, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((3, d, d)), np.abs(rng.standard_normal((3, d))) + 0.1


def test_matrix_and_noise_use_the_kernels_order_of_operations():
    L, e = _family()
    a_of = lambda t: (1.0 + t, -0.7 * t, 0.0 if t < 1 else 3.0)                              # noqa: E731
    op = TimeDependentOperator(L, e, a_of)
    assert op.num_operators == 3
    for t in (0.0, 0.3, 1.5):                                   # a zero and a negative coefficient among them
        a = np.asarray(a_of(t))
        want = a[0] * L[0]
        want = want + a[1] * L[1]
        want = want + a[2] * L[2]
        assert np.array_equal(op.matrix(t), want)
        q = (a[0] * e[0]) * (a[0] * e[0])
        q = q + (a[1] * e[1]) * (a[1] * e[1])
        q = q + (a[2] * e[2]) * (a[2] * e[2])
        E = op.noise_sqrtm(t)
        assert np.array_equal(E, np.diag(np.sqrt(q))) and np.all(np.diag(E) >= 0.0)
        np.testing.assert_allclose(E @ E.T, sum((a[r] * e[r]) ** 2 for r in range(3)) * np.eye(5), rtol=1e-15)
    # exact cases the GPU tests lean on: 1 * v, v + 0 * g, (1 e)^2 + (0 e')^2
    op2 = TimeDependentOperator(L[:2], e[:2], lambda t: (1.0, 0.0))
    assert np.array_equal(op2.matrix(0.0), L[0]) and np.array_equal(op2.noise_sqrtm(0.0), np.diag(e[0]))
    one = TimeDependentOperator(L[0], e[0], lambda t: -2.0)                                 # R = 1: a scalar coefficient
    assert np.array_equal(one.matrix(0.0), -2.0 * L[0]) and np.array_equal(one.noise_sqrtm(0.0), np.diag(2.0 * e[0]))
    # diagonal matrices are taken as their diagonals
    as_matrices = TimeDependentOperator(L, np.stack([np.diag(x) for x in e]), a_of)
    assert np.array_equal(as_matrices.noise_diagonals, e)


def test_table_follows_the_constant_schedule_runt_step_included():
    pde, solver, _, _ = orf.pair("B", 24, 2, "neumann", 12.3)
    ts, dts = solver._constant_schedule(pde, None)
    assert len(dts) == 13 and dts[-1] < dts[0]
    op = pde.time_dependent_operator
    table = op.table(ts)
    assert table.shape == (13, 2) and np.array_equal(table, solver._operator_table(pde, ts))
    c = orf.velocity_of(12.3)
    for k in range(13):
        assert np.array_equal(table[k], np.array([orf.KAPPA, -c(ts[k + 1])]))
    assert np.any(table[:, 1] > 0) and np.any(table[:, 1] < 0) and op.coefficients(pde.t0)[1] == 0.0
    assert op.table(ts[:1]).shape == (0, 2)
    plan = solver._loop_plan(pde, None, None, None)
    assert np.array_equal(plan.operator, table) and plan.forcing is None and plan.points is None
    assert solver._loop_plan(pde, 0, None, None).operator is None


def test_validation_on_the_host():
    L, e = _family()
    ok = lambda t: (1.0, 2.0, 3.0)                                                          # noqa: E731
    with pytest.raises(ValueError, match=r"R = 5"):
        TimeDependentOperator(np.zeros((5, 3, 3)), np.zeros((5, 3)), ok)
    with pytest.raises(ValueError, match=r"\(R, d, d\)"):
        TimeDependentOperator(np.zeros((2, 3, 4)), np.zeros((2, 3)), ok)
    with pytest.raises(ValueError, match="noise_diagonals"):
        TimeDependentOperator(L, e[:2], ok)
    dense = np.stack([np.diag(x) for x in e])
    dense[1, 0, 2] = 1e-9
    with pytest.raises(ValueError, match="only diagonal"):
        TimeDependentOperator(L, dense, ok)
    bad = L.copy()
    bad[2, 1, 3] = np.nan
    with pytest.raises(ValueError, match="operator 2 is not finite at row 1, column 3"):
        TimeDependentOperator(bad, e, ok)
    bad_e = e.copy()
    bad_e[1, 4] = np.inf
    with pytest.raises(ValueError, match="noise diagonal of operator 1 is not finite at row 4"):
        TimeDependentOperator(L, bad_e, ok)
    with pytest.raises(TypeError, match="callable"):
        TimeDependentOperator(L, e, (1.0, 2.0, 3.0))
    op = TimeDependentOperator(L, e, lambda t: (1.0, 2.0) if t > 0.5 else (1.0, np.nan, 0.0))
    with pytest.raises(ValueError, match="not finite"):
        op.matrix(0.0)
    with pytest.raises(ValueError, match="shape"):
        op.table(np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="1-d time grid"):
        TimeDependentOperator(L, e, ok).table(np.zeros((2, 2)))


def test_recipes_carry_the_operator_and_pose_t0():
    kw = dict(dx=1.0 / 15, tmax=1.0, kernel=pnmol.kernels.SquareExponential())
    heat = examples.heat_1d_discretized(diffusion_rate=1.0, **kw)
    kappa = lambda t: 0.05 * (1.0 + 0.5 * np.sin(t + 1.0))                                  # noqa: E731
    pde = examples.heat_1d_time_varying_discretized(diffusion_rate=kappa, **kw)
    op = pde.time_dependent_operator
    assert op.num_operators == 1 and np.array_equal(op.operators[0], heat.L)
    assert np.array_equal(op.noise_diagonals[0], np.diag(heat.E_sqrtm))
    assert np.array_equal(pde.L, kappa(0.0) * heat.L) and np.array_equal(pde.E_sqrtm, np.diag(np.abs(kappa(0.0) * np.diag(heat.E_sqrtm))))
    assert np.array_equal(pde.y0, heat.y0) and np.array_equal(pde.B, heat.B)
    adv = examples.advection_diffusion_1d_discretized(0.05, velocity=lambda t: np.sin(3.0 * t), gradient_stencil_size=5, **kw)
    op = adv.time_dependent_operator
    G, Ge = pnmol.discretize.fd_probabilistic(pnmol.diffops.gradient(), mesh_spatial=adv.mesh_spatial, kernel=kw["kernel"],
                                              stencil_size_interior=5, stencil_size_boundary=5, nugget_gram_matrix=0.0)
    assert np.array_equal(op.operators, np.stack([heat.L, G])) and np.array_equal(op.noise_diagonals[1], np.diag(Ge))
    assert np.all((G != 0).sum(axis=1) == 5) and np.all((heat.L != 0).sum(axis=1) == 3)      # the union is wider than pde.L
    assert np.array_equal(adv.L, 0.05 * heat.L) and np.array_equal(op.coefficients(0.5), [0.05, -np.sin(1.5)])
    # reaction= and forcing= go through
    from pnmol.pde.forcing import Forcing

    both = examples.heat_1d_time_varying_discretized(diffusion_rate=kappa, reaction=reactions.logistic(3.0),
                                                     forcing=Forcing(source=lambda t, X: np.ones(X.shape[0])), **kw)
    assert both.reaction is not None and both.forcing is not None and both.time_dependent_operator is not None
    assert np.array_equal(both.y0, heat.y0)
    with pytest.raises(TypeError, match="callable"):
        examples.heat_1d_time_varying_discretized(diffusion_rate=0.05, **kw)
    with pytest.raises(TypeError, match="callable"):
        examples.advection_diffusion_1d_discretized(0.05, velocity=1.0, **kw)


def test_linearize_returns_the_operator_of_t():
    pde, solver, _, _ = orf.pair("A", 24, 2, "neumann", 12)
    M, shift = solver._linearize(pde, pde.y0, 0.07)
    assert np.array_equal(M, pde.time_dependent_operator.matrix(0.07)) and not np.any(shift)
    lpde, lsolver, _, _ = orf.logistic_pair()
    u = 0.2 + 0.1 * np.cos(np.arange(lpde.L.shape[0]))
    M, shift = lsolver._linearize(lpde, u, 0.07)
    J = np.diag(orf.LOGISTIC_RATE * (1.0 - 2.0 * u))
    np.testing.assert_allclose(M, lpde.time_dependent_operator.matrix(0.07) + J, rtol=1e-14, atol=1e-14)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_device_work(monkeypatch):
    monkeypatch.setattr(_hip.Filter, "__init__", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("device work")))
    monkeypatch.setattr(_hip.SqrtFilter, "__init__", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("device work")))
    monkeypatch.setattr(_hip.Context, "default", classmethod(lambda cls, device=None: (_ for _ in ()).throw(AssertionError("device work"))))
    rule = pnmol.odetools.step.Constant(orf.DT)
    kernel = pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise()
    pde, solver, _, _ = orf.pair("A", 24, 1, "dirichlet", 12)
    tpde, tsolver, _, _ = orf.logistic_pair()

    def every_entry(s, p, iterated=False):
        calls = [lambda: s.solve(p), lambda: s.solve_marginals(p), lambda: s.solve_on_device(p), lambda: s.initialize(p)]
        if iterated:
            calls.append(lambda: s.solve_iterated(p))
        return calls

    f32 = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=rule, spatial_kernel=kernel)
    f32.dtype = "f32"
    host_route = orf.make_solver(2, rule, semilinear=True)
    host_route.reaction_on_device = False
    no_term = examples.spruce_budworm_1d_discretized(tmax=12 * orf.DT, dx=1.0 / 23, kernel=pnmol.kernels.SquareExponential())
    no_term.time_dependent_operator = pde.time_dependent_operator           # host callables only: no term for the device
    system = examples.reaction_diffusion_system_1d_discretized(reactions.lotka_volterra(0.5, 0.4, 0.4, 0.5), diffusion_rates=(0.1, 0.1),
                                                               y0_fun=examples.lotka_volterra_y0, dx=1.0 / 11, tmax=12 * orf.DT)
    L2 = np.kron(np.eye(2), np.eye(12))
    system.time_dependent_operator = TimeDependentOperator(L2, np.ones(24), lambda t: 1.0)
    burgers = examples.burgers_1d_discretized(dx=1.0 / 23, tmax=12 * orf.DT, kernel=pnmol.kernels.SquareExponential())
    burgers.time_dependent_operator = pde.time_dependent_operator
    refused = [
        (pnmol.sqrtform.LinearWhiteNoiseEK1(num_derivatives=1, steprule=rule, spatial_kernel=kernel), pde, False),
        (pnmol.sqrtform.SemiLinearWhiteNoiseEK1(num_derivatives=2, steprule=rule, spatial_kernel=kernel), tpde, False),
        (pnmol.sqrtform.LinearLatentForceEK1(num_derivatives=1, steprule=rule), pde, False),
        (pnmol.sqrtform.SemiLinearLatentForceEK1(num_derivatives=1, steprule=rule), tpde, False),
        (pnmol.latent.LinearLatentForceEK1(num_derivatives=1, steprule=rule), pde, False),
        (pnmol.latent.SemiLinearLatentForceEK1(num_derivatives=1, steprule=rule), tpde, False),
        (f32, pde, False),
        (host_route, tpde, True),
        (tsolver, no_term, True),
        (orf.make_solver(2, rule, semilinear=True), system, True),
        (orf.make_solver(2, rule, semilinear=True), burgers, True),
    ]
    for s, p, iterated in refused:
        for call in every_entry(s, p, iterated):
            with pytest.raises(TypeError, match="time_dependent_operator"):
                call()
        state = pdefilter.PDEFilterState(t=p.t0, y=None, error_estimate=None, reference_state=None, diffusion_squared_local=[])
        if type(s).__module__ == "pnmol.white":
            with pytest.raises(TypeError, match="time_dependent_operator"):
                s.attempt_step(state, orf.DT, p)
    # coefficients that are wrong: ValueError from the table, in front of the device
    good = pde.time_dependent_operator
    pde.time_dependent_operator = TimeDependentOperator(good.operators, good.noise_diagonals,
                                                        lambda t: np.nan if t > 5 * orf.DT else 1.0)
    for call in (lambda: solver.solve_marginals(pde), lambda: solver.solve_on_device(pde)):
        with pytest.raises(ValueError, match="not finite"):
            call()
    pde.time_dependent_operator = good
    # the supported combinations pass the refusals and reach the device
    adaptive = orf.make_solver(1, pnmol.odetools.step.Adaptive())
    for s, p, iterated in ((solver, pde, False), (tsolver, tpde, True)):
        for call in every_entry(s, p, iterated):
            with pytest.raises(AssertionError, match="device work"):
                call()
    with pytest.raises(AssertionError, match="device work"):
        adaptive.solve(pde)


# ------------------------------------------------------------------------------------------------ the loop driver's option
class StubFilter(drv.StubFilter):
    """The driver tests' stub with the operator option."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.counts["operator"] = 0

    def set_operator_schedule(self, a):
        self.call("set_operator_schedule")
        self.counts["operator"] = len(a)

    def clear_operator_schedule(self):
        self.call("clear_operator_schedule")
        self.counts["operator"] = 0

    operator_schedule_pending = lambda self: self._pending("operator")                      # noqa: E731


def _stubbed(monkeypatch, pde, solver, **kw):
    on_device = solver._reaction_for_device(pde) is not None
    flt = StubFilter(solver.num_derivatives + 1, pde.L.shape[0], pde.L.shape[0] + pde.B.shape[0],
                     pde.reaction if on_device else None, **kw)

    def initialize(self, p):
        self._device_filter, self._device_pde = flt, p
        dev = drv.StubState(flt)
        return pdefilter.PDEFilterState(t=p.t0, y=rv.DeviceMultivariateNormal(dev.mean(), dev), error_estimate=None,
                                        reference_state=None, diffusion_squared_local=[])

    monkeypatch.setattr(type(solver), "initialize", initialize)
    monkeypatch.setattr(_hip.Filter, "__init__", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("device work")))
    return flt


def _driven_problem():
    """Family (A) with the logistic term and a source, 4.5 steps: points, forcing and operator all apply."""
    from pnmol.pde.forcing import Forcing

    K = 4.5
    pde = orf.problem("A", 16, K, "dirichlet", reaction=reactions.logistic(3.0),
                      forcing=Forcing(source=lambda t, X: np.sin(t) * np.ones(X.shape[0])))
    return pde, orf.make_solver(2, pnmol.odetools.step.Constant(orf.DT), semilinear=True)


@pytest.mark.parametrize("entry", ["solve_marginals", "solve_on_device", "solve_iterated"])
def test_operator_option_is_installed_last_and_cleared_last(monkeypatch, entry):
    pde, solver = _driven_problem()
    flt = _stubbed(monkeypatch, pde, solver)
    d = pde.L.shape[0]
    args = dict(iterations=0, smooth=None, start=np.full((5, d), 0.1)) if entry == "solve_iterated" else dict(linearize_at=np.full((5, d), 0.1))
    getattr(solver, entry)(pde, **args)
    recorder = entry != "solve_marginals"
    want = (["set_recorder"] if recorder else []) + ["set_linearization_points", "set_forcing", "set_operator_schedule"]
    want += (["clone"] if recorder else []) + ["steps(4)", "steps(1)"] + (["clear_recorder"] if recorder else [])
    want += ["clear_linearization_points", "clear_forcing", "clear_operator_schedule"]
    assert flt.calls == want
    assert flt.error_model_dt is None                           # the loop prepares no error model for a changing operator


def test_linear_problem_installs_the_operator_alone_and_prepares_no_error_model(monkeypatch):
    pde, solver, _, _ = orf.pair("A", 16, 2, "dirichlet", 4.5)
    flt = _stubbed(monkeypatch, pde, solver)
    solver.solve_marginals(pde)
    assert flt.calls == "set_operator_schedule steps(4) steps(1) clear_operator_schedule".split()
    assert flt.error_model_dt is None


@pytest.mark.parametrize("failure", ["set_operator_schedule", "steps", "clear_operator_schedule", "set_forcing"])
def test_operator_option_is_cleared_on_failure(monkeypatch, failure):
    pde, solver = _driven_problem()
    error = drv.Boom("the loop failed") if failure == "steps" else _hip.PnmolHipError(failure)
    flt = _stubbed(monkeypatch, pde, solver, fail={failure: error})
    with pytest.raises(type(error), match="the loop failed" if failure == "steps" else failure):
        solver.solve_marginals(pde)
    attempted_operator = failure != "set_forcing"               # (forcing is installed in front of it)
    assert ("set_operator_schedule" in flt.calls) == attempted_operator
    assert flt.calls.count("clear_operator_schedule") == int(attempted_operator)
    assert flt.calls.count("clear_forcing") == 1
    tail = ["clear_forcing"] + (["clear_operator_schedule"] if attempted_operator else [])
    assert flt.calls[-len(tail):] == tail


@pytest.mark.parametrize("entry", ["solve_marginals", "solve_on_device", "solve_iterated"])
def test_every_entry_point_checks_that_the_loop_consumed_the_schedule(monkeypatch, entry):
    pde, solver = _driven_problem()
    flt = _stubbed(monkeypatch, pde, solver, leftover="operator")
    args = dict(iterations=0, smooth=None) if entry == "solve_iterated" else {}
    with pytest.raises(RuntimeError, match="did not consume every row of coefficients"):
        getattr(solver, entry)(pde, **args)
    assert flt.calls[-1] == "clear_operator_schedule"


def test_no_step_installs_nothing(monkeypatch):
    pde, solver = _driven_problem()
    flt = _stubbed(monkeypatch, pde, solver)
    solver.solve_marginals(pde, num_steps=0)
    assert flt.calls == []


# ------------------------------------------------------------------------------------ conditions on the inputs of the GPU tests
def _moved(a, b):
    return float(np.abs(a - b).max() / np.abs(a).max())


@pytest.mark.parametrize("family, shape", [("A", s) for s in orf.SHAPES] + [("B", s) for s in orf.SHAPES_B])
def test_the_schedule_moves_the_cases_by_100_tolerances(family, shape):
    """On the oracle alone: the reference is finite, and against constant coefficients (a = 1, c = 0) means and stds move by at
    least 100 times the tolerances of the GPU tests, so a schedule that is ignored, or applied without its noise, cannot pass."""
    _, means, stds = orf.reference(family, *shape)
    _, means0, stds0 = orf.reference(family, *shape, constant=True)
    assert np.all(np.isfinite(means)) and np.all(np.isfinite(stds))
    moved, moved_std = _moved(means, means0), _moved(stds, stds0)
    print(f"({family}) {shape}: means move by {moved:.2e} of their largest entry, stds by {moved_std:.2e}")
    assert moved >= 100 * orf.MEAN_RTOL and moved_std >= 100 * orf.STD_RTOL
    if family == "A" and shape[0] < 255:                        # the figures of the issue: 2 - 8 % and 10 - 35 %
        assert 0.015 <= moved <= 0.09 and 0.09 <= moved_std <= 0.36


def test_the_noise_scaling_alone_moves_the_stds():
    """The operator applied with the noise left at E(t0): the stds differ from the reference by 100 tolerances."""
    N, nu, bcond, K = orf.SHAPES[0]
    pde, _, opde, osolver = orf.pair("A", N, nu, bcond, K)
    frozen = type("Frozen", (orf.TimeVaryingOraclePde,), {"E_sqrtm": property(lambda self: np.array(pde.E_sqrtm))})(
        opde._opde, pde.time_dependent_operator)
    import pnmol_oracle as oracle

    sol = osolver.solve(frozen)
    _, stds_frozen = oracle.read_mean_and_std(sol, osolver.E0)
    _, _, stds = orf.reference("A", N, nu, bcond, K)
    assert _moved(stds, stds_frozen) >= 100 * orf.STD_RTOL


def test_the_logistic_case_is_finite_and_moved():
    _, means, stds = orf.logistic_reference()
    assert np.all(np.isfinite(means)) and np.all(np.isfinite(stds))
    N, nu, bcond, K = orf.LOGISTIC
    import pnmol_oracle as oracle

    pde = orf.problem("A", N, K, bcond, reaction=reactions.logistic(orf.LOGISTIC_RATE), constant=True)
    opde = orf.oracle_problem(pde, N, K, bcond, extra_f=lambda _t, x: orf.LOGISTIC_RATE * x * (1.0 - x),
                              extra_df=lambda _t, x: np.diag(orf.LOGISTIC_RATE * (1.0 - 2.0 * x)))
    osolver = orf.make_osolver(nu, oracle.Constant(orf.DT))
    means0, _ = oracle.read_mean_and_std(osolver.solve(opde), osolver.E0)
    assert _moved(means, means0) >= 100 * orf.MEAN_RTOL
