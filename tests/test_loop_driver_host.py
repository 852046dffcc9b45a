"""CPU tests of the one driver behind `solve_marginals`, `solve_on_device` and `solve_iterated` (pnmol/white.py: `_loop_plan`,
`_loop_options`, `_loop_consumed`) and of the one constant schedule (`pnmol.data.constant_schedule`).  A stub stands in for
`_hip.Filter`: it records the calls made on it and raises at one of them when told to, so the order in which the loop's options are
installed, run and cleared -- also behind a failure -- is checked without a device.  No GPU."""

import types

import numpy as np
import pytest

import pnmol
from pnmol import _hip, data, pdefilter
from pnmol.base import rv
from pnmol.pde import examples, reactions
from pnmol.pde.forcing import Forcing

DT, NU = 2.0 ** -4, 2
TMAX = 4.5 * DT                                                 # a run of four steps and a runt step
INSTALL = ("observations", "recorder", "points", "forcing")
CLEAR = ("recorder", "observations", "points", "forcing")
SETTER = dict(observations="set_observations", recorder="set_recorder", points="set_linearization_points", forcing="set_forcing")
CLEARER = dict(observations="clear_observations", recorder="clear_recorder", points="clear_linearization_points",
               forcing="clear_forcing")


class Boom(Exception):
    """The failure of the solve itself in these tests: not a `PnmolHipError`."""


class StubState:
    def __init__(self, flt):
        self.filter = flt

    def mean(self):
        return np.zeros((self.filter.n, self.filter.ds))

    def marginal_var(self):
        return np.ones((self.filter.n, self.filter.ds))

    def clone(self):
        self.filter.call("clone")
        return StubState(self.filter)


class StubFilter:
    """What the drivers use of `_hip.Filter`.  `calls`: the names of the calls that change the filter or advance a state, in order
    (`steps` with its count); queries are not recorded.  fail = {name: exception}: raised by that call, behind its record.
    leftover: the option whose `*_pending()` reports one entry that the loop did not use."""

    def __init__(self, n, d, m, reaction=None, fail=None, leftover=None):
        self.n, self.d, self.ds, self.m, self.reaction = n, d, d, m, reaction
        self.fail, self.leftover, self.calls, self.error_model_dt = dict(fail or {}), leftover, [], None
        self.counts = dict.fromkeys(INSTALL, 0)

    def call(self, name, shown=None):
        self.calls.append(shown or name)
        if name in self.fail:
            raise self.fail[name]

    def new_state(self):
        return StubState(self)

    def prepare_error_model(self, dt):
        self.error_model_dt = float(dt)

    def observe(self, state, C, y, R_sqrtm=None):
        assert C.shape[1] == self.ds
        self.call("observe")
        return StubState(self), types.SimpleNamespace(log_likelihood=-1.0)

    def steps(self, state, k, dt):
        self.call("steps", f"steps({k})")
        infos = [types.SimpleNamespace(diffusion_squared_local=1.0) for _ in range(k)]
        return np.zeros((k, self.d)), np.ones((k, self.d)), infos

    def smoother_steps(self, states, dts):
        return np.zeros((len(states), self.d)), np.ones((len(states), self.d))

    def recorder_means(self, first, count):
        return np.zeros((count, self.n, self.ds))

    def observation_results(self, first, count):
        return [types.SimpleNamespace(log_likelihood=-2.0 - i) for i in range(count)]

    def _pending(self, option):
        count = self.counts[option]
        return (count - (self.leftover == option) if count else 0), count

    def _set(self, option, count):
        self.call(SETTER[option])
        self.counts[option] = count

    def _clear(self, option):
        self.call(CLEARER[option])
        self.counts[option] = 0

    def set_observations(self, times, C, ys, R_sqrtm=None):
        assert C.shape[1] == self.ds and len(times) == len(ys)
        self._set("observations", len(times))

    set_recorder = lambda self, states: self._set("recorder", len(states))                                      # noqa: E731
    set_linearization_points = lambda self, points: self._set("points", len(points))                            # noqa: E731
    set_forcing = lambda self, rhs: self._set("forcing", len(rhs))                                              # noqa: E731
    clear_observations = lambda self: self._clear("observations")                                               # noqa: E731
    clear_recorder = lambda self: self._clear("recorder")                                                       # noqa: E731
    clear_linearization_points = lambda self: self._clear("points")                                             # noqa: E731
    clear_forcing = lambda self: self._clear("forcing")                                                         # noqa: E731
    observations_pending = lambda self: self._pending("observations")                                           # noqa: E731
    recorder_pending = lambda self: self._pending("recorder")                                                   # noqa: E731
    linearization_pending = lambda self: self._pending("points")                                                # noqa: E731
    forcing_pending = lambda self: self._pending("forcing")                                                     # noqa: E731


def heat_problem():
    pde = examples.heat_1d_discretized(tmax=TMAX, dx=1.0 / 15, kernel=pnmol.kernels.SquareExponential())
    return pde, pnmol.white.LinearWhiteNoiseEK1(num_derivatives=NU, steprule=pnmol.odetools.step.Constant(DT))


def term_problem():
    """A logistic term the device linearises, and a source: linearisation points and forcing both apply."""
    forcing = Forcing(source=lambda t, X: np.sin(t) * np.ones(X.shape[0]))
    pde = examples.reaction_diffusion_1d_discretized(reactions.logistic(3.0), tmax=TMAX, dx=1.0 / 15, forcing=forcing,
                                                     kernel=pnmol.kernels.SquareExponential())
    return pde, pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=NU, steprule=pnmol.odetools.step.Constant(DT))


def observations(pde):
    C = data.select_nodes(pde.L.shape[0], [3, 7])
    return [data.Observation(t, C, np.zeros(2), 1e-3) for t in (pde.t0, pde.t0 + 2 * DT)]


def stubbed(monkeypatch, pde, solver, **kw):
    """`solver` with `initialize` bound to a `StubFilter` in place of the device; returns the stub."""
    on_device = solver._reaction_for_device(pde) is not None
    flt = StubFilter(NU + 1, pde.L.shape[0], pde.L.shape[0] + pde.B.shape[0], pde.reaction if on_device else None, **kw)

    def initialize(self, p):
        self._device_filter, self._device_pde = flt, p
        dev = StubState(flt)
        return pdefilter.PDEFilterState(t=p.t0, y=rv.DeviceMultivariateNormal(dev.mean(), dev), error_estimate=None,
                                        reference_state=None, diffusion_squared_local=[])

    monkeypatch.setattr(type(solver), "initialize", initialize)
    monkeypatch.setattr(_hip.Filter, "__init__", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("device work")))
    return flt


# option set -> (problem, with observations, with linearize_at); a problem with a term and a source always has the forcing table
OPTION_SETS = dict(plain=(heat_problem, False, False), observed=(heat_problem, True, False),
                   term=(term_problem, False, True), all=(term_problem, True, True))


def run(monkeypatch, entry, option_set, **kw):
    """One solve of `entry` with `option_set` on a stub: (the stub, the options the driver has to install, the call)."""
    problem, observed, points = OPTION_SETS[option_set]
    pde, solver = problem()
    flt = stubbed(monkeypatch, pde, solver, **kw)
    args = dict(observations=observations(pde)) if observed else {}
    T, d = 5, pde.L.shape[0]
    if entry == "solve_iterated":
        args.update(iterations=0, smooth=None, **(dict(start=np.full((T, d), 0.5)) if points else {}))
    elif points:
        args.update(linearize_at=np.full((T, d), 0.5))
    present = dict(observations=observed, recorder=entry != "solve_marginals", points=points,
                   forcing=getattr(pde, "forcing", None) is not None)
    return flt, [o for o in INSTALL if present[o]], lambda: getattr(solver, entry)(pde, **args)


def cases():
    """entry point x option set x failure point.  A failure: None; "steps" (the solve's own failure, alone or with every clear
    failing too); a setter; a clear behind a solve that succeeded."""
    out = []
    for entry in ("solve_marginals", "solve_on_device", "solve_iterated"):
        for option_set, (_, observed, points) in OPTION_SETS.items():
            if entry == "solve_iterated" and option_set in ("plain", "observed"):
                continue                                        # (needs a term the device linearises)
            options = [o for o, there in zip(INSTALL, (observed, entry != "solve_marginals", points, points)) if there]
            failures = [None, "steps", "steps+clears"] + [SETTER[o] for o in options] + [CLEARER[o] for o in options]
            out.extend((entry, option_set, failure) for failure in failures)
    return out


@pytest.mark.parametrize("entry, option_set, failure", cases())
def test_options_are_installed_run_and_cleared_in_order(monkeypatch, entry, option_set, failure):
    fail = {}
    if failure in ("steps", "steps+clears"):
        fail["steps"] = Boom("the loop failed")
    if failure == "steps+clears":
        fail.update({name: _hip.PnmolHipError(name) for name in CLEARER.values()})
    elif failure is not None and failure != "steps":
        fail[failure] = _hip.PnmolHipError(failure)
    flt, options, call = run(monkeypatch, entry, option_set, fail=fail)
    observed = "observations" in options

    # what the driver has to do: the update at t0, the setters in install order up to one that fails, the loop, and the clears
    # of every option whose setter was attempted, in clear order -- all of them even where one fails
    want = ["observe"] if observed else []
    attempted = []
    for option in options:
        attempted.append(option)
        want.append(SETTER[option])
        if failure == SETTER[option]:
            break
    else:
        want += (["clone"] if entry != "solve_marginals" else []) + ["steps(4)"] + ([] if "steps" in fail else ["steps(1)"])
    want += [CLEARER[o] for o in CLEAR if o in attempted]

    if failure is None:
        result = call()
    elif "steps" in fail:
        with pytest.raises(Boom, match="the loop failed"):      # the solve's own failure, whatever the clears do
            call()
    else:
        with pytest.raises(_hip.PnmolHipError, match=failure):  # of a setter; of a clear behind a solve that succeeded
            call()
    assert flt.calls == want
    assert [flt.calls.count(CLEARER[o]) for o in attempted] == [1] * len(attempted)

    if failure is None:                                         # the result: five steps, the log-likelihoods t0 first
        lls = [-1.0, -2.0] if observed else None
        if entry == "solve_marginals":
            assert len(result) == (6 if observed else 5) and result[0].shape == (6,) and result[1].shape[0] == 6
            info = result[5] if observed else dict(data_log_likelihoods=None)
        else:
            sol = result.filtered if entry == "solve_iterated" else result
            assert sol.t.shape == (6,) and sol.mean.shape[0] == 6 and sol.info["num_steps"] == 5
            info = sol.info
        assert info.get("data_log_likelihoods") == lls
        if observed:
            assert info["data_log_likelihood"] == -3.0


def test_parent_call_sequences(monkeypatch):
    """The sequences of the drivers before they were one, as traced then."""
    traced = {
        ("solve_marginals", "plain"): "steps(4) steps(1)",      # the fast path: no option call
        ("solve_marginals", "observed"): "observe set_observations steps(4) steps(1) clear_observations",
        ("solve_on_device", "plain"): "set_recorder clone steps(4) steps(1) clear_recorder",
        ("solve_on_device", "observed"): "observe set_observations set_recorder clone steps(4) steps(1) clear_recorder "
                                         "clear_observations",
    }
    for (entry, option_set), want in traced.items():
        flt, _, call = run(monkeypatch, entry, option_set)
        call()
        assert flt.calls == want.split(), (entry, option_set)
    # linearisation points and forcing: behind the recorder, in front of the first steps; their clears last, in that order
    flt, _, call = run(monkeypatch, "solve_on_device", "all")
    call()
    c = flt.calls
    assert c.index("set_recorder") < c.index("set_linearization_points") < c.index("set_forcing") < c.index("steps(4)")
    assert c[-2:] == ["clear_linearization_points", "clear_forcing"]
    flt, _, call = run(monkeypatch, "solve_marginals", "term")
    call()
    assert flt.calls == "set_linearization_points set_forcing steps(4) steps(1) clear_linearization_points clear_forcing".split()


LEFTOVERS = dict(recorder="were not recorded", observations="were not reached by the loop",
                 points="did not consume every linearisation point", forcing="did not consume every right-hand side of the forcing")


@pytest.mark.parametrize("entry, option", [(e, o) for e in ("solve_marginals", "solve_on_device", "solve_iterated") for o in LEFTOVERS
                                           if (e, o) != ("solve_marginals", "recorder")])     # (which has no recorder)
def test_every_entry_point_checks_that_the_loop_consumed_its_options(monkeypatch, entry, option):
    message = LEFTOVERS[option]
    flt, options, call = run(monkeypatch, entry, "all", leftover=option)
    with pytest.raises(RuntimeError, match=message):
        call()
    assert flt.calls[-len(options):] == [CLEARER[o] for o in CLEAR if o in options]     # and everything is cleared


def test_no_step_installs_nothing(monkeypatch):
    for entry in ("solve_marginals", "solve_on_device"):
        pde, solver = term_problem()
        flt = stubbed(monkeypatch, pde, solver)
        result = getattr(solver, entry)(pde, num_steps=0, observations=observations(pde)[:1],
                                        linearize_at=np.zeros((0, pde.L.shape[0])))
        assert [c for c in flt.calls if c != "clone"] == ["observe"]
        info = result[5] if entry == "solve_marginals" else result.info
        assert info["num_steps"] == 0 and info["data_log_likelihoods"] == [-1.0]


# ------------------------------------------------------------------------------------------------ the schedule
SCHEDULES = [(0.0, 4.5 * DT, DT, None), (0.0, 4.0 * DT, DT, None), (0.25, 1.0, 0.3, None), (0.0, 4.5 * DT, DT, 3),
             (0.0, 4.5 * DT, DT, 0), (0.0, 1.0, 0.1, None)]


@pytest.mark.parametrize("t0, tmax, dt0, num_steps", SCHEDULES)
def test_one_schedule(t0, tmax, dt0, num_steps):
    """`data.constant_schedule`, `data.constant_step_grid` and the solvers' `_constant_schedule` are one schedule: the
    t-accumulation of the reference's loop, bit for bit, a runt last step included."""
    ts, dts, t, dt = [t0], [], t0, dt0                          # the reference's loop, written out
    while t < tmax and (num_steps is None or len(dts) < num_steps):
        dts.append(dt)
        t = t + dt
        ts.append(t)
        dt = min(dt0, tmax - t)
    got_ts, got_dts = data.constant_schedule(t0, tmax, dt0, num_steps)
    assert np.array_equal(got_ts, ts) and np.array_equal(got_dts, dts) and len(got_ts) == len(got_dts) + 1
    assert list(data.equal_step_runs(got_dts)) == [(sum(1 for x in dts if x == v), v) for v in dict.fromkeys(dts)]
    pde = types.SimpleNamespace(t0=t0, tmax=tmax)
    for module in (pnmol.white, pnmol.sqrtform, pnmol.latent):
        solver = module.LinearWhiteNoiseEK1 if module is not pnmol.latent else module.LinearLatentForceEK1
        s_ts, s_dts = solver(num_derivatives=NU, steprule=pnmol.odetools.step.Constant(dt0))._constant_schedule(pde, num_steps)
        assert np.array_equal(s_ts, ts) and np.array_equal(s_dts, dts)
    if num_steps is None:
        grid = data.constant_step_grid(t0, tmax, dt0)
        assert isinstance(grid, np.ndarray) and np.array_equal(grid, ts)
    if (tmax, num_steps) == (4.5 * DT, None):
        assert len(dts) == 5 and dts[-1] == 0.5 * DT and ts[-1] == tmax         # the runt step
    if (tmax, num_steps) == (4.0 * DT, None):
        assert dts == [DT] * 4 and ts[-1] == tmax                               # an exact multiple: no runt step
    if num_steps is not None:
        assert len(dts) == num_steps


@pytest.mark.parametrize("num_steps", [None, 3, 0])
def test_square_root_form_takes_the_same_schedule(monkeypatch, num_steps):
    pde, _ = heat_problem()
    solver = pnmol.sqrtform.LinearWhiteNoiseEK1(num_derivatives=NU, steprule=pnmol.odetools.step.Constant(DT))
    n, d, calls = NU + 1, pde.L.shape[0], []

    class StubSqrtFilter:
        def set_state(self, t, mean, C):
            pass

        def steps(self, k, dt):
            calls.append((k, dt))
            return np.zeros((k, d)), np.ones((k, d)), [types.SimpleNamespace(diffusion_squared_local=1.0) for _ in range(k)]

        def get_state(self):
            return 0.0, np.zeros((n, d)), np.eye(n * d)

    def initialize(self, p):
        self._sqrt_filter, self._device_pde, self._sqrt_last = StubSqrtFilter(), p, None
        return pdefilter.PDEFilterState(t=p.t0, y=rv.MultivariateNormal(np.zeros((n, d)), np.eye(n * d)), error_estimate=None,
                                        reference_state=None, diffusion_squared_local=[])

    monkeypatch.setattr(type(solver), "initialize", initialize)
    ts, means, stds, sig, final = solver.solve_marginals(pde, num_steps=num_steps)
    want_ts, want_dts = solver._constant_schedule(pde, num_steps)
    assert np.array_equal(ts, want_ts) and np.array_equal(ts, data.constant_step_grid(pde.t0, pde.tmax, DT)[:len(ts)])
    assert calls == {None: [(4, DT), (1, 0.5 * DT)], 3: [(3, DT)], 0: []}[num_steps]
    assert means.shape == stds.shape == (len(want_dts) + 1, d) and sig.shape == (len(want_dts),) and final.t == ts[-1]
