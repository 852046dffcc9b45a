"""CPU tests of sensor data in the device-resident loop (`solve_marginals(pde, observations=...)`,
`pnmol_filter_set_observations`): `pnmol.data.shared_sensors`, the host-side validation in front of any device work, the C ABI's
new names, and the reference of every schedule of tests/test_gpu_observe_loop.py against itself in covariance form.  No GPU."""

import pathlib
import re

import numpy as np
import pytest

import pnmol
import observe_reference as ref
from helpers import make_pair
from observe_loop_cases import SCHEDULES, schedule_run
from pnmol import _hip, data

ROOT = pathlib.Path(__file__).resolve().parents[1]
NAMES = ("pnmol_filter_set_observations", "pnmol_filter_observations_pending", "pnmol_filter_observation_results",
         "pnmol_state_observe_planned")


def test_shared_sensors():
    C = data.select_nodes(8, [1, 5])
    obs = [data.Observation(0.25 * (i + 1), C, [1.0 + i, 2.0 - i], 0.1) for i in range(3)]
    times, Cs, R, ys = data.shared_sensors(obs)
    np.testing.assert_array_equal(times, [0.25, 0.5, 0.75])
    np.testing.assert_array_equal(Cs, C)
    np.testing.assert_array_equal(R, 0.1 * np.eye(2))
    np.testing.assert_array_equal(ys, [[1.0, 2.0], [2.0, 1.0], [3.0, 0.0]])
    # noise-free throughout: no factor; equal factors given in different forms are equal sensors
    free = [data.Observation(0.5 * (i + 1), C, [0.0, 0.0]) for i in range(2)]
    assert data.shared_sensors(free)[2] is None
    mixed_form = [data.Observation(0.5, C, [0.0, 0.0], 0.1), data.Observation(1.0, C, [0.0, 0.0], [0.1, 0.1])]
    np.testing.assert_array_equal(data.shared_sensors(mixed_form)[2], 0.1 * np.eye(2))
    # a differing C: the first offender is named, the message points at solve()
    other = data.Observation(1.0, data.select_nodes(8, [1, 6]), [0.0, 0.0], 0.1)
    with pytest.raises(ValueError, match=r"observation 3 .*another C.*solve\(pde, observations"):
        data.shared_sensors(obs + [other, other])
    with pytest.raises(ValueError, match="observation 1 .*another C"):
        data.shared_sensors([obs[0], data.Observation(0.5, np.vstack((C, C[:1])), [0.0, 0.0, 0.0], 0.1)])
    # noise on one entry only
    with pytest.raises(ValueError, match=r"observation 2 .*noise factor.*solve\("):
        data.shared_sensors([free[0], free[1], data.Observation(2.0, C, [0.0, 0.0], 0.1)])
    with pytest.raises(ValueError, match="observation 1 .*noise factor"):
        data.shared_sensors([obs[0], data.Observation(0.5, C, [0.0, 0.0], 0.2)])
    with pytest.raises(ValueError):
        data.shared_sensors([])


def test_solve_marginals_rejects_bad_observations_before_any_device_work(monkeypatch):
    dt, K, N = 2.0 ** -4, 12, 16
    pde, solver, _, _ = make_pair(N, 2, dt, K)
    calls = []
    monkeypatch.setattr(type(solver), "initialize", lambda self, p: calls.append(p) or (_ for _ in ()).throw(AssertionError))
    monkeypatch.setattr(_hip.Filter, "__init__", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("device work")))
    C = data.select_nodes(N, [3])

    def ob(t, C=C, noise=1e-3):
        return data.Observation(t, C, np.zeros(C.shape[0]), noise)

    with pytest.raises(ValueError, match="is not a grid time"):                      # the message data.prepare gives
        solver.solve_marginals(pde, observations=[ob(4.5 * dt)])
    with pytest.raises(ValueError, match="strictly increasing"):
        solver.solve_marginals(pde, observations=[ob(8 * dt), ob(4 * dt)])
    with pytest.raises(ValueError, match=r"must lie in \[t0, tmax\]"):
        solver.solve_marginals(pde, observations=[ob((K + 1) * dt)])
    with pytest.raises(ValueError, match="another C"):
        solver.solve_marginals(pde, observations=[ob(4 * dt), ob(8 * dt, data.select_nodes(N, [4]))])
    with pytest.raises(ValueError, match="noise factor"):
        solver.solve_marginals(pde, observations=[ob(4 * dt), ob(8 * dt, noise=None)])
    with pytest.raises(ValueError, match="behind the last step taken"):
        solver.solve_marginals(pde, num_steps=6, observations=[ob(4 * dt), ob(8 * dt)])
    with pytest.raises(TypeError):
        solver.solve_marginals(pde, observations=[(4 * dt, C, [0.0])])
    assert calls == []
    # valid data reaches initialize (and nothing before it touched the device)
    with pytest.raises(AssertionError):
        solver.solve_marginals(pde, num_steps=8, observations=[ob(4 * dt), ob(8 * dt)])
    assert len(calls) == 1
    # the solvers _check_observations_supported refuses are refused here with its TypeError
    sq = pnmol.sqrtform.LinearWhiteNoiseEK1(num_derivatives=2, steprule=pnmol.odetools.step.Constant(dt))
    with pytest.raises(TypeError, match="observations are supported"):
        sq.solve_marginals(pde, observations=[ob(4 * dt)])
    f32 = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(dt))
    f32.dtype = "f32"
    with pytest.raises(TypeError, match="observations are supported"):
        f32.solve_marginals(pde, observations=[ob(4 * dt)])
    adaptive = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=2, steprule=pnmol.odetools.step.Adaptive())
    with pytest.raises(TypeError, match="Constant"):
        adaptive.solve_marginals(pde, observations=[ob(4 * dt)])


def test_plan_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "pnmol_hip.h").read_text()
    lib = _hip.load_library()
    for name in NAMES:
        assert name in _hip.SYMBOLS
        assert re.search(rf"\bint {name}\(", header)
        assert hasattr(lib, name)
    assert lib.pnmol_abi_version() == 3
    for method in ("set_observations", "clear_observations", "observations_pending", "observation_results", "observe_planned"):
        assert method in dir(_hip.Filter)


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_schedule_reference_forms_agree(name):
    """As tests/test_observe_host.py::test_reference_update_forms_agree, for the schedules of the loop tests: the reference's
    square-root update and the covariance form the device computes agree to 1e-12 at every update, the innovation matrices are well
    conditioned, and the data moves the means by more than 100 times the parity floor -- a later change of the inputs cannot quietly
    leave the regime the GPU bounds were measured in."""
    run = schedule_run(name)
    N, nu, bcond, q, K, behind, at_t0 = SCHEDULES[name]
    assert len(run.updates) == len(behind) + int(at_t0)
    steps = int(np.ceil(K))
    assert run.solution.t.shape == (steps + 1,)
    for u, j in zip(run.updates[int(at_t0):], behind):
        assert data.times_agree(u.t, run.solution.t[j], ref.case_dt(nu))
    # (the updates of the loop.  The one at t0 of the runt schedule goes through `pnmol_state_observe` in front of the loop, and the
    # initial state is pinned to y0 at the 1e-10 level: its mean increment is 2e-13, rounding noise of the means themselves, so a
    # figure relative to that increment measures nothing)
    for u in run.updates[int(at_t0):]:
        m2, P2, ll2, maha2, logdet2 = ref.update_cov_form(u.m, u.P, u.H, u.y, u.R)
        inc = u.m_post - u.m
        assert np.abs(m2 - u.m - inc).max() / np.abs(inc).max() <= 1e-12
        assert np.abs(P2 - u.P_post).max() / np.abs(u.P).max() <= 1e-12
        for a, b in ((ll2, u.log_likelihood), (maha2, u.mahalanobis), (logdet2, u.logdet)):
            assert abs(a - b) <= 1e-12 * abs(b)
        S = u.H @ u.P @ u.H.T + u.R @ u.R.T
        assert np.linalg.cond(S) < 1e4
    plain = run.osolver.solve(run.opde)
    moved = np.abs(run.solution.mean[:, 0] - plain.mean[:, 0]).max()
    assert moved > 100 * 1e-5 * np.abs(plain.mean[:, 0]).max()
