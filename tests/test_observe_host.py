"""CPU tests of the measurement update's host side: the reference helper (tests/observe_reference.py) against itself in
covariance form, the validation of `pnmol.data`, and the C ABI's new names.  No GPU."""

import pathlib
import re

import numpy as np
import pytest

import pnmol
from helpers import make_pair
from pnmol import _hip, data
import observe_reference as ref

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _rel(a, b, scale):
    return np.abs(a - b).max() / scale


@pytest.mark.parametrize("N,nu,bcond,q", ref.CASES[:6])
def test_reference_update_forms_agree(N, nu, bcond, q):
    """The square-root update of the reference run and the covariance-form update the device computes agree to 1e-12: the
    mean increment relative to its largest entry, the covariance relative to its largest entry, the three scalars relatively.
    The inputs are well conditioned by construction (noise std comparable to the prior std), which is asserted too."""
    run = ref.reference_run(N, nu, bcond, q)
    assert len(run.updates) == ref.STEPS // ref.EVERY and run.solution.t.shape == (ref.STEPS + 1,)
    for u in run.updates:
        m2, P2, ll2, maha2, logdet2 = ref.update_cov_form(u.m, u.P, u.H, u.y, u.R)
        inc = u.m_post - u.m
        assert _rel(m2 - u.m, inc, np.abs(inc).max()) <= 1e-12
        assert _rel(P2, u.P_post, np.abs(u.P).max()) <= 1e-12
        for a, b in ((ll2, u.log_likelihood), (maha2, u.mahalanobis), (logdet2, u.logdet)):
            assert abs(a - b) <= 1e-12 * abs(b)
        S = u.H @ u.P @ u.H.T + u.R @ u.R.T
        assert np.linalg.cond(S) < 1e4
    # the data matters: the conditioned means leave the unobserved ones by far more than the parity floor of the GPU tests
    plain = run.osolver.solve(run.opde)
    moved = np.abs(run.solution.mean[:, 0] - plain.mean[:, 0]).max()
    assert moved > 100 * 1e-5 * np.abs(plain.mean[:, 0]).max()


def test_reference_latent_update_forms_agree():
    run = ref.latent_reference_run(32, 1, "dirichlet", 3)
    assert len(run.updates) == 3 and run.updates[0].H.shape == (3, 2 * 2 * 32)
    assert not np.any(run.updates[0].H[:, 2 * 32:])                      # H = [C E0_u, 0]
    for u in run.updates:
        m2, P2, ll2, _, _ = ref.update_cov_form(u.m, u.P, u.H, u.y, u.R)
        inc = u.m_post - u.m
        assert _rel(m2 - u.m, inc, np.abs(inc).max()) <= 1e-12
        assert _rel(P2, u.P_post, np.abs(u.P).max()) <= 1e-12
        assert abs(ll2 - u.log_likelihood) <= 1e-12 * abs(u.log_likelihood)


def test_observation_validation():
    C = data.select_nodes(8, [1, 5])
    assert C.shape == (2, 8) and C[0, 1] == C[1, 5] == 1.0 and C.sum() == 2.0
    ob = data.Observation(0.5, C, [1.0, 2.0], 0.1)
    np.testing.assert_array_equal(ob.R_sqrtm, 0.1 * np.eye(2))
    np.testing.assert_array_equal(data.Observation(0.5, C, [1.0, 2.0], [0.1, 0.2]).R_sqrtm, np.diag([0.1, 0.2]))
    L = np.array([[0.1, 0.0], [0.05, 0.2]])
    np.testing.assert_array_equal(data.Observation(0.5, C, [1.0, 2.0], L).R_sqrtm, L)
    assert data.Observation(0.5, C, [1.0, 2.0]).R_sqrtm is None and data.Observation(0.5, C, [1.0, 2.0], 0.0).R_sqrtm is None
    for bad in (dict(C=np.zeros(8)), dict(y=[1.0]), dict(y=[[1.0, 2.0]]), dict(noise_sqrtm=-1.0), dict(noise_sqrtm=[0.1]),
                dict(noise_sqrtm=np.ones((2, 2))), dict(noise_sqrtm=np.eye(3)), dict(t=float("nan")), dict(y=[1.0, np.inf]),
                dict(C=np.zeros((0, 8)), y=[])):
        kw = dict(t=0.5, C=C, y=[1.0, 2.0], noise_sqrtm=0.1)
        kw.update(bad)
        with pytest.raises(ValueError):
            data.Observation(**kw)
    for bad in ([], [[1, 2]], [8], [-1], [0.5]):
        with pytest.raises(ValueError):
            data.select_nodes(8, bad)


def test_solver_rejects_bad_observations_before_any_device_work(monkeypatch):
    """Unsorted times, times outside [t0, tmax], wrong widths, off-grid times under `Constant` and unsupported solvers raise
    from the first `next()` of the generator, before `initialize` (which is what binds the device filter)."""
    dt, K, N = 2.0 ** -4, 12, 16
    pde, solver, _, _ = make_pair(N, 2, dt, K)
    calls = []
    monkeypatch.setattr(type(solver), "initialize", lambda self, p: calls.append(p) or (_ for _ in ()).throw(AssertionError))
    C = data.select_nodes(N, [3])

    def ob(t, C=C):
        return data.Observation(t, C, np.zeros(C.shape[0]), 1e-3)

    for obs, exc in (([ob(8 * dt), ob(4 * dt)], ValueError),          # unsorted
                     ([ob(4 * dt), ob(4 * dt)], ValueError),          # twice the same time
                     ([ob(4.5 * dt)], ValueError),                    # off the constant grid
                     ([ob(4 * dt * (1 + 1e-9))], ValueError),         # ... by more than 16 ulp
                     ([ob(-dt)], ValueError), ([ob((K + 1) * dt)], ValueError),
                     ([ob(4 * dt, data.select_nodes(N + 1, [3]))], ValueError),
                     ([(4 * dt, C, [0.0])], TypeError)):
        with pytest.raises(exc):
            solver.solve(pde, observations=obs)
        with pytest.raises(exc):
            solver.simulate_final_state(pde, observations=obs)
    # a grid time up to rounding is accepted by the check (and the solve then reaches initialize)
    with pytest.raises(AssertionError):
        solver.solve(pde, observations=[ob(4 * dt * (1 + 2e-16)), ob(K * dt)])
    assert len(calls) == 1
    # the adaptive rule takes any time inside the span
    adaptive = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=2, steprule=pnmol.odetools.step.Adaptive())
    monkeypatch.setattr(type(adaptive), "initialize", lambda self, p: (_ for _ in ()).throw(AssertionError))
    with pytest.raises(AssertionError):
        adaptive.solve(pde, observations=[ob(4.5 * dt)])
    # unsupported: QR-form solvers and fp32
    sq = pnmol.sqrtform.LinearWhiteNoiseEK1(num_derivatives=2, steprule=pnmol.odetools.step.Constant(dt))
    with pytest.raises(TypeError, match="observations"):
        sq.solve(pde, observations=[ob(4 * dt)])
    f32 = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(dt))
    f32.dtype = "f32"
    with pytest.raises(TypeError, match="observations"):
        f32.solve(pde, observations=[ob(4 * dt)])


def test_merged_stops_and_grid():
    obs = [data.Observation(t, np.eye(1), [0.0]) for t in (0.0, 0.3, 0.7)]
    assert data.merged_stops(None, obs, 0.0) == [0.3, 0.7]
    assert data.merged_stops([0.5, 0.3 * (1 + 2e-16), 0.7], obs, 0.0) == [0.3, 0.5, 0.7]
    grid = data.constant_step_grid(0.0, 1.0, 0.3)
    np.testing.assert_allclose(grid, [0.0, 0.3, 0.6, 0.9, 1.0], rtol=0, atol=1e-15)
    assert data.times_agree(0.1 + 0.2, 0.3, 0.1) and not data.times_agree(0.3, 0.3 + 1e-13, 0.1)


def test_new_symbols_are_declared_and_exported():
    assert "pnmol_state_observe" in _hip.SYMBOLS
    header = (ROOT / "include" / "pnmol_hip.h").read_text()
    assert re.search(r"\bint pnmol_state_observe\(", header) and "pnmol_observe_out" in header
    assert hasattr(_hip.load_library(), "pnmol_state_observe")
    fields = [f for f, _ in _hip.ObserveOut._fields_]
    assert fields == ["log_likelihood", "mahalanobis", "logdet", "info"]
    assert "observe" in dir(_hip.Filter)
