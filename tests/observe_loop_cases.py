"""The schedules of the sensor-plan tests (tests/test_observe_loop_host.py, tests/test_gpu_observe_loop.py): the heat problem and
the data recipe of tests/observe_reference.py (model kappa = 0.05, data = oracle mean at kappa = 0.1 plus noise of std 3e-4,
`case_dt(nu)`), with the observations behind chosen steps of a constant-step run.  The reference is `observe_reference.drive`: the
oracle's own steps with `oracle.update_sqrt` at the observation times."""

import functools

import numpy as np

import observe_reference as ref
from helpers import make_pair
from pnmol import data

EVERY12 = tuple(range(1, 13))

# name -> (N, nu, bcond, q, K (steps; 6.5: a runt seventh step), the steps (1-based) with data behind them, data at t0 too)
SCHEDULES = {
    "lead-consecutive-chunks": (32, 2, "dirichlet", 3, 25, (1, 2, 13, 25), False),   # eager lead step, consecutive updates, inside
    "every-q3": (32, 2, "dirichlet", 3, 12, EVERY12, False),                         # ... and at the end of the graph chunks
    "every-q32": (32, 1, "neumann", 32, 12, EVERY12, False),
    "every-n128": (128, 2, "dirichlet", 5, 12, EVERY12, False),
    "sweep-q33": (48, 2, "neumann", 33, 12, (1, 2, 7, 12), False),
    "nu3": (32, 3, "neumann", 3, 12, (1, 2, 7, 12), False),
    "runt": (32, 2, "dirichlet", 3, 6.5, (6, 7), True),
}


@functools.lru_cache(maxsize=None)
def schedule_run(name):
    """The reference of one schedule (computed once per process): an `observe_reference.Run`."""
    N, nu, bcond, q, K, behind, at_t0 = SCHEDULES[name]
    dt = ref.case_dt(nu)
    pde, solver, opde, osolver = make_pair(N, nu, dt, K, bcond, kappa=ref.KAPPA_MODEL)
    _, _, tpde, tsolver = make_pair(N, nu, dt, K, bcond, kappa=ref.KAPPA_TRUTH)
    truth = tsolver.solve(tpde)
    idx = np.array(behind)
    C = ref.sensor_matrix(N, q)
    obs = ref.make_observations(truth.t[idx], truth.mean[idx, 0], C, seed=N + 7 * nu + q + len(behind))
    if at_t0:   # as tests/test_gpu_observe.py::test_simulate_final_state_and_initial_time_observation builds it
        obs = [data.Observation(pde.t0, C, C @ pde.y0 + 1e-4, ref.NOISE_STD)] + obs
    sol, updates = ref.drive(osolver, opde, obs)
    assert len(updates) == len(obs)
    return ref.Run(sol, updates, obs, pde, solver, opde, osolver)
