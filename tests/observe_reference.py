"""Dense fp64 NumPy reference of the measurement update (`pnmol_state_observe`, `solve(pde, observations=...)`): the oracle's
own steps (`attempt_step`) with `oracle.update_sqrt(C E0, cov_sqrtm, R_sqrtm)` applied at the observation times, returned as an
`oracle.Solution` so that smooth_reference.rts_on_oracle and sample_reference.maps_on_oracle work on it unchanged.

The cases of tests/test_observe_host.py and tests/test_gpu_observe.py: the heat problem of helpers.make_pair with model
kappa = 0.05, data y = C u_truth + noise with u_truth the oracle mean at kappa = 0.1, noise std 3e-4, an observation every 4th
step of 12; rows of C average two neighbouring nodes, or C = I.  dt makes the prior std comparable to the noise: 2^-4 at
nu = 2, 3 and 2^-7 at nu = 1."""

import functools
from collections import namedtuple

import numpy as np
import scipy.linalg

import pnmol
import pnmol_oracle as oracle
from helpers import make_pair

NOISE_STD = 3e-4
KAPPA_MODEL, KAPPA_TRUTH = 0.05, 0.1
STEPS, EVERY = 12, 4

# (N, nu, bcond, q) of the stage-parity test; the first five also run end to end
CASES = [(32, 2, "dirichlet", 1), (32, 2, "dirichlet", 3), (32, 1, "neumann", 32), (48, 2, "neumann", 33),
         (128, 2, "dirichlet", 5), (32, 3, "neumann", 3), (576, 1, "dirichlet", 576)]

# one update of the reference run: time, the flat state before it (H acts on it), the update's inputs, the two forms' results
Update = namedtuple("Update", "t m P H y R m_post P_post log_likelihood mahalanobis logdet")
Run = namedtuple("Run", "solution updates observations pde solver opde osolver")


def case_dt(nu):
    return 2.0 ** -7 if nu == 1 else 2.0 ** -4


def sensor_matrix(d, q):
    """q rows that average two neighbouring nodes, spread over the interior; q = d: the identity."""
    if q == d:
        return np.eye(d)
    left = np.round(np.linspace(1, d - 3, q)).astype(int)
    assert len(set(left)) == q
    C = np.zeros((q, d))
    C[np.arange(q), left] = C[np.arange(q), left + 1] = 0.5
    return C


def flat_mean(mean, latent):
    """An (n, d_state) array as a vector in the order of the oracle's covariance factor (latent: [u; eps], each point-major)."""
    mean = np.asarray(mean)
    if not latent:
        return mean.reshape(-1, order="F")
    d = mean.shape[1] // 2
    return np.hstack((mean[:, :d].reshape(-1, order="F"), mean[:, d:].reshape(-1, order="F")))


def unflat_state(m, n, latent):
    if not latent:
        return m.reshape((n, -1), order="F")
    half = m.shape[0] // 2
    return np.hstack((m[:half].reshape((n, -1), order="F"), m[half:].reshape((n, -1), order="F")))


def observation_matrix(osolver, C, latent):
    """H = C E0 on the flat state (latent: [C E0_u, 0])."""
    H = C @ osolver.E0
    return np.hstack((H, np.zeros_like(H))) if latent else H


def update_sqrt_form(m, Cl, H, y, R):
    """The reference's square-root update: (m_post, C_post, log_likelihood, mahalanobis, logdet)."""
    C_post, K, Sl = oracle.update_sqrt(H, Cl, R)
    v = y - H @ m
    w = scipy.linalg.solve_triangular(Sl, v, lower=True)
    maha, logdet = float(w @ w), float(2.0 * np.sum(np.log(np.abs(np.diag(Sl)))))
    return m + K @ v, C_post, -0.5 * (maha + logdet + len(y) * np.log(2.0 * np.pi)), maha, logdet


def update_cov_form(m, P, H, y, R):
    """The same update in covariance form (what the device computes): (m_post, P_post, log_likelihood, mahalanobis, logdet)."""
    S = H @ P @ H.T + (0.0 if R is None else R @ R.T)
    Ls = np.linalg.cholesky(0.5 * (S + S.T))
    W = scipy.linalg.solve_triangular(Ls, H @ P, lower=True).T
    w = scipy.linalg.solve_triangular(Ls, y - H @ m, lower=True)
    maha, logdet = float(w @ w), float(2.0 * np.sum(np.log(np.diag(Ls))))
    return m + W @ w, P - W @ W.T, -0.5 * (maha + logdet + len(y) * np.log(2.0 * np.pi)), maha, logdet


def drive(osolver, opde, observations, latent=False, stop_at=None, max_updates=None):
    """The oracle's solve loop (`solution_generator`) with the square-root update behind every accepted step that lands on an
    observation time; stops after `max_updates` updates if given.  Returns (oracle.Solution, [Update])."""
    pending = list(observations)
    n = osolver.num_derivatives + 1
    updates = []

    def condition(state, dt):
        if not pending or not pnmol.data.times_agree(pending[0].t, state.t, dt):
            return state
        ob = pending.pop(0)
        H = observation_matrix(osolver, ob.C, latent)
        m, Cl = flat_mean(state.y.mean, latent), np.asarray(state.y.cov_sqrtm)
        m_post, C_post, ll, maha, logdet = update_sqrt_form(m, Cl, H, ob.y, ob.R_sqrtm)
        updates.append(Update(state.t, m, Cl @ Cl.T, H, ob.y, ob.R_sqrtm, m_post, C_post @ C_post.T, ll, maha, logdet))
        mean = unflat_state(m_post, n, latent)
        ref = None if state.reference_state is None else np.abs(mean[0])
        return state._replace(y=oracle.MVN(mean, C_post), reference_state=ref)

    stopper = oracle._TimeStopper(stop_at) if stop_at is not None else None
    state = osolver.initialize(opde)
    dt = osolver.steprule.first_dt(opde)
    state = condition(state, dt)
    ts, means, covs, d2 = [state.t], [state.y.mean], [state.y.cov_sqrtm], []
    info = dict(num_f_evaluations=0, num_df_evaluations=0, num_df_diagonal_evaluations=0, num_steps=0, num_attempted_steps=0)
    while state.t < opde.tmax and (max_updates is None or len(updates) < max_updates):
        if stopper is not None:
            dt = stopper.adjust_dt_to_time_stops(state.t, dt)
        t_before = state.t
        state, dt, sinfo = osolver.perform_full_step(state, dt, opde)
        info["num_steps"] += 1
        for key in ("num_f_evaluations", "num_df_evaluations", "num_df_diagonal_evaluations", "num_attempted_steps"):
            info[key] += sinfo[key]
        d2.append(state.diffusion_squared_local)
        state = condition(state, state.t - t_before)
        ts.append(state.t), means.append(state.y.mean), covs.append(state.y.cov_sqrtm)
    info["data_log_likelihoods"] = [u.log_likelihood for u in updates]
    info["data_log_likelihood"] = float(sum(info["data_log_likelihoods"]))
    return oracle.Solution(np.stack(ts), np.stack(means), np.stack(covs), info, float(np.mean(np.array(d2)))), updates


def make_observations(ts, u_truth, C, seed):
    """y = C u_truth(t) + N(0, NOISE_STD^2) at the times ts (u_truth: one row per time)."""
    rng = np.random.default_rng(seed)
    return [pnmol.data.Observation(t, C, C @ u + NOISE_STD * rng.standard_normal(C.shape[0]), NOISE_STD)
            for t, u in zip(ts, u_truth)]


@functools.lru_cache(maxsize=None)
def reference_run(N, nu, bcond, q, max_updates=None):
    """The constant-step reference of one case (computed once per process): a `Run`."""
    dt = case_dt(nu)
    steps = STEPS if max_updates is None else EVERY * max_updates
    pde, solver, opde, osolver = make_pair(N, nu, dt, steps, bcond, kappa=KAPPA_MODEL)
    _, _, tpde, tsolver = make_pair(N, nu, dt, steps, bcond, kappa=KAPPA_TRUTH)
    truth = tsolver.solve(tpde)
    idx = np.arange(EVERY, steps + 1, EVERY)
    obs = make_observations(truth.t[idx], truth.mean[idx, 0], sensor_matrix(N, q), seed=N + 7 * nu + q)
    sol, updates = drive(osolver, opde, obs, max_updates=max_updates)
    return Run(sol, updates, obs, pde, solver, opde, osolver)


def latent_pair(N, nu, dt, K, bcond, kappa):
    """The latent-force twin of helpers.make_pair (the recipe of tests/test_latent.py)."""
    kw = dict(tmax=K * dt, dx=1.0 / (N - 1), diffusion_rate=kappa, bcond=bcond, stencil_size_interior=3,
              stencil_size_boundary=3, nugget_gram_matrix_fd=0.0)
    pde = pnmol.pde.examples.heat_1d_discretized(kernel=pnmol.kernels.SquareExponential(), **kw)
    opde = oracle.heat_1d_discretized(kernel=oracle.SquareExponential(), **kw)
    solver = pnmol.latent.LinearLatentForceEK1(num_derivatives=nu, steprule=pnmol.odetools.step.Constant(dt),
                                               spatial_kernel=pnmol.kernels.SquareExponential() + pnmol.kernels.WhiteNoise())
    osolver = oracle.LatentForceEK1(num_derivatives=nu, steprule=oracle.Constant(dt), canonical_factor_signs=True,
                                    spatial_kernel=oracle.SquareExponential() + oracle.WhiteNoise())
    return pde, solver, opde, osolver


@functools.lru_cache(maxsize=None)
def latent_reference_run(N, nu, bcond, q):
    dt = case_dt(nu)
    pde, solver, opde, osolver = latent_pair(N, nu, dt, STEPS, bcond, KAPPA_MODEL)
    _, _, tpde, tsolver = latent_pair(N, nu, dt, STEPS, bcond, KAPPA_TRUTH)
    truth = tsolver.solve(tpde)
    idx = np.arange(EVERY, STEPS + 1, EVERY)
    obs = make_observations(truth.t[idx], truth.mean[idx, 0, :N], sensor_matrix(N, q), seed=1000 + N + q)
    sol, updates = drive(osolver, opde, obs, latent=True)
    return Run(sol, updates, obs, pde, solver, opde, osolver)
