"""Sensor data for the PDE filters: linear observations of the solution at given times.

An `Observation` says  y = C u(t) + e,  e ~ N(0, R R^T):  q linear functionals of the solution at the mesh points (derivative 0
of the state).  `solve(pde, observations=[...])` conditions the state on each of them right behind the accepted step that lands
on its time, on the device (`pnmol_state_observe`); the smoother, the joint draws and dense output then
give the posterior under physics and data, and `info["data_log_likelihood"]` is the evidence of the data under the model.

No reference counterpart: the reference solves the PDE without data.
"""

import itertools

import numpy as np

_EPS = 2.220446049250313e-16


def times_agree(a, b, dt):
    """Two times are the same grid point (dt: the step they are measured against): the rule of the C library."""
    return abs(a - b) <= 16.0 * _EPS * max(abs(a), abs(b), abs(dt))


def select_nodes(d, indices):
    """C (len(indices), d) that reads the solution at the mesh nodes `indices`."""
    idx = np.asarray(indices)
    if idx.ndim != 1 or idx.size < 1 or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError(f"select_nodes: indices must be a non-empty 1-d integer sequence, got {indices!r}")
    if np.any(idx < 0) or np.any(idx >= d):
        raise ValueError(f"select_nodes: indices must lie in [0, {d}), got {idx.min()}..{idx.max()}")
    C = np.zeros((idx.size, int(d)))
    C[np.arange(idx.size), idx] = 1.0
    return C


class Observation:
    """y = C u(t) + e at time t.  C (q, d), y (q,); noise_sqrtm: None or 0 (noise-free), a scalar std, a vector of q stds or a
    lower-triangular (q, q) matrix R with cov(e) = R R^T.  `R_sqrtm` is the (q, q) factor handed to the device, or None."""

    def __init__(self, t, C, y, noise_sqrtm=None):
        self.t = float(t)
        if not np.isfinite(self.t):
            raise ValueError(f"Observation: t must be finite, got {t!r}")
        self.C = np.ascontiguousarray(np.asarray(C, dtype=np.float64))
        if self.C.ndim != 2 or self.C.shape[0] < 1:
            raise ValueError(f"Observation: C must be (q, d) with q >= 1, got shape {self.C.shape}")
        q = self.C.shape[0]
        self.y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
        if self.y.shape != (q,):
            raise ValueError(f"Observation: y must have shape ({q},) like the rows of C, got {self.y.shape}")
        if not (np.all(np.isfinite(self.C)) and np.all(np.isfinite(self.y))):
            raise ValueError("Observation: C and y must be finite")
        self.R_sqrtm = self._noise_factor(noise_sqrtm, q)

    @staticmethod
    def _noise_factor(noise, q):
        if noise is None:
            return None
        R = np.asarray(noise, dtype=np.float64)
        if not np.all(np.isfinite(R)):
            raise ValueError("Observation: noise_sqrtm must be finite")
        if R.ndim == 0:
            if R < 0:
                raise ValueError(f"Observation: a scalar noise std must be >= 0, got {float(R)}")
            R = float(R) * np.eye(q)
        elif R.ndim == 1:
            if R.shape != (q,) or np.any(R < 0):
                raise ValueError(f"Observation: a vector noise_sqrtm must hold {q} stds >= 0, got shape {R.shape}")
            R = np.diag(R)
        elif R.shape != (q, q):
            raise ValueError(f"Observation: a matrix noise_sqrtm must be ({q}, {q}), got {R.shape}")
        elif np.any(np.triu(R, 1) != 0.0):
            raise ValueError("Observation: a matrix noise_sqrtm must be lower triangular")
        return None if not np.any(R) else np.ascontiguousarray(R)

    @property
    def q(self):
        return self.C.shape[0]

    def __repr__(self):
        return f"Observation(t={self.t}, q={self.q}, noise={'none' if self.R_sqrtm is None else 'given'})"


def constant_schedule(t0, tmax, dt0, num_steps=None):
    """(times, steps) of the constant-step loop, as lists: the t-accumulation of the reference's loop (pdefilter.py:140-160,
    :220-223), a runt final step included when sum(dt) lands short of tmax; at most `num_steps` steps."""
    ts, dts, t, dt = [t0], [], t0, dt0
    while t < tmax and (num_steps is None or len(dts) < num_steps):
        dts.append(dt)
        t = t + dt
        ts.append(t)
        dt = min(dt0, tmax - t)
    return ts, dts


def constant_step_grid(t0, tmax, dt0):
    """The times of the constant-step loop (`constant_schedule`) as an array."""
    return np.array(constant_schedule(t0, tmax, dt0)[0])


def equal_step_runs(dts):
    """(count, dt) per run of equal steps in `dts`: what the device loops take in one call each."""
    for dt, run in itertools.groupby(dts):
        yield sum(1 for _ in run), dt


def prepare(observations, pde, steprule, d):
    """Validate `observations` for a solve of `pde` (host only, before any device work); returns them as a list.

    Every entry an `Observation` whose C has d columns, times strictly increasing inside [pde.t0, pde.tmax]; under the
    `Constant` step rule every time must be a grid time (`times_agree`)."""
    from .odetools import step

    obs = list(observations)
    for o in obs:
        if not isinstance(o, Observation):
            raise TypeError(f"observations must be pnmol.data.Observation objects, got {type(o).__name__}")
        if o.C.shape[1] != d:
            raise ValueError(f"observation at t={o.t}: C must have {d} columns (mesh points), got {o.C.shape[1]}")
        if o.q > d:
            raise ValueError(f"observation at t={o.t}: at most {d} rows, got {o.q}")
    ts = np.array([o.t for o in obs])
    if np.any(np.diff(ts) <= 0.0):
        raise ValueError("observations must be sorted by strictly increasing t")
    scale = max(abs(pde.t0), abs(pde.tmax))
    if ts.size and (ts[0] < pde.t0 - 16.0 * _EPS * scale or ts[-1] > pde.tmax + 16.0 * _EPS * scale):
        raise ValueError(f"observation times must lie in [t0, tmax] = [{pde.t0}, {pde.tmax}]")
    if isinstance(steprule, step.Constant):
        grid = constant_step_grid(pde.t0, pde.tmax, steprule.dt)
        for o in obs:
            k = int(np.argmin(np.abs(grid - o.t)))
            if not times_agree(grid[k], o.t, steprule.dt):
                raise ValueError(f"observation time {o.t} is not a grid time of the constant step {steprule.dt} "
                                 f"(nearest: {grid[k]}); use the Adaptive step rule or move the observation")
    return obs


def shared_sensors(observations):
    """(times, C, R_sqrtm, ys) of observations that share one sensor array: what the device-resident loop takes
    (`solve_marginals(pde, observations=...)`, `pnmol_filter_set_observations`).  ys is (nobs, q); R_sqrtm is None when noise-free."""
    obs = list(observations)
    if not obs:
        raise ValueError("shared_sensors: no observations")
    first = obs[0]
    for i, o in enumerate(obs[1:], start=1):
        same_noise = (o.R_sqrtm is None) == (first.R_sqrtm is None) and (o.R_sqrtm is None or (
            o.R_sqrtm.shape == first.R_sqrtm.shape and np.array_equal(o.R_sqrtm, first.R_sqrtm)))
        if o.C.shape != first.C.shape or not np.array_equal(o.C, first.C) or not same_noise:
            what = "C" if o.C.shape != first.C.shape or not np.array_equal(o.C, first.C) else "noise factor"
            raise ValueError(f"observation {i} (t={o.t}) has another {what} than observation 0: the device-resident loop takes one "
                             f"sensor array for all times; use solve(pde, observations=...) for per-time sensors")
    return (np.array([o.t for o in obs]), first.C, first.R_sqrtm, np.stack([o.y for o in obs]))


def merged_stops(stop_at, obs, t0):
    """`stop_at` with the observation times behind t0 merged in, sorted; a stop that agrees with an observation time
    (`times_agree`) gives way to it, so that no step of a rounding error's length is taken between the two."""
    tagged = [(float(s), False) for s in (() if stop_at is None else stop_at)] + [(o.t, True) for o in obs if o.t > t0]
    tagged.sort(key=lambda p: (p[0], not p[1]))
    out = []
    for t, is_obs in tagged:
        if out and times_agree(out[-1][0], t, 0.0):
            if is_obs and not out[-1][1]:
                out[-1] = (t, True)
            continue
        out.append((t, is_obs))
    return [t for t, _ in out]
