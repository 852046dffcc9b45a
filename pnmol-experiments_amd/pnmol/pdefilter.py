"""PDE filter driver (reference: src/pnmol/pdefilter.py).

Host-side loop shell: time stepping, accept/reject, info counters, solution stacking.  The
per-step arithmetic is behind `attempt_step` (see pnmol.white).  Differences to the reference:
`PDESolution.cov_sqrtm` is derived lazily from the device-resident covariances (the reference
stacks (T+1) dense D x D factors eagerly, pdefilter.py:87,100), and `marginal_std` gives the
quantity experiments/figure1.py:76-80 reads out without forming any factor.
"""

from abc import ABC, abstractmethod
from collections import namedtuple
from typing import Iterable

import numpy as np

from . import kernels
from .odetools import step


class PDEFilterState(namedtuple("_", "t y error_estimate reference_state diffusion_squared_local")):
    """PDE filter state (pdefilter.py:17-22)."""


class DenseOutput(namedtuple("_DenseOutput", "t mean marginal_std")):
    """Posterior between (or at) grid times: t (Tq,), mean (Tq, n, d), marginal_std (Tq, n, d), uncalibrated."""


class PDESolution:
    """t (T+1,), mean (T+1,n,d), cov_sqrtm (T+1,D,D) [lazy], info, diffusion_squared_calibrated
    (pdefilter.py:25-31).

    Beyond the reference: `solution(t)` and `solution.state_at(t)` evaluate the posterior at ANY t >= t[0] (dense output,
    DESIGN.md section 14).  A filtering solution answers by prediction from the grid state on the left; a smoothed one
    (`solver.smooth`) from the bridges it keeps per step (`bridges`: a list of T `pnmol._hip.Bridge`, or None), and beyond the
    last grid time by prediction as well."""

    def __init__(self, t, mean, ys, info, diffusion_squared_calibrated, bridges=None, smoothed=False):
        self.t, self.mean, self.info = t, mean, info
        self.diffusion_squared_calibrated = diffusion_squared_calibrated
        self._ys = ys
        self._cov_sqrtm = None
        self.bridges = bridges
        self.smoothed = smoothed

    def _dense_setup(self, t, what):
        from .base import rv

        ts = np.atleast_1d(np.asarray(t, dtype=np.float64))
        if ts.ndim != 1 or ts.size < 1:
            raise ValueError(f"{what}: expected a time or a non-empty 1-d array of times, got shape {np.shape(t)}")
        grid = np.asarray(self.t, dtype=np.float64)
        if not np.all(np.isfinite(ts)) or np.any(ts < grid[0]):
            raise ValueError(f"{what}: times must be finite and >= t[0] = {grid[0]} (the posterior is not defined before the "
                             f"initial time)")
        if not self._ys or not all(isinstance(y, rv.DeviceMultivariateNormal) for y in self._ys):
            raise TypeError(f"{what} needs the device-resident states of this package's solve() / smooth()")
        k = np.searchsorted(grid, ts, side="right") - 1
        inside = k < len(grid) - 1
        if self.smoothed and self.bridges is None and np.any(inside & (grid[k] != ts)):
            raise RuntimeError(f'{what}: this smoothed solution keeps no bridges (it was made with dense=None); call '
                               f'solver.smooth(solution, dense="marginal") (or dense="full" for state_at)')
        return ts, grid, k

    def __call__(self, t):
        """Posterior mean and marginal std of all derivatives at the time(s) t >= self.t[0]: a `DenseOutput` with t (Tq,),
        mean (Tq, n, d), marginal_std (Tq, n, d), uncalibrated like `marginal_std`.  Queries may come in any order; they are
        grouped per grid interval and answered by one device call per touched interval.  A grid time returns the stored
        values."""
        ts, grid, k = self._dense_setup(t, "PDESolution.__call__")
        flt = self._ys[0].device_state.filter
        mean, std = np.empty((ts.size, flt.n, flt.d)), np.empty((ts.size, flt.n, flt.d))
        on_grid = grid[k] == ts
        for i in np.unique(k):
            sel = np.flatnonzero(k == i)
            stored = sel[on_grid[sel]]
            if stored.size:
                mean[stored] = self.mean[i]
                std[stored] = np.sqrt(np.maximum(self._ys[i].marginal_var, 0.0))
            sel = sel[~on_grid[sel]]
            if not sel.size:
                continue
            if self.smoothed and i < len(grid) - 1:
                mean[sel], std[sel] = self.bridges[i].eval(ts[sel])
            else:
                mean[sel], std[sel] = flt.predict_marginals(self._ys[i].device_state, ts[sel] - grid[i])
        return DenseOutput(t=ts, mean=mean, marginal_std=std)

    def state_at(self, t):
        """The full posterior at one time t >= self.t[0] as a `DeviceMultivariateNormal` (mean, `cov`, `cov_sqrtm`,
        `marginal_var`).  Inside a smoothed solution this needs `smooth(solution, dense="full")`; a filtering solution, and any
        t beyond the last grid time, is answered by prediction.  A grid time returns the stored state."""
        from .base import rv

        if np.ndim(t) != 0:
            raise ValueError("PDESolution.state_at: expected a single time")
        ts, grid, k = self._dense_setup(t, "PDESolution.state_at")
        i, tq = int(k[0]), float(ts[0])
        if grid[i] == tq:
            return self._ys[i]
        flt = self._ys[0].device_state.filter
        if self.smoothed and i < len(grid) - 1:
            if not self.bridges[i].full:
                raise RuntimeError('PDESolution.state_at: the full covariance between grid times needs the cross-covariances '
                                   'of the smoother; call solver.smooth(solution, dense="full")')
            dev = self.bridges[i].state(self._ys[i].device_state, self._ys[i + 1].device_state, tq)
        else:
            dev = flt.predict(self._ys[i].device_state, tq - grid[i])
        return rv.DeviceMultivariateNormal(dev.mean(), dev)

    @property
    def cov_sqrtm(self):
        if self._cov_sqrtm is None:
            self._cov_sqrtm = np.stack([y.cov_sqrtm for y in self._ys])
        return self._cov_sqrtm

    @property
    def marginal_std(self):
        """sqrt(diag(cov)) as (T+1, n, d), uncalibrated."""
        out = []
        for y in self._ys:
            var = y.marginal_var if hasattr(y, "marginal_var") else \
                np.einsum("ij,ij->i", y.cov_sqrtm, y.cov_sqrtm).reshape(y.mean.shape, order="F")
            out.append(np.sqrt(np.maximum(var, 0.0)))
        return np.stack(out)


class PDEFilter(ABC):
    """Interface of the filtering-based PDE solvers (pdefilter.py:34-235)."""

    def __init__(self, *, steprule=None, num_derivatives=2, spatial_kernel=None, diffuse_prior_scale=1e0):
        self.steprule = steprule or step.Adaptive()
        self.num_derivatives = num_derivatives
        self.iwp = None
        self.spatial_kernel = spatial_kernel or kernels.Matern52() + kernels.WhiteNoise()
        self.E0 = None
        self.E1 = None
        self.diffuse_prior_scale = diffuse_prior_scale

    def __repr__(self):
        return (f"{self.__class__.__name__}(num_derivatives={self.num_derivatives}, steprule={self.steprule}, "
                f"spatial_kernel={self.spatial_kernel})")

    @staticmethod
    def _collect(diffusion_squared_list, state):
        if isinstance(state.diffusion_squared_local, list):
            diffusion_squared_list.extend(state.diffusion_squared_local)
        else:
            diffusion_squared_list.append(state.diffusion_squared_local)

    def solve(self, *args, **kwargs):
        times, means, ys, info, d2 = [], [], [], dict(), []
        for state, info in self.solution_generator(*args, **kwargs):
            times.append(state.t)
            means.append(state.y.mean)
            ys.append(state.y)
            self._collect(d2, state)
        return PDESolution(t=np.stack(times), mean=np.stack(means), ys=ys, info=info,
                           diffusion_squared_calibrated=np.mean(np.array(d2)))

    def simulate_final_state(self, *args, **kwargs):
        state, info, d2 = None, None, []
        for state, info in self.solution_generator(*args, **kwargs):
            self._collect(d2, state)
        cov_sqrtm_new = state.y.cov_sqrtm * np.sqrt(np.mean(np.array(d2)))
        return state._replace(y=state.y._replace(cov_sqrtm=cov_sqrtm_new)), info

    def _check_observations_supported(self):
        raise TypeError(f"{type(self).__name__} does not take observations")

    def _observe(self, state, observation):
        raise NotImplementedError

    def solution_generator(self, pde, /, *, stop_at=None, progressbar=False, observations=None):
        """Generate solver steps, starting with the initial state (pdefilter.py:118-165).

        observations (beyond the reference): a sequence of `pnmol.data.Observation`, sorted by t.  The accepted step that lands
        on an observation's time (`pnmol.data.times_agree`) is followed by the measurement update on the device, and the updated
        state is what is yielded; an observation at pde.t0 updates the initial state.  `Constant` steps: every observation time
        must be a grid time (ValueError otherwise, before any device work); `Adaptive`: the times are merged into `stop_at`.
        `info` then carries `data_log_likelihood` (the sum) and `data_log_likelihoods` (one entry per observation): log p(y_k |
        y_1..k-1, PDE) under the uncalibrated (sigma^2 = 1) prior, against which the observation noise is weighed."""
        pending = None
        if observations is not None:
            from . import data

            self._check_observations_supported()
            pending = data.prepare(observations, pde, self.steprule, pde.y0.shape[0])
            if not isinstance(self.steprule, step.Constant):
                stops = data.merged_stops(stop_at, pending, pde.t0)
                stop_at = stops if stops else None
        time_stopper = _TimeStopper(stop_at) if stop_at is not None else None
        state = self.initialize(pde)
        info = dict(num_f_evaluations=0, num_df_evaluations=0, num_df_diagonal_evaluations=0, num_steps=0,
                    num_attempted_steps=0)
        if pending is not None:
            info["data_log_likelihood"], info["data_log_likelihoods"] = 0.0, []
            state = self._apply_due_observations(state, pending, info, self.steprule.first_dt(pde))
        yield state, info
        dt = self.steprule.first_dt(pde)
        pbar = None
        if progressbar:
            from tqdm import tqdm
            pbar = tqdm(total=100)
            threshold = increment = pde.tmax / 100
        while state.t < pde.tmax:
            if pbar is not None:
                while state.t + dt >= threshold:
                    pbar.update()
                    threshold += increment
                pbar.set_description(f"t={state.t:.4f}, dt={dt:.2E}")
            if time_stopper is not None:
                dt = time_stopper.adjust_dt_to_time_stops(state.t, dt)
            t_before = state.t
            state, dt, step_info = self.perform_full_step(state, dt, pde)
            info["num_steps"] += 1
            for key in ("num_f_evaluations", "num_df_evaluations", "num_df_diagonal_evaluations",
                        "num_attempted_steps"):
                info[key] += step_info[key]
            if pending:
                state = self._apply_due_observations(state, pending, info, state.t - t_before)
            yield state, info
        if pbar is not None:
            pbar.update()
            pbar.close()

    def _apply_due_observations(self, state, pending, info, dt):
        """Condition `state` on the head of `pending` if its time is state.t (dt: the step just taken); a time the loop has
        stepped over is an error (it cannot happen with the checks of `pnmol.data.prepare` and the merged stops)."""
        from . import data

        if pending and data.times_agree(pending[0].t, state.t, dt):
            state, log_likelihood = self._observe(state, pending.pop(0))
            info["data_log_likelihoods"].append(log_likelihood)
            info["data_log_likelihood"] += log_likelihood
        if pending and pending[0].t < state.t:
            raise RuntimeError(f"the step to t={state.t} passed the observation at t={pending[0].t}")
        return state

    def perform_full_step(self, state, initial_dt, pde):
        """One accepted step incl. the accept/reject loop of the step rule (pdefilter.py:177-227)."""
        dt, accepted, proposed = initial_dt, False, None
        step_info = dict(num_f_evaluations=0, num_df_evaluations=0, num_df_diagonal_evaluations=0,
                         num_attempted_steps=0)
        while not accepted:
            proposed, attempt_info = self.attempt_step(state, dt, pde)
            step_info["num_attempted_steps"] += 1
            for key in ("num_f_evaluations", "num_df_evaluations", "num_df_diagonal_evaluations"):
                step_info[key] += attempt_info.get(key, 0)
            # NB the reference multiplies the (already dt-scaled) estimate by dt again (pdefilter.py:210)
            internal_norm = self.steprule.scale_error_estimate(
                unscaled_error_estimate=dt * proposed.error_estimate if proposed.error_estimate is not None else None,
                reference_state=proposed.reference_state)
            accepted = self.steprule.is_accepted(internal_norm)
            suggested_dt = self.steprule.suggest(dt, internal_norm, local_convergence_rate=self.num_derivatives + 1)
            dt = min(suggested_dt, pde.tmax - (proposed.t if accepted else state.t))
            assert dt >= 0, f"Invalid step size: dt={dt}"
        return proposed, dt, step_info

    @abstractmethod
    def initialize(self, pde):
        raise NotImplementedError

    @abstractmethod
    def attempt_step(self, state, dt, pde):
        raise NotImplementedError


class _TimeStopper:
    """Make the solver stop at specified time-points (pdefilter.py:238-256)."""

    def __init__(self, locations: Iterable):
        self._locations = iter(locations)
        self._next_location = next(self._locations)

    def adjust_dt_to_time_stops(self, t, dt):
        if t >= self._next_location:
            try:
                self._next_location = next(self._locations)
            except StopIteration:
                self._next_location = np.inf
        if t + dt > self._next_location:
            dt = self._next_location - t
        return dt
