"""Linear functionals of a whole trajectory: the result of `solver.functionals(solution, weights)` and builders of weights.

A functional is q = sum_k sum_j w[k, j] u(x_j, t_k) over the T+1 grid times of a solution and the d mesh points.  The builders
return one functional as an array (T+1, d); stack Q of them with `np.stack` into the (Q, T+1, d) that `functionals` takes.
Weights on the time derivatives of u use the long form (Q, T+1, n, d)."""

import dataclasses

import numpy as np


@dataclasses.dataclass(frozen=True)
class FunctionalPosterior:
    """Posterior N(mean, cov) of Q functionals: `mean` (Q,), `cov` (Q, Q) symmetric; `std` = sqrt of the diagonal."""

    mean: np.ndarray
    cov: np.ndarray

    @property
    def std(self):
        return np.sqrt(np.maximum(np.diag(self.cov), 0.0))


def checked_weights(weights, T, n, d):
    """`weights` as a contiguous fp64 array (Q, T+1, n, d); the short form (Q, T+1, d) weighs derivative 0.  ValueError for any
    other shape, Q < 1 or entries that are not finite."""
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim == 3 and w.shape[1:] == (T + 1, d):
        full = np.zeros((w.shape[0], T + 1, n, d))
        full[:, :, 0] = w
        w = full
    if w.ndim != 4 or w.shape[1:] != (T + 1, n, d) or w.shape[0] < 1:
        raise ValueError(f"functionals(): weights must have shape (Q, {T + 1}, {d}) or (Q, {T + 1}, {n}, {d}) with Q >= 1, "
                         f"got {np.shape(weights)}")
    if not np.all(np.isfinite(w)):
        raise ValueError("functionals(): weights must be finite")
    return np.ascontiguousarray(w)


def point(T, d, k, j):
    """u(x_j, t_k): one at (k, j), zero elsewhere."""
    w = np.zeros((T + 1, d))
    w[k, j] = 1.0
    return w


def trapezoid_in_time(t, node_weights):
    """The trapezoid rule over the grid times `t` (T+1,) of sum_j node_weights[j] u(x_j, .): an approximation of the time integral
    at a sensor (`node_weights` a unit vector) or of a weighted total.  The time weights sum to t[-1] - t[0]."""
    t = np.asarray(t, dtype=np.float64)
    c = np.zeros(t.size)
    if t.size > 1:
        h = np.diff(t)
        c[:-1] += 0.5 * h
        c[1:] += 0.5 * h
    return np.outer(c, np.asarray(node_weights, dtype=np.float64))


def space_time_mean(t, d):
    """The mean of u over the mesh points and, by the trapezoid rule, over [t[0], t[-1]] (one grid time: the spatial mean)."""
    t = np.asarray(t, dtype=np.float64)
    if t.size == 1:
        return np.full((1, d), 1.0 / d)
    return trapezoid_in_time(t, np.full(d, 1.0 / d)) / (t[-1] - t[0])


def difference(T, d, a, b):
    """u(x_ja, t_ka) - u(x_jb, t_kb) for a = (ka, ja), b = (kb, jb)."""
    return point(T, d, *a) - point(T, d, *b)
