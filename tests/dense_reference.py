"""Dense output the textbook way, in dense fp64 NumPy: the reference that the bridge formulas (`pnmol.base.iwp.
bridge_coefficients`) and the device's dense output are checked against.

A query time t is INSERTED into the oracle's filtered trajectory as a grid point: the filtered state there is the prediction
from the point before it (there is no measurement at t), and the ordinary RTS pass (tests/smooth_reference.py) over the
augmented grid gives the smoothing posterior at t.  Nothing here uses the bridge."""

import types

import numpy as np

from smooth_reference import rts_step


def filtered_on_oracle(osol):
    """Filtered (means, covs) of an oracle `solve()` as flat point-major vectors / (D, D) matrices."""
    return [mu.reshape(-1, order="F") for mu in osol.mean], [C @ C.T for C in osol.cov_sqrtm]


def predict(osolver, m, P, dt):
    """The prior alone over dt, raw coordinates."""
    Phi, Ql = osolver.iwp.non_preconditioned_discretize(dt)
    return Phi @ m, Phi @ P @ Phi.T + Ql @ Ql.T


def augment(osolver, osol, ts):
    """The filtered trajectory with the times `ts` (any order, >= osol.t[0]) inserted.  Returns a namespace with `t`, `means`,
    `covs` (lists over the augmented grid), and `where[q]` = position of ts[q] in it.  A time equal to a grid time is not
    inserted: `where` points at the grid point."""
    ts = np.atleast_1d(np.asarray(ts, dtype=float))
    grid = np.asarray(osol.t, dtype=float)
    if np.any(ts < grid[0]):
        raise ValueError("dense reference: a query time lies before the first grid time")
    means, covs = filtered_on_oracle(osol)
    items = [(t, None) for t in grid]
    for q in np.argsort(ts, kind="stable"):
        if not np.any(grid == ts[q]):
            items.append((ts[q], int(q)))
    items.sort(key=lambda it: it[0])
    out_t, out_m, out_P, where = [], [], [], {}
    g = 0
    for t, q in items:
        if q is None:
            out_m.append(means[g]), out_P.append(covs[g])
            g += 1
        elif out_t and out_t[-1] == t:          # the same time asked for twice
            where[q] = len(out_t) - 1
            continue
        else:
            m, P = predict(osolver, out_m[-1], out_P[-1], t - out_t[-1])
            out_m.append(m), out_P.append(P)
            where[q] = len(out_t)
        out_t.append(t)
    for q in range(len(ts)):
        if q not in where:
            where[q] = int(np.flatnonzero(np.asarray(out_t) == ts[q])[0])
    return types.SimpleNamespace(t=np.array(out_t), means=out_m, covs=out_P, where=[where[q] for q in range(len(ts))])


def rts_over(osolver, aug):
    """RTS pass over an augmented grid: smoothed (means, covs), lists over that grid."""
    A, Ql = osolver.iwp.preconditioned_discretize
    Q = Ql @ Ql.T
    ms, Ps = [aug.means[-1]], [aug.covs[-1]]
    for k in range(len(aug.t) - 2, -1, -1):
        Pc, Pcinv = osolver.iwp.nordsieck_preconditioner(aug.t[k + 1] - aug.t[k])
        m, P = rts_step(aug.means[k], aug.covs[k], ms[-1], Ps[-1], A, Q, Pc, Pcinv)
        ms.append(m), Ps.append(P)
    ms.reverse(), Ps.reverse()
    return ms, Ps


def _pick(means, covs, where, shape):
    n, d = shape
    m = np.stack([means[i].reshape((n, d), order="F") for i in where])
    s = np.stack([np.sqrt(np.maximum(np.diag(covs[i]), 0.0)).reshape((n, d), order="F") for i in where])
    return m, s, [covs[i] for i in where]


def smoothed_dense(osolver, osol, ts, base=None):
    """Smoothing posterior at `ts`: means (Tq, n, d), marginal stds (Tq, n, d), covariances (list of (D, D), point-major).

    Every query is inserted ON ITS OWN (several insertions into one interval make sub-steps of a few per cent of the step,
    whose predicted covariances the dense RTS step inverts badly: 4e-4 of the largest std was seen with five of them at
    nu = 2).  The smoothed states to the right of an insertion do not depend on it, so the pass over the augmented grid
    reduces to the original pass (`base` = `rts_on_oracle(osolver, osol)`, computed here if not given) plus, per query, the
    prediction to t and ONE more RTS step from there to the next grid point; `rts_over(augment(...))` with a single query is
    the same computation (tests/test_dense_host.py checks that)."""
    from smooth_reference import rts_on_oracle

    ts = np.atleast_1d(np.asarray(ts, dtype=float))
    grid = np.asarray(osol.t, dtype=float)
    if np.any(ts < grid[0]):
        raise ValueError("dense reference: a query time lies before the first grid time")
    gm, gP = rts_on_oracle(osolver, osol) if base is None else base
    fm, fP = filtered_on_oracle(osol)
    A, Ql = osolver.iwp.preconditioned_discretize
    Q = Ql @ Ql.T
    means, covs = [], []
    for t in ts:
        k = int(np.searchsorted(grid, t, side="right")) - 1
        if grid[k] == t:
            m, P = gm[k].reshape(-1, order="F"), gP[k]
        else:
            m, P = predict(osolver, fm[k], fP[k], t - grid[k])
            if k + 1 < len(grid):
                Pc, Pcinv = osolver.iwp.nordsieck_preconditioner(grid[k + 1] - t)
                m, P = rts_step(m, P, gm[k + 1].reshape(-1, order="F"), gP[k + 1], A, Q, Pc, Pcinv)
        means.append(m), covs.append(P)
    return _pick(means, covs, range(len(ts)), osol.mean.shape[1:])


def filtered_dense(osolver, osol, ts):
    """Filtering posterior at `ts` (prediction from the grid point on the left), same layout."""
    aug = augment(osolver, osol, ts)
    return _pick(aug.means, aug.covs, aug.where, osol.mean.shape[1:])


def bridge_on_oracle(osolver, osol, k, theta, bridge_coefficients):
    """NOT the reference: the bridge formulas under test, restated in dense NumPy on the oracle's
    trajectory, with the (B_minus, B_plus, Qb) of the function handed in.  Posterior (mean (n, d), cov (D, D) point-major) at
    t_k + theta h.  tests/test_dense_host.py pins it against `smoothed_dense`."""
    import scipy.linalg

    from smooth_reference import rts_on_oracle

    n, d = osol.mean.shape[1:]
    A, Ql = osolver.iwp.preconditioned_discretize
    Q = Ql @ Ql.T
    K = osolver.iwp.gamma @ osolver.iwp.gamma.T
    Pc, Pcinv = osolver.iwp.nordsieck_preconditioner(osol.t[k + 1] - osol.t[k])
    means, covs = filtered_on_oracle(osol)
    ms, Ps = rts_on_oracle(osolver, osol)
    Ph = Pcinv @ covs[k] @ Pcinv.T
    G = scipy.linalg.cho_solve(scipy.linalg.cho_factor(A @ Ph @ A.T + Q, lower=True), A @ Ph).T
    msl, msr = Pcinv @ ms[k].reshape(-1, order="F"), Pcinv @ ms[k + 1].reshape(-1, order="F")
    Psl, Psr = Pcinv @ Ps[k] @ Pcinv.T, Pcinv @ Ps[k + 1] @ Pcinv.T
    C = G @ Psr
    Bm, Bp, Qb = bridge_coefficients(theta, n - 1)
    Bm, Bp = np.kron(np.eye(d), Bm), np.kron(np.eye(d), Bp)
    m = Bm @ msl + Bp @ msr
    cross = Bm @ C @ Bp.T
    P = Bm @ Psl @ Bm.T + cross + cross.T + Bp @ Psr @ Bp.T + np.kron(K, Qb)
    return (Pc @ m).reshape((n, d), order="F"), Pc @ P @ Pc.T


def as_solution(aug, shape):
    """An augmented grid dressed as an oracle solution (`t`, `mean` (T', n, d), `cov_sqrtm`), so that the chain of
    tests/sample_reference.py (`maps_on_oracle`) runs over it: an inserted point is a filtered state like any other."""
    from sample_reference import psd_factor

    n, d = shape
    return types.SimpleNamespace(t=aug.t, mean=np.stack([m.reshape((n, d), order="F") for m in aug.means]),
                                 cov_sqrtm=[psd_factor(P) for P in aug.covs])
