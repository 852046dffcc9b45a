"""Dense fp64 NumPy RTS smoother: the reference that the device smoother (`pnmol.white.*.smooth`) is checked against."""

import numpy as np
import scipy.linalg


def rts_step(m, P, m_next, P_next, A, Q, Pc, Pcinv):
    """One backward step (kalman.py:33-46 of the reference) in the Nordsieck frame (Pc, Pcinv) of the step, on raw inputs;
    returns the smoothed (mean, cov) in raw coordinates."""
    mh, Ph = Pcinv @ m, Pcinv @ P @ Pcinv.T
    mnh, Pnh = Pcinv @ m_next, Pcinv @ P_next @ Pcinv.T
    m_pred, P_pred = A @ mh, A @ Ph @ A.T + Q
    G = scipy.linalg.cho_solve(scipy.linalg.cho_factor(P_pred, lower=True), A @ Ph).T  # P A^T (P-)^-1
    msh = mh + G @ (mnh - m_pred)
    Psh = Ph + G @ (Pnh - P_pred) @ G.T
    return Pc @ msh, Pc @ Psh @ Pc.T


def rts_on_oracle(osolver, osol):
    """Smoothed means (T+1, n, d) and covariances (T+1, D, D) of an oracle `solve()` (point-major state order)."""
    A, Ql = osolver.iwp.preconditioned_discretize
    Q = Ql @ Ql.T
    n, d = osol.mean.shape[1:]
    means = [mu.reshape(-1, order="F") for mu in osol.mean]
    covs = [C @ C.T for C in osol.cov_sqrtm]
    ms, Ps = [means[-1]], [covs[-1]]
    for k in range(len(means) - 2, -1, -1):
        Pc, Pcinv = osolver.iwp.nordsieck_preconditioner(osol.t[k + 1] - osol.t[k])
        m, P = rts_step(means[k], covs[k], ms[-1], Ps[-1], A, Q, Pc, Pcinv)
        ms.append(m), Ps.append(P)
    ms.reverse(), Ps.reverse()
    return np.stack([m.reshape((n, d), order="F") for m in ms]), np.stack(Ps)


def marginal_std(covs, n, d):
    """sqrt(diag cov) as (T+1, n, d)."""
    return np.stack([np.sqrt(np.maximum(np.diag(P), 0.0)).reshape((n, d), order="F") for P in covs])
