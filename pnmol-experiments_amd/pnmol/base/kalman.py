"""Gaussian filtering and smoothing routines (reference: src/pnmol/base/kalman.py), computed on the GPU.

The same three functions, names, arguments and return tuples.  As in `pnmol.base.sqrt`, the QRs and Cholesky factors run on
the device (`pnmol_qr_r`, `pnmol_sqrt_propagate_cholesky_factor`, `pnmol_sqrt_update_no_meascov`, `pnmol_cholesky_lower`);
the small glue around them stays on the host.  Factors have a non-negative diagonal (the reference's carry LAPACK's
data-dependent signs); every product formed from them is the same.  The PDE solvers' own smoother is
`pnmol.white.LinearWhiteNoiseEK1.smooth` (one device call per step, covariance form).  No CPU fallback.
"""

import numpy as np
import scipy.linalg

from pnmol import _hip
from pnmol.base import sqrt


def _ctx(ctx):
    return ctx if ctx is not None else _hip.Context.default()


def _f64(*arrays):
    return [np.asarray(a, dtype=np.float64) for a in arrays]


def filter_step(m, sc, phi, sq, h, b, data, *, ctx=None):
    """Predict with (phi, sq), update on `data` through (h, b); also the smoothing gain (kalman.py:11-28).
    Returns (m, sc, sgain, m_pred, sc_pred, x1)."""
    m, sc, phi, sq, h, b, data = _f64(m, sc, phi, sq, h, b, data)
    m_pred = phi @ m
    x1 = phi @ sc
    sc_pred = sqrt.propagate_cholesky_factor(x1, sq, ctx=ctx)
    cross = (x1 @ sc.T).T
    sgain = scipy.linalg.cho_solve((sc_pred, True), cross.T).T
    sc_new, kgain, _ = sqrt.update_sqrt_no_meascov(h, sc_pred, ctx=ctx)
    z = h @ m_pred + b
    m_new = m_pred - kgain @ (z - data)
    return m_new, sc_new, sgain, m_pred, sc_pred, x1


def smoother_step_traditional(m, sc, m_fut, sc_fut, sgain, mp, scp, *, ctx=None):
    """Covariance-form smoothing step (kalman.py:31-45).  Returns (new_mean, new_sc)."""
    m, sc, m_fut, sc_fut, sgain, mp, scp = _f64(m, sc, m_fut, sc_fut, sgain, mp, scp)
    c = sc @ sc.T
    c_fut = sc_fut @ sc_fut.T
    cp = scp @ scp.T
    new_mean = m + sgain @ (m_fut - mp)
    new_cov = c + sgain @ (c_fut - cp) @ sgain.T
    new_sc = _ctx(ctx).cholesky(0.5 * (new_cov + new_cov.T))
    return new_mean, new_sc


def smoother_step_sqrt(m, sc, m_fut, sc_fut, sgain, sq, mp, x, *, ctx=None):
    """Square-root smoothing step: one QR of the (3d, 2d) block matrix (kalman.py:48-66).  Returns (new_mean, new_sc)."""
    m, sc, m_fut, sc_fut, sgain, sq, mp, x = _f64(m, sc, m_fut, sc_fut, sgain, sq, mp, x)
    new_mean = m - sgain @ (mp - m_fut)
    d = m.shape[0]
    zeros = np.zeros((d, d))
    M = np.block([[x.T, sc.T], [sq.T, zeros.T], [zeros.T, sc_fut.T @ sgain.T]])
    R = _ctx(ctx).qr_r(M)
    return new_mean, R[d:2 * d, d:].T
