"""Integrated Wiener process prior (reference: src/pnmol/base/iwp.py).

Host-side description of the prior.  The dense Kronecker matrices are only materialised when a
caller asks for them (tests, `projection_matrix`); the device works on the n x n blocks A1, Q1.
"""

from collections import namedtuple
from functools import cached_property

import numpy as np
import scipy.linalg
import scipy.special


def _partial_interval(theta, num_derivatives):
    """(A_th, Q_th): transition and process noise of the IWP over the fraction theta of a step, in the Nordsieck frame of
    the WHOLE step.  A_th[a, b] = A1[a, b] th^(b - a), Q_th[a, b] = Q1[a, b] th^(2 nu + 1 - a - b), entry by entry: every
    exponent that meets a non-zero entry is >= 0 (A1 is upper triangular), so nothing is divided by a power of theta."""
    n = num_derivatives + 1
    A1 = np.flip(scipy.linalg.pascal(n, kind="lower", exact=False))
    Q1 = np.flip(scipy.linalg.hilbert(n))
    a = np.arange(n)
    A = np.triu(A1) * theta ** np.maximum(a[None, :] - a[:, None], 0)
    Q = Q1 * theta ** (2 * num_derivatives + 1 - a[:, None] - a[None, :])
    return A, Q


def bridge_coefficients(theta, num_derivatives):
    """(B_minus, B_plus, Qb), each (n, n): the IWP prior's bridge over one step, in the Nordsieck frame of that step.

    With x_l, x_r the states at the two ends of a step h and t = t_l + theta h, 0 < theta < 1,
        x_t | x_l, x_r ~ N((B_minus (x) I) x_l + (B_plus (x) I) x_r, Qb (x) K).
    There is no measurement inside a step, so the same law holds under the filtering / smoothing posterior: it is what
    dense output and draws between grid times are built from.  By Chapman-Kolmogorov,
    A_(1-th) Q_th A_(1-th)^T + Q_(1-th) = Q1, the gain of conditioning x_t on x_r is B_plus = Q_th A_(1-th)^T Q1^-1; then
    B_minus = (I - B_plus A_(1-th)) A_th and Qb in Joseph form (symmetric positive semi-definite by construction)."""
    theta = float(theta)
    if not 0.0 < theta < 1.0:
        raise ValueError(f"bridge_coefficients: theta must lie strictly inside (0, 1), got {theta}")
    n = num_derivatives + 1
    Q1 = np.flip(scipy.linalg.hilbert(n))
    A_th, Q_th = _partial_interval(theta, num_derivatives)
    A_c, Q_c = _partial_interval(1.0 - theta, num_derivatives)
    B_plus = scipy.linalg.cho_solve(scipy.linalg.cho_factor(Q1, lower=True), A_c @ Q_th).T
    M = np.eye(n) - B_plus @ A_c
    B_minus = M @ A_th
    Qb = M @ Q_th @ M.T + B_plus @ Q_c @ B_plus.T
    return B_minus, B_plus, 0.5 * (Qb + Qb.T)


class IntegratedWienerTransition(namedtuple("_IWP", "wiener_process_dimension num_derivatives wp_diffusion_sqrtm")):
    @cached_property
    def preconditioned_discretize_1d(self):
        """(A_1d, chol(Q_1d)); np.flip without axis reverses both axes (iwp.py:13-30)."""
        n = self.num_derivatives + 1
        A_1d = np.flip(scipy.linalg.pascal(n, kind="lower", exact=False))
        Q_1d = np.flip(scipy.linalg.hilbert(n))
        return A_1d, np.linalg.cholesky(Q_1d)

    @cached_property
    def preconditioned_discretize(self):
        A_1d, L_Q1d = self.preconditioned_discretize_1d
        return np.kron(np.eye(self.wiener_process_dimension), A_1d), np.kron(self.wp_diffusion_sqrtm, L_Q1d)

    def nordsieck_preconditioner_1d_raw(self, dt):  # iwp.py:55-62
        powers = np.arange(self.num_derivatives, -1, -1)
        scales = scipy.special.factorial(powers)
        powers = powers + 0.5
        return (np.abs(dt) ** powers) / scales, (np.abs(dt) ** (-powers)) * scales

    def nordsieck_preconditioner_1d(self, dt):
        s, sinv = self.nordsieck_preconditioner_1d_raw(dt)
        return np.diag(s), np.diag(sinv)

    def nordsieck_preconditioner(self, dt):
        p, pinv = self.nordsieck_preconditioner_1d(dt)
        eye = np.eye(self.wiener_process_dimension)
        return np.kron(eye, p), np.kron(eye, pinv)

    def non_preconditioned_discretize(self, dt):
        P, Pinv = self.nordsieck_preconditioner(dt)
        A, Ql = self.preconditioned_discretize
        return P @ A @ Pinv, P @ Ql

    def projection_matrix(self, derivative_to_project_onto):
        # = np.kron(np.eye(d), e_q^T) (base/iwp.py:125-133), written directly: kron of a 4096-identity takes seconds
        d, n = self.wiener_process_dimension, self.num_derivatives + 1
        out = np.zeros((d, n * d))
        out[np.arange(d), np.arange(d) * n + derivative_to_project_onto] = 1.0
        return out

    def projection_matrix_1d(self, derivative_to_project_onto):
        return np.eye(1, self.num_derivatives + 1, derivative_to_project_onto)

    @property
    def state_dimension(self):
        return self.wiener_process_dimension * (self.num_derivatives + 1)
