"""References for `pnmol_functionals` (posterior of linear functionals q = sum_k W_k x_k of the whole trajectory).  NumPy only.

Three evaluations of the same quantity from the same filtered states (raw (mean (n, d), covariance (D, D)) pairs, the way
`pnmol_state_set` takes and `State.mean()` / `State.cov()` return them; flat state index j n + a, the reference's order):

  1. `dense_reference`: fp64, the textbook route.  Gains with `smooth_reference.rts_step`'s algebra, the smoothed states by
     `rts_step` itself, the joint covariance blocks Cov(x_k, x_l) = G_k ... G_{l-1} Ps_l (k < l) explicitly, then W Cov W^T.
  2. `restate`: fp64, the device's order of operations (csrc/pnmol_functional.hip): the adjoint recursion in ascending k.
  3. `truth`: that recursion in np.longdouble on the pieces of tests/stage_reference.py (longdouble products, the one solve per
     step refined on longdouble residuals: `gain_truth`).

`trajectory_case` extends `stage_reference.synthetic_case` to T + 1 well-conditioned states with unequal steps."""

import functools
import types

import numpy as np
import scipy.linalg

import smooth_reference
import stage_reference as sr

LD = sr.LD
STEP_FACTORS = (1.0, 0.7, 1.9)   # steps h, 0.7 h, 1.9 h: the frame of the dual vector changes between them


def flat_weights(W):
    """(Q, T+1, n, d) -> (Q, T+1, D) in the flat state order j n + a."""
    W = np.asarray(W)
    return np.stack([[sr.flat(W[q, k]) for k in range(W.shape[1])] for q in range(W.shape[0])])


def error(X, X_true):
    """max|X - X_true| / max|X_true| (the metric of stage_reference, over a mean vector or a covariance)."""
    return float(np.abs(np.asarray(X).astype(LD) - X_true).max() / np.abs(X_true).max())


# ---- inputs ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trajectory_case(N, nu, bcond, T=3, seed=1):
    """`synthetic_case(N, nu, bcond)` with a trajectory of T + 1 independent states: state k is well conditioned in the frame of
    its own step dts[k] = STEP_FACTORS[k] h (eigenvalues as stage_reference draws them for a filtered state), the terminal one in
    the frame of the last step.  Read-only: shared between tests."""
    c = sr.synthetic_case(N, nu, bcond)
    rng = np.random.default_rng(seed)
    dts = [f * c.h for f in STEP_FACTORS[:T]]
    lam_f = sr.LAMBDA_FILT.get(c.key, sr.LAMBDA)
    states = []
    for k in range(T + 1):
        h = dts[min(k, T - 1)] if T else c.h
        s = np.tile(sr.scales(c.nu, h, np.float64)[0], c.d)
        Qm, R = np.linalg.qr(rng.standard_normal((c.D, c.D)))
        U = Qm * np.sign(np.diag(R))
        lam = lam_f if k < T else sr.LAMBDA
        Wm = (U * rng.uniform(lam[0], lam[1], c.D)) @ U.T
        P = np.outer(s, s) * (0.5 * (Wm + Wm.T))
        assert np.array_equal(P, P.T)
        states.append(((s * rng.standard_normal(c.D)).reshape((c.n, c.d), order="F").copy(), P))
    t = np.concatenate(([0.0], np.cumsum(dts)))
    return types.SimpleNamespace(c=c, T=T, dts=dts, t=t, states=states)


def random_weights(tc, Q, seed=2):
    """(Q, T+1, n, d) standard normals on all derivative rows, raw coordinates."""
    return np.random.default_rng(seed).standard_normal((Q, tc.T + 1, tc.c.n, tc.c.d))


def predicted_condition(tc):
    """max over the steps of cond(P-) in the frame of the step."""
    c, out = tc.c, 0.0
    for (m, P), h in zip(tc.states, tc.dts):
        ts = 1.0 / np.tile(sr.scales(c.nu, h, np.float64)[0], c.d)
        out = max(out, float(np.linalg.cond(c.A @ (np.outer(ts, ts) * P) @ c.A.T + c.Q)))
    return out


# ---- 1. the dense reference -------------------------------------------------------------------------------------------------
def dense_reference(A, Q, preconditioner, states, dts, W):
    """(mean (Q,), cov (Q, Q), smoothed means (T+1, D), smoothed covariances (T+1, D, D)), fp64.  A, Q: the preconditioned
    transition; preconditioner(h) -> (Pc, Pcinv) of the Nordsieck frame of h."""
    T = len(dts)
    Wf = flat_weights(W)
    ms, Ps, Gs = [sr.flat(states[T][0])], [states[T][1]], [None] * T
    for k in range(T - 1, -1, -1):
        Pc, Pcinv = preconditioner(dts[k])
        m, P = sr.flat(states[k][0]), states[k][1]
        Ph = Pcinv @ P @ Pcinv.T
        P_pred = A @ Ph @ A.T + Q
        G = scipy.linalg.cho_solve(scipy.linalg.cho_factor(P_pred, lower=True), A @ Ph).T      # rts_step's gain
        Gs[k] = Pc @ G @ Pcinv
        mk, Pk = smooth_reference.rts_step(m, P, ms[0], Ps[0], A, Q, Pc, Pcinv)
        ms.insert(0, mk), Ps.insert(0, Pk)
    mean = sum(Wf[:, k] @ ms[k] for k in range(T + 1))
    cov = np.zeros((Wf.shape[0],) * 2)
    for l in range(T + 1):
        C = Ps[l]
        cov += Wf[:, l] @ C @ Wf[:, l].T
        for k in range(l - 1, -1, -1):
            C = Gs[k] @ C                                                                     # Cov(x_k, x_l)
            X = Wf[:, k] @ C @ Wf[:, l].T
            cov += X + X.T
    return mean, 0.5 * (cov + cov.T), np.stack(ms), np.stack(Ps)


# ---- 2. the device's order of operations, fp64 --------------------------------------------------------------------------------
def restate(A, Q, nu, d, states, dts, W):
    """(mean, cov, gross): the recursion of csrc/pnmol_functional.hip in fp64 NumPy.  gross[q] = sum_k (Lam_k^T P_k Lam_k)_qq, the
    positive part of cov_qq before the conditioning terms are subtracted: cov_qq / gross[q] says how much a functional cancels."""
    T = len(dts)
    Wf = flat_weights(W)
    nq = Wf.shape[0]
    mean, cov, gross = np.zeros(nq), np.zeros((nq, nq)), np.zeros(nq)
    Mu = s_before = None
    for k in range(T):
        s = np.tile(sr.scales(nu, dts[k], np.float64)[0], d)
        ts = 1.0 / s
        mh, Ph = ts * sr.flat(states[k][0]), np.outer(ts, ts) * states[k][1]
        Lam = s[:, None] * Wf[:, k].T
        if k > 0:
            Lam = Lam + (s / s_before)[:, None] * Mu
        U = Ph @ Lam
        L = np.linalg.cholesky(A @ Ph @ A.T + Q)
        Y = scipy.linalg.solve_triangular(L, A @ U, lower=True)
        Mu = scipy.linalg.solve_triangular(L.T, Y, lower=False)
        g1 = Lam.T @ U
        mean += Lam.T @ mh - Mu.T @ (A @ mh)
        cov += g1 - Y.T @ Y
        gross += np.diag(g1)
        s_before = s
    Lam = Wf[:, T].T if T == 0 else Wf[:, T].T + Mu / s_before[:, None]
    g1 = Lam.T @ (states[T][1] @ Lam)
    mean += Lam.T @ sr.flat(states[T][0])
    cov += g1
    gross += np.diag(g1)
    return mean, 0.5 * (cov + cov.T), gross


# ---- 3. extended precision ----------------------------------------------------------------------------------------------------
def truth(c, states, dts, W):
    """(mean, cov) in np.longdouble for a `synthetic_case` c: the same recursion with `stage_reference.gain_truth` per step."""
    T = len(dts)
    Wf = flat_weights(W).astype(LD)
    nq = Wf.shape[0]
    mean, cov = np.zeros(nq, dtype=LD), np.zeros((nq, nq), dtype=LD)
    lam_raw = Wf[:, 0].T
    for k in range(T):
        g = sr.gain_truth(c, states[k][0], states[k][1], dts[k])
        s = np.tile(sr.scales(c.nu, dts[k])[0], c.d)
        Lam = s[:, None] * lam_raw
        Mu = g.G.T @ Lam
        mean += Lam.T @ g.mh - Mu.T @ sr.kron_left(c.A1x, g.mh)
        cov += Lam.T @ g.Ph @ Lam - Mu.T @ g.Pm @ Mu
        lam_raw = Wf[:, k + 1].T + Mu / s[:, None]
    mean += lam_raw.T @ sr.flat(states[T][0]).astype(LD)
    cov += lam_raw.T @ states[T][1].astype(LD) @ lam_raw
    return mean, 0.5 * (cov + cov.T)
