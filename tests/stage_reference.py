"""Stage references for the post-filter kernels (`pnmol_smoother_step`, `pnmol_state_predict`, `pnmol_bridge_state`,
`pnmol_samples_draw`, `pnmol_samples_step_back`): synthetic inputs, extended-precision truths and fp64 restatements of the
device's algebra.  NumPy only, no GPU.  tests/test_stage_reference_host.py pins the truths against the older references,
tests/test_gpu_stage_parity.py holds the device to them on every entry of the state.

Method
  - Inputs are not heat posteriors: `pnmol_state_set` takes any mean and covariance, so the states are drawn well conditioned
    in the Nordsieck frame of the step, W = U diag(lambda) U^T with Haar U and lambda in [0.5, 2], and uploaded in raw
    coordinates.  Then cond(P-) stays below 1e4, every tile of every matrix carries O(1) numbers, and an fp64 evaluation sits
    within 1e-15 .. 1e-13 of the exact result.
  - A truth starts from the very fp64 arrays that are uploaded and evaluates the model in `np.longdouble` (eps 1.1e-19): products in
    longdouble, the one factorisation in fp64 with iterative refinement on longdouble residuals, the n x n bridge coefficients in
    mpmath.  The frame change uses longdouble scales, so the truth is that of the exact model.
  - A restatement repeats, in plain fp64 NumPy, the operations in the order the .hip files document.  Its error against the truth
    is the yardstick: the device performs the same fp64 operations in another summation order and is held to
    FACTOR * max(e64, 2^-52) (`bound`).
  - Everything is compared in the Nordsieck frame of the step, where all derivative blocks are O(1): `cov_error` is
    max|X - X_true| / max|X_true|, `vec_error` the same over all n derivative rows of a mean or a draw.

State order is the reference's: flat index j n + a is derivative a at mesh point j; means cross the API as (n, d)."""

import functools
import types

import mpmath
import numpy as np
import scipy.linalg
import scipy.special

from helpers import make_pair, to_device_layout

LD = np.longdouble
H = 2.0 ** -7
EPS = 2.0 ** -52
FACTOR = 16.0
SEED = 0
# the last correction of the gain's iterative refinement, relative, sits at eps_longdouble * cond(P-), a thousand times below what
# fp64 resolves at the same condition number; it has to stay below the smallest e64 that `bound` ever uses
REFINEMENT_FLOOR = EPS
refinement_steps = []   # (diagnostic: the last relative correction of every refined solve)

# (N, nu, bcond): the smallest shapes at which each path can go wrong.  Dp = n round_up(N, 32); the sweep the smoother and the
# backward draw reuse runs register-resident with CB <= 9 up to Dp = 288, with CB <= 17 up to Dp = 544, left-looking above
# (launch_sweep, pnmol_hip.hip).
CASES = [
    (20, 1, "dirichlet"),    # Dp = 64: one tile; 12 padded points
    (32, 2, "neumann"),      # Dp = 96: edge tile of the 64-tiling; no padded point
    (33, 2, "dirichlet"),    # Dp = 192: 31 padded points with unit pivots
    (40, 3, "dirichlet"),    # Dp = 256: the N = 4 instantiations
    (96, 2, "neumann"),      # Dp = 288: last size of the CB <= 9 sweep
    (150, 1, "neumann"),     # Dp = 320: first size of the CB <= 17 sweep
    (170, 2, "dirichlet"),   # Dp = 576: left-looking sweep; Dp mod 64 = 0 with 22 padded points
]


# Eigenvalue range of the states in the frame of h.  At nu = 3 the filtered state takes a narrower and smaller one: the conditional
# covariance of a backward draw is (P^-1 + A^T Q^-1 A)^-1 and cond(Q1) = 1.6e4 at n = 4, so with lambda in [0.5, 2] its
# smallest eigenvalue is 8e-5 of its largest (the host test asks for 1e-3); shrinking P towards Q's small end lifts that ratio
# (1 / (r (1 + 6e3 a)) for lambda in [a, r a]) while cond(P-) grows towards cond(Q) = 2e4 (asked: <= 1e4).  Successor and
# terminal state keep the full range.
LAMBDA = (0.5, 2.0)
LAMBDA_FILT = {(40, 3, "dirichlet"): (0.06, 0.09)}   # cond(P-) = 8.5e3, eigenvalue ratio 1.2e-3: the two pull against each other


def case_id(case):
    return f"N{case[0]}-nu{case[1]}-{case[2]}"


def padded_dim(case):
    N, nu, _ = case
    return (nu + 1) * ((N + 31) // 32) * 32


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _haar(rng, D):
    Qm, R = np.linalg.qr(rng.standard_normal((D, D)))
    return Qm * np.sign(np.diag(R))


def _frame_state(rng, D, lam):
    U = _haar(rng, D)
    W = (U * rng.uniform(lam[0], lam[1], D)) @ U.T
    return 0.5 * (W + W.T), rng.standard_normal(D)


@functools.lru_cache(maxsize=None)
def synthetic_case(N, nu, bcond, h=H, seed=SEED, lam_filt=None):
    """Product and oracle solver of the heat problem (d = N) with three independent states that are well conditioned in the frame
    of h -- `filt` (filtered, t = 0), `succ` (a smoothed successor, t = h) and `term` (a terminal state, t = h) -- as raw
    (mean (n, d), covariance (D, D)) pairs the way `pnmol_state_set` takes them.  Treat the result as read-only: it is shared."""
    pde, solver, opde, osolver = make_pair(N, nu, h, 1, bcond)
    osolver.iwp, osolver.E0, osolver.E1, _ = osolver.initialize_iwp(opde)
    iwp = osolver.iwp
    A, Ql = iwp.preconditioned_discretize
    A1, LQ1 = iwp.preconditioned_discretize_1d
    Pc, Pcinv = iwp.nordsieck_preconditioner(h)
    n, d = nu + 1, N
    D = n * d
    s = np.diag(Pc).copy()
    rng = np.random.default_rng(seed)
    states = {}
    for name in ("filt", "succ", "term"):
        W, w = _frame_state(rng, D, (lam_filt or LAMBDA_FILT.get((N, nu, bcond), LAMBDA)) if name == "filt" else LAMBDA)
        P = np.outer(s, s) * W                                     # = Pc W Pc^T, symmetric to the bit (s_i s_j commutes)
        assert np.array_equal(P, P.T)
        states[name] = ((s * w).reshape((n, d), order="F").copy(), P)
    c = types.SimpleNamespace(key=(N, nu, bcond), N=N, nu=nu, n=n, d=d, D=D, h=h, pde=pde, solver=solver, opde=opde, osolver=osolver,
                              A=A, Ql=Ql, Q=Ql @ Ql.T, A1=A1, LQ1=LQ1, gamma=iwp.gamma, Pc=Pc, Pcinv=Pcinv, **states)
    # the model in extended precision: Q = Ql Ql^T = (gamma gamma^T) (x) (LQ1 LQ1^T)
    g, l1 = iwp.gamma.astype(LD), LQ1.astype(LD)
    c.Kx, c.Q1x, c.A1x = g @ g.T, l1 @ l1.T, A1.astype(LD)
    c.Qx = np.kron(c.Kx, c.Q1x)
    return c


def flat(m_nd):
    return np.asarray(m_nd).reshape(-1, order="F")


# ---- frames and metrics ---------------------------------------------------------------------------------------------------
def scales(nu, h, dtype=LD):
    """(s, 1 / s) of the Nordsieck frame of h per derivative, a = 0 .. nu: s_a = h^(nu - a + 1/2) / (nu - a)!."""
    p = np.arange(nu, -1, -1)
    s = dtype(h) ** (p.astype(dtype) + dtype(0.5)) / scipy.special.factorial(p).astype(dtype)
    return s, dtype(1.0) / s


class Frame:
    """Raw fp64 arrays -> longdouble arrays in the Nordsieck frame of h (exact scales up to longdouble rounding)."""

    def __init__(self, case, h):
        self.h = h
        _, sinv = scales(case.nu, h)
        self.sinv = np.tile(sinv, case.d)

    def cov(self, P):
        return self.sinv[:, None] * np.asarray(P).astype(LD) * self.sinv[None, :]

    def vec(self, m):
        """A mean as it crosses the API, (n, d)."""
        m = np.asarray(m)
        assert m.shape[0] * m.shape[1] == self.sinv.size and m.shape[0] <= 4
        return self.sinv * flat(m).astype(LD)

    def flat(self, v):
        """A flat vector (D,) or vectors as columns (D, S), raw."""
        v = np.asarray(v).astype(LD)
        return self.sinv * v if v.ndim == 1 else self.sinv[:, None] * v

    def draws(self, x_Snd):
        """`Samples.get()` (S, n, d) -> (D, S) in the frame."""
        S = x_Snd.shape[0]
        X = np.stack([flat(x) for x in x_Snd], axis=1)
        assert X.shape == (self.sinv.size, S)
        return self.sinv[:, None] * X.astype(LD)


def cov_error(X, X_true):
    return float(np.abs(np.asarray(X).astype(LD) - X_true).max() / np.abs(X_true).max())


vec_error = cov_error


def bound(e64):
    """The device's allowance for a quantity whose fp64 restatement sits e64 from the truth.  Device and restatement perform the
    same fp64 operations and differ in summation order (MFMA chains over K in blocks of 16 against BLAS); both sit under the same
    first-order bound c K eps cond, and one realisation may exceed another by a small factor."""
    return FACTOR * max(float(e64), EPS)


def tile_error_map(X, X_true, case, tile=64):
    """Largest |X - X_true| / max|X_true| per tile x tile block of the device's layout (derivative-major, points padded to 32):
    where a failing comparison went wrong."""
    n, d = case.n, case.d
    dp = (d + 31) // 32 * 32
    E = to_device_layout(np.abs(np.asarray(X).astype(LD) - X_true).astype(np.float64), n, d, dp) / float(np.abs(X_true).max())
    nt = (n * dp + tile - 1) // tile
    out = np.zeros((nt, nt))
    for i in range(nt):
        for j in range(nt):
            out[i, j] = E[i * tile:(i + 1) * tile, j * tile:(j + 1) * tile].max()
    return out


# ---- Kronecker helpers: (I_d (x) M1) with M1 (n, n), point-major -----------------------------------------------------------
def kron_left(M1, X):
    """(I (x) M1) X for X (D,) or (D, c)."""
    n = M1.shape[0]
    Y = np.matmul(M1, X.reshape((-1, n) + ((1,) if X.ndim == 1 else (X.shape[1],))))
    return Y.reshape(X.shape)


def kron_right(X, M1):
    """X (I (x) M1)^T for X (r, D)."""
    return kron_left(M1, np.ascontiguousarray(X.T)).T


# ---- extended-precision truths --------------------------------------------------------------------------------------------
def _solve_refined(Pm, B):
    """X (longdouble) with Pm X = B for a symmetric positive definite Pm: fp64 Cholesky, refined to convergence on longdouble
    residuals (each round gains a factor eps64 cond)."""
    cf = scipy.linalg.cho_factor(Pm.astype(np.float64), lower=True)
    X = scipy.linalg.cho_solve(cf, B.astype(np.float64)).astype(LD)
    last = np.inf
    for _ in range(8):
        dX = scipy.linalg.cho_solve(cf, (B - Pm @ X).astype(np.float64))
        X = X + dX
        step = float(np.abs(dX).max() / np.abs(X).max())
        if step <= 4.0 * float(np.finfo(LD).eps) or step >= 0.25 * last:   # converged, or at the floor eps_ld cond
            break
        last = step
    refinement_steps.append(step)
    if step > REFINEMENT_FLOOR:
        raise RuntimeError(f"stage_reference: iterative refinement stalled at {step:.1e}")
    return X


def predict_truth(case, m, P, dt):
    """The prior alone over dt from the raw state (m, P): (A m, A P A^T + Q) in the frame of dt, longdouble."""
    fr = Frame(case, dt)
    mh, Ph = fr.vec(m), fr.cov(P)
    Pm = kron_right(kron_left(case.A1x, Ph), case.A1x) + case.Qx
    return kron_left(case.A1x, mh), 0.5 * (Pm + Pm.T)


def gain_truth(case, m, P, h):
    """What the backward steps share, in the frame of h: m^h, P^h, P-, P^h A^T and the gain G = P A^T (P-)^-1."""
    fr = Frame(case, h)
    mh, Ph = fr.vec(m), fr.cov(P)
    Ph = 0.5 * (Ph + Ph.T)
    APh = kron_left(case.A1x, Ph)
    Pm = kron_right(APh, case.A1x) + case.Qx
    Pm = 0.5 * (Pm + Pm.T)
    G = _solve_refined(Pm, APh).T
    return types.SimpleNamespace(frame=fr, mh=mh, Ph=Ph, Pm=Pm, PAt=APh.T, G=G)


def rts_truth(case, filt, succ, h, gain=None):
    """One RTS backward step (include/pnmol_hip.h, `pnmol_smoother_step`) on raw inputs: G, ms, Ps and the lag-one cross-covariance
    C = G Ps', in the frame of h.  Ps = P + G (Ps' - P-) G^T is evaluated as P + (C - P A^T) G^T (G P- = P A^T)."""
    g = gain or gain_truth(case, filt[0], filt[1], h)
    msn, Psn = g.frame.vec(succ[0]), g.frame.cov(succ[1])
    C = g.G @ Psn
    Ps = g.Ph + (C - g.PAt) @ g.G.T
    ms = g.mh + g.G @ (msn - kron_left(case.A1x, g.mh))
    return types.SimpleNamespace(G=g.G, ms=ms, Ps=0.5 * (Ps + Ps.T), C=C, msn=msn, Psn=Psn, gain=g)


def backward_draw_truth(case, filt, h, gain=None):
    """The law of x_k | x_{k+1} (include/pnmol_hip.h, "Joint draws"), frame of h: x_k = a + G x_{k+1} + noise of covariance
    P - G P- G^T (= P - P A^T G^T)."""
    g = gain or gain_truth(case, filt[0], filt[1], h)
    a = g.mh - g.G @ kron_left(case.A1x, g.mh)
    S = g.Ph - g.PAt @ g.G.T
    return types.SimpleNamespace(a=a, G=g.G, cov=0.5 * (S + S.T), gain=g)


def _to_mp(x):
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi)))


def _from_mp(M, n):
    out = np.zeros((n, n), dtype=LD)
    for a in range(n):
        for b in range(n):
            hi = float(M[a, b])
            out[a, b] = LD(hi) + LD(float(M[a, b] - mpmath.mpf(hi)))
    return out


def bridge_coefficients_truth(case, theta):
    """(B-, B+, Qb), n x n longdouble, by Gaussian conditioning of the prior in mpmath (50 digits).  Over a part tau = theta h of
    the step the oracle's IWP moves by S(tau) A1 S(tau)^-1 with noise S(tau) Q1 S(tau) (S = the Nordsieck scales); in the frame
    of the whole step h that is D A1 D^-1 and D Q1 D with D = diag(theta^(nu - a + 1/2)).  With x_t = A_th x_l + q_th and
    x_r = A_c x_t + q_c:  Cov(x_r | x_l) = S = A_c Q_th A_c^T + Q_c,  Cov(x_t, x_r | x_l) = Q_th A_c^T,  so
    B+ = Q_th A_c^T S^-1,  B- = (I - B+ A_c) A_th,  Qb = Q_th - B+ S B+^T."""
    n, nu = case.n, case.nu
    with mpmath.workdps(50):
        A1 = mpmath.matrix([[_to_mp(v) for v in row] for row in case.A1x])
        Q1 = mpmath.matrix([[_to_mp(v) for v in row] for row in case.Q1x])

        def part(th):
            Dm = mpmath.diag([mpmath.mpf(th) ** (mpmath.mpf(nu - a) + mpmath.mpf(1) / 2) for a in range(n)])
            Di = mpmath.diag([1 / Dm[a, a] for a in range(n)])
            return Dm * A1 * Di, Dm * Q1 * Dm

        th = mpmath.mpf(float(theta))
        A_th, Q_th = part(th)
        A_c, Q_c = part(1 - th)
        S = A_c * Q_th * A_c.T + Q_c
        Bp = Q_th * A_c.T * mpmath.inverse(S)
        Bm = (mpmath.eye(n) - Bp * A_c) * A_th
        Qb = Q_th - Bp * S * Bp.T
        return _from_mp(Bm, n), _from_mp(Bp, n), _from_mp(Qb, n)


def bridge_truth(case, rts, theta):
    """Mean and covariance at t_k + theta h given the joint law [[Ps_k, C], [C^T, Ps_{k+1}]] of the two ends (`rts` from
    `rts_truth`), frame of h: the bridge maps the ends by [B- (x) I, B+ (x) I] and adds Qb (x) K."""
    Bm, Bp, Qb = bridge_coefficients_truth(case, theta)
    m = kron_left(Bm, rts.ms) + kron_left(Bp, rts.msn)
    cross = kron_right(kron_left(Bm, rts.C), Bp)
    P = (kron_right(kron_left(Bm, rts.Ps), Bm) + cross + cross.T + kron_right(kron_left(Bp, rts.Psn), Bp)
         + np.kron(case.Kx, 0.5 * (Qb + Qb.T)))
    return m, 0.5 * (P + P.T)


# ---- fp64 restatements of the device's algebra ----------------------------------------------------------------------------
def _ratio64(case, from_h, to_h):
    """frame_ratio of pnmol_internal.hpp per state component: from the frame of from_h (0: raw) into that of to_h, fp64."""
    s_to, _ = scales(case.nu, to_h, np.float64)
    s_from = np.ones(case.n) if from_h == 0.0 else scales(case.nu, from_h, np.float64)[0]
    return np.tile(s_from / s_to, case.d)


def restate_predict(case, m, P, dt, from_h=0.0):
    """k_dn_predict / predict_block: P^h = ts ts^T . P, then A P^h A^T + Q and A m^h."""
    ts = _ratio64(case, from_h, dt)
    Ph = np.outer(ts, ts) * P
    return case.A @ (ts * flat(m)), case.A @ Ph @ case.A.T + case.Q


def restate_sweep(case, m, P, h, from_h=0.0):
    """The part of pnmol_smooth.hip the draws share: k_sm_build and the sweep [P-; P A^T; 0; I] -> [L; V; 0; T]."""
    ts = _ratio64(case, from_h, h)
    Ph = np.outer(ts, ts) * P
    PAt = Ph @ case.A.T
    Pm = case.A @ PAt + case.Q
    L = np.linalg.cholesky(Pm)
    V = scipy.linalg.solve_triangular(L, PAt.T, lower=True).T          # P A^T L^-T
    T = scipy.linalg.solve_triangular(L, np.eye(case.D), lower=True).T   # L^-T, explicit
    return types.SimpleNamespace(ts=ts, mh=ts * flat(m), Ph=Ph, Pm=Pm, L=L, V=V, T=T)


def restate_rts(case, filt, succ, h, from_h=0.0, succ_h=0.0):
    """pnmol_smooth.hip in its order: the sweep, G = V T^T, C = G Ps', Ps = P - V V^T + C G^T, ms = m + G (ms' - A m)."""
    w = restate_sweep(case, filt[0], filt[1], h, from_h)
    tsn = _ratio64(case, succ_h, h)
    msn, Psn = tsn * flat(succ[0]), np.outer(tsn, tsn) * succ[1]
    G = w.V @ w.T.T
    C = G @ Psn
    Ps = w.Ph - w.V @ w.V.T + C @ G.T
    ms = w.mh + G @ (msn - case.A @ w.mh)
    return types.SimpleNamespace(G=G, C=C, Ps=Ps, ms=ms, msn=msn, Psn=Psn, sweep=w)


def bridge_coefficients64(case, theta):
    """The coefficients as include/pnmol_hip.h ("Dense output") states them, in fp64: A_th, Q_th entry by entry,
    B+ = Q_th A_(1-th)^T Q1^-1, B- = (I - B+ A_(1-th)) A_th, Qb in Joseph form."""
    n, nu = case.n, case.nu
    p = nu - np.arange(n) + 0.5
    A1, Q1 = case.A1, case.LQ1 @ case.LQ1.T

    def part(th):
        return A1 * th ** (p[:, None] - p[None, :]), Q1 * th ** (p[:, None] + p[None, :])

    A_th, Q_th = part(theta)
    A_c, Q_c = part(1.0 - theta)
    Bp = np.linalg.solve(Q1, A_c @ Q_th).T
    M = np.eye(n) - Bp @ A_c
    return M @ A_th, Bp, M @ Q_th @ M.T + Bp @ Q_c @ Bp.T


def restate_bridge(case, r, theta):
    """k_dn_state: the bridge formula on the restated smoother's Ps_k, C_k and the successor."""
    Bm, Bp, Qb = bridge_coefficients64(case, theta)
    Bm, Bp = np.kron(np.eye(case.d), Bm), np.kron(np.eye(case.d), Bp)
    cross = Bm @ r.C @ Bp.T
    P = Bm @ r.Ps @ Bm.T + cross + cross.T + Bp @ r.Psn @ Bp.T + np.kron(case.gamma @ case.gamma.T, Qb)
    return Bm @ r.ms + Bp @ r.msn, P


def restate_draw(case, m, P):
    """pnmol_samples_draw with noise [0; I]: x = m + C e_i in the state's own (raw) coordinates, C = chol(P); the columns the test
    recovers are fl(fl(m + C e_i) - m), returned raw as (D, D)."""
    mf = flat(m)
    C = np.linalg.cholesky(P)
    return (mf[:, None] + C) - mf[:, None]


def restate_step_back_affine(case, filt, Xn_raw, h):
    """pnmol_samples_step_back with zero noise on the successor draws Xn_raw (D, S) raw: xt = m^h, r = tsn x' - A xt,
    x = xt + V (T^T r).  Frame of h, (D, S)."""
    w = restate_sweep(case, filt[0], filt[1], h)
    tsn = _ratio64(case, 0.0, h)
    R = tsn[:, None] * Xn_raw - (case.A @ w.mh)[:, None]
    return w.mh[:, None] + w.V @ (w.T.T @ R)


def restate_step_back_law(case, filt, xn_raw, h, scale=1.0):
    """pnmol_samples_step_back from one successor point with noise [0; I_2D]: xt = m^h + s C xi_1 (C = chol(P^h)),
    r = tsn x' - A xt - s Gamma_Q xi_2, x = xt + V (T^T r); returns the deviations of the 2D noisy columns from the noise-free
    one, frame of h, (D, 2D)."""
    w = restate_sweep(case, filt[0], filt[1], h)
    D = case.D
    C = np.linalg.cholesky(w.Ph)
    Xt = w.mh[:, None] + np.hstack((np.zeros((D, 1)), scale * C, np.zeros((D, D))))
    noise2 = np.hstack((np.zeros((D, 1 + D)), scale * case.Ql))
    R = (_ratio64(case, 0.0, h) * xn_raw)[:, None] - case.A @ Xt - noise2
    X = Xt + w.V @ (w.T.T @ R)
    return X[:, 1:] - X[:, :1]
