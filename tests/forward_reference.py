"""Stage reference of the forward step (`pnmol_filter_step`, `pnmol_filter_steps`): synthetic inputs, an extended-precision truth of
one step and of a chain of steps, and the fp64 restatement of the device's algebra.  NumPy and SciPy only, no GPU.
tests/test_forward_reference_host.py pins the truth against `oracle.attempt_step`, tests/test_gpu_forward_parity.py holds the
device to it on every entry of the state.  Frames, metrics, the refined solve and `bound` are those of tests/stage_reference.py.

Method (what differs from section 21)
  - Fixed mesh width.  The heat problem of `helpers.make_pair` with dx = 1/31 on the domain [0, (N - 1)/31], kappa = 0.05,
    h = 2^-7.  With dx = 1/(N - 1) the operator grows like N^2 and cond(S) like N^4 (at N = 287, nu = 2 the refined solve stalls
    above its floor); with a fixed dx the measurement operator still matters and S stays well conditioned at every N.
  - Inputs as in `stage_reference.synthetic_case`: W = U diag(lambda) U^T with Haar U in the frame of h, uploaded raw as
    P = (s s^T) . W.  Only a filtered state is drawn.
  - Truth of one step, `np.longdouble`, frame of h:  P- = A P A^T + Q, m- = A m;  H = E1 Pc - M E0 Pc stacked on B E0 Pc,
    z = H m- + [shift; 0];  S = H P- H^T + E E^T;  X = S^-1 H P-, v = S^-1 z by `_solve_refined`;  P = P- - (H P-)^T X,
    m = m- - (H P-)^T v;  sigma2_whitened = z^T v / m;  diffusion_squared_local = z^T (Ls^T Ls)^-1 z / m with the Cholesky factor
    Ls of S (quirk Q1: what `oracle.attempt_step` returns with canonical signs) from a column-wise longdouble Cholesky;  the
    error estimate h sqrt(diag Sq) sqrt(z^T Sq^-1 z / m), Sq = H Q H^T + E E^T, without the boundary rows.  H has a few
    non-zeros per row and derivative block, which the longdouble products use (`_rows_times`).
  - A chain of K steps starts each step from the previous step's truth (one frame: no rescaling between them).
  - Restatement, fp64 NumPy, in the order `launch_step` documents: ts ts^T . P;  A P A^T + Q;  G = [S; P- H^T];  Cholesky Ls,
    W = P- H^T Ls^-T, r = Ls^-1 z;  P = P- - W W^T, m = m- - W r.  A restated chain starts each step from the previous
    restated step, as the device does.
  - Yardstick of the scalars.  One realisation of a scalar can sit at 0 ulp from the truth by luck, so e64 of `sigma2_whitened`,
    `diffusion_squared_local`, `error_sigma2` and of the error estimate is the largest error over the restatement evaluated with
    the measurement rows in ORDERS random orders (seeded): the exact result does not depend on the row order, the summation order
    does.  `diffusion_squared_local` depends on the order through Ls, so each order's factor is brought back to THE factor of S
    by a QR (rows of the permuted factor un-permuted, R^T of its transpose with a positive diagonal): another fp64 route to the
    same exact Ls.

State order is the reference's: flat index j n + a is derivative a at mesh point j; means cross the API as (n, d)."""

import concurrent.futures
import functools
import os
import types

import numpy as np
import scipy.linalg

import stage_reference as sr
from helpers import make_pair
from stage_reference import LD, EPS, FACTOR, H, SEED, Frame, bound, cov_error, flat, kron_left, kron_right, tile_error_map, vec_error  # noqa: F401

DX = 1.0 / 31.0
KAPPA = 0.05
ORDERS = 8
NB = 32                       # column block of the sweep kernels
COND_S_MAX = {1: 1e7, 2: 1e7, 3: 1e10}    # input conditions (tests/test_forward_reference_host.py)
COND_PM_MAX = 1e4

# (N, nu, bcond): each the smallest shape on its side of a boundary of the sweep launch (m = N + 2 measurement rows,
# mp = round_up(m, 32), CB = mp / 32 column blocks, nreal = m - 32 (CB - 1) real columns in the last panel)
CASES = [
    (20, 1, "dirichlet"),    # m = 22, CB = 1: one column block, 12 padded points
    (30, 2, "neumann"),      # m = 32, CB = 1: full single block
    (31, 2, "dirichlet"),    # m = 33, CB = 2, nreal = 1: short last panel
    (38, 3, "dirichlet"),    # m = 40, CB = 2, nreal = 8: first non-short panel; n = 4: sweep_mode 1 with k_downdate
    (286, 1, "neumann"),     # m = 288, CB = 9: last k_sweep_rl<.., 9>
    (287, 2, "dirichlet"),   # m = 289, CB = 10, nreal = 1: first k_sweep_rl<.., 17>, short panel, n = 3 as in the headline
    (350, 1, "neumann"),     # m = 352, CB = 11: last shape without split rows of S in the XCD-local layout
    (351, 1, "dirichlet"),   # m = 353, CB = 12, nreal = 1: first shape with them
    (542, 1, "neumann"),     # m = 544, CB = 17: the headline's mp; last register-resident shape
    (543, 1, "dirichlet"),   # m = 545, CB = 18, nreal = 1: first left-looking k_sweep
]
# what the table above claims, checked against `shape` by the host test
TABLE = {(20, 1): (22, 1, 22), (30, 2): (32, 1, 32), (31, 2): (33, 2, 1), (38, 3): (40, 2, 8), (286, 1): (288, 9, 32),
         (287, 2): (289, 10, 1), (350, 1): (352, 11, 32), (351, 1): (353, 12, 1), (542, 1): (544, 17, 32), (543, 1): (545, 18, 1)}
DD_BIG_CASE = (126, 1, "neumann")   # dp = 128, Dp = 256, mp = 128: k_downdate_big with a diagonal and an off-diagonal 128-tile
FRAME_CASES = [CASES[2], CASES[3], CASES[5]]
LOOP_CASES = [CASES[0], CASES[2], CASES[5], CASES[7], CASES[8], CASES[3]]    # the last one is not fused (n = 4)
DIAGONAL_CASES = [CASES[2], CASES[5]]
DENSE_CASE = CASES[3]
SWEEP1_CASES = [CASES[2], CASES[5]]
LAYOUT_CASES = [CASES[0], CASES[5], CASES[6], CASES[7], CASES[8]]
DIAGONAL_FACTOR = 0.5         # j uniform in [-1, 1] * DIAGONAL_FACTOR * max|diag L|

case_id = sr.case_id


def shape(case):
    N, nu, _ = case
    m = N + 2
    mp, dp = (m + NB - 1) // NB * NB, (N + NB - 1) // NB * NB
    CB = mp // NB
    return dict(m=m, mp=mp, CB=CB, nreal=m - NB * (CB - 1), n=nu + 1, dp=dp, Dp=(nu + 1) * dp)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def problem(case):
    """Product and oracle problem and solver of a case (fresh objects)."""
    N, nu, bcond = case
    return make_pair(N, nu, H, 1, bcond, dx=DX, kappa=KAPPA, bbox=(0.0, (N - 1) / 31.0))


@functools.lru_cache(maxsize=None)
def forward_case(N, nu, bcond, seed=SEED):
    """The problem with one state `filt` that is well conditioned in the frame of h, raw (mean (n, d), covariance (D, D)) the way
    `pnmol_state_set` takes it.  Treat the result as read-only: it is shared."""
    pde, solver, opde, osolver = problem((N, nu, bcond))
    assert opde.L.shape == (N, N) and pde.L.shape == (N, N)
    # Everything the device is given comes from the PRODUCT's problem -- L, B, E_sqrtm, R_sqrtm and the Gram matrix K of its
    # spatial kernel (`pnmol_filter_desc.K`, used as it is: Q = Q1 (x) K) --, not from the oracle's: the two discretisations
    # agree to 1e-12 only (the uncertainty of a kernel stencil is a difference that cancels), which is an input, not a finding.
    # The oracle's problem takes the same arrays, so that `oracle.attempt_step` sees the same model.
    opde.L, opde.B, opde.E_sqrtm, opde.R_sqrtm = (np.array(x, dtype=np.float64) for x in (pde.L, pde.B, pde.E_sqrtm, pde.R_sqrtm))
    X = pde.mesh_spatial.points
    gram = np.asarray(solver.spatial_kernel(X, X.T), dtype=np.float64)
    gram = np.tril(gram) + np.tril(gram, -1).T                        # (the library mirrors the lower triangle)
    osolver.iwp, osolver.E0, osolver.E1, _ = osolver.initialize_iwp(opde)
    iwp = osolver.iwp
    A, _ = iwp.preconditioned_discretize
    A1, LQ1 = iwp.preconditioned_discretize_1d
    Pc, _ = iwp.nordsieck_preconditioner(H)
    n, d = nu + 1, N
    D = n * d
    s = np.diag(Pc).copy()
    rng = np.random.default_rng(seed)
    # (at nu = 3 the narrower range of stage_reference: cond(P-) grows towards cond(Q) = 2e4 with the full one)
    W, w = sr._frame_state(rng, D, sr.LAMBDA_FILT[(40, 3, "dirichlet")] if nu == 3 else sr.LAMBDA)
    P = np.outer(s, s) * W
    assert np.array_equal(P, P.T)
    E = scipy.linalg.block_diag(opde.E_sqrtm, opde.R_sqrtm)
    Q1 = 1.0 / (2 * n - 1 - np.add.outer(np.arange(n), np.arange(n)))         # flip(hilbert), rounded as the library rounds it
    c = types.SimpleNamespace(key=(N, nu, bcond), N=N, nu=nu, n=n, d=d, D=D, m=d + opde.B.shape[0], h=H, pde=pde, solver=solver,
                              opde=opde, osolver=osolver, A=A, Q=np.kron(gram, Q1), A1=A1, LQ1=LQ1, gram=gram, L=opde.L, B=opde.B,
                              E=E, filt=((s * w).reshape((n, d), order="F").copy(), P))
    # the model in extended precision: Q = Q1 (x) K with the exact Q1[a, b] = 1 / (2 nu + 1 - a - b)
    c.Kx, c.A1x = gram.astype(LD), A1.astype(LD)
    c.Q1x = LD(1.0) / (2 * n - 1 - np.add.outer(np.arange(n), np.arange(n))).astype(LD)
    c.Qx = np.kron(c.Kx, c.Q1x)
    c.EEtx = _rows_times(E.astype(LD), E.T.astype(LD))
    c.base = Operator(c, c.L, None, "base")
    return c


class Operator:
    """M (d, d) and shift (d,) of `pnmol_filter_set_operator`: H = [E1 Pc - M E0 Pc; B E0 Pc], z = H m- + [shift; 0]
    (include/pnmol_hip.h: "shift b = J_x m_at - f(t, m_at)", added to the residual).  Holds what depends on the operator alone."""

    def __init__(self, case, M, shift, tag):
        self.tag, self.M, self.shift = tag, np.asarray(M, dtype=np.float64), np.zeros(case.d) if shift is None else np.asarray(shift)
        self.Mx = self.M.astype(LD)
        self.zshift = np.concatenate((self.shift, np.zeros(case.m - case.d)))
        s, _ = sr.scales(case.nu, case.h, np.float64)
        H64 = np.zeros((case.m, case.D))
        H64[:case.d, 0::case.n] = -(s[0] * self.M)
        H64[np.arange(case.d), np.arange(case.d) * case.n + 1] = s[1]
        H64[case.d:, 0::case.n] = s[0] * case.B
        self.H64 = H64
        self._error_model = None


def diagonal_operator(case, factor=DIAGONAL_FACTOR, seed=SEED):
    """M = L + diag(j), j uniform in [-1, 1] * factor * max|diag L|, and a random shift: (Operator, j, shift)."""
    rng = np.random.default_rng(seed + 101)
    j = rng.uniform(-1.0, 1.0, case.d) * factor * np.abs(np.diag(case.L)).max()
    shift = rng.standard_normal(case.d)
    M = case.L.copy()
    M[np.arange(case.d), np.arange(case.d)] += j                     # (fp64, as the device adds it to the stencil's entry)
    op = Operator(case, M, shift, f"diagonal{factor}")
    op.Mx = case.L.astype(LD)
    op.Mx[np.arange(case.d), np.arange(case.d)] += j.astype(LD)      # (the truth: the exact sum)
    return op, j, shift


def dense_operator(case, factor=DIAGONAL_FACTOR, seed=SEED):
    """M = L + a dense perturbation with entries uniform in [-1, 1] * factor * max|diag L| / sqrt(d) (a matrix of the size of the
    diagonal one in the spectral norm), and a random shift."""
    rng = np.random.default_rng(seed + 202)
    M = case.L + rng.uniform(-1.0, 1.0, (case.d, case.d)) * factor * np.abs(np.diag(case.L)).max() / np.sqrt(case.d)
    return Operator(case, M, rng.standard_normal(case.d), f"dense{factor}")


# ---- longdouble products ----------------------------------------------------------------------------------------------------
_POOL = concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))


def _mm(A, B):
    """A @ B in longdouble (no BLAS for this type): row chunks of A on a thread pool, B in column-major order so that the inner
    loop runs over contiguous memory."""
    A, B = np.ascontiguousarray(A, dtype=LD), np.asfortranarray(B, dtype=LD)
    if A.shape[0] * A.shape[1] * (B.shape[1] if B.ndim == 2 else 1) < 2_000_000:
        return A @ B
    chunks = np.array_split(np.arange(A.shape[0]), 4 * _POOL._max_workers)
    return np.concatenate(list(_POOL.map(lambda r: A[r[0]:r[-1] + 1] @ B, [r for r in chunks if r.size])), axis=0)


def _rows_times(Mx, X):
    """Mx @ X for a longdouble Mx with few non-zeros per row (a stencil matrix): gathers, one per slot; dense otherwise."""
    nz = Mx != 0
    w = int(nz.sum(axis=1).max())
    if w > 8:
        return _mm(Mx, X)
    cols = np.argsort(~nz, axis=1, kind="stable")[:, :w]              # the non-zeros of a row first; padding slots hold zeros
    vals = np.take_along_axis(Mx, cols, axis=1)
    tail = (slice(None),) + (None,) * (X.ndim - 1)
    out = vals[:, 0][tail] * X[cols[:, 0]]
    for k in range(1, w):
        out = out + vals[:, k][tail] * X[cols[:, k]]
    return out


def h_apply(case, op, X):
    """H X for X (D,) or (D, c) in the frame of h, longdouble: H = s1 [I; 0] (x) e1^T + s0 [-M; B] (x) e0^T."""
    s, _ = sr.scales(case.nu, case.h)
    X0, X1 = X[0::case.n], X[1::case.n]
    return np.concatenate((s[1] * X1 - s[0] * _rows_times(op.Mx, X0), s[0] * _rows_times(case.B.astype(LD), X0)), axis=0)


def cholesky_ld(S):
    """Lower Cholesky factor in longdouble, column by column."""
    m = S.shape[0]
    L = np.zeros((m, m), dtype=LD)
    for j in range(m):
        col = S[j:, j] - L[j:, :j] @ L[j, :j]
        if not col[0] > 0:
            raise RuntimeError(f"forward_reference: pivot {j} is not positive")
        L[j:, j] = col / np.sqrt(col[0])
    return L


def _solve_upper_ld(U, b):
    x = np.zeros(b.shape, dtype=LD)
    for i in range(b.size - 1, -1, -1):
        x[i] = (b[i] - U[i, i + 1:] @ x[i + 1:]) / U[i, i]
    return x


# ---- extended-precision truth ---------------------------------------------------------------------------------------------
def error_model_truth(case, op, Qx=None, EEtx=None):
    """(Sq, diag Sq) of `estimate_error` for the operator, longdouble: Sq = H Q H^T + E E^T in the frame of h.  With the case's
    own Q and E E^T it is kept on the operator; with another process noise or measurement covariance (tests/sqrt_reference.py,
    which keeps its own per case and operator) it is computed and returned."""
    if Qx is None and EEtx is None:
        if op._error_model is None:
            HQ = h_apply(case, op, case.Qx)
            Sq = h_apply(case, op, np.ascontiguousarray(HQ.T)) + case.EEtx
            op._error_model = 0.5 * (Sq + Sq.T)
        return op._error_model
    HQ = h_apply(case, op, case.Qx if Qx is None else Qx)
    Sq = h_apply(case, op, np.ascontiguousarray(HQ.T)) + (case.EEtx if EEtx is None else EEtx)
    return 0.5 * (Sq + Sq.T)


def step_truth_frame(case, mh, Ph, op=None, Qx=None, EEtx=None, Sq=None):
    """One step from the state (mh (D,), Ph (D, D)) given in the frame of h, longdouble.  Qx, EEtx: the process noise and the
    measurement covariance E E^T of the model (default: the case's); Sq: `error_model_truth` of that model, where the caller
    has it already."""
    op = op or case.base
    mrows = case.m
    mm = kron_left(case.A1x, mh)
    Pm = kron_right(kron_left(case.A1x, Ph), case.A1x) + (case.Qx if Qx is None else Qx)
    Pm = 0.5 * (Pm + Pm.T)
    HP = h_apply(case, op, Pm)                                                   # (m, D)
    z = h_apply(case, op, mm) + op.zshift.astype(LD)
    S = h_apply(case, op, np.ascontiguousarray(HP.T)) + (case.EEtx if EEtx is None else EEtx)
    S = 0.5 * (S + S.T)
    X = _solve_refined(S, HP)
    v = _solve_refined(S, z)
    P = Pm - _mm(HP.T, X)
    m = mm - HP.T @ v
    Ls = cholesky_ld(S)
    r = _solve_upper_ld(Ls.T, z)                                                 # Ls^-T z: quirk Q1
    Sq = error_model_truth(case, op, Qx, EEtx) if Sq is None else Sq
    vq = _solve_refined(Sq, z)
    err_sigma2 = z @ vq / mrows
    return types.SimpleNamespace(mm=mm, Pm=Pm, z=z, S=S, m=m, P=0.5 * (P + P.T), sigma2_whitened=z @ v / mrows,
                                 diffusion_squared_local=r @ r / mrows, error_sigma2=err_sigma2,
                                 error=case.h * np.sqrt(np.diag(Sq)[:case.d]) * np.sqrt(err_sigma2))


def _solve_refined(Sm, Bm):
    """`stage_reference._solve_refined` with its longdouble residual product on the thread pool."""
    if Bm.ndim == 1 or Sm.shape[0] * Sm.shape[0] * Bm.shape[1] < 2_000_000:
        return sr._solve_refined(Sm, Bm)
    return sr._solve_refined(_PooledLeft(Sm), Bm)


class _PooledLeft:
    """A symmetric longdouble matrix whose `@` runs on the thread pool; what `stage_reference._solve_refined` asks of its matrix."""

    def __init__(self, Sm):
        self.Sm = Sm

    def astype(self, dtype):
        return self.Sm.astype(dtype)

    def __matmul__(self, X):
        return _mm(self.Sm, X)


def step_truth(case, m, P, h, op=None):
    """One step of size h (the case's) from the raw fp64 state (m (n, d), P (D, D))."""
    assert h == case.h
    fr = Frame(case, h)
    Ph = fr.cov(P)
    return step_truth_frame(case, fr.vec(m), 0.5 * (Ph + Ph.T), op)


@functools.lru_cache(maxsize=None)
def chain_truth(key, K=1, op_kind="base"):
    """K steps from the case's `filt`, each from the previous step's truth: a tuple of K step truths.  Cached per process; a longer
    chain reuses a shorter one's steps."""
    case = forward_case(*key)
    op = operator(key, op_kind)
    if K == 1:
        return (step_truth(case, *case.filt, case.h, op),)
    prev = chain_truth(key, K - 1, op_kind)
    return prev + (step_truth_frame(case, prev[-1].m, prev[-1].P, op),)


@functools.lru_cache(maxsize=None)
def operator(key, kind="base"):
    case = forward_case(*key)
    if kind == "base":
        return case.base
    if kind.startswith("diagonal"):
        return diagonal_operator(case, float(kind[8:] or DIAGONAL_FACTOR))[0]
    if kind.startswith("dense"):
        return dense_operator(case, float(kind[5:] or DIAGONAL_FACTOR))
    raise ValueError(kind)


# ---- fp64 restatement of the device's algebra ------------------------------------------------------------------------------
def _front(case, mh, Ph, op):
    """What does not depend on the order of the measurement rows: P-, m-, P- H^T, S, z."""
    mm = case.A @ mh
    Pm = case.A @ Ph @ case.A.T + case.Q
    PHt = Pm @ op.H64.T
    S = op.H64 @ PHt + case.E @ case.E.T
    z = op.H64 @ mm + op.zshift
    return types.SimpleNamespace(mm=mm, Pm=Pm, PHt=PHt, S=S, z=z)


def _error_model64(case, op):
    return op.H64 @ case.Q @ op.H64.T + case.E @ case.E.T


def _back(case, f, op, perm=None):
    """The factorisation and what follows it with the measurement rows in the order `perm`."""
    mrows = case.m
    p = np.arange(mrows) if perm is None else perm
    Ls = np.linalg.cholesky(f.S[np.ix_(p, p)])
    W = scipy.linalg.solve_triangular(Ls, f.PHt[:, p].T, lower=True).T
    r = scipy.linalg.solve_triangular(Ls, f.z[p], lower=True)
    out = types.SimpleNamespace(P=f.Pm - W @ W.T, m=f.mm - W @ r, sigma2_whitened=r @ r / mrows, Ls=Ls)
    # THE factor of S from this order's: S = B B^T with B = Ls[p^-1] (rows back in place), chol(S)^T = R of qr(B^T), diag > 0
    Bf = np.empty_like(Ls)
    Bf[p] = Ls
    R = np.linalg.qr(Bf.T, mode="r")
    R = R * np.where(np.diag(R) < 0, -1.0, 1.0)[:, None]
    r1 = scipy.linalg.solve_triangular(R, f.z, lower=False)
    out.diffusion_squared_local = r1 @ r1 / mrows
    Sq = _error_model64(case, op)
    Lq = np.linalg.cholesky(Sq[np.ix_(p, p)])
    rq = scipy.linalg.solve_triangular(Lq, f.z[p], lower=True)
    out.error_sigma2 = rq @ rq / mrows
    out.error = case.h * np.sqrt(np.diag(Sq)[:case.d]) * np.sqrt(out.error_sigma2)
    return out


def restate_step(case, m, P, h, from_h=0.0, op=None, perm=None):
    """One step from the raw state (or from one in the frame of from_h): ts ts^T . P first, then `_front` and `_back`."""
    op = op or case.base
    ts = sr._ratio64(case, from_h, h)
    return _back(case, _front(case, ts * flat(m), np.outer(ts, ts) * P, op), op, perm)


def restate_chain(case, K, op=None):
    """K restated steps from `filt`, each from the previous restated step (frame of h throughout)."""
    op = op or case.base
    out = [restate_step(case, *case.filt, case.h, 0.0, op)]
    for _ in range(K - 1):
        out.append(_back(case, _front(case, out[-1].m, out[-1].P, op), op))
    return out


SCALARS = ("sigma2_whitened", "diffusion_squared_local", "error_sigma2")


def rel_scalar(x, x_true):
    return float(abs(LD(x) - x_true) / abs(x_true))


def scalar_yardsticks(case, truth, mh, Ph, op=None, seed=SEED):
    """e64 of the three scalars and of the error estimate: the largest error over the restatement from the frame-of-h state
    (mh, Ph) with the measurement rows in ORDERS random orders."""
    op = op or case.base
    f = _front(case, mh, Ph, op)
    rng = np.random.default_rng(seed + 7)
    e = dict.fromkeys(SCALARS + ("error",), 0.0)
    for _ in range(ORDERS):
        q = _back(case, f, op, rng.permutation(case.m))
        for k in SCALARS:
            e[k] = max(e[k], rel_scalar(getattr(q, k), getattr(truth, k)))
        e["error"] = max(e["error"], vec_error(q.error, truth.error))
    return e


def frame64(case, m, P, h, from_h=0.0):
    """The raw fp64 state scaled into the frame of h in fp64 (what the restatement starts from)."""
    ts = sr._ratio64(case, from_h, h)
    return ts * flat(m), np.outer(ts, ts) * P
