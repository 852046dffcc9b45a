"""Stage reference of the square-root filter step (`pnmol_sqrt_filter_step`, `pnmol_sqrt_filter_steps`, csrc/pnmol_sqrt.hip): the
cases at the shape boundaries of its QRs, the inputs as uploaded FACTORS, an extended-precision truth of one step and of a chain,
and the fp64 (fp32) restatement of the device's algebra.  NumPy and SciPy only, no GPU.  tests/test_sqrt_reference_host.py asserts
the input conditions and the branch table and pins the truth against the oracle; tests/test_gpu_sqrt_parity.py holds the device
to the truth on the whole state.  Inputs, frames, metrics, the truth of a step and `bound` are those of
tests/forward_reference.py and tests/stage_reference.py.

Method (what differs from section 23)
  - The upload is a factor.  C_tri = cholesky(P) of the synthetic state of `forward_case` (lower triangular: the structured
    member lists of the predict QR), C_dense = C_tri Qo with a seeded Haar Qo (the dense lists).  The truth starts from what is
    uploaded: P_in = C C^T formed in longdouble from the fp64 factor.
  - The filter is made from the product problem's L, B, E_sqrtm, R_sqrtm and Gamma = cholesky(gram); the truth's process noise is
    (Gamma Gamma^T) (x) Q1 in longdouble from that Gamma (rounding of inputs is not counted).
  - The truth of a step is `forward_reference.step_truth_frame`: the posterior does not depend on the algorithm.
  - Yardstick.  The restatement repeats the device's algebra in the frame of h with `numpy.linalg.qr`, by two routes to the same
    exact R: as written (R of [(A Cl)^T; Ql^T], then R of [[R H^T, R], [E^T, 0]]) and the one-QR route (Rc of
    [[Ql^T H^T, Ql^T], [E^T, 0]], then R of [[T1^T H^T, T1^T], [Rc]]).  From R = [[R1, R2], [0, R3]]: y = R1^-T z,
    m = m- - R2^T y, C = R3^T with a non-negative diagonal.  e64 of a quantity is the larger error of the two routes; for a
    scalar, the largest over the two routes and ORDERS seeded permutations of the measurement rows (columns of the first block
    column of the pre-array).  The fp32 build: both pre-arrays rounded to float32 and the QRs in float32, everything else fp64.
  - No comparison of factor entries: the posterior is singular to working precision (the PDE rows have a noise of 1e-8), so a
    triangular factor is defined to cond * eps only; C C^T is compared, the product in longdouble from the fp64 factor.
  - The correlation-scaled metric |dP_ij| / sqrt(P_ii P_jj) over the indices whose true variance exceeds 1e-12 of the largest:
    every entry to its own scale.  Which indices that excludes is a condition (`excluded_indices`), not a measurement.

State order is the reference's: flat index j n + a is derivative a at component j; means cross the API as (n, ds)."""

import functools
import types

import numpy as np
import scipy.linalg

import forward_reference as fw
import stage_reference as sr
from forward_reference import (LD, EPS, FACTOR, ORDERS, SEED, COND_S_MAX, Frame, Operator, bound, case_id, cov_error, flat,  # noqa: F401
                               forward_case, rel_scalar, vec_error)

EPS32 = 2.0 ** -23
QB, FAN, SQ_ELLW = 32, 8, 8        # csrc/pnmol_sqrt.hip: panel width = row-block height, members per chunk, ELL width limit
VAR_FLOOR = 1e-12                  # the scaled metric runs over the indices with P_ii > VAR_FLOOR max diag P

# (N, nu, bcond): D = n N, m = N + 2, Dtop = round_up(D, 32), nb2 = ceil((D + m) / 32) row blocks of the update QR
CASES = [
    (20, 1, "dirichlet"),    # one level everywhere; Dtop = 64 > D; m < 32; the one-QR list never reaches p >= stacked_tri
    (30, 2, "neumann"),      # m = 32: full single diagonal block of k_sq_trsv; first shape with p >= stacked_tri
    (31, 2, "dirichlet"),    # m = 33: second diagonal block of one row
    (32, 1, "neumann"),      # D mod 32 = 0: Dtop = D
    (38, 3, "dirichlet"),    # n = 4 = SQN; cond(S) = 1.2e9
    (84, 1, "neumann"),      # nb2 = 8: last one-level update QR
    (85, 1, "dirichlet"),    # nb2 = 9: first two-level update QR
    (100, 2, "neumann"),     # two levels in the structured predict QR (from panel 6 on) and in the one-QR step
    (682, 1, "neumann"),     # nb2 = 64: last two-level update QR
    (683, 1, "dirichlet"),   # nb2 = 65: first three-level update QR
]
# (D, m, D + m, nb2) as the table of DESIGN.md section 26 states them, checked against `shape` by the host test
TABLE = {(20, 1): (40, 22, 62, 2), (30, 2): (90, 32, 122, 4), (31, 2): (93, 33, 126, 4), (32, 1): (64, 34, 98, 4),
         (38, 3): (152, 40, 192, 6), (84, 1): (168, 86, 254, 8), (85, 1): (170, 87, 257, 9), (100, 2): (300, 102, 402, 13),
         (682, 1): (1364, 684, 2048, 64), (683, 1): (1366, 685, 2051, 65)}
_BY = {c[:2]: c for c in CASES}
LARGE_CASES = [_BY[(682, 1)], _BY[(683, 1)]]                     # only in the first step and the one-QR step
DENSE_FIRST_CASES = [_BY[(31, 2)], _BY[(85, 1)], _BY[(100, 2)]]
DENSE_ONE_QR_CASES = [_BY[(31, 2)], _BY[(100, 2)]]
LOOP_CASES = [_BY[(20, 1)], _BY[(31, 2)], _BY[(38, 3)], _BY[(85, 1)], _BY[(100, 2)]]
OPERATOR_CASES = [(_BY[(31, 2)], "diagonal"), (_BY[(100, 2)], "diagonal"), (_BY[(38, 3)], "dense"), (_BY[(31, 2)], "band7"),
                  (_BY[(31, 2)], "band8")]
SWITCH_CASES = [_BY[(85, 1)], _BY[(100, 2)]]
SWITCHES = [("PNMOL_SQRT_ONE_QR", "0"), ("PNMOL_SQRT_ELL", "0"), ("PNMOL_QR_FUSE", "0"), ("PNMOL_QR_INLOOP", "0"),
            ("PNMOL_QR_OWNER", "0"), ("PNMOL_QR_PRE", "1")]
F32_CASES = [_BY[(31, 2)], _BY[(85, 1)], _BY[(100, 2)]]
LOOP_STEPS = 3


# ---- the member-list arithmetic of `qr_inplace` ---------------------------------------------------------------------------------
def _round_up(x, q=QB):
    return (x + q - 1) // q * q


def levels(cnt):
    """Tree levels of a panel with `cnt` members (`qr_launch_panel`: chunks of FAN members, level after level, until one is left)."""
    lvl, s = 1, 1
    while ((cnt + s - 1) // s + FAN - 1) // FAN > 1:
        lvl, s = lvl + 1, s * FAN
    return lvl


def member_counts(rows, cols, tri_bot0=0, stacked_tri=0):
    """(cnt, in_triangle) per panel of the QR of a rows x cols work matrix: the three `MemberMap` branches of `qr_inplace`."""
    ld = _round_up(cols)
    nrb, ncb = _round_up(max(rows, ld)) // QB, ld // QB
    out = []
    for p in range(ncb):
        if stacked_tri > 0:
            nbot = nrb - stacked_tri
            if p < stacked_tri:
                out.append((stacked_tri - p + min(p + 1, nbot), False))
            else:
                out.append((min(p, nbot - 1) - (p - stacked_tri) + 1, True))
        elif tri_bot0 > 0:
            out.append((min(2, tri_bot0 - p) + min(p + 1, nrb - tri_bot0), False))
        else:
            out.append((nrb - p, False))
    return out


def shape(case):
    """What the launch of a step depends on: sizes, the member counts of each QR's panels and their tree levels."""
    N, nu, _ = case
    n, m = nu + 1, N + 2
    D = n * N
    Dtop, ld2 = _round_up(D), _round_up(D + m)
    qrs = dict(predict_tri=member_counts(Dtop + D, D, tri_bot0=Dtop // QB), predict_dense=member_counts(Dtop + D, D),
               update=member_counts(D + m, m + D), one_qr=member_counts(Dtop + ld2, m + D, stacked_tri=Dtop // QB),
               error_model=member_counts(D + m, m))
    return dict(n=n, m=m, D=D, Dtop=Dtop, nb2=ld2 // QB, solve_blocks=(m + QB - 1) // QB, qrs=qrs,
                levels={k: max(levels(c) for c, _ in v) for k, v in qrs.items()},
                in_triangle=[p for p, (_, tri) in enumerate(qrs["one_qr"]) if tri])


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sqrt_case(N, nu, bcond):
    """The forward case with what the square-root filter is given: Gamma, both factors of the synthetic covariance, and the model
    in the frame of h as the device forms it.  Treat the result as read-only: it is shared."""
    c = forward_case(N, nu, bcond)
    Gamma = np.linalg.cholesky(c.gram)
    C_tri = np.linalg.cholesky(c.filt[1])
    assert np.all(np.triu(C_tri, 1) == 0)
    Qo = sr._haar(np.random.default_rng(SEED + 303), c.D)
    n = c.n
    Q1 = 1.0 / (2 * n - 1 - np.add.outer(np.arange(n), np.arange(n)))
    s64 = np.tile(sr.scales(nu, c.h, np.float64)[0], c.d)
    g = Gamma.astype(LD)
    sc = types.SimpleNamespace(key=(N, nu, bcond), c=c, Gamma=Gamma, mean=c.filt[0], factors=dict(tri=C_tri, dense=C_tri @ Qo),
                               s64=s64, QlT=np.kron(Gamma, np.linalg.cholesky(Q1)).T.copy(), Qx=np.kron(fw._mm(g, g.T), c.Q1x))
    return sc


def resolve(key):
    """The case of a key: (N, nu, bcond) white-noise model, (N, nu, bcond, "latent") latent-force model."""
    return latent_case(*key) if len(key) == 4 else sqrt_case(*key)


def filter_arguments(sc):
    """Keyword arguments of `pnmol._hip.SqrtFilter` for the case."""
    if hasattr(sc, "filter_arguments"):
        return sc.filter_arguments
    pde = sc.c.pde
    return dict(L=pde.L, B=pde.B, E_sqrtm=pde.E_sqrtm, R_sqrtm=pde.R_sqrtm, Gamma=sc.Gamma, num_derivatives=sc.c.nu)


@functools.lru_cache(maxsize=None)
def operator(key, kind="base"):
    """The operators of the tests as (d, d) matrices M with a shift, as `set_operator` takes them; the truth uses the uploaded M."""
    if len(key) == 4:
        assert kind == "base"
        return latent_case(*key).c.base
    c = forward_case(*key)
    if kind == "base":
        return c.base
    if kind == "diagonal":
        op = fw.diagonal_operator(c)[0]
        return Operator(c, op.M, op.shift, kind)
    if kind == "dense":
        op = fw.dense_operator(c)
        return Operator(c, op.M, op.shift, kind)
    if kind in ("band7", "band8"):
        # L and a perturbation on the band |i - j| <= 3 (7 entries a row, 8 in H with the derivative entry: the gather kernels at
        # full width), or with the entry j = i + 4 (mod d) as well (9 in H: past SQ_ELLW, the dense kernels)
        rng = np.random.default_rng(SEED + 404)
        i, j = np.indices((c.d, c.d))
        band = np.abs(i - j) <= 3
        if kind == "band8":
            band |= (j - i) % c.d == 4
        assert np.all(band[c.L != 0])
        M = c.L + band * rng.uniform(-1.0, 1.0, (c.d, c.d)) * fw.DIAGONAL_FACTOR * np.abs(np.diag(c.L)).max() / np.sqrt(7.0)
        return Operator(c, M, rng.standard_normal(c.d), kind)
    raise ValueError(kind)


def row_width(op):
    """Longest row of H in non-zeros: up to SQ_ELLW the step runs the gather kernels, above it the dense products."""
    return int((op.H64 != 0).sum(axis=1).max())


# ---- extended-precision truth ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def uploaded_state(key, factor="tri"):
    """(m, P) in the frame of h, longdouble, of the uploaded (mean, factor): P = C C^T from the fp64 factor."""
    sc = resolve(key)
    fr = Frame(sc.c, sc.c.h)
    Cx = fr.flat(sc.factors[factor])
    P = fw._mm(Cx, np.ascontiguousarray(Cx.T))
    return fr.vec(sc.mean), 0.5 * (P + P.T)


@functools.lru_cache(maxsize=None)
def _error_model(key, op_kind):
    """Sq = H Q H^T + E E^T of the case's model with the uploaded Gamma, longdouble: once per case and operator."""
    sc = sqrt_case(*key)
    return fw.error_model_truth(sc.c, operator(key, op_kind), Qx=sc.Qx)


@functools.lru_cache(maxsize=None)
def chain_truth(key, K=1, factor="tri", op_kind="base"):
    """K steps from the uploaded state, each from the previous step's truth: a tuple of K step truths.  Cached per process."""
    sc = resolve(key)
    op = operator(key, op_kind)
    step = (lambda mh, Ph: dense_step_truth(sc.c, op, sc.Qx, mh, Ph)) if len(key) == 4 else \
        (lambda mh, Ph: fw.step_truth_frame(sc.c, mh, Ph, op, Qx=sc.Qx, Sq=_error_model(key, op_kind)))
    if K == 1:
        return (step(*uploaded_state(key, factor)),)
    prev = chain_truth(key, K - 1, factor, op_kind)
    return prev + (step(prev[-1].m, prev[-1].P),)


def excluded_indices(P_true):
    """Flat indices whose true variance is at most VAR_FLOOR of the largest: left out of the scaled metric."""
    dg = np.diag(P_true)
    return np.flatnonzero(~(dg > VAR_FLOOR * dg.max()))


def scaled_error(X, P_true):
    """max |X_ij - P_ij| / sqrt(P_ii P_jj) over the kept indices."""
    dg = np.diag(P_true)
    keep = dg > VAR_FLOOR * dg.max()
    sd = np.sqrt(dg[keep])
    return float((np.abs(np.asarray(X)[np.ix_(keep, keep)] - P_true[np.ix_(keep, keep)]) / np.outer(sd, sd)).max())


def factor_cov(case, C_raw, fr=None):
    """C C^T in the frame of h, the product in longdouble from the raw fp64 factor (what a read-back factor stands for)."""
    Cx = (fr or Frame(case, case.h)).flat(C_raw)
    return fw._mm(Cx, np.ascontiguousarray(Cx.T))


# ---- the latent-force layout (ds = 2d) --------------------------------------------------------------------------------------------
# L = [L, I], B = [B, 0], Gamma = blockdiag(chol K, E_sqrtm), zero noise factors: the update is `update_sqrt_no_meascov`.
# Keys carry a fourth entry "latent"; `resolve`, `operator`, `chain_truth` and `yardsticks` take both kinds of key.
LATENT_CASES = [(24, 2, "neumann", "latent"),      # D = 144
                (43, 1, "dirichlet", "latent")]    # D = 172, m = 45, D mod 32 != 0


def dense_step_truth(c, op, Qx, mh, Ph):
    """One step of a model given by dense matrices, longdouble, frame of h: A = c.Ax, Q = Qx, H = op.Hx, E E^T = c.EEtx."""
    mm = c.Ax @ mh
    Pm = c.Ax @ Ph @ c.Ax.T + Qx
    Pm = 0.5 * (Pm + Pm.T)
    HP = op.Hx @ Pm
    z = op.Hx @ mm + op.zshift.astype(LD)
    S = HP @ op.Hx.T + c.EEtx
    S = 0.5 * (S + S.T)
    X, v = sr._solve_refined(S, HP), sr._solve_refined(S, z)
    P = Pm - HP.T @ X
    Ls = fw.cholesky_ld(S)
    r = fw._solve_upper_ld(Ls.T, z)
    Sq = op.Hx @ Qx @ op.Hx.T + c.EEtx
    Sq = 0.5 * (Sq + Sq.T)
    err_sigma2 = z @ sr._solve_refined(Sq, z) / c.m
    return types.SimpleNamespace(mm=mm, Pm=Pm, z=z, S=S, m=mm - HP.T @ v, P=0.5 * (P + P.T), sigma2_whitened=z @ v / c.m,
                                 diffusion_squared_local=r @ r / c.m, error_sigma2=err_sigma2,
                                 error=c.h * np.sqrt(np.diag(Sq)[:c.npde]) * np.sqrt(err_sigma2))


@functools.lru_cache(maxsize=None)
def latent_case(N, nu, bcond, tag="latent", seed=SEED):
    """The latent-force model of the case's heat problem with a synthetic state over all n * 2d components that is well conditioned
    in the frame of h; the same fields as `sqrt_case`, the case `c` with d = 2d state components and `npde` = d PDE rows."""
    b = forward_case(N, nu, bcond)
    d, n, nB = b.d, b.n, b.B.shape[0]
    ds, m = 2 * d, b.m
    D = n * ds
    Es = np.asarray(b.pde.E_sqrtm, dtype=np.float64)
    Gamma = scipy.linalg.block_diag(np.linalg.cholesky(b.gram), Es)
    assert np.all(np.triu(Gamma, 1) == 0)                                 # (the filter reads the lower triangle)
    M, B = np.hstack((b.L, np.eye(d))), np.hstack((b.B, np.zeros((nB, d))))
    H = {}
    for dtype in (np.float64, LD):
        s, _ = sr.scales(nu, b.h, dtype)
        Hm = np.zeros((m, D), dtype=dtype)
        Hm[:d, 0::n] = -(s[0] * M.astype(dtype))
        Hm[np.arange(d), np.arange(d) * n + 1] += s[1]
        Hm[d:, 0::n] = s[0] * B.astype(dtype)
        H[dtype] = Hm
    op = types.SimpleNamespace(tag="base", M=M, shift=None, H64=H[np.float64], Hx=H[LD], zshift=np.zeros(m))
    s64 = np.tile(sr.scales(nu, b.h, np.float64)[0], ds)
    W, w = sr._frame_state(np.random.default_rng(seed + 505), D, sr.LAMBDA)
    P = np.outer(s64, s64) * W
    Q1 = 1.0 / (2 * n - 1 - np.add.outer(np.arange(n), np.arange(n)))
    c = types.SimpleNamespace(key=(N, nu, bcond, tag), N=N, nu=nu, n=n, d=ds, npde=d, D=D, m=m, h=b.h, A=np.kron(np.eye(ds), b.A1),
                              Ax=np.kron(np.eye(ds).astype(LD), b.A1x), E=np.zeros((m, m)),
                              EEtx=np.zeros((m, m), dtype=LD), base=op, opde=b.opde)
    g = Gamma.astype(LD)
    return types.SimpleNamespace(key=c.key, c=c, Gamma=Gamma, mean=(s64 * w).reshape((n, ds), order="F").copy(),
                                 factors=dict(tri=np.linalg.cholesky(P)), s64=s64, QlT=np.kron(Gamma, np.linalg.cholesky(Q1)).T.copy(),
                                 Qx=np.kron(g @ g.T, b.Q1x),
                                 filter_arguments=dict(L=M, B=B, E_sqrtm=np.zeros((d, d)), R_sqrtm=np.zeros((nB, nB)), Gamma=Gamma,
                                                       num_derivatives=nu))


# ---- restatement of the device's algebra ----------------------------------------------------------------------------------------
def _qr_r(X):
    return np.linalg.qr(X, mode="r")


def _wt(dtype):
    return np.float32 if dtype == "f32" else np.float64


def _front(sc, mean_flat_raw, C_raw, op):
    """k_sq_mean, k_sq_rows, k_sq_gemv_z: m- = A Pinv m, T1 = A Pinv Cl, z = H m- + shift."""
    pinv = 1.0 / sc.s64
    mm = sc.c.A @ (pinv * mean_flat_raw)
    T1 = sc.c.A @ (pinv[:, None] * C_raw)
    return types.SimpleNamespace(mm=mm, T1=T1, z=op.H64 @ mm + op.zshift)


@functools.lru_cache(maxsize=None)
def _invariant(key, op_kind, dtype):
    """Rc: R of the rows of the stacked pre-array that do not depend on the state, and the first block column it came from."""
    sc, op = resolve(key), operator(key, op_kind)
    c, W = sc.c, _wt(dtype)
    pre = np.zeros((c.D + c.m, c.m + c.D), dtype=W)
    pre[:c.D, :c.m] = sc.QlT @ op.H64.T
    pre[:c.D, c.m:] = sc.QlT
    pre[c.D:, :c.m] = c.E.T
    return _qr_r(pre), pre[:, :c.m].copy()


def _stacked_r(sc, f, op, route, dtype):
    """R = [[R1, R2], [0, R3]] of the step by one of the two routes, in the work type."""
    c, W = sc.c, _wt(dtype)
    if route == "two":
        R = _qr_r(np.vstack((f.T1.T, sc.QlT)).astype(W))
        pre = np.zeros((c.D + c.m, c.m + c.D), dtype=W)
        pre[:c.D, :c.m] = R.astype(np.float64) @ op.H64.T
        pre[:c.D, c.m:] = R
        pre[c.D:, :c.m] = c.E.T
        return _qr_r(pre), pre[:, :c.m]
    Rc, _ = _invariant(sc.key, op.tag, dtype)
    pre = np.vstack((np.hstack(((f.T1.T @ op.H64.T).astype(W), f.T1.T.astype(W))), Rc))
    return _qr_r(pre)[:c.m + c.D], None


def _solves(c, R1, z):
    """k_sq_trsv: |R1^-T z|^2 / m and |R1c^-1 z|^2 / m, R1c = R1 with rows flipped to a positive diagonal; y = R1^-T z."""
    y = scipy.linalg.solve_triangular(R1, z, trans="T", lower=False)
    x = scipy.linalg.solve_triangular(R1 * np.where(np.diag(R1) < 0, -1.0, 1.0)[:, None], z, lower=False)
    return y, y @ y / c.m, x @ x / c.m


def restate_step(sc, mean_flat_raw, C_raw, op, route, dtype="f64"):
    """One step from the raw state by `route` ("two": as written; "one": the one-QR step).  mean (D,) and factor (D, D) come
    back RAW, as the device stores them (k_sq_mean_update, k_sq_state_out scale by the Nordsieck factors in fp64)."""
    c = sc.c
    f = _front(sc, mean_flat_raw, C_raw, op)
    R, _ = _stacked_r(sc, f, op, route, dtype)
    R = R.astype(np.float64)
    R1, R2, R3 = R[:c.m, :c.m], R[:c.m, c.m:], R[c.m:, c.m:]
    y, s2w, dsl = _solves(c, R1, f.z)
    C = (R3 * np.where(np.diag(R3) < 0, -1.0, 1.0)[:, None]).T
    return types.SimpleNamespace(mean=sc.s64 * (f.mm - R2.T @ y), C=sc.s64[:, None] * C, sigma2_whitened=s2w,
                                 diffusion_squared_local=dsl)


def _scalars_in_orders(sc, f, op, dtype, seed=SEED):
    """sigma2_whitened, diffusion_squared_local, error_sigma2 and the error estimate with the measurement rows in ORDERS random
    orders: only the first block column of the pre-arrays enters R1 (and Rq)."""
    c, W = sc.c, _wt(dtype)
    R = _qr_r(np.vstack((f.T1.T, sc.QlT)).astype(W))
    col = np.vstack(((R.astype(np.float64) @ op.H64.T).astype(W), c.E.T.astype(W)))
    colq = _invariant(sc.key, op.tag, dtype)[1]
    rng = np.random.default_rng(seed + 7)
    out = []
    for k in range(ORDERS + 1):
        p = np.arange(c.m) if k == 0 else rng.permutation(c.m)
        R1 = _qr_r(col[:, p]).astype(np.float64)
        _, s2w, _ = _solves(c, R1, f.z[p])
        Bf = np.empty_like(R1)
        Bf[p] = R1.T                                                  # S = Bf Bf^T with the rows back in place
        _, _, dsl = _solves(c, _qr_r(Bf.T), f.z)
        Rq = _qr_r(colq[:, p]).astype(np.float64)
        _, esig, _ = _solves(c, Rq, f.z[p])
        sqd = np.empty(c.m)
        sqd[p] = (Rq * Rq).sum(axis=0)
        out.append(dict(sigma2_whitened=s2w, diffusion_squared_local=dsl, error_sigma2=esig,
                        error=c.h * np.sqrt(sqd[:getattr(c, "npde", c.d)]) * np.sqrt(esig)))
    return out


SCALARS = ("sigma2_whitened", "diffusion_squared_local", "error_sigma2")
QUANTITIES = ("cov", "scaled", "mean", "mean0", "var0") + SCALARS + ("error",)


def state_errors(c, truth, mean_flat_raw, C_raw, fr=None):
    """The figures of a raw (mean, factor) against a step truth: whole covariance, scaled covariance, whole mean, and the two
    read-outs of the loop (derivative-0 mean in the metric of the mean, derivative-0 variance in that of the covariance)."""
    fr = fr or Frame(c, c.h)
    P = factor_cov(c, C_raw, fr)
    mh = fr.flat(mean_flat_raw)
    return dict(cov=cov_error(P, truth.P), scaled=scaled_error(P, truth.P), mean=vec_error(mh, truth.m),
                mean0=float(np.abs(mh[0::c.n] - truth.m[0::c.n]).max() / np.abs(truth.m).max()),
                var0=float(np.abs(np.diag(P)[0::c.n] - np.diag(truth.P)[0::c.n]).max() / np.abs(truth.P).max()))


@functools.lru_cache(maxsize=None)
def yardsticks(key, K=1, factor="tri", op_kind="base", dtype="f64"):
    """Per step of the chain the yardstick (e64, or e32 for dtype "f32") of every quantity in QUANTITIES: the larger error of the
    two routes from the same start, for the scalars the largest over the routes and the row orders.  The restated chain goes on
    from the route the device takes (step 0: two QRs, then the one-QR step)."""
    sc, op = resolve(key), operator(key, op_kind)
    c = sc.c
    truths = chain_truth(key, K, factor, op_kind)
    fr = Frame(c, c.h)
    state = (flat(sc.mean), sc.factors[factor])
    out = []
    for k, t in enumerate(truths):
        routes = {r: restate_step(sc, *state, op, r, dtype) for r in ("two", "one")}
        e = dict.fromkeys(QUANTITIES, 0.0)
        for q in routes.values():
            for name, v in state_errors(c, t, q.mean, q.C, fr).items():
                e[name] = max(e[name], v)
            for name in SCALARS[:2]:
                e[name] = max(e[name], rel_scalar(getattr(q, name), getattr(t, name)))
        for s in _scalars_in_orders(sc, _front(sc, *state, op), op, dtype):
            for name in SCALARS:
                e[name] = max(e[name], rel_scalar(s[name], getattr(t, name)))
            e["error"] = max(e["error"], vec_error(s["error"], t.error))
        out.append(e)
        nxt = routes["two" if k == 0 else "one"]
        state = (nxt.mean, nxt.C)
    return tuple(out)


def bound_for(e, dtype="f64"):
    """`bound` with the floor of the QR's number format: FACTOR max(e64, 2^-52), or FACTOR max(e32, 2^-23) for the fp32 QR."""
    return bound(e) if dtype == "f64" else FACTOR * max(float(e), EPS32)
