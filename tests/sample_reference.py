"""Dense fp64 NumPy restatement of the joint posterior draw (`pnmol.white.*.sample`, `pnmol_samples_step_back`): the backward
recursion  x_T ~ N(m_T, P_T),  x_k | x_{k+1} ~ N(m_k + G_k (x_{k+1} - A m_k), P_k - G_k P-_k G_k^T)  by Matheron's rule, in the
Nordsieck frame of each step (pattern of smooth_reference.rts_step), returned as affine maps in raw coordinates."""

import numpy as np
import scipy.linalg


def psd_factor(P):
    """C with C C^T = P for a covariance that is PSD only up to rounding (negative eigenvalues clipped).  `eigh` runs on the
    correlation matrix: its error is eps of the LARGEST entry, and in the Nordsieck frame the variances of a state span many
    orders of magnitude (highest derivative's prior ~1e2 against a solution variance of 1e-18), so a factor of P itself would
    lose the small ones; scaled, the error of (C C^T)_ij is eps sqrt(P_ii P_jj), like a Cholesky factor's."""
    P = 0.5 * (P + P.T)
    s = np.sqrt(np.where(np.diag(P) > 0.0, np.diag(P), 1.0))
    w, U = np.linalg.eigh(P / np.outer(s, s))
    return s[:, None] * (U * np.sqrt(np.clip(w, 0.0, None)))


def sample_step(m, P, A, Q, Ql, Pc, Pcinv):
    """The affine map of one backward step on raw inputs:  x_k = a + G x_{k+1} + B xi,  xi = [xi_1 (D); xi_2 (cols of Ql)]:
    in the frame,  xt = m + C xi_1,  x_k = xt + G (x_{k+1} - A xt - Ql xi_2).  Returns (a, G, B) in raw coordinates."""
    mh, Ph = Pcinv @ m, Pcinv @ P @ Pcinv.T
    P_pred = A @ Ph @ A.T + Q
    G = scipy.linalg.cho_solve(scipy.linalg.cho_factor(P_pred, lower=True), A @ Ph).T  # P A^T (P-)^-1
    IGA = np.eye(len(m)) - G @ A
    B = np.hstack((IGA @ psd_factor(Ph), -G @ Ql))
    return Pc @ (IGA @ mh), Pc @ G @ Pcinv, Pc @ B


def maps_on_oracle(osolver, osol):
    """The chain over an oracle `solve()`: (m_T, C_T, [(a_k, G_k, B_k) for k = 0..T-1]), point-major state order, raw."""
    A, Ql = osolver.iwp.preconditioned_discretize
    Q = Ql @ Ql.T
    means = [mu.reshape(-1, order="F") for mu in osol.mean]
    covs = [C @ C.T for C in osol.cov_sqrtm]
    steps = []
    for k in range(len(means) - 1):
        Pc, Pcinv = osolver.iwp.nordsieck_preconditioner(osol.t[k + 1] - osol.t[k])
        steps.append(sample_step(means[k], covs[k], A, Q, Ql, Pc, Pcinv))
    return means[-1], psd_factor(covs[-1]), steps


def zero_noise_path(mT, steps):
    """The trajectory of the chain with all noise zero, (T+1, D)."""
    xs = [mT]
    for a, G, _ in reversed(steps):
        xs.append(a + G @ xs[-1])
    xs.reverse()
    return np.stack(xs)


def noise_maps(CT, steps):
    """M[j][k] (j <= k): the linear map from the noise of time point k to x_j;  M[T][T] = C_T, M[k][k] = B_k,
    M[j][k] = G_j M[j+1][k]."""
    T = len(steps)
    M = [dict() for _ in range(T + 1)]
    M[T][T] = CT
    for j in range(T - 1, -1, -1):
        _, G, B = steps[j]
        M[j][j] = B
        for k in range(j + 1, T + 1):
            M[j][k] = G @ M[j + 1][k]
    return M


def joint_covariance(CT, steps):
    """Covariance of the whole trajectory (x_0 .. x_T) implied by the chain, ((T+1) D, (T+1) D)."""
    T, D = len(steps), CT.shape[0]
    M = noise_maps(CT, steps)
    Sig = np.zeros(((T + 1) * D, (T + 1) * D))
    for i in range(T + 1):
        for j in range(i, T + 1):
            blk = sum(M[i][k] @ M[j][k].T for k in range(j, T + 1))
            Sig[i * D:(i + 1) * D, j * D:(j + 1) * D] = blk
            Sig[j * D:(j + 1) * D, i * D:(i + 1) * D] = blk.T
    return Sig


def marginal_covariances(CT, steps):
    """(T+1, D, D): the diagonal blocks of `joint_covariance`."""
    T = len(steps)
    M = noise_maps(CT, steps)
    return np.stack([sum(M[j][k] @ M[j][k].T for k in range(j, T + 1)) for j in range(T + 1)])


def increment_std(Ps, steps, n, d):
    """std of x_{j+1} - x_j per component, (T, n, d): the chain has Cov(x_j, x_{j+1}) = G_j Ps_{j+1}, so the increment has
    covariance Ps_j + Ps_{j+1} - G_j Ps_{j+1} - (G_j Ps_{j+1})^T  (Ps: the RTS covariances, raw)."""
    out = []
    for j, (_, G, _) in enumerate(steps):
        X = G @ Ps[j + 1]
        V = np.diag(Ps[j] + Ps[j + 1] - X - X.T)
        out.append(np.sqrt(np.maximum(V, 0.0)).reshape((n, d), order="F"))
    return np.stack(out)


def run_chain(mT, CT, steps, noise):
    """Draws of the chain for given noise: noise[k] (S, width of B_k) for k < T, noise[T] (S, D); returns (S, T+1, D)."""
    xs = [mT + noise[-1] @ CT.T]
    for k in range(len(steps) - 1, -1, -1):
        a, G, B = steps[k]
        xs.append(a + xs[-1] @ G.T + noise[k] @ B.T)
    xs.reverse()
    return np.stack(xs, axis=1)


# ---- the device generator, restated (include/pnmol_hip.h, "Generator") -------------------------------------------------------
def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays of uint32: counter (..., 4), key (2,) -> (..., 4)."""
    c = [np.asarray(counter[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack(c, axis=-1).astype(np.uint32)


def device_noise(seed, step_index, rows, cols):
    """(rows, cols) standard normals: the map (seed, step_index, draw i, column) -> double of the device generator."""
    npairs = (cols + 1) // 2
    ctr = np.zeros((rows, npairs, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(npairs)[None, :]
    ctr[..., 1] = np.arange(rows)[:, None]
    ctr[..., 2] = step_index & 0xFFFFFFFF
    ctr[..., 3] = step_index >> 32
    w = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).astype(np.uint64)
    u1 = ((w[..., 0] + ((w[..., 1] & np.uint64(0xFFFFF)) << np.uint64(32))).astype(np.float64) + 0.5) * 2.0 ** -52
    u2 = ((w[..., 2] + ((w[..., 3] & np.uint64(0xFFFFF)) << np.uint64(32))).astype(np.float64) + 0.5) * 2.0 ** -52
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.stack((r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)), axis=-1).reshape(rows, 2 * npairs)
    return z[:, :cols]
