"""The NumPy chain the GPU sampler is checked against (tests/sample_reference.py), pinned on the CPU: its zero-noise path and
its implied marginals against the RTS pass (smooth_reference.rts_on_oracle), its full joint covariance against joint Gaussian
conditioning of a whole short trajectory; the restated generator against Philox's published test vectors; the import surface."""

import numpy as np
import pytest
import scipy.linalg

from helpers import assert_mean_std_parity, make_pair
from sample_reference import (device_noise, joint_covariance, maps_on_oracle, marginal_covariances, philox4x32_10, run_chain,
                              zero_noise_path)
from smooth_reference import marginal_std, rts_on_oracle


@pytest.mark.parametrize("nu", [1, 2, 3])
@pytest.mark.parametrize("bcond", ["dirichlet", "neumann"])
def test_chain_has_the_rts_marginals(nu, bcond):
    """Zero noise gives the RTS means; sum_k M_jk M_jk^T gives the RTS stds (north-star tolerances)."""
    _, _, opde, osolver = make_pair(32, nu, 2.0 ** -7, 12, bcond)
    osol = osolver.solve(opde)
    ms, Ps = rts_on_oracle(osolver, osol)
    n, d = osol.mean.shape[1:]
    mT, CT, steps = maps_on_oracle(osolver, osol)
    path = zero_noise_path(mT, steps).reshape((-1, d, n)).transpose(0, 2, 1)
    std = marginal_std(marginal_covariances(CT, steps), n, d)
    ostd = marginal_std(Ps, n, d)
    err = np.abs(std[:, 0] - ostd[:, 0]).max() / ostd[:, 0].max()
    print(f"nu={nu} {bcond}: largest std error {err:.2e} of the largest std")
    assert_mean_std_parity(path[:, 0], std[:, 0], ms[:, 0], ostd[:, 0])


def test_chain_equals_joint_gaussian_conditioning():
    """The construction of test_smooth_host.py::test_numpy_rts_equals_joint_gaussian_conditioning: the FULL joint covariance
    implied by the chain, cross-time blocks included, equals the conditioned joint Gaussian's."""
    _, _, opde, osolver = make_pair(6, 1, 0.05, 3, "neumann")
    osol = osolver.solve(opde)
    n, d = osol.mean.shape[1:]
    D, T = n * d, len(osol.t) - 1
    E0, E1 = osolver.E0, osolver.E1
    H = np.vstack((E1 - opde.L @ E0, opde.B @ E0))
    E = scipy.linalg.block_diag(opde.E_sqrtm, opde.R_sqrtm)
    R = E @ E.T
    mu = np.zeros((T + 1) * D)
    Sig = np.zeros(((T + 1) * D, (T + 1) * D))
    mu[:D] = osol.mean[0].reshape(-1, order="F")
    Sig[:D, :D] = osol.cov_sqrtm[0] @ osol.cov_sqrtm[0].T
    for k in range(T):
        Phi, Ql = osolver.iwp.non_preconditioned_discretize(osol.t[k + 1] - osol.t[k])
        a, b = slice(k * D, (k + 1) * D), slice((k + 1) * D, (k + 2) * D)
        mu[b] = Phi @ mu[a]
        Sig[b, :(k + 1) * D] = Phi @ Sig[a, :(k + 1) * D]
        Sig[:(k + 1) * D, b] = Sig[b, :(k + 1) * D].T
        Sig[b, b] = Phi @ Sig[a, a] @ Phi.T + Ql @ Ql.T
    m = H.shape[0]
    HH = np.zeros((T * m, (T + 1) * D))
    for k in range(1, T + 1):
        HH[(k - 1) * m:k * m, k * D:(k + 1) * D] = H
    S = HH @ Sig @ HH.T + np.kron(np.eye(T), R)
    K = scipy.linalg.solve(S, HH @ Sig, assume_a="pos").T
    mu_post = mu - K @ (HH @ mu)
    Sig_post = Sig - K @ HH @ Sig

    mT, CT, steps = maps_on_oracle(osolver, osol)
    np.testing.assert_allclose(zero_noise_path(mT, steps).reshape(-1), mu_post, rtol=1e-6, atol=1e-8 * np.abs(mu_post).max())
    J = joint_covariance(CT, steps)
    scale = np.abs(np.diag(Sig_post)).max()
    print(f"largest joint covariance error {np.abs(J - Sig_post).max() / scale:.2e} of the largest diagonal entry")
    np.testing.assert_allclose(J, Sig_post, rtol=1e-5, atol=1e-8 * scale)


def test_run_chain_is_the_affine_map_of_its_noise():
    _, _, opde, osolver = make_pair(8, 1, 2.0 ** -6, 3, "dirichlet")
    osol = osolver.solve(opde)
    mT, CT, steps = maps_on_oracle(osolver, osol)
    rng = np.random.default_rng(0)
    noise = [rng.standard_normal((4, B.shape[1])) for _, _, B in steps] + [rng.standard_normal((4, CT.shape[1]))]
    zero = [np.zeros_like(x) for x in noise]
    x0, x1 = run_chain(mT, CT, steps, zero), run_chain(mT, CT, steps, noise)
    np.testing.assert_allclose(x0[0], zero_noise_path(mT, steps), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(x1[:, -1] - x0[:, -1], noise[-1] @ CT.T, rtol=1e-10, atol=1e-14)


def test_restated_generator_is_philox4x32_10():
    """Known-answer vectors of Random123 (kat_vectors, philox4x32 10)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = philox4x32_10(np.array(ctr, dtype=np.uint64), key)
        assert tuple(int(x) for x in got) == want
    z = device_noise(3, 5, 64, 7)
    assert z.shape == (64, 7) and np.all(np.isfinite(z))
    assert np.array_equal(z[:8], device_noise(3, 5, 8, 7))              # draw i depends on (seed, i) only
    assert np.array_equal(z[:, :4], device_noise(3, 5, 64, 4))
    big = device_noise(0, 0, 512, 512).ravel()
    M = big.size
    assert abs(big.mean()) <= 5 / np.sqrt(M) and abs(big.var() - 1) <= 5 * np.sqrt(2 / M)


def test_sample_is_part_of_the_white_noise_solvers():
    import pnmol

    assert callable(pnmol.white.LinearWhiteNoiseEK1.sample) and callable(pnmol.white.SemiLinearWhiteNoiseEK1.sample)
    from pnmol import _hip

    for name in ("pnmol_samples_create", "pnmol_samples_destroy", "pnmol_samples_draw", "pnmol_samples_step_back",
                 "pnmol_samples_get", "pnmol_samples_get_time", "pnmol_sample_noise"):
        assert name in _hip.SYMBOLS
    assert callable(_hip.Filter.new_samples) and callable(_hip.Samples.step_back)
