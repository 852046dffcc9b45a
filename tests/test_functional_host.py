"""Host-side checks of the functionals feature (no GPU): the three references of tests/functional_reference.py against each
other, against the RTS smoother and against the sampler's reference map; the conditions on the inputs that the GPU tests rely on;
the weight builders, the Python layer's argument checks and the C symbol."""

import ctypes
import pathlib
import re

import numpy as np
import pytest

import functional_reference as fr
import sample_reference
import stage_reference as sr
from helpers import assert_mean_std_parity, make_pair
from pnmol import _hip, functionals as fn
from smooth_reference import rts_on_oracle

ROOT = pathlib.Path(__file__).resolve().parents[1]
CASES = [(20, 1, "dirichlet"), (33, 2, "dirichlet"), (40, 3, "dirichlet"), (96, 2, "neumann"), (150, 1, "neumann"),
         (170, 2, "dirichlet")]
HEAT = [(N, nu, bc) for N in (32, 33) for nu in (1, 2) for bc in ("dirichlet", "neumann")]
K = 6


@pytest.mark.parametrize("case", CASES, ids=[sr.case_id(c) for c in CASES])
def test_dense_reference_and_restatement_agree(case):
    """(1) and (2) sit equally close to the truth (3), and the inputs are what the GPU test's
    bound assumes: cond(P-) <= 1e4 at every step, and none of the 64 random functionals cancels (cov_qq >= 1e-3 of the sum of the
    positive terms it is accumulated from)."""
    tc = fr.trajectory_case(*case)
    c = tc.c
    assert fr.predicted_condition(tc) <= 1e4
    W = fr.random_weights(tc, 64)
    m2, c2, gross = fr.restate(c.A, c.Q, c.nu, c.d, tc.states, tc.dts, W)
    assert np.all(np.diag(c2) >= 1e-3 * gross)
    W3 = W[:3]
    m1, c1, _, _ = fr.dense_reference(c.A, c.Q, c.osolver.iwp.nordsieck_preconditioner, tc.states, tc.dts, W3)
    mt, ct = fr.truth(c, tc.states, tc.dts, W3)
    for x1, x2, xt in ((m1, m2[:3], mt), (c1, c2[:3, :3], ct)):
        e1, e2 = fr.error(x1, xt), fr.error(x2, xt)
        # two fp64 evaluations of the same quantity: each within the allowance the other one's error sets (the device's rule)
        assert e2 <= sr.bound(e1) and e1 <= sr.bound(e2), (e1, e2)


def _oracle_run(N, nu, bcond):
    _, _, opde, osolver = make_pair(N, nu, 2.0 ** -7, K, bcond)
    osol = osolver.solve(opde)
    A, Ql = osolver.iwp.preconditioned_discretize
    states = [(mu, C @ C.T) for mu, C in zip(osol.mean, osol.cov_sqrtm)]
    return osolver, osol, A, Ql @ Ql.T, states, list(np.diff(osol.t))


@pytest.mark.parametrize("N,nu,bcond", HEAT)
def test_restatement_meets_the_north_star_tolerances_on_heat_posteriors(N, nu, bcond):
    """The cases of the GPU test against the smoother: on the oracle's trajectory the device's order of operations (2), in fp64,
    gives the dense reference (1) at the tolerances the device is held to there; a `point` functional is the RTS marginal."""
    osolver, osol, A, Q, states, dts = _oracle_run(N, nu, bcond)
    where = [(k, j) for k in (0, 3, K) for j in (1, N // 2, N - 2)]
    W = np.stack([fn.point(K, N, k, j) for k, j in where]
                 + [fn.space_time_mean(osol.t, N), fn.trapezoid_in_time(osol.t, np.eye(N)[N // 2])])
    W = fn.checked_weights(W, K, nu + 1, N)
    m1, c1, _, _ = fr.dense_reference(A, Q, osolver.iwp.nordsieck_preconditioner, states, dts, W)
    m2, c2, gross = fr.restate(A, Q, nu, N, states, dts, W)
    assert np.all(np.diag(c2) >= 1e-3 * gross), np.diag(c2) / gross               # held at a relative tolerance: none cancels
    assert_mean_std_parity(m2, np.sqrt(np.diag(c2)), m1, np.sqrt(np.diag(c1)))
    ms, Ps = rts_on_oracle(osolver, osol)
    rm = np.array([ms[k, 0, j] for k, j in where])
    rs = np.array([np.sqrt(Ps[k][j * (nu + 1), j * (nu + 1)]) for k, j in where])
    assert_mean_std_parity(m1[:9], np.sqrt(np.diag(c1))[:9], rm, rs)
    assert_mean_std_parity(m2[:9], np.sqrt(np.diag(c2))[:9], rm, rs)


def test_covariance_from_the_samplers_noise_map():
    """Independent derivation: the sampler's reference chain maps noise to the trajectory linearly, x_j = sum_k M[j][k] xi_k, so
    cov = sum_k (sum_j W_j M[j][k]) (...)^T, and the zero-noise path gives the mean."""
    N, nu = 32, 2
    osolver, osol, A, Q, states, dts = _oracle_run(N, nu, "dirichlet")
    W = np.stack([fn.space_time_mean(osol.t, N), fn.trapezoid_in_time(osol.t, np.eye(N)[N // 2]), fn.point(K, N, 2, 7),
                  fn.difference(K, N, (K, N // 2), (1, 3))])
    W = fn.checked_weights(W, K, nu + 1, N)
    Wf = fr.flat_weights(W)
    mT, CT, steps = sample_reference.maps_on_oracle(osolver, osol)
    M = sample_reference.noise_maps(CT, steps)
    cov = np.zeros((4, 4))
    for k in range(K + 1):
        B = sum(Wf[:, j] @ M[j][k] for j in range(k + 1))
        cov += B @ B.T
    mean = np.einsum("qkd,kd->q", Wf, sample_reference.zero_noise_path(mT, steps))
    m1, c1, _, _ = fr.dense_reference(A, Q, osolver.iwp.nordsieck_preconditioner, states, dts, W)
    m2, c2, _ = fr.restate(A, Q, nu, N, states, dts, W)
    for m, c in ((m1, c1), (m2, c2)):
        assert_mean_std_parity(m, np.sqrt(np.diag(c)), mean, np.sqrt(np.diag(cov)))
        np.testing.assert_allclose(c, cov, rtol=1e-4, atol=1e-4 * np.sqrt(np.outer(np.diag(cov), np.diag(cov))).max())


def test_weight_builders():
    t = np.array([0.0, 0.1, 0.25, 0.3, 0.7])
    T, d = t.size - 1, 5
    w = fn.trapezoid_in_time(t, np.eye(d)[2])
    assert w.shape == (T + 1, d) and not w[:, [0, 1, 3, 4]].any()
    assert np.isclose(w.sum(), t[-1] - t[0], rtol=1e-15)
    assert np.isclose(fn.trapezoid_in_time(t, np.ones(d))[:, 0].sum(), t[-1] - t[0], rtol=1e-15)
    assert np.allclose(w[:, 2], [0.05, 0.125, 0.1, 0.225, 0.2], rtol=1e-14)
    assert np.isclose(fn.space_time_mean(t, d).sum(), 1.0, rtol=1e-15)
    assert np.array_equal(fn.space_time_mean(t[:1], d), np.full((1, d), 0.2))
    p = fn.point(T, d, 3, 4)
    assert p.sum() == 1.0 and p[3, 4] == 1.0
    df = fn.difference(T, d, (4, 1), (0, 1))
    assert df[4, 1] == 1.0 and df[0, 1] == -1.0 and np.abs(df).sum() == 2.0
    post = fn.FunctionalPosterior(mean=np.zeros(2), cov=np.array([[4.0, 1.0], [1.0, -1e-20]]))
    assert np.array_equal(post.std, [2.0, 0.0])


def test_checked_weights():
    T, n, d = 3, 2, 5
    w = np.arange(2.0 * 4 * 5).reshape(2, T + 1, d)
    full = fn.checked_weights(w, T, n, d)
    assert full.shape == (2, T + 1, n, d) and np.array_equal(full[:, :, 0], w) and not full[:, :, 1].any()
    assert fn.checked_weights(full, T, n, d) is not None and full.flags.c_contiguous
    for bad in (np.zeros((2, T, d)), np.zeros((T + 1, d)), np.zeros((0, T + 1, d)), np.zeros((2, T + 1, n + 1, d)),
                np.zeros((2, T + 1, d + 1))):
        with pytest.raises(ValueError, match="weights must have shape"):
            fn.checked_weights(bad, T, n, d)
    for v in (np.nan, np.inf):
        w[1, 2, 3] = v
        with pytest.raises(ValueError, match="finite"):
            fn.checked_weights(w, T, n, d)


def test_symbol_is_declared_and_exported():
    import pnmol

    header = (ROOT / "include" / "pnmol_hip.h").read_text()
    assert re.search(r"\bint pnmol_functionals\(", header) and "#define PNMOL_FUNCTIONALS_MAX_Q 64" in header
    assert "pnmol_functionals" in _hip.SYMBOLS
    lib = _hip.load_library()
    assert hasattr(lib, "pnmol_functionals") and lib.pnmol_abi_version() == 3
    assert lib.pnmol_functionals(None, 0, None, None, 1, None, None, None) == -1   # the argument check needs no GPU
    assert callable(_hip.Filter.functionals)
    assert callable(pnmol.white.LinearWhiteNoiseEK1.functionals) and callable(pnmol.white.SemiLinearWhiteNoiseEK1.functionals)
    assert (ROOT / "pnmol-experiments_amd" / "csrc" / "pnmol_functional.hip") in __import__("__graft_entry__").SOURCES
    assert ctypes.c_int == _hip.SYMBOLS["pnmol_functionals"][0]
