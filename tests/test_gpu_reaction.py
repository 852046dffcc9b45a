"""Pointwise reaction terms linearised on the device (`pnmol_filter_set_reaction`, `pnmol_filter_linearize`,
csrc/pnmol_reaction.hip): the single-step route against the host route stage by stage, `solve()`,
`solve_marginals`, adaptive steps, smoothing and sampling against the oracle, clearing, fallbacks and refusals.
dt = 2^-6, kappa = 0.05; the oracle side is its spruce-budworm recipe with f, df overwritten by the closed forms.  Run with -m gpu."""

import ctypes

import numpy as np
import pytest

import pnmol
import pnmol_oracle as oracle
from helpers import assert_mean_std_parity, assert_parity as _assert_parity, per_step as _per_step, rel as _rel
from pnmol import _hip
from pnmol.pde import reactions
from smooth_reference import marginal_std, rts_on_oracle

pytestmark = pytest.mark.gpu

DT = 2.0 ** -6

# name -> (descriptor, closed-form f, closed-form diagonal of df): the oracle gets the closed forms, the product the descriptor
REACTIONS = {
    "logistic": (lambda: reactions.logistic(1.0), lambda x: x * (1.0 - x), lambda x: 1.0 - 2.0 * x),
    "allen_cahn": (reactions.allen_cahn, lambda x: x - x ** 3, lambda x: 1.0 - 3.0 * x ** 2),
    "budworm": (lambda: reactions.budworm(0.5, 3.0), lambda x: 0.5 * x * (1.0 - x / 3.0) - x ** 2 / (1.0 + x ** 2),
                lambda x: 0.5 * (1.0 - 2.0 * x / 3.0) - 2.0 * x / (1.0 + x ** 2) ** 2),
    "none": (lambda: reactions.Reaction(p=(0.0,)), None, None),
}


def _kw(N, bcond, tmax):
    return dict(tmax=tmax, dx=1.0 / (N - 1), diffusion_rate=0.05, bcond=bcond, stencil_size_interior=3, stencil_size_boundary=3)


def _product(name, N, nu, bcond, tmax, steprule=None, **attrs):
    pde = pnmol.pde.examples.reaction_diffusion_1d_discretized(REACTIONS[name][0](), kernel=pnmol.kernels.SquareExponential(),
                                                               nugget_gram_matrix_fd=0.0, **_kw(N, bcond, tmax))
    solver = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=nu, steprule=steprule or pnmol.odetools.step.Constant(DT),
                                                 spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
    for key, value in attrs.items():
        setattr(solver, key, value)
    return pde, solver


_ORACLE = {}


def _oracle(name, N, nu, bcond, tmax, adaptive=None):
    """(osolver, osol, means, stds) of the oracle, computed once per case and shared (nothing modifies them)."""
    key = (name, N, nu, bcond, tmax, None if adaptive is None else tuple(sorted(adaptive.items())))
    if key not in _ORACLE:
        opde = oracle.spruce_budworm_1d_discretized(kernel=oracle.SquareExponential(), **_kw(N, bcond, tmax))
        f, dfd = REACTIONS[name][1:]
        opde.f = lambda _t, x: f(x)
        opde.df = lambda _t, x: np.diag(dfd(x))
        rule = oracle.Constant(DT) if adaptive is None else oracle.Adaptive(**adaptive)
        osolver = oracle.WhiteNoiseEK1(num_derivatives=nu, steprule=rule, semilinear=True, canonical_factor_signs=True,
                                       spatial_kernel=oracle.Matern52() + oracle.WhiteNoise())
        osol = osolver.solve(opde)
        _ORACLE[key] = (osolver, osol) + tuple(oracle.read_mean_and_std(osol, osolver.E0))
    return _ORACLE[key]


# ------------------------------------------------------------------------------------------------------------ 1. stage parity
# The two routes run the same step kernels; they differ only in where r(u), r'(u) and the shift are evaluated.  k_linearize
# rounds every operation on its own, in the order of `Reaction.value` / `derivative` and of `pnmol_filter_predict_mean`, and the
# fp64 division of the device is correctly rounded, so the operator and the shift are the same bits on both routes and so is
# everything behind them.  Measured on an MI355X over the cases below (both sizes, raw frame, same frame, frame change): 0 for
# the mean, the marginal variances, diffusion_squared_local and the error estimate.  Ten times the measured figure (the
# convention of DESIGN.md section 15) is 0: the test asserts equality.
STAGE_BOUND = 0.0


@pytest.mark.parametrize("N", [33, 264])
def test_linearize_route_equals_the_host_route_stage_by_stage(hip_ctx, N):
    """`linearize` + `prepare_error_model` + `step` against `predict_mean` -> `Reaction.value` / `derivative` on the host ->
    `set_operator_diagonal` + `prepare_error_model` + `step` on a second filter of the same problem: from the raw frame, from
    the frame of the previous step, and across a frame change.  N = 33: d is no multiple of 32; N = 264: two blocks of
    k_linearize."""
    pde, dev_solver = _product("budworm", N, 2, "dirichlet", 24 * DT)
    _, host_solver = _product("budworm", N, 2, "dirichlet", 24 * DT, reaction_on_device=False)
    r = pde.reaction
    a = dev_solver.initialize(pde).y.device_state
    b = host_solver.initialize(pde).y.device_state
    fa, fb = dev_solver._device_filter, host_solver._device_filter
    assert fa.reaction is r and fb.reaction is None
    assert np.array_equal(a.mean(), b.mean()) and np.array_equal(a.cov(), b.cov())
    worst = dict(mean=0.0, var=0.0, sigma=0.0, error=0.0)
    for dt in (DT, DT, 0.6 * DT):
        fa.linearize(a, dt)
        fa.prepare_error_model(dt)
        a, ia, ea = fa.step(a, dt)
        m_at = fb.predict_mean(b, dt)
        jdiag, fx = r.derivative(m_at), r.value(m_at)
        fb.set_operator_diagonal(jdiag, jdiag * m_at - fx)
        fb.prepare_error_model(dt)
        b, ib, eb = fb.step(b, dt)
        assert np.abs(jdiag).max() > 0.1 and np.all(np.isfinite(ea)) and ia.info == -1 and ib.info == -1
        worst["mean"] = max(worst["mean"], _rel(a.mean(), b.mean()))
        worst["var"] = max(worst["var"], _rel(a.marginal_var(), b.marginal_var()))
        worst["sigma"] = max(worst["sigma"], _rel(ia.diffusion_squared_local, ib.diffusion_squared_local))
        worst["error"] = max(worst["error"], _rel(ea, eb))
    print(f"stage parity N={N}: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for kind, v in worst.items():
        assert v <= STAGE_BOUND, (kind, v)


# ------------------------------------------------------------------------------------------------------------ 2. solve()
SOLVE_CASES = [("logistic", 32, 2, "dirichlet", 24), ("allen_cahn", 48, 1, "neumann", 24), ("budworm", 33, 2, "dirichlet", 24)]


@pytest.mark.parametrize("name,N,nu,bcond,K", SOLVE_CASES)
def test_solve_against_the_oracle(hip_ctx, name, N, nu, bcond, K):
    pde, solver = _product(name, N, nu, bcond, K * DT)
    sol = solver.solve(pde)
    assert solver._device_filter.reaction is pde.reaction
    osolver, osol, om, os_ = _oracle(name, N, nu, bcond, K * DT)
    assert np.allclose(sol.t, osol.t, rtol=0, atol=1e-15) and sol.info == osol.info
    assert sol.info["num_f_evaluations"] == sol.info["num_df_evaluations"] == K
    assert_mean_std_parity(sol.mean[:, 0], sol.marginal_std[:, 0], om, os_)
    np.testing.assert_allclose(sol.diffusion_squared_calibrated, osol.diffusion_squared_calibrated, rtol=1e-5)
    # the reaction matters: the same run without it differs by more than 1e-2 of the largest mean entry
    pde0, solver0 = _product("none", N, nu, bcond, K * DT)
    sol0 = solver0.solve(pde0)
    moved = np.abs(sol.mean[:, 0] - sol0.mean[:, 0]).max() / np.abs(sol.mean[:, 0]).max()
    print(f"{name}: the reaction moves the mean by {moved:.3f} of its largest entry")
    assert moved > 1e-2


# ------------------------------------------------------------------------------------------------------------ 3. solve_marginals
MARGINAL_CASES = SOLVE_CASES + [
    ("budworm", 33, 3, "dirichlet", 12),      # n = 4: sweep_mode 1
    ("logistic", 264, 2, "dirichlet", 9),     # two blocks of k_linearize
    ("logistic", 32, 2, "dirichlet", 25),     # odd number of steps: the result lives in the filter's spare buffers
    ("logistic", 32, 2, "dirichlet", 8.3),    # runt last step: another dt, a frame change inside k_linearize
]


@pytest.mark.parametrize("name,N,nu,bcond,K", MARGINAL_CASES)
def test_solve_marginals_against_the_oracle_and_solve(hip_ctx, name, N, nu, bcond, K):
    pde, solver = _product(name, N, nu, bcond, K * DT)
    t, means, stds, sig, final = solver.solve_marginals(pde)
    osolver, osol, om, os_ = _oracle(name, N, nu, bcond, K * DT)
    steps = int(np.ceil(K))
    assert t.shape == (steps + 1,) and np.allclose(t, osol.t, rtol=0, atol=1e-15) and sig.shape == (steps,)
    if steps != K:
        assert abs((t[-1] - t[-2]) - 0.3 * DT) < 1e-12
    _assert_parity(means, stds, om, os_, nu)
    np.testing.assert_allclose(final.y.mean[0], om[-1], rtol=1e-5, atol=1e-5 * np.abs(om).max())
    # ... and against solve() of the same solver, step by step
    sm, ss, ssig = _per_step(solver, pde)
    same = np.array_equal(means, sm) and np.array_equal(stds, ss) and np.array_equal(sig, ssig)
    print(f"solve_marginals vs solve ({name}, N={N}, nu={nu}, K={K}): bit-identical {same}; mean {_rel(means, sm):.2e}, "
          f"std {_rel(stds, ss):.2e}, sigma {_rel(sig, ssig):.2e}")
    _assert_parity(means, stds, sm, ss, nu)
    np.testing.assert_allclose(sig, ssig, rtol=1e-5)


def test_two_steps_calls_equal_one_call_of_the_summed_length(hip_ctx):
    pde, solver = _product("budworm", 33, 2, "dirichlet", 24 * DT)
    a = solver.initialize(pde).y.device_state
    flt = solver._device_filter
    b = a.clone()
    m1, s1, i1 = flt.steps(a, 5, DT)          # eager lead step (raw frame) + two captured pairs
    m2, s2, i2 = flt.steps(a, 7, DT)          # three pairs + an eager step
    m, s, i = flt.steps(b, 12, DT)            # lead step + the ten-step graph + an eager step
    assert np.array_equal(np.vstack((m1, m2)), m) and np.array_equal(np.vstack((s1, s2)), s)
    sig = [o.diffusion_squared_local for o in list(i1) + list(i2)]
    assert sig == [o.diffusion_squared_local for o in i] and all(o.info == -1 for o in i)
    assert all(np.isnan(o.error_sigma2) for o in i)            # no error model inside the loop
    assert np.array_equal(a.mean(), b.mean()) and np.array_equal(a.cov(), b.cov())
    assert np.array_equal(a.marginal_var(), b.marginal_var()) and a.t == b.t


# ------------------------------------------------------------------------------------------------------------ 4. adaptive steps
def test_adaptive_steps_against_the_oracle(hip_ctx):
    """abstol = 1e-4, reltol = 1e-3: the oracle rejects one of its 14 attempts, and its scaled error norms stay 7 % or more
    away from the acceptance threshold for this input, so the decisions are not a matter of rounding."""
    tol = dict(abstol=1e-4, reltol=1e-3)
    pde, solver = _product("logistic", 48, 2, "neumann", 24 * DT, steprule=pnmol.odetools.step.Adaptive(**tol))
    sol = solver.solve(pde)
    osolver, osol, om, os_ = _oracle("logistic", 48, 2, "neumann", 24 * DT, adaptive=tol)
    assert solver._device_filter.reaction is pde.reaction
    assert sol.info == osol.info and sol.info["num_attempted_steps"] > sol.info["num_steps"] > 3
    np.testing.assert_allclose(sol.t, osol.t, rtol=1e-9)
    assert_mean_std_parity(sol.mean[:, 0], sol.marginal_std[:, 0], om, os_)


# ------------------------------------------------------------------------------------------------------------ 5. downstream
def test_smooth_and_sample_of_a_device_linearised_solve(hip_ctx):
    name, N, nu, bcond, K = SOLVE_CASES[2]
    pde, solver = _product(name, N, nu, bcond, K * DT)
    sol = solver.solve(pde)
    osolver, osol, _, _ = _oracle(name, N, nu, bcond, K * DT)
    ms, Ps = rts_on_oracle(osolver, osol)
    n, d = osol.mean.shape[1:]
    ostd = marginal_std(Ps, n, d)
    ssol = solver.smooth(sol)
    assert_mean_std_parity(ssol.mean[:, 0], ssol.marginal_std[:, 0], ms[:, 0], ostd[:, 0])
    noise = [np.zeros((2, 2 * n * d)) for _ in range(K)] + [np.zeros((2, n * d))]
    x = solver.sample(sol, 2, noise=noise)
    assert x.shape == (2, K + 1, n, d) and np.array_equal(x[0], x[1])
    np.testing.assert_allclose(x[0][:, 0], ms[:, 0], rtol=1e-5, atol=1e-5 * np.abs(ms[:, 0]).max())


# ------------------------------------------------------------------------------------------------------------ 6. clearing
def test_cleared_filter_equals_a_fresh_linear_filter_bit_for_bit(hip_ctx):
    N, K = 33, 6
    pde, solver = _product("budworm", N, 2, "dirichlet", 24 * DT)
    lin = pnmol.pde.examples.heat_1d_discretized(kernel=pnmol.kernels.SquareExponential(), nugget_gram_matrix_fd=0.0,
                                                 y0_fun=pnmol.pde.examples.sin_bell_1d, **_kw(N, "dirichlet", 24 * DT))
    assert np.array_equal(lin.L, pde.L) and np.array_equal(lin.B, pde.B)
    lsolver = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=2, steprule=pnmol.odetools.step.Constant(DT),
                                              spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
    ref = lsolver.initialize(lin).y.device_state
    mean0, cov0 = ref.mean(), ref.cov()
    used = solver.initialize(pde).y.device_state
    flt = solver._device_filter
    flt.steps(used, 4, DT)                                      # graphs captured with the reaction
    flt.linearize(used, DT)                                     # ... and a patched operator left behind
    flt.prepare_error_model(DT)
    flt.set_reaction(None)
    assert flt.reaction is None
    a = flt.new_state()
    a.set(0.0, mean0, cov0)
    b = lsolver._device_filter.new_state()
    b.set(0.0, mean0, cov0)
    ma, sa, ia = flt.steps(a, K, DT)
    mb, sb, ib = lsolver._device_filter.steps(b, K, DT)
    assert np.array_equal(ma, mb) and np.array_equal(sa, sb)
    for oa, ob in zip(ia, ib):
        assert (oa.diffusion_squared_local, oa.sigma2_whitened, oa.info) == (ob.diffusion_squared_local, ob.sigma2_whitened, ob.info)
        assert np.isnan(oa.error_sigma2) and np.isnan(ob.error_sigma2)
    assert np.array_equal(a.mean(), b.mean()) and np.array_equal(a.cov(), b.cov())
    # clearing twice, and clearing a filter that never had a reaction, are no-ops
    flt.set_reaction(None)
    lsolver._device_filter.set_reaction(None)
    # and the host route works again on the cleared filter
    flt.set_operator_diagonal(np.zeros(flt.d), np.zeros(flt.d))


# ------------------------------------------------------------------------------------------------------------ 7. fallbacks, refusals
def test_host_fallback_matches_the_oracle(hip_ctx):
    name, N, nu, bcond, K = SOLVE_CASES[2]
    pde, solver = _product(name, N, nu, bcond, K * DT, reaction_on_device=False)
    sol = solver.solve(pde)
    assert solver._device_filter.reaction is None
    _, osol, om, os_ = _oracle(name, N, nu, bcond, K * DT)
    assert sol.info == osol.info
    assert_mean_std_parity(sol.mean[:, 0], sol.marginal_std[:, 0], om, os_)
    with pytest.raises(TypeError, match="needs a linear PDE; use solve"):
        solver.solve_marginals(pde)


def test_fp32_fallback_matches_the_oracle(hip_ctx):
    """dtype = "f32" (nu = 1) takes the host callables.  Mean at the north-star tolerance; std at rtol 1e-4 on the entries that
    are at least 1 % of the largest, the criterion of tests/test_gpu_fp32.py (the fp32 covariance has a floor below that,
    DESIGN.md section 11)."""
    name, N, nu, bcond, K = SOLVE_CASES[1]
    pde, solver = _product(name, N, nu, bcond, K * DT, dtype="f32")
    sol = solver.solve(pde)
    assert solver._device_filter.reaction is None and solver._device_filter.dtype == "f32"
    _, osol, om, os_ = _oracle(name, N, nu, bcond, K * DT)
    np.testing.assert_allclose(sol.mean[:, 0], om, rtol=1e-5, atol=1e-5 * np.abs(om).max())
    stds = sol.marginal_std[:, 0]
    big = os_ >= 1e-2 * os_.max()
    np.testing.assert_allclose(stds[big], os_[big], rtol=1e-4)
    with pytest.raises(TypeError, match="needs a linear PDE; use solve"):
        solver.solve_marginals(pde)


def test_pde_without_a_reaction_keeps_the_type_error(hip_ctx):
    pde = pnmol.pde.examples.spruce_budworm_1d_discretized(kernel=pnmol.kernels.SquareExponential(),
                                                           **_kw(24, "dirichlet", 4 * DT))
    solver = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=2, steprule=pnmol.odetools.step.Constant(DT))
    with pytest.raises(TypeError, match="solve_marginals keeps the loop on the device and needs a linear PDE; use solve\\(\\)"):
        solver.solve_marginals(pde)
    sol = solver.solve(pde)                                      # the host route, as before
    assert solver._device_filter.reaction is None and len(sol.t) == 5


def _desc(p=(), a=None, b=None, degs=None):
    d = reactions.ReactionDesc()
    d.deg_p, d.deg_a, d.deg_b = len(p) - 1, -1 if a is None else len(a) - 1, -1 if b is None else len(b) - 1
    for dst, src in ((d.p, p), (d.a, a or ()), (d.b, b or ())):
        for k, c in enumerate(src):
            dst[k] = c
    if degs is not None:
        d.deg_p, d.deg_a, d.deg_b = degs
    return d


def test_every_refusal_of_the_abi(hip_ctx):
    pde, solver = _product("logistic", 24, 2, "dirichlet", 2 * DT, reaction_on_device=False)
    state = solver.initialize(pde).y.device_state
    flt = solver._device_filter
    lib, h = flt.lib, flt.handle
    good = reactions.logistic(1.0).to_ctypes()
    err = lambda: lib.pnmol_last_error(flt.ctx.handle).decode()
    assert lib.pnmol_filter_set_reaction(None, ctypes.byref(good)) == -1
    for bad, why in [(_desc(degs=(8, -1, -1)), "degree"), (_desc(degs=(-2, -1, -1)), "degree"),
                     (_desc(p=(1.0,), degs=(0, 9, 0)), "degree"), (_desc(a=(1.0,)), "together"), (_desc(b=(1.0,)), "together"),
                     (_desc(p=(0.0, np.nan)), "finite"), (_desc(a=(np.inf,), b=(1.0,)), "finite"),
                     (_desc(a=(1.0,), b=(1.0, -np.inf)), "finite"), (_desc(a=(1.0,), b=(0.0, 0.0, 0.0)), "identically zero")]:
        assert lib.pnmol_filter_set_reaction(h, ctypes.byref(bad)) == -1
        assert why in err(), (why, err())
    # no reaction set: linearize refuses, the operator calls work
    assert lib.pnmol_filter_linearize(h, state.handle, DT) == -1 and "no reaction" in err()
    with pytest.raises(_hip.PnmolHipError, match="pnmol_filter_linearize"):
        flt.linearize(state, DT)
    assert lib.pnmol_filter_set_reaction(h, ctypes.byref(good)) == 0
    assert lib.pnmol_filter_linearize(None, state.handle, DT) == -1
    assert lib.pnmol_filter_linearize(h, None, DT) == -1
    assert lib.pnmol_filter_linearize(h, state.handle, 0.0) == -1
    assert lib.pnmol_filter_linearize(h, state.handle, -DT) == -1
    assert lib.pnmol_filter_linearize(h, state.handle, float("nan")) == -1
    pde2, solver2 = _product("logistic", 24, 2, "dirichlet", 2 * DT)
    foreign = solver2.initialize(pde2).y.device_state
    assert lib.pnmol_filter_linearize(h, foreign.handle, DT) == -1
    assert lib.pnmol_filter_linearize(h, state.handle, DT) == 0
    # the operator calls are refused while a reaction is set
    d = flt.d
    M, z = np.ascontiguousarray(pde.L, dtype=np.float64), np.zeros(d)
    dp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.pnmol_filter_set_operator(h, dp(M), dp(z)) == -1 and "clear the reaction first" in err()
    assert lib.pnmol_filter_set_operator_diagonal(h, dp(z), dp(z)) == -1 and "clear the reaction first" in err()
    assert lib.pnmol_filter_set_reaction(h, None) == 0
    assert lib.pnmol_filter_set_operator(h, dp(M), dp(z)) == 0
    assert lib.pnmol_filter_set_operator_diagonal(h, dp(z), dp(z)) == 0
    # fp32 and latent-force filters have no device path
    kw = dict(L=pde.L, B=pde.B, E_sqrtm=pde.E_sqrtm, R_sqrtm=pde.R_sqrtm, num_derivatives=1)
    gamma = np.linalg.cholesky(solver._gram)
    f32 = _hip.Filter(flt.ctx, Gamma=gamma, dtype="f32", **kw)
    assert lib.pnmol_filter_set_reaction(f32.handle, ctypes.byref(good)) == -1 and "fp32" in err()
    assert lib.pnmol_filter_set_reaction(f32.handle, None) == 0
    with pytest.raises(_hip.PnmolHipError, match="pnmol_filter_set_reaction"):
        f32.set_reaction(reactions.logistic(1.0))
    assert f32.reaction is None
    lkw = dict(kw, L=np.hstack((pde.L, np.eye(d))), B=np.hstack((pde.B, np.zeros_like(pde.B))))
    latent = _hip.Filter(flt.ctx, Gamma=np.linalg.cholesky(np.kron(np.eye(2), solver._gram)), **lkw)
    assert lib.pnmol_filter_set_reaction(latent.handle, ctypes.byref(good)) == -1 and "latent" in err()
    # an operator row without a diagonal entry
    Lnd = pde.L.copy()
    Lnd[3, 3] = 0.0
    nodiag = _hip.Filter(flt.ctx, Gamma=gamma, **dict(kw, L=Lnd))
    assert lib.pnmol_filter_set_reaction(nodiag.handle, ctypes.byref(good)) == -1 and "diagonal" in err()
