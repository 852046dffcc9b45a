"""Burgers-type convection terms linearised on the device (`pnmol_filter_set_convection`, k_linearize_convection,
csrc/pnmol_reaction.hip): the single-step route against the host route stage by stage, the loop against
single steps, `solve()` and `solve_marginals` against the oracle, adaptive steps, clearing, replacing, refusals and the host
routes.  kappa = 0.02, dt = 2^-7, y0 = sin(pi x); the oracle side is tests/convection_reference.py.  Run with -m gpu."""

import ctypes

import numpy as np
import pytest

import pnmol
from convection_reference import CASES, DT, KAPPA, RATE, kw, oracle_solve, product
from helpers import assert_mean_std_parity, assert_parity as _assert_parity, per_step as _per_step, rel as _rel
from pnmol import _hip
from pnmol.pde import reactions

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------ 1. stage parity
# Both routes run the same step kernels on the same operator image; they differ in where u, g = G u, c, c', r, r', the operator
# entries and the shift are formed.  k_linearize_convection and `Convection.linearization` take the same IEEE operations in the
# same order (no contraction on the device, NumPy elementwise on the host; fp64 division is correctly rounded on both), and -M is
# formed as (-L) - c G [- q] on the device and as -((L + c G) [+ q]) by the dense upload: negation is exact.  The bound is zero
# by construction, not a measured tolerance.
STAGE_CASES = [("burgers", 33, "dirichlet", 3), ("burgers", 33, "neumann", 3), ("burgers", 264, "dirichlet", 3),
               ("burgers_fisher", 33, "dirichlet", 3), ("burgers_fisher", 264, "dirichlet", 3),
               ("burgers", 33, "dirichlet", 5)]             # 5-point gradient over a 3-point Laplacian: the union is wider


@pytest.mark.parametrize("variant,N,bcond,gss", STAGE_CASES)
def test_linearize_route_equals_the_host_route_stage_by_stage(hip_ctx, variant, N, bcond, gss):
    """`linearize` + `prepare_error_model` + `step` against `predict_mean` -> `Convection.linearization` on the host ->
    `set_operator(M, shift)` + `prepare_error_model` + `step` on a second filter of the same problem: from the raw frame, from
    the frame of the previous step, and across a frame change to 0.6 dt.  N = 33: m = 35, padded rows; N = 264: two blocks."""
    pde, dev_solver = product(variant, N, 2, bcond, 24 * DT, gradient_stencil_size=gss)
    _, host_solver = product(variant, N, 2, bcond, 24 * DT, gradient_stencil_size=gss, reaction_on_device=False)
    term = pde.reaction
    a = dev_solver.initialize(pde).y.device_state
    b = host_solver.initialize(pde).y.device_state
    fa, fb = dev_solver._device_filter, host_solver._device_filter
    assert fa.reaction is term and fb.reaction is None
    union = ((term.G != 0.0) | (pde.L != 0.0)).sum(axis=1).max()
    assert union == gss and (pde.L != 0.0).sum(axis=1).max() == 3
    assert np.array_equal(a.mean(), b.mean()) and np.array_equal(a.cov(), b.cov())
    worst = dict(mean=0.0, var=0.0, sigma=0.0, error=0.0)
    for dt in (DT, DT, 0.6 * DT):
        fa.linearize(a, dt)
        fa.prepare_error_model(dt)
        a, ia, ea = fa.step(a, dt)
        m_at = fb.predict_mean(b, dt)
        M, shift = term.linearization(m_at, L=pde.L)
        fb.set_operator(M, shift)
        fb.prepare_error_model(dt)
        b, ib, eb = fb.step(b, dt)
        assert np.abs(M - pde.L).max() > 0.1 and np.abs(shift).max() > 0.1       # the term is there
        assert np.all(np.isfinite(ea)) and ia.info == -1 and ib.info == -1
        worst["mean"] = max(worst["mean"], _rel(a.mean(), b.mean()))
        worst["var"] = max(worst["var"], _rel(a.marginal_var(), b.marginal_var()))
        worst["sigma"] = max(worst["sigma"], _rel(ia.diffusion_squared_local, ib.diffusion_squared_local))
        worst["error"] = max(worst["error"], _rel(ea, eb))
    print(f"stage parity {variant} N={N} {bcond} gss={gss}: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for kind, v in worst.items():
        assert v == 0.0, (kind, v)


# ------------------------------------------------------------------------------------------------------------ 2. loop against steps
LOOP_CASES = [("burgers", 33, 2, "dirichlet", 24), ("burgers", 33, 2, "neumann", 8.3),     # runt last step: another dt
              ("burgers", 33, 3, "dirichlet", 12), ("burgers_fisher", 33, 2, "dirichlet", 9), ("burgers", 264, 2, "dirichlet", 3)]


@pytest.mark.parametrize("variant,N,nu,bcond,K", LOOP_CASES)
def test_solve_marginals_equals_solve_step_by_step(hip_ctx, variant, N, nu, bcond, K):
    """Means and diffusion_squared_local bit-identical; stds within 2 units in the last place (the loop and the single step read
    the marginal variances out in different launches: the one-ulp difference of DESIGN.md section 16)."""
    pde, solver = product(variant, N, nu, bcond, K * DT)
    t, means, stds, sig, final = solver.solve_marginals(pde)
    steps = int(np.ceil(K))
    assert t.shape == (steps + 1,) and sig.shape == (steps,) and np.all(np.isfinite(means)) and np.all(np.isfinite(stds))
    if steps != K:
        assert abs((t[-1] - t[-2]) - (K - steps + 1) * DT) < 1e-12
    sm, ss, ssig = _per_step(solver, pde)
    ulps = np.abs(stds - ss) / np.spacing(np.maximum(np.abs(stds), np.abs(ss)))
    print(f"solve_marginals vs solve ({variant}, N={N}, nu={nu}, K={K}): mean {_rel(means, sm):.2e}, sigma {_rel(sig, ssig):.2e}, "
          f"std off by at most {ulps.max():.1f} ulp")
    assert np.array_equal(means, sm) and np.array_equal(sig, ssig)
    assert ulps.max() <= 2.0
    assert np.array_equal(final.y.mean[0], sm[-1])


# ------------------------------------------------------------------------------------------------------------ 3. oracle parity
ORACLE_CASES = [("burgers",) + c for c in CASES] + [("burgers_fisher", 33, 2, "dirichlet", 24)]


@pytest.mark.parametrize("variant,N,nu,bcond,K", ORACLE_CASES)
def test_solve_and_solve_marginals_against_the_oracle(hip_ctx, variant, N, nu, bcond, K):
    osolver, osol, om, os_ = oracle_solve(variant, N, nu, bcond, K)
    pde, solver = product(variant, N, nu, bcond, K * DT)
    sol = solver.solve(pde)
    assert solver._device_filter.reaction is pde.reaction
    assert np.allclose(sol.t, osol.t, rtol=0, atol=1e-15) and sol.info == osol.info
    assert sol.info["num_f_evaluations"] == sol.info["num_df_evaluations"] == K
    _assert_parity(sol.mean[:, 0], sol.marginal_std[:, 0], om, os_, nu)
    np.testing.assert_allclose(sol.diffusion_squared_calibrated, osol.diffusion_squared_calibrated, rtol=1e-5)
    pde, solver = product(variant, N, nu, bcond, K * DT)
    t, means, stds, sig, final = solver.solve_marginals(pde)
    assert t.shape == (K + 1,) and np.allclose(t, osol.t, rtol=0, atol=1e-15) and sig.shape == (K,)
    _assert_parity(means, stds, om, os_, nu)
    np.testing.assert_allclose(final.y.mean[0], om[-1], rtol=1e-5, atol=1e-5 * np.abs(om).max())
    # the term matters (tests/test_convection_host.py asserts the same on the oracle alone)
    _, _, om0, _ = oracle_solve("heat", N, nu, bcond, K)
    assert np.abs(means[-1] - om0[-1]).max() >= 0.1 * np.abs(means[-1]).max()


# ------------------------------------------------------------------------------------------------------------ 4. adaptive steps
def test_adaptive_steps_against_the_oracle(hip_ctx):
    """Burgers, N = 48, nu = 2, Neumann, abstol = 1e-4, reltol = 1e-3, tmax = 24 dt.  Found on the CPU with the oracle alone: 16
    attempts, one rejected (scaled error norm 1.176), the accepted ones between 0.144 and 0.832: the closest norm is 16.8 % away
    from the acceptance threshold 1, so the decisions are not a matter of rounding.  The margin is asserted first."""
    tol = dict(abstol=1e-4, reltol=1e-3)
    osolver, osol, om, os_ = oracle_solve("burgers", 48, 2, "neumann", 24, adaptive=tol)
    norms = np.array(osolver.steprule.norms)
    assert norms.size == osol.info["num_attempted_steps"] and np.abs(norms - 1.0).min() >= 0.05, norms
    pde, solver = product("burgers", 48, 2, "neumann", 24 * DT, steprule=pnmol.odetools.step.Adaptive(**tol))
    sol = solver.solve(pde)
    assert solver._device_filter.reaction is pde.reaction
    assert sol.info == osol.info and sol.info["num_attempted_steps"] > sol.info["num_steps"] > 3
    np.testing.assert_allclose(sol.t, osol.t, rtol=1e-9)
    assert_mean_std_parity(sol.mean[:, 0], sol.marginal_std[:, 0], om, os_)


# ------------------------------------------------------------------------------------------------------------ 5. clearing
def _loop(flt, mean0, cov0, K=6):
    s = flt.new_state()
    s.set(0.0, mean0, cov0)
    m, sd, infos = flt.steps(s, K, DT)
    scal = [(o.diffusion_squared_local, o.sigma2_whitened, o.info) for o in infos]
    assert all(np.isnan(o.error_sigma2) for o in infos)
    return m, sd, scal, s.mean(), s.cov()


def _same(x, y):
    return (np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2] and np.array_equal(x[3], y[3])
            and np.array_equal(x[4], y[4]))


@pytest.mark.parametrize("gss", [3, 5])
def test_cleared_filter_equals_a_fresh_linear_filter_bit_for_bit(hip_ctx, gss):
    """gss = 5: the union image is wider than the base image, so clearing also restores the width."""
    N = 33
    pde, solver = product("burgers", N, 2, "dirichlet", 24 * DT, gradient_stencil_size=gss)
    lin = pnmol.pde.examples.heat_1d_discretized(kernel=pnmol.kernels.SquareExponential(), nugget_gram_matrix_fd=0.0,
                                                 diffusion_rate=KAPPA, **kw(N, "dirichlet", 24 * DT))
    assert np.array_equal(lin.L, pde.L) and np.array_equal(lin.B, pde.B) and np.array_equal(lin.y0, pde.y0)
    lsolver = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=2, steprule=pnmol.odetools.step.Constant(DT),
                                              spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
    ref = lsolver.initialize(lin).y.device_state
    mean0, cov0 = ref.mean(), ref.cov()
    used = solver.initialize(pde).y.device_state
    flt = solver._device_filter
    flt.steps(used, 4, DT)                                      # graphs captured with the term
    flt.linearize(used, DT)                                     # ... and a rewritten operator left behind
    flt.prepare_error_model(DT)
    flt.set_reaction(None)
    assert flt.reaction is None
    assert _same(_loop(flt, mean0, cov0), _loop(lsolver._device_filter, mean0, cov0))
    # clearing twice, and through the convection setter itself, are no-ops
    flt.set_reaction(None)
    assert flt.lib.pnmol_filter_set_convection(flt.handle, None, None) == 0
    assert lsolver._device_filter.lib.pnmol_filter_set_convection(lsolver._device_filter.handle, None, None) == 0
    # and the diagonal host route finds its slots on the cleared filter: the same bits as on the fresh one
    jd, sh = np.linspace(-1.0, 1.0, flt.d), np.linspace(0.5, 2.0, flt.d)
    outs = []
    for f in (flt, lsolver._device_filter):
        f.set_operator_diagonal(jd, sh)
        f.prepare_error_model(DT)
        s = f.new_state()
        s.set(0.0, mean0, cov0)
        o, info, err = f.step(s, DT)
        outs.append((o.mean(), o.marginal_var(), info.diffusion_squared_local, err))
    assert all(np.array_equal(x, y) for x, y in zip(*outs))


# ------------------------------------------------------------------------------------------------------------ 6. replacing
def test_swapping_a_convection_for_a_reaction_and_back(hip_ctx):
    """A filter that goes convection -> Reaction -> convection gives, at each stage, the bits of a filter that only ever had that
    term.  The 5-point gradient makes the swap change the stencil width both ways."""
    N = 33
    pde, conv_only = product("burgers_fisher", N, 2, "dirichlet", 24 * DT, gradient_stencil_size=5)
    _, swapper = product("burgers_fisher", N, 2, "dirichlet", 24 * DT, gradient_stencil_size=5)
    rpde = pnmol.pde.examples.reaction_diffusion_1d_discretized(
        reactions.logistic(RATE), diffusion_rate=KAPPA, kernel=pnmol.kernels.SquareExponential(), nugget_gram_matrix_fd=0.0,
        **kw(N, "dirichlet", 24 * DT))
    assert np.array_equal(rpde.L, pde.L) and np.array_equal(rpde.B, pde.B)
    reac_only = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=2, steprule=pnmol.odetools.step.Constant(DT),
                                                    spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
    ref = conv_only.initialize(pde).y.device_state
    mean0, cov0 = ref.mean(), ref.cov()
    swapper.initialize(pde)
    reac_only.initialize(rpde)
    fc, fs, fr = conv_only._device_filter, swapper._device_filter, reac_only._device_filter
    want_conv, want_reac = _loop(fc, mean0, cov0), _loop(fr, mean0, cov0)
    assert not np.array_equal(want_conv[0], want_reac[0])
    assert _same(_loop(fs, mean0, cov0), want_conv)
    fs.set_reaction(rpde.reaction)
    assert _same(_loop(fs, mean0, cov0), want_reac)
    fs.set_reaction(pde.reaction)
    assert _same(_loop(fs, mean0, cov0), want_conv)
    # the single-step route after the swaps as well
    outs = []
    for f in (fs, fc):
        s = f.new_state()
        s.set(0.0, mean0, cov0)
        f.linearize(s, DT)
        f.prepare_error_model(DT)
        o, info, err = f.step(s, DT)
        outs.append((o.mean(), o.marginal_var(), info.diffusion_squared_local, err))
    assert all(np.array_equal(x, y) for x, y in zip(*outs))


def test_a_system_and_a_convection_term_share_one_image_slot(hip_ctx):
    """A filter owns one term image: system (built) -> convection (replaces it, wider) -> the same system (rebuilt) -> cleared
    gives, segment by segment, the bits of a fresh filter that only ever held that term.  d = 34, nu = 2: Lotka-Volterra on the
    two halves of the mesh adds one same-point column to every row (width 4), the 5-point gradient two (width 5)."""
    N = 34
    pde, conv_only = product("burgers", N, 2, "dirichlet", 24 * DT, gradient_stencil_size=5)
    bare = [product("burgers", N, 2, "dirichlet", 24 * DT, gradient_stencil_size=5, reaction_on_device=False)[1] for _ in range(3)]
    ref = conv_only.initialize(pde).y.device_state
    mean0, cov0 = ref.mean(), ref.cov()
    for s in bare:
        s.initialize(pde)
    fc, (fs, fsys, flin) = conv_only._device_filter, (s._device_filter for s in bare)
    assert fc.reaction is pde.reaction and fs.reaction is fsys.reaction is flin.reaction is None and fs.d == N
    system = reactions.lotka_volterra()
    fsys.set_reaction(system)
    want_sys, want_conv, want_lin = _loop(fsys, mean0, cov0), _loop(fc, mean0, cov0), _loop(flin, mean0, cov0)
    assert not np.array_equal(want_sys[0], want_conv[0]) and not np.array_equal(want_sys[0], want_lin[0])
    assert not np.array_equal(want_conv[0], want_lin[0])
    fs.set_reaction(system)
    assert _same(_loop(fs, mean0, cov0), want_sys)
    fs.set_reaction(pde.reaction)
    assert _same(_loop(fs, mean0, cov0), want_conv)
    fs.set_reaction(system)
    assert _same(_loop(fs, mean0, cov0), want_sys)
    fs.set_reaction(None)
    assert _same(_loop(fs, mean0, cov0), want_lin)


# ------------------------------------------------------------------------------------------------------------ 7. refusals
def _desc(c=(0.0, -1.0), deg_c=None, r=None):
    d = reactions.ConvectionDesc()
    d.deg_c = len(c) - 1 if deg_c is None else deg_c
    for k, v in enumerate(c):
        d.c[k] = v
    if r is None:
        d.r.deg_p = d.r.deg_a = d.r.deg_b = -1
    else:
        d.r = r
    return d


def _rdesc(p=(), a=None, b=None, degs=None):
    d = reactions.ReactionDesc()
    d.deg_p, d.deg_a, d.deg_b = len(p) - 1, -1 if a is None else len(a) - 1, -1 if b is None else len(b) - 1
    for dst, src in ((d.p, p), (d.a, a or ()), (d.b, b or ())):
        for k, v in enumerate(src):
            dst[k] = v
    if degs is not None:
        d.deg_p, d.deg_a, d.deg_b = degs
    return d


def test_every_refusal_of_the_abi(hip_ctx):
    pde, solver = product("burgers", 24, 2, "dirichlet", 2 * DT, reaction_on_device=False)
    state = solver.initialize(pde).y.device_state
    flt = solver._device_filter
    lib, h, d = flt.lib, flt.handle, flt.d
    dp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    G = np.ascontiguousarray(pde.reaction.G)
    good = _desc()
    err = lambda: lib.pnmol_last_error(flt.ctx.handle).decode()
    assert lib.pnmol_filter_set_convection(None, ctypes.byref(good), dp(G)) == -1
    assert lib.pnmol_filter_set_convection(h, ctypes.byref(good), None) == -1 and "needs its operator G" in err()
    for bad, why in [(_desc(deg_c=8), "degree"), (_desc(deg_c=-2), "degree"), (_desc(r=_rdesc(degs=(9, -1, -1))), "degree"),
                     (_desc(r=_rdesc(degs=(-1, -3, -1))), "degree"), (_desc(c=(0.0, np.nan)), "finite"),
                     (_desc(r=_rdesc(p=(np.inf,))), "finite"), (_desc(r=_rdesc(a=(1.0,))), "together"),
                     (_desc(r=_rdesc(b=(1.0,))), "together"), (_desc(r=_rdesc(a=(1.0,), b=(0.0, 0.0))), "identically zero")]:
        assert lib.pnmol_filter_set_convection(h, ctypes.byref(bad), dp(G)) == -1
        assert why in err(), (why, err())
    for poison in (np.nan, np.inf):
        Gbad = G.copy()
        Gbad[d - 1, d - 1] = poison
        assert lib.pnmol_filter_set_convection(h, ctypes.byref(good), dp(Gbad)) == -1 and "G is not finite" in err()
    # nothing was set by the refused calls: linearize refuses, the operator calls work
    assert lib.pnmol_filter_linearize(h, state.handle, DT) == -1 and "no reaction" in err()
    M, z = np.ascontiguousarray(pde.L, dtype=np.float64), np.zeros(d)
    assert lib.pnmol_filter_set_operator(h, dp(M), dp(z)) == 0
    assert lib.pnmol_filter_set_convection(h, ctypes.byref(good), dp(G)) == 0
    assert lib.pnmol_filter_linearize(h, state.handle, DT) == 0
    assert lib.pnmol_filter_set_operator(h, dp(M), dp(z)) == -1 and "clear the reaction first" in err()
    assert lib.pnmol_filter_set_operator_diagonal(h, dp(z), dp(z)) == -1 and "clear the reaction first" in err()
    assert lib.pnmol_filter_set_convection(h, None, None) == 0
    assert lib.pnmol_filter_set_operator_diagonal(h, dp(z), dp(z)) == 0
    # the Python wrapper refuses a term without G and a G of another size before any device call
    with pytest.raises(ValueError, match="no operator G"):
        flt.set_reaction(reactions.burgers())
    with pytest.raises(ValueError, match="expected shape"):
        flt.set_reaction(reactions.burgers().set_operator(np.eye(d + 1)))
    assert flt.reaction is None
    # fp32 and latent-force filters have no device path
    fkw = dict(L=pde.L, B=pde.B, E_sqrtm=pde.E_sqrtm, R_sqrtm=pde.R_sqrtm, num_derivatives=1)
    gamma = np.linalg.cholesky(solver._gram)
    f32 = _hip.Filter(flt.ctx, Gamma=gamma, dtype="f32", **fkw)
    assert lib.pnmol_filter_set_convection(f32.handle, ctypes.byref(good), dp(G)) == -1 and "fp32" in err()
    assert lib.pnmol_filter_set_convection(f32.handle, None, None) == 0
    with pytest.raises(_hip.PnmolHipError, match="pnmol_filter_set_convection"):
        f32.set_reaction(pde.reaction)
    assert f32.reaction is None
    lkw = dict(fkw, L=np.hstack((pde.L, np.eye(d))), B=np.hstack((pde.B, np.zeros_like(pde.B))))
    latent = _hip.Filter(flt.ctx, Gamma=np.linalg.cholesky(np.kron(np.eye(2), solver._gram)), **lkw)
    assert lib.pnmol_filter_set_convection(latent.handle, ctypes.byref(good), dp(G)) == -1 and "latent" in err()
    # an operator row without a diagonal entry
    Lnd = pde.L.copy()
    Lnd[3, 3] = 0.0
    nodiag = _hip.Filter(flt.ctx, Gamma=gamma, **dict(fkw, L=Lnd))
    assert lib.pnmol_filter_set_convection(nodiag.handle, ctypes.byref(good), dp(G)) == -1 and "diagonal" in err()


# ------------------------------------------------------------------------------------------------------------ 8. host routes
@pytest.mark.parametrize("route", ["reaction_on_device=False", "sqrtform"])
def test_host_routes_match_the_oracle(hip_ctx, route):
    variant, N, nu, bcond, K = "burgers", 33, 2, "dirichlet", 24
    if route == "sqrtform":
        pde, solver = product(variant, N, nu, bcond, K * DT, solver_cls=pnmol.sqrtform.SemiLinearWhiteNoiseEK1)
    else:
        pde, solver = product(variant, N, nu, bcond, K * DT, reaction_on_device=False)
    sol = solver.solve(pde)
    flt = getattr(solver, "_device_filter", None)
    assert flt is None or flt.reaction is None
    _, osol, om, os_ = oracle_solve(variant, N, nu, bcond, K)
    assert sol.info == osol.info and np.allclose(sol.t, osol.t, rtol=0, atol=1e-15)
    assert_mean_std_parity(sol.mean[:, 0], sol.marginal_std[:, 0], om, os_)
    with pytest.raises(TypeError, match="needs a linear PDE; use solve"):
        solver.solve_marginals(pde)
