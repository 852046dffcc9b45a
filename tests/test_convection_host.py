"""Convection terms on the host (`pnmol.pde.reactions.Convection`, `pde.examples.convection_diffusion_1d_discretized`): the
structured linearisation against finite differences and the dense callables, its order of operations, the ctypes encoding,
argument checks, the recipe, the solver's choice of route, and -- with the oracle alone -- that the Burgers term moves the
solution far enough for parity against the oracle to mean something.  No GPU."""

import ctypes

import numpy as np
import pytest

import pnmol
import pnmol_oracle as oracle
from convection_reference import CASES, DT, KAPPA, oracle_gradient, oracle_problem, oracle_solve, product
from pnmol import _hip
from pnmol.pde import examples, reactions


def _term(variant="burgers_fisher", d=9, seed=0, speed=None):
    rng = np.random.default_rng(seed)
    G = np.zeros((d, d))
    for i in range(d):                                           # three-point rows, one wider row, one row without entries
        for k in (i - 1, i, i + 1):
            if 0 <= k < d:
                G[i, k] = rng.standard_normal()
    G[4, 0], G[2, :] = 0.7, 0.0
    term = {"burgers": reactions.burgers(), "burgers_fisher": reactions.burgers_fisher(0.8),
            "cubic": reactions.Convection(speed or (0.3, -1.0, 0.0, 0.25), reaction=reactions.budworm(0.5, 3.0))}[variant]
    return term.set_operator(G), G, rng.uniform(0.2, 1.5, d)


@pytest.mark.parametrize("variant", ["burgers", "burgers_fisher", "cubic"])
def test_linearization_is_the_jacobian_of_value(variant):
    term, G, u = _term(variant)
    J, shift = term.linearization(u)
    h = 1e-6
    Jn = np.stack([(term.value(u + h * e) - term.value(u - h * e)) / (2 * h) for e in np.eye(u.size)], axis=1)
    np.testing.assert_allclose(J, Jn, rtol=1e-6, atol=1e-7 * np.abs(J).max())
    # the row without entries of G: r' alone, on the diagonal
    assert np.array_equal(J[2] != 0.0, (np.arange(u.size) == 2) & (variant != "burgers"))
    # shift = J u - f: a row has at most 4 products and sums of size |J u|
    scale = np.abs(J * u[None]).max()
    np.testing.assert_allclose(shift, J @ u - term.value(u), rtol=0, atol=16 * np.finfo(float).eps * scale)
    assert np.abs(shift).max() > 1e-2


def test_value_matches_the_closed_forms():
    term, G, u = _term("burgers")
    np.testing.assert_allclose(term.value(u), -u * (G @ u), rtol=1e-13, atol=1e-15)
    term, G, u = _term("burgers_fisher")
    np.testing.assert_allclose(term.value(u), -u * (G @ u) + 0.8 * u * (1.0 - u), rtol=1e-13, atol=1e-15)
    J, _ = term.linearization(u)
    np.testing.assert_allclose(J, -(np.diag(G @ u) + u[:, None] * G) + np.diag(0.8 * (1.0 - 2.0 * u)), rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("variant", ["burgers", "burgers_fisher", "cubic"])
def test_callables_agree_with_linearization(variant):
    term, G, u = _term(variant)
    f, df, dfd = term.callables()
    assert dfd is None
    J, shift = term.linearization(u)
    assert np.array_equal(f(0.3, u), term.value(u))
    np.testing.assert_allclose(df(0.3, u), J, rtol=1e-15, atol=0)
    scale = np.abs(J * u[None]).max()
    np.testing.assert_allclose(df(0.3, u) @ u - f(0.3, u), shift, rtol=0, atol=16 * np.finfo(float).eps * scale)


def test_order_of_operations_is_the_documented_one():
    """g over the non-zero entries of a row of G in ascending column order from the first product; q = c' g + r'; entries
    L_ij + c_i G_ij, the diagonal one (L_ii + c_i G_ii) + q_i; shift q u - r; every operation rounded on its own."""
    term, G, u = _term("burgers_fisher")
    d = u.size
    L = np.random.default_rng(1).standard_normal((d, d))
    M, shift = term.linearization(u, L=L)
    r, dr = term.reaction.value(u), term.reaction.derivative(u)
    for i in range(d):
        cols = np.flatnonzero(G[i])
        g = 0.0
        for n, k in enumerate(cols):
            g = G[i, k] * u[k] if n == 0 else g + G[i, k] * u[k]
        c = -1.0 * u[i] + 0.0                                    # Horner: v = c[1]; v = v * u + c[0]
        q = -1.0 * g + dr[i]                                     # c' = 1 * c[1]
        for k in range(d):
            want = L[i, k] + c * G[i, k]
            if k == i:
                want = want + q
            assert M[i, k] == want, (i, k)
        assert shift[i] == q * u[i] - r[i]
    # without a reaction q is c' g alone and the shift q u
    term, G, u = _term("burgers")
    J, shift = term.linearization(u)
    g = term._gradient(u)
    assert np.array_equal(np.diag(J), (-u) * np.diag(G) + (-1.0) * g) and np.array_equal(shift, ((-1.0) * g) * u)
    assert np.array_equal(term.linearization(u, L=np.zeros((d, d)))[0], J)


def test_ctypes_encoding_round_trips():
    assert ctypes.sizeof(reactions.ConvectionDesc) == 8 + 64 + ctypes.sizeof(reactions.ReactionDesc) == 280
    for term in (reactions.burgers(), reactions.burgers_fisher(0.3),
                 reactions.Convection((0.1,) * 8, reaction=reactions.budworm(0.5, 3.0))):
        desc = term.to_ctypes()
        assert desc.deg_c == len(term.speed) - 1 and tuple(desc.c[: desc.deg_c + 1]) == term.speed
        back = reactions.Convection.from_ctypes(desc)
        assert back.speed == term.speed and (back.reaction is None) == (term.reaction is None)
        if term.reaction is not None:
            assert (back.reaction.p, back.reaction.a, back.reaction.b) == (term.reaction.p, term.reaction.a, term.reaction.b)
    d = reactions.burgers().to_ctypes()
    assert (d.deg_c, d.c[0], d.c[1], d.r.deg_p, d.r.deg_a, d.r.deg_b) == (1, 0.0, -1.0, -1, -1, -1)
    d = reactions.burgers_fisher(2.0).to_ctypes()
    assert (d.r.deg_p, d.r.deg_a, d.r.deg_b) == (2, -1, -1) and tuple(d.r.p[:3]) == (0.0, 2.0, -2.0)


def test_invalid_arguments_raise_before_any_device_call():
    C = reactions.Convection
    with pytest.raises(ValueError, match="Convection: speed has degree 8"):
        C((1.0,) * 9)
    with pytest.raises(ValueError, match="Convection: speed has a coefficient that is not finite"):
        C((0.0, np.nan))
    with pytest.raises(ValueError, match="Convection: speed must be a 1-d sequence"):
        C(np.ones((2, 2)))
    with pytest.raises(ValueError, match="speed is empty"):
        C(())
    with pytest.raises(TypeError, match="Reaction or None"):
        C((0.0, -1.0), reaction=reactions.lotka_volterra())
    term = reactions.burgers()
    with pytest.raises(ValueError, match="no operator G"):
        term.value(np.ones(3))
    with pytest.raises(ValueError, match="square"):
        term.set_operator(np.ones((3, 4)))
    with pytest.raises(ValueError, match="not finite"):
        term.set_operator(np.array([[1.0, np.inf], [0.0, 1.0]]))
    term.set_operator(np.eye(3))
    with pytest.raises(ValueError, match="expected a vector of 3 entries"):
        term.value(np.ones(4))
    with pytest.raises(ValueError, match="L has shape"):
        term.linearization(np.ones(3), L=np.eye(4))


def test_library_exports_the_convection_setter():
    assert _hip.SYMBOLS["pnmol_filter_set_convection"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p,
                                                                           ctypes.POINTER(ctypes.c_double)])
    lib = _hip.load_library()                                   # exported; argument checks need no GPU
    assert lib.pnmol_filter_set_convection(None, None, None) == -1
    desc = reactions.burgers().to_ctypes()
    G = np.eye(3)
    assert lib.pnmol_filter_set_convection(None, ctypes.byref(desc), G.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == -1
    assert lib.pnmol_abi_version() == 3


@pytest.mark.parametrize("bcond", ["dirichlet", "neumann"])
def test_burgers_recipe(bcond):
    N = 33
    h = 1.0 / (N - 1)
    pde = examples.burgers_1d_discretized(dx=h, bcond=bcond, tmax=1.0, kernel=pnmol.kernels.SquareExponential())
    heat = examples.heat_1d_discretized(dx=h, bcond=bcond, tmax=1.0, diffusion_rate=0.02, kernel=pnmol.kernels.SquareExponential())
    term = pde.reaction
    assert isinstance(term, reactions.Convection) and term.speed == (0.0, -1.0) and term.reaction is None
    for attr in ("L", "B", "E_sqrtm", "R_sqrtm"):                # the Laplacian's, E_sqrtm included
        assert np.array_equal(getattr(pde, attr), getattr(heat, attr)), attr
    G = term.G
    assert G.shape == (N, N) and pde.df_diagonal is None
    rows = np.array([G[i, i - 1:i + 2] for i in range(1, N - 1)]) * 2 * h
    worst = np.abs(rows - np.array([-1.0, 0.0, 1.0])).max()
    print(f"interior rows of G times 2h: largest deviation from [-1, 0, 1] {worst:.2e}")
    assert worst < 1e-3
    assert np.array_equal(G != 0.0, pde.L != 0.0)                # equal stencil sizes: the pattern of L
    # ... and it is the oracle's kernel finite-difference gradient, whose uncertainty stays unmodelled
    oG, unc = oracle_gradient(oracle.RectMesh.from_bbox_1d(np.array([0.0, 1.0]), step=h), oracle.SquareExponential())
    np.testing.assert_allclose(G, oG, rtol=1e-12, atol=1e-13 * np.abs(oG).max())
    assert 0.0 <= np.abs(unc).max() < 1e-6
    x = pde.y0 * 1.01 + 0.3
    np.testing.assert_allclose(pde.f(0.0, x), -x * (G @ x), rtol=1e-13, atol=1e-15)
    M, shift = pnmol.white.SemiLinearWhiteNoiseEK1._linearize(pde, x, 0.0)
    assert np.array_equal(M, term.linearization(x, L=pde.L)[0]) and np.array_equal(shift, term.linearization(x)[1])
    np.testing.assert_allclose(M, pde.L + pde.df(0.0, x), rtol=1e-13, atol=1e-13 * np.abs(M).max())
    wide = examples.burgers_1d_discretized(dx=h, bcond=bcond, gradient_stencil_size=5)
    assert (wide.reaction.G != 0.0).sum(axis=1).max() == 5 and (wide.L != 0.0).sum(axis=1).max() == 3
    with pytest.raises(ValueError):
        examples.burgers_1d_discretized(dx=h, bcond="periodic")


def test_solver_chooses_the_device_path_only_where_it_exists():
    pde, solver = product("burgers", 17, 1, "dirichlet", 2 * DT)
    plain = examples.spruce_budworm_1d_discretized(dx=1.0 / 16, tmax=2 * DT)
    term = pde.reaction
    assert solver._reaction_for_device(pde) is term and solver._reaction_for_device(plain) is None
    solver.reaction_on_device = False
    assert solver._reaction_for_device(pde) is None
    kw = dict(num_derivatives=1, steprule=pnmol.odetools.step.Constant(DT))
    f32 = pnmol.white.SemiLinearWhiteNoiseEK1(**kw)
    f32.dtype = "f32"
    assert f32._reaction_for_device(pde) is None
    assert pnmol.sqrtform.SemiLinearWhiteNoiseEK1(**kw)._reaction_for_device(pde) is None
    assert pnmol.latent.SemiLinearLatentForceEK1(**kw)._reaction_for_device(pde) is None
    # every host route takes the structured form
    x = pde.y0 * 0.9 + 0.1
    for cls in (pnmol.white.SemiLinearWhiteNoiseEK1, pnmol.sqrtform.SemiLinearWhiteNoiseEK1, pnmol.latent.SemiLinearLatentForceEK1):
        M, shift = cls._linearize(pde, x, 0.0)
        assert np.array_equal(M, term.linearization(x, L=pde.L)[0]) and np.array_equal(shift, term.linearization(x)[1])


def test_product_problem_equals_the_oracle_problem():
    for N, _, bcond, K in CASES[:3]:
        pde, _ = product("burgers_fisher", N, 2, bcond, K * DT)
        op = oracle_problem("burgers_fisher", N, bcond, K * DT)
        for attr in ("L", "B", "R_sqrtm", "y0"):
            np.testing.assert_allclose(getattr(pde, attr), getattr(op, attr), rtol=1e-13, atol=1e-15, err_msg=attr)
        assert pde.diffop_scale == KAPPA
        x = pde.y0 * 0.9 + 0.1
        np.testing.assert_allclose(pde.f(0.0, x), op.f(0.0, x), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(pde.df(0.0, x), op.df(0.0, x), rtol=1e-12, atol=1e-13 * np.abs(op.df(0.0, x)).max())


@pytest.mark.parametrize("N,nu,bcond,K", CASES)
def test_the_burgers_term_moves_the_oracle_solution(N, nu, bcond, K):
    """The oracle alone, Burgers against heat with the same data: the final means differ by at least a tenth of the largest
    entry (measured 0.32, 0.32, 0.21, 0.155), so parity of the device route against the oracle is no parity of heat solvers."""
    _, _, m, s = oracle_solve("burgers", N, nu, bcond, K)
    _, _, m0, _ = oracle_solve("heat", N, nu, bcond, K)
    assert np.all(np.isfinite(m)) and np.all(np.isfinite(s)) and m.shape == (K + 1, N)
    moved = np.abs(m[-1] - m0[-1]).max() / np.abs(m[-1]).max()
    print(f"N={N} nu={nu} {bcond}: the convection term moves the final mean by {moved:.3f} of its largest entry")
    assert moved >= 0.1
