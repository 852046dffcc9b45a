"""Coupled reaction descriptors (`pnmol.pde.reactions.SystemReaction`): host arithmetic against the closed forms of the system
recipes, the ctypes encoding, refusals, the problem factory.  No GPU."""

import ctypes

import numpy as np
import pytest

import pnmol
from pnmol import _hip
from pnmol.pde import examples, reactions

DX = 0.2


def _gray_scott_closed(feed, kill):
    def f(_t, x):
        u, v = np.split(x, 2)
        return np.concatenate((-u * v ** 2 + feed * (1.0 - u), u * v ** 2 - (feed + kill) * v))

    def df(_t, x):
        u, v = np.split(x, 2)
        return np.block([[np.diag(-v ** 2 - feed), np.diag(-2.0 * u * v)],
                         [np.diag(v ** 2), np.diag(2.0 * u * v - (feed + kill))]])

    return f, df


def _cases():
    lv, sir = examples.lotka_volterra_1d_discretized(dx=DX), examples.sir_1d_discretized(dx=DX)
    gs_f, gs_df = _gray_scott_closed(0.04, 0.06)
    return {"lotka_volterra": (reactions.lotka_volterra(), lv.f, lv.df, lv.y0 * 1.01 + 0.3),
            "sir": (reactions.sir(), sir.f, sir.df, sir.y0 * 1.01 + 0.3),
            "gray_scott": (reactions.gray_scott(0.04, 0.06), gs_f, gs_df, lv.y0 * 1.01 + 0.3)}


CASES = _cases()


def _scatter(blocks):
    C, _, N = blocks.shape
    out = np.zeros((C * N, C * N))
    for c in range(C):
        for k in range(C):
            out[c * N + np.arange(N), k * N + np.arange(N)] = blocks[c, k]
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_presets_match_the_closed_forms(name):
    r, f, df, x = CASES[name]
    N = x.size // r.ncomp
    assert r.value(x).shape == (r.ncomp * N,) and r.jacobian_blocks(x).shape == (r.ncomp, r.ncomp, N)
    J = df(0.0, x)
    np.testing.assert_allclose(r.value(x), f(0.0, x), rtol=1e-13)
    np.testing.assert_allclose(_scatter(r.jacobian_blocks(x)), J, rtol=1e-13)
    assert np.array_equal(_scatter(r.jacobian_blocks(x)) != 0.0, J != 0.0)         # the same structural zeros
    fc, dfc, dfd = r.callables()
    assert dfd is None and np.array_equal(fc(0.3, x), r.value(x)) and np.array_equal(dfc(0.3, x), _scatter(r.jacobian_blocks(x)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_jacobian_matches_central_differences(name):
    """The tolerances of tests/test_systems.py::test_system_recipes_match_oracle."""
    r, _, _, x = CASES[name]
    J = _scatter(r.jacobian_blocks(x))
    h = 1e-6
    Jn = np.stack([(r.value(x + h * e) - r.value(x - h * e)) / (2 * h) for e in np.eye(x.size)], axis=1)
    np.testing.assert_allclose(J, Jn, rtol=1e-6, atol=1e-7 * np.abs(J).max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_shift_is_the_jacobian_times_the_state_minus_the_value(name):
    r, _, _, x = CASES[name]
    J, v = r.jacobian_blocks(x), r.value(x)
    us = x.reshape(r.ncomp, -1)
    want = np.einsum("ckj,kj->cj", J, us).reshape(-1) - v
    # C products and C additions of terms of size |J u| <= C max|J_ck u_k|: a few roundings of that size
    scale = np.abs(J * us[None]).max()
    np.testing.assert_allclose(r.shift(x), want, rtol=0, atol=8 * np.finfo(float).eps * scale)
    assert r.shift(x).shape == x.shape and np.abs(r.shift(x)).max() > 0.0


def test_order_of_operations_is_the_documented_one():
    """A monomial starts from its coefficient and takes u_0 first; a polynomial starts from its first term; the derivative starts
    from e * coef."""
    r = reactions.SystemReaction(2, p=[[(0.1, (2, 1)), (0.3, (0, 3))], []])
    u, v = np.array([1.1, 0.7, 3.3]), np.array([0.9, 1.7, 0.3])
    x = np.concatenate((u, v))
    assert np.array_equal(r.value(x)[:3], ((0.1 * u) * u) * v + ((0.3 * v) * v) * v)
    J = r.jacobian_blocks(x)
    assert np.array_equal(J[0, 0], ((2 * 0.1) * u) * v)
    assert np.array_equal(J[0, 1], (0.1 * u) * u + ((3 * 0.3) * v) * v)
    assert np.array_equal(J[1], np.zeros((2, 3))) and np.array_equal(r.value(x)[3:], np.zeros(3))
    assert np.array_equal(r.shift(x)[:3], (J[0, 0] * u + J[0, 1] * v) - r.value(x)[:3])


def test_ctypes_encoding_round_trips():
    assert (reactions.MAXCOMP, reactions.MAXTERMS) == (4, 8)
    assert ctypes.sizeof(reactions.MonomialDesc) == 24 and ctypes.sizeof(reactions.SystemPolyDesc) == 200
    assert ctypes.sizeof(reactions.SystemReactionDesc) == 2408
    full = reactions.SystemReaction(4, p=[[(float(t + 1), (t % 8, 7, 0, 1)) for t in range(8)]] + [[]] * 3,
                                    a=[[], [(1.0, (0, 0, 0, 0))], [], []], b=[[], [(2.0, (1, 0, 0, 1)), (0.5, (0, 0, 0, 0))], [], []])
    for r in (reactions.lotka_volterra(), reactions.sir(), reactions.gray_scott(0.04, 0.06), full,
              reactions.SystemReaction(1, p=[[]])):
        desc = r.to_ctypes()
        assert desc.ncomp == r.ncomp
        for c in range(r.ncomp):
            assert (desc.p[c].nterms, desc.a[c].nterms, desc.b[c].nterms) == (len(r.p[c]), len(r.a[c]), len(r.b[c]))
        for c in range(r.ncomp, 4):
            assert (desc.p[c].nterms, desc.a[c].nterms, desc.b[c].nterms) == (0, 0, 0)
        back = reactions.SystemReaction.from_ctypes(desc)
        assert (back.ncomp, back.p, back.a, back.b) == (r.ncomp, r.p, r.a, r.b)
    d = reactions.sir().to_ctypes()
    assert d.a[0].term[0].coef == -0.3 and list(d.a[0].term[0].pow) == [1, 1, 0, 0] and d.b[1].nterms == 3


def test_library_exports_the_system_setter():
    assert _hip.SYMBOLS["pnmol_filter_set_reaction_system"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
    lib = _hip.load_library()                                   # exported; argument checks need no GPU
    assert lib.pnmol_filter_set_reaction_system(None, None) == -1
    desc = reactions.lotka_volterra().to_ctypes()
    assert lib.pnmol_filter_set_reaction_system(None, ctypes.byref(desc)) == -1


def test_invalid_descriptors_raise_before_any_device_call():
    S = reactions.SystemReaction
    one = [(1.0, (1, 0))]
    with pytest.raises(ValueError, match="ncomp = 0"):
        S(0, p=[])
    with pytest.raises(ValueError, match="ncomp = 5"):
        S(5, p=[[]] * 5)
    with pytest.raises(ValueError, match="p has 1 entries for ncomp = 2"):
        S(2, p=[one])
    with pytest.raises(ValueError, match="9 terms"):
        S(2, p=[one * 9, []])
    with pytest.raises(ValueError, match=r"exponent outside \[0, 7\]"):
        S(2, p=[[(1.0, (8, 0))], []])
    with pytest.raises(ValueError, match=r"exponent outside \[0, 7\]"):
        S(2, p=[[(1.0, (0, -1))], []])
    with pytest.raises(ValueError, match="species >= ncomp"):
        S(2, p=[[(1.0, (1, 0, 1))], []])
    with pytest.raises(ValueError, match="not \\(coefficient, exponents\\)"):
        S(2, p=[[(1.0, (1, 0, 0, 0, 0))], []])
    with pytest.raises(ValueError, match="not \\(coefficient, exponents\\)"):
        S(2, p=[[(1.0, (1.5, 0))], []])
    with pytest.raises(ValueError, match="not \\(coefficient, exponents\\)"):
        S(2, p=[[1.0], []])
    with pytest.raises(ValueError, match="together"):
        S(2, p=[[], []], a=[one, []])
    with pytest.raises(ValueError, match="together"):
        S(2, p=[[], []], a=[one, []], b=[[], []])
    with pytest.raises(ValueError, match="together"):
        S(2, p=[[], []], a=[[], []], b=[[], one])
    with pytest.raises(ValueError, match="not finite"):
        S(2, p=[[(np.nan, (1, 0))], []])
    with pytest.raises(ValueError, match="not finite"):
        S(2, p=[[], []], a=[one, []], b=[[(np.inf, (0, 0))], []])
    with pytest.raises(ValueError, match="identically zero"):
        S(2, p=[[], []], a=[one, []], b=[[(0.0, (0, 0)), (0.0, (1, 0))], []])
    with pytest.raises(ValueError, match="ncomp \\* N"):
        reactions.lotka_volterra().value(np.ones(5))


@pytest.mark.parametrize("name,ncomp", [("lotka_volterra", 2), ("sir", 3)])
def test_new_recipe_discretises_like_the_existing_ones(name, ncomp):
    ref = getattr(examples, name + "_1d_discretized")(dx=DX, tmax=2.0)
    r = getattr(reactions, name)()
    y0 = examples.lotka_volterra_y0 if ncomp == 2 else examples.sir_y0
    pde = examples.reaction_diffusion_system_1d_discretized(r, diffusion_rates=(0.1,) * ncomp, y0_fun=y0, dx=DX, tmax=2.0)
    assert pde.reaction is r and type(pde) is type(ref) and not hasattr(ref, "reaction")
    for attr in ("L", "B", "E_sqrtm", "R_sqrtm", "y0"):
        assert np.array_equal(getattr(pde, attr), getattr(ref, attr)), attr
    assert (pde.t0, pde.tmax) == (ref.t0, ref.tmax) and pde.df_diagonal is None
    x = pde.y0 * 1.01 + 0.3
    assert np.array_equal(pde.f(0.0, x), r.value(x))
    np.testing.assert_allclose(pde.f(0.0, x), ref.f(0.0, x), rtol=1e-13)
    np.testing.assert_allclose(pde.df(0.0, x), ref.df(0.0, x), rtol=1e-13)
    with pytest.raises(ValueError, match="diffusion rates"):
        examples.reaction_diffusion_system_1d_discretized(r, diffusion_rates=(0.1,), y0_fun=y0, dx=DX)


def test_solver_chooses_the_device_path_only_where_it_exists():
    r = reactions.lotka_volterra()
    pde = examples.reaction_diffusion_system_1d_discretized(r, diffusion_rates=(0.1, 0.1), y0_fun=examples.lotka_volterra_y0,
                                                            dx=DX, tmax=0.1)
    plain = examples.lotka_volterra_1d_discretized(dx=DX, tmax=0.1)
    kw = dict(num_derivatives=1, steprule=pnmol.odetools.step.Constant(0.01))
    solver = pnmol.white.SemiLinearWhiteNoiseEK1(**kw)
    assert solver._reaction_for_device(pde) is r and solver._reaction_for_device(plain) is None
    solver.reaction_on_device = False
    assert solver._reaction_for_device(pde) is None
    f32 = pnmol.white.SemiLinearWhiteNoiseEK1(**kw)
    f32.dtype = "f32"
    assert f32._reaction_for_device(pde) is None
    assert pnmol.sqrtform.SemiLinearWhiteNoiseEK1(**kw)._reaction_for_device(pde) is None
    assert pnmol.latent.SemiLinearLatentForceEK1(**kw)._reaction_for_device(pde) is None
    with pytest.raises(TypeError, match="needs a linear PDE; use solve"):
        pnmol.white.SemiLinearWhiteNoiseEK1(**kw).solve_marginals(plain)
