"""Reaction descriptors (`pnmol.pde.reactions`): host arithmetic, the problem factory, the ctypes encoding.  No GPU."""

import ctypes

import numpy as np
import pytest

import pnmol
from pnmol import _hip
from pnmol.pde import reactions

U = np.linspace(-1.5, 2.5, 41)

# (constructor, closed-form value, closed-form derivative)
CLOSED_FORMS = {
    "logistic": (lambda: reactions.logistic(0.7), lambda u: 0.7 * u * (1.0 - u), lambda u: 0.7 * (1.0 - 2.0 * u)),
    "allen_cahn": (reactions.allen_cahn, lambda u: u - u ** 3, lambda u: 1.0 - 3.0 * u ** 2),
    "nagumo": (lambda: reactions.nagumo(0.3), lambda u: u * (1.0 - u) * (u - 0.3),
               lambda u: (1.0 - 2.0 * u) * (u - 0.3) + u * (1.0 - u)),
    "budworm": (lambda: reactions.budworm(0.5, 3.0), lambda u: 0.5 * u * (1.0 - u / 3.0) - u ** 2 / (1.0 + u ** 2),
                lambda u: 0.5 * (1.0 - 2.0 * u / 3.0) - 2.0 * u / (1.0 + u ** 2) ** 2),
}


@pytest.mark.parametrize("name", sorted(CLOSED_FORMS))
def test_value_and_derivative_match_the_closed_forms(name):
    make, value, derivative = CLOSED_FORMS[name]
    r = make()
    # Horner against the closed form: a handful of roundings of O(|u|^3) terms
    np.testing.assert_allclose(r.value(U), value(U), rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(r.derivative(U), derivative(U), rtol=1e-13, atol=1e-14)
    assert r.value(U).shape == U.shape and r.value(0.25).shape == ()


@pytest.mark.parametrize("name", sorted(CLOSED_FORMS))
def test_derivative_matches_central_differences(name):
    r = CLOSED_FORMS[name][0]()
    h = 1e-5                                                    # truncation h^2 |r'''| / 6 ~ 1e-10, rounding eps |r| / h ~ 1e-10
    fd = (r.value(U + h) - r.value(U - h)) / (2.0 * h)
    np.testing.assert_allclose(r.derivative(U), fd, rtol=0, atol=1e-8)


def test_general_rational_reaction():
    r = reactions.Reaction(p=(0.5,), a=(1.0, 2.0, 0.0, -1.0), b=(2.0, 0.0, 0.5))
    A, dA = 1.0 + 2.0 * U - U ** 3, 2.0 - 3.0 * U ** 2
    B, dB = 2.0 + 0.5 * U ** 2, U
    np.testing.assert_allclose(r.value(U), 0.5 + A / B, rtol=1e-13)
    np.testing.assert_allclose(r.derivative(U), (dA * B - A * dB) / B ** 2, rtol=1e-12, atol=1e-14)
    zero = reactions.Reaction()
    assert np.array_equal(zero.value(U), np.zeros_like(U)) and np.array_equal(zero.derivative(U), np.zeros_like(U))
    const = reactions.Reaction(p=(0.0,))
    assert np.array_equal(const.value(U), np.zeros_like(U)) and np.array_equal(const.derivative(U), np.zeros_like(U))


def test_callables_agree_with_each_other():
    r = reactions.budworm(0.5, 3.0)
    f, df, df_diagonal = r.callables()
    u = U[:9]
    assert np.array_equal(f(0.3, u), r.value(u))
    assert np.array_equal(df_diagonal(0.3, u), r.derivative(u))
    J = df(0.3, u)
    assert J.shape == (9, 9) and np.array_equal(np.diag(J), df_diagonal(0.3, u))
    assert np.array_equal(J, np.diag(np.diag(J)))


@pytest.mark.parametrize("bcond", ["dirichlet", "neumann"])
def test_factory_takes_its_callables_from_the_reaction(bcond):
    r = reactions.logistic(1.0)
    kw = dict(tmax=0.5, dx=1.0 / 15, diffusion_rate=0.05, bcond=bcond)
    pde = pnmol.pde.examples.reaction_diffusion_1d_discretized(r, kernel=pnmol.kernels.SquareExponential(), **kw)
    ref = pnmol.pde.examples.spruce_budworm_1d_discretized(kernel=pnmol.kernels.SquareExponential(), **kw)
    assert pde.reaction is r and type(pde) is type(ref)
    u = np.asarray(pde.y0)
    assert np.array_equal(pde.f(0.0, u), r.value(u))
    assert np.array_equal(pde.df_diagonal(0.0, u), r.derivative(u))
    assert np.array_equal(np.diag(pde.df(0.0, u)), r.derivative(u))
    # the same discretisation as the spruce-budworm recipe, whose problem carries no reaction
    assert np.array_equal(pde.L, ref.L) and np.array_equal(pde.B, ref.B) and np.array_equal(pde.y0, ref.y0)
    assert np.array_equal(pde.E_sqrtm, ref.E_sqrtm) and pde.tmax == ref.tmax
    assert not hasattr(ref, "reaction")
    np.testing.assert_allclose(pde.f(0.0, u), ref.f(0.0, u), rtol=1e-14, atol=1e-16)


def test_ctypes_encoding_round_trips():
    assert reactions.MAXDEG == 7
    assert ctypes.sizeof(reactions.ReactionDesc) == 4 * 4 + 3 * 8 * 8   # three ints, padding, 3 x 8 doubles (pnmol_reaction)
    for r in (reactions.budworm(0.5, 3.0), reactions.nagumo(0.25), reactions.Reaction(),
              reactions.Reaction(p=np.arange(1.0, 9.0), a=(1.0,), b=np.arange(8.0, 0.0, -1.0))):
        desc = r.to_ctypes()
        assert desc.deg_p == len(r.p) - 1
        assert (desc.deg_a, desc.deg_b) == ((-1, -1) if r.a is None else (len(r.a) - 1, len(r.b) - 1))
        assert list(desc.p[len(r.p):]) == [0.0] * (8 - len(r.p))
        back = reactions.Reaction.from_ctypes(desc)
        assert (back.p, back.a, back.b) == (r.p, r.a, r.b)
    assert _hip.SYMBOLS["pnmol_filter_set_reaction"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
    assert _hip.SYMBOLS["pnmol_filter_linearize"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double])
    lib = _hip.load_library()                                   # exported; argument checks need no GPU
    assert lib.pnmol_filter_set_reaction(None, None) == -1
    assert lib.pnmol_filter_linearize(None, None, 0.1) == -1


def test_invalid_descriptors_raise_before_any_device_call():
    with pytest.raises(ValueError, match="together"):
        reactions.Reaction(a=(1.0,))
    with pytest.raises(ValueError, match="together"):
        reactions.Reaction(p=(1.0,), b=(1.0,))
    with pytest.raises(ValueError, match="degree 8"):
        reactions.Reaction(p=np.ones(9))
    with pytest.raises(ValueError, match="degree 8"):
        reactions.Reaction(a=(1.0,), b=np.ones(9))
    with pytest.raises(ValueError, match="not finite"):
        reactions.Reaction(p=(0.0, np.nan))
    with pytest.raises(ValueError, match="not finite"):
        reactions.Reaction(a=(np.inf,), b=(1.0,))
    with pytest.raises(ValueError, match="identically zero"):
        reactions.Reaction(a=(1.0,), b=(0.0, 0.0))
    with pytest.raises(ValueError, match="a is empty"):
        reactions.Reaction(a=(), b=(1.0,))
    with pytest.raises(ValueError, match="b is empty"):
        reactions.Reaction(a=(1.0,), b=())
    with pytest.raises(ValueError, match="1-d"):
        reactions.Reaction(p=np.ones((2, 2)))


def test_solver_chooses_the_device_path_only_where_it_exists():
    r = reactions.logistic(1.0)
    pde = pnmol.pde.examples.reaction_diffusion_1d_discretized(r, tmax=0.1, dx=0.1, diffusion_rate=0.05)
    plain = pnmol.pde.examples.spruce_budworm_1d_discretized(tmax=0.1, dx=0.1, diffusion_rate=0.05)
    kw = dict(num_derivatives=1, steprule=pnmol.odetools.step.Constant(0.01))
    solver = pnmol.white.SemiLinearWhiteNoiseEK1(**kw)
    assert solver.reaction_on_device is True and solver._reaction_for_device(pde) is r
    assert solver._reaction_for_device(plain) is None
    solver.reaction_on_device = False
    assert solver._reaction_for_device(pde) is None
    f32 = pnmol.white.SemiLinearWhiteNoiseEK1(**kw)
    f32.dtype = "f32"
    assert f32._reaction_for_device(pde) is None
    assert pnmol.sqrtform.SemiLinearWhiteNoiseEK1(**kw)._reaction_for_device(pde) is None
    assert pnmol.white.LinearWhiteNoiseEK1(**kw)._reaction_for_device(pde) is None
    assert pnmol.latent.SemiLinearLatentForceEK1(**kw)._reaction_for_device(pde) is None
    with pytest.raises(TypeError, match="needs a linear PDE; use solve"):
        pnmol.white.SemiLinearWhiteNoiseEK1(**kw).solve_marginals(plain)
