"""CPU tests of driven problems (`pnmol.pde.forcing`, `pnmol_filter_set_forcing`, `pnmol_filter_force_at`): the
host logic of the table of right-hand sides (csrc/pnmol_forcing_plan.hpp, nothing of HIP in it) under AddressSanitizer + UBSan --
tests/forcing_plan_check.cpp is a stand-alone program that includes nothing but that header --, the C ABI's new names,
`Forcing.table` against the constant schedule, the refusals in front of any device work, the recipes' `f`, and the condition
that the cases of tests/test_gpu_forcing.py must meet on the NumPy reference alone (tests/forcing_reference.py).  No GPU."""

import pathlib
import re
import subprocess

import numpy as np
import pytest

import pnmol
import forcing_reference as fr
from pnmol import _hip
from pnmol.pde import examples, reactions
from pnmol.pde.forcing import Forcing

ROOT = pathlib.Path(__file__).resolve().parent.parent
CLANG = pathlib.Path("/opt/rocm/lib/llvm/bin/clang++")
NAMES = ("pnmol_filter_set_forcing", "pnmol_filter_forcing_pending", "pnmol_filter_force_at")


@pytest.mark.skipif(not CLANG.exists(), reason="the ROCm clang++ is not available")
def test_forcing_plan_host_logic_under_asan_ubsan(tmp_path):
    exe = tmp_path / "forcing_plan_check"
    subprocess.run([str(CLANG), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'pnmol-experiments_amd' / 'csrc'}", str(ROOT / "tests" / "forcing_plan_check.cpp"), "-o", str(exe)],
                   check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "forcing plan: ok" and "runtime error" not in run.stderr


def test_forcing_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "pnmol_hip.h").read_text()
    lib = _hip.load_library()
    for name in NAMES:
        assert name in _hip.SYMBOLS
        assert re.search(rf"\bint {name}\(", header)
        assert hasattr(lib, name)
    assert lib.pnmol_abi_version() == 3
    for method in ("set_forcing", "clear_forcing", "forcing_pending", "force_at"):
        assert method in dir(_hip.Filter)
    assert (ROOT / "pnmol-experiments_amd" / "csrc" / "pnmol_forcing.hip") in __import__("__graft_entry__").SOURCES


def test_table_follows_the_constant_schedule_runt_step_included():
    dt = fr.DT
    pde, solver, _, _ = fr.linear_pair(20, 1, "dirichlet", "both", K=12.3)
    ts, dts = solver._constant_schedule(pde, None)
    assert len(dts) == 13 and dts[-1] < dts[0]
    table = pde.forcing.table(ts, pde)
    d, nB = pde.L.shape[0], pde.B.shape[0]
    assert table.shape == (13, d + nB) and np.array_equal(table, solver._forcing_table(pde, ts))
    for k in range(13):
        assert np.array_equal(table[k, :d], fr.source(ts[k + 1], pde.mesh_spatial.points))
        assert np.array_equal(table[k, d:], pde.B @ pde.y0 + fr.G_AMP * np.sin(fr.G_RATE * ts[k + 1]))
        assert np.array_equal(table[k], pde.forcing.rhs(ts[k + 1], pde))
    assert ts[-1] == pde.tmax and ts[-2] == 12 * dt
    ts5, _ = solver._constant_schedule(pde, 5)
    assert np.array_equal(pde.forcing.table(ts5, pde), table[:5])
    assert pde.forcing.table(ts[:1], pde).shape == (0, d + nB)
    # None means zeros
    only_g = Forcing(boundary_values=pde.forcing.boundary_values)
    assert np.array_equal(only_g.rhs(0.1, pde), np.concatenate((np.zeros(d), pde.forcing.boundary(0.1, pde))))
    assert np.array_equal(Forcing().rhs(0.3, pde), np.zeros(d + nB))
    # shape and finiteness, on the host
    with pytest.raises(ValueError, match=r"source\(t, X\).*shape"):
        Forcing(source=lambda t, X: np.zeros(d + 1)).rhs(0.0, pde)
    with pytest.raises(ValueError, match=r"boundary_values\(t\).*shape"):
        Forcing(boundary_values=lambda t: np.zeros(nB + 1)).table(ts, pde)
    with pytest.raises(ValueError, match="not finite"):
        Forcing(source=lambda t, X: np.full(d, np.nan if t > 5 * dt else 0.0)).table(ts, pde)
    with pytest.raises(ValueError, match="not finite"):
        Forcing(boundary_values=lambda t: np.full(nB, np.inf)).rhs(0.0, pde)
    with pytest.raises(TypeError, match="callable"):
        Forcing(source=np.zeros(d))
    with pytest.raises(TypeError, match="Forcing"):
        examples.heat_1d_discretized(dx=0.1, forcing=lambda t: 0.0)


def test_recipes_carry_the_forcing_and_their_f_includes_the_source():
    kernel = pnmol.kernels.SquareExponential()
    s1 = lambda t, X: fr.source(t, X)                                                       # noqa: E731
    s2 = lambda t, X: fr.source(t, X, 2)                                                    # noqa: E731
    kw = dict(dx=1.0 / 15, kernel=kernel)
    made = [      # (recipe, its term -- a fresh one per problem: a convection term holds its own operator --, keywords, source)
        (examples.reaction_diffusion_1d_discretized, lambda: (reactions.logistic(3.0),), kw, s1),
        (examples.convection_diffusion_1d_discretized, lambda: (reactions.burgers(),), kw, s1),
        (examples.burgers_1d_discretized, lambda: (), kw, s1),
        (examples.reaction_diffusion_system_1d_discretized, lambda: (reactions.lotka_volterra(0.5, 0.4, 0.4, 0.5),),
         dict(diffusion_rates=(0.1, 0.1), y0_fun=examples.lotka_volterra_y0, dx=1.0 / 15), s2),
    ]
    for recipe, args, kwargs, s in made:
        plain = recipe(*args(), **kwargs)
        forced = recipe(*args(), forcing=Forcing(source=s), **kwargs)
        assert getattr(plain, "forcing", None) is None and isinstance(forced.forcing, Forcing)
        u = 0.3 + 0.1 * np.cos(np.arange(plain.L.shape[0]))
        for t in (0.0, 0.37):
            want = np.asarray(plain.f(t, u)) + s(t, plain.mesh_spatial.points)
            assert np.array_equal(np.asarray(forced.f(t, u)), want), recipe.__name__
            assert np.array_equal(np.asarray(forced.df(t, u)), np.asarray(plain.df(t, u)))
        assert forced.reaction is not None
    heat = examples.heat_1d_discretized(forcing=Forcing(source=s1), **kw)
    assert isinstance(heat.forcing, Forcing) and not hasattr(heat, "f")
    assert getattr(examples.heat_1d_discretized(**kw), "forcing", None) is None
    # boundary values alone leave f as it was
    only_g = examples.reaction_diffusion_1d_discretized(reactions.logistic(3.0), forcing=Forcing(boundary_values=lambda t: np.zeros(2)),
                                                        **kw)
    u = np.linspace(0.0, 1.0, only_g.L.shape[0])
    assert np.array_equal(only_g.f(0.2, u), reactions.logistic(3.0).callables()[0](0.2, u))


def test_refusals_come_before_any_device_work(monkeypatch):
    monkeypatch.setattr(_hip.Filter, "__init__", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("device work")))
    monkeypatch.setattr(_hip.SqrtFilter, "__init__", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("device work")))
    monkeypatch.setattr(_hip.Context, "default", classmethod(lambda cls, device=None: (_ for _ in ()).throw(AssertionError("device work"))))
    dt = fr.DT
    rule = pnmol.odetools.step.Constant(dt)
    kernel = pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise()
    pde, solver, _, _ = fr.linear_pair(20, 1, "dirichlet", "both")
    tpde, tsolver, _, _ = fr.term_pair("logistic-source")

    def every_entry(s, p, iterated=False):
        calls = [lambda: s.solve(p), lambda: s.solve_marginals(p), lambda: s.solve_on_device(p), lambda: s.initialize(p)]
        if iterated:
            calls.append(lambda: s.solve_iterated(p))
        return calls

    f32 = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=rule, spatial_kernel=kernel)
    f32.dtype = "f32"
    _, host_route, _, _ = fr.term_pair("logistic-source", reaction_on_device=False)
    plain_semilinear = examples.spruce_budworm_1d_discretized(tmax=12 * dt, dx=1.0 / 19, kernel=pnmol.kernels.SquareExponential())
    plain_semilinear.forcing = pde.forcing                      # host callables only: no term for the device
    refused = [
        (pnmol.sqrtform.LinearWhiteNoiseEK1(num_derivatives=1, steprule=rule, spatial_kernel=kernel), pde, False),
        (pnmol.sqrtform.SemiLinearWhiteNoiseEK1(num_derivatives=2, steprule=rule, spatial_kernel=kernel), tpde, False),
        (pnmol.sqrtform.LinearLatentForceEK1(num_derivatives=1, steprule=rule), pde, False),
        (f32, pde, False),
        (pnmol.latent.SemiLinearLatentForceEK1(num_derivatives=1, steprule=rule), tpde, False),
        (host_route, tpde, True),
        (tsolver, plain_semilinear, True),
    ]
    for s, p, iterated in refused:
        for call in every_entry(s, p, iterated):
            with pytest.raises(TypeError, match="forcing"):
                call()
    adaptive = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=pnmol.odetools.step.Adaptive(), spatial_kernel=kernel)
    with pytest.raises(TypeError, match="Constant"):            # (an existing refusal, unchanged)
        adaptive.solve_marginals(pde)

    # a forcing whose values are wrong: ValueError from the table, in front of the device
    d, nB = pde.L.shape[0], pde.B.shape[0]
    for bad, what in ((Forcing(source=lambda t, X: np.zeros(d - 1)), "shape"),
                      (Forcing(boundary_values=lambda t: np.full(nB, np.nan)), "not finite")):
        pde.forcing = bad
        for call in (lambda: solver.solve_marginals(pde), lambda: solver.solve_on_device(pde)):
            with pytest.raises(ValueError, match=what):
                call()

    # the supported combinations pass the refusals and reach the device
    good, _ = fr.make_forcing("source")
    pde.forcing = good
    lpde, lsolver, _, _ = fr.latent_pair("both")
    for s, p, iterated in ((solver, pde, False), (tsolver, tpde, True), (lsolver, lpde, False)):
        for call in every_entry(s, p, iterated):
            with pytest.raises(AssertionError, match="device work"):
                call()


# ------------------------------------------------------------------------------------ conditions on the inputs of the GPU tests
def _moved(forced, plain):
    return float(np.abs(forced - plain).max() / np.abs(forced).max())


@pytest.mark.parametrize("mode", fr.MODES)
@pytest.mark.parametrize("shape", fr.SHAPES)
def test_forcing_moves_the_linear_cases_by_1e3_tolerances(shape, mode):
    """On the oracle alone: the forced and the unforced trajectories differ by at least 1e3 times the mean tolerance of the GPU
    tests (rtol 1e-5 with the floor 1e-5 max|mean|), so a device that ignores the right-hand sides cannot pass them; and the
    Dirichlet nodes of a mean driven at the boundary equal g."""
    sol, means, stds = fr.linear_reference(*shape, mode)
    _, plain, _ = fr.linear_reference(*shape, None)
    moved = _moved(means, plain)
    print(f"{shape} {mode}: forced and unforced oracle means differ by {moved:.2e} of the largest mean; at the last time by "
          f"{np.abs(means[-1] - plain[-1]).max():.3f}")
    assert moved >= 1e3 * fr.MEAN_RTOL
    assert np.all(np.isfinite(means)) and np.all(np.isfinite(stds))
    if shape[2] == "dirichlet" and mode != "source":
        _, _, opde, osolver = fr.linear_pair(*shape, mode)
        for k, t in enumerate(sol.t):
            np.testing.assert_allclose(opde.B @ means[k], osolver.boundary_values(t), rtol=0, atol=1e-9)


def test_forcing_moves_the_other_cases_by_1e3_tolerances():
    N, nu, bcond, K = fr.BIG
    _, big, _ = fr.linear_reference(N, nu, bcond, "both", K)
    _, big_plain, _ = fr.linear_reference(N, nu, bcond, None, K)
    assert _moved(big, big_plain) >= 1e3 * fr.MEAN_RTOL
    import observe_reference as oref
    import pnmol_oracle as oracle

    N, nu, bcond = fr.LATENT
    _, _, popde, posolver = oref.latent_pair(N, nu, fr.DT, fr.STEPS, bcond, 0.05)
    plain = posolver.solve(popde)
    lat_plain, _ = oracle.read_mean_and_std_latent(plain, posolver.E0)
    for mode in fr.MODES:                                       # every mode the GPU file runs, and both halves of the state
        lsol, lat, _ = fr.latent_reference(mode)
        moved = _moved(lat, lat_plain)
        eps_moved = _moved(lsol.mean[:, 0, N:], plain.mean[:, 0, N:])
        print(f"latent {mode}: u moved by {moved:.2e}, eps by {eps_moved:.2e}")
        assert moved >= 1e3 * fr.MEAN_RTOL and eps_moved >= 1e3 * fr.MEAN_RTOL
    for name in fr.TERMS:
        _, forced, _ = fr.term_reference(name)
        _, plain, _ = fr.term_reference(name, False)
        C = 2 if fr.TERMS[name].kind == "lotka_volterra" else 1
        n = forced.shape[1] // C
        moved = min(_moved(forced[:, c * n:(c + 1) * n], plain[:, c * n:(c + 1) * n]) for c in range(C))
        print(f"{name}: moved by {moved:.2e}")
        assert moved >= 1e3 * fr.MEAN_RTOL
