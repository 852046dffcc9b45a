"""CPU tests of the iterated EK1 smoother (`pnmol_filter_set_linearization_points`, `pnmol_filter_linearize_at`, `solve_iterated`;
DESIGN.md section 22): the host logic of the table of linearisation points (csrc/pnmol_linearize_plan.hpp, nothing of HIP in it)
under AddressSanitizer + UBSan -- tests/linearize_plan_check.cpp is a stand-alone program that includes nothing but that header, and
tests/cursor_plan_check.cpp one for the cursor that every table of the loop shares (csrc/pnmol_cursor_plan.hpp) --,
the C ABI's new names, the refusals of `solve_iterated` and of `linearize_at` in front of any device work, and the conditions that
the cases of tests/test_gpu_iterated.py must meet on the NumPy reference alone (tests/iterated_reference.py).  No GPU."""

import pathlib
import re
import subprocess

import numpy as np
import pytest

import pnmol
import iterated_reference as ir
from helpers import make_pair
from pnmol import _hip

ROOT = pathlib.Path(__file__).resolve().parent.parent
CLANG = pathlib.Path("/opt/rocm/lib/llvm/bin/clang++")
RESULT = pnmol.white.IteratedSolution      # (the feature's own name at import: no test of this file passes without the feature)
NAMES = ("pnmol_filter_set_linearization_points", "pnmol_filter_linearization_pending", "pnmol_filter_linearize_at")


def _check_program(tmp_path, name, says):
    exe = tmp_path / name
    subprocess.run([str(CLANG), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'pnmol-experiments_amd' / 'csrc'}", str(ROOT / "tests" / f"{name}.cpp"), "-o", str(exe)],
                   check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == says and "runtime error" not in run.stderr


@pytest.mark.skipif(not CLANG.exists(), reason="the ROCm clang++ is not available")
def test_linearize_plan_host_logic_under_asan_ubsan(tmp_path):
    _check_program(tmp_path, "linearize_plan_check", "linearize plan: ok")


@pytest.mark.skipif(not CLANG.exists(), reason="the ROCm clang++ is not available")
def test_cursor_plan_host_logic_under_asan_ubsan(tmp_path):
    """The cursor and the set-call rule that the table of points shares with the loop's other tables (csrc/pnmol_cursor_plan.hpp)."""
    _check_program(tmp_path, "cursor_plan_check", "cursor plan: ok")


def test_iterated_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "pnmol_hip.h").read_text()
    lib = _hip.load_library()
    for name in NAMES:
        assert name in _hip.SYMBOLS
        assert re.search(rf"\bint {name}\(", header)
        assert hasattr(lib, name)
    assert lib.pnmol_abi_version() == 3
    for method in ("set_linearization_points", "clear_linearization_points", "linearization_pending", "linearize_at"):
        assert method in dir(_hip.Filter)
    assert callable(pnmol.white.SemiLinearWhiteNoiseEK1.solve_iterated)
    assert RESULT._fields[:4] == ("filtered", "means", "stds", "smoothed")


def test_refusals_come_before_any_device_work(monkeypatch):
    name = "fisher-neumann"
    pde, solver = ir.product(name)
    dt, d, T = ir.CASES[name].dt, pde.L.shape[0], 13
    calls = []
    for cls in (pnmol.white.SemiLinearWhiteNoiseEK1, pnmol.white.LinearWhiteNoiseEK1, pnmol.latent.SemiLinearLatentForceEK1,
                pnmol.sqrtform.SemiLinearWhiteNoiseEK1):
        monkeypatch.setattr(cls, "initialize", lambda self, p: calls.append(p) or (_ for _ in ()).throw(AssertionError))
    monkeypatch.setattr(_hip.Filter, "__init__", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("device work")))
    rule, kernel = pnmol.odetools.step.Constant(dt), pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise()

    # solve_iterated: the step rule, the solver, the term
    adaptive = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=2, steprule=pnmol.odetools.step.Adaptive(), spatial_kernel=kernel)
    with pytest.raises(TypeError, match="Constant"):
        adaptive.solve_iterated(pde)
    for other in (pnmol.latent.SemiLinearLatentForceEK1(num_derivatives=2, steprule=rule),
                  pnmol.sqrtform.SemiLinearWhiteNoiseEK1(num_derivatives=2, steprule=rule, spatial_kernel=kernel),
                  pnmol.white.LinearWhiteNoiseEK1(num_derivatives=2, steprule=rule, spatial_kernel=kernel)):
        with pytest.raises(TypeError, match="solve_iterated"):
            other.solve_iterated(pde)
    f32 = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=1, steprule=rule, spatial_kernel=kernel)
    f32.dtype = "f32"
    with pytest.raises(TypeError, match="solve_iterated"):
        f32.solve_iterated(pde)
    _, host_route = ir.product(name, reaction_on_device=False)
    with pytest.raises(TypeError, match="solve_iterated"):
        host_route.solve_iterated(pde)
    plain = pnmol.pde.examples.spruce_budworm_1d_discretized(tmax=T * dt, dx=1.0 / 32, kernel=pnmol.kernels.SquareExponential())
    assert getattr(plain, "reaction", None) is None             # (host callables only)
    with pytest.raises(TypeError, match="solve_iterated"):
        solver.solve_iterated(plain)
    with pytest.raises(ValueError, match="smooth must be"):
        solver.solve_iterated(pde, smooth="dense")
    with pytest.raises(ValueError, match="relaxation"):
        solver.solve_iterated(pde, relaxation=0.0)

    # the shape of `start` / `linearize_at` against the constant schedule, a runt last step included
    for bad in (np.zeros((T - 1, d)), np.zeros((T + 1, d)), np.zeros((T, d + 1)), np.zeros(d), np.zeros((T, d, 1))):
        with pytest.raises(ValueError, match="linearize_at must have shape"):
            solver.solve_iterated(pde, start=bad)
        with pytest.raises(ValueError, match="linearize_at must have shape"):
            solver.solve_on_device(pde, linearize_at=bad)
        with pytest.raises(ValueError, match="linearize_at must have shape"):
            solver.solve_marginals(pde, linearize_at=bad)
    with pytest.raises(ValueError, match=r"\(5, 33\)"):
        solver.solve_on_device(pde, num_steps=5, linearize_at=np.zeros((T, d)))
    runt_pde, runt_solver = ir.product("fisher-dirichlet-runt")
    with pytest.raises(ValueError, match=r"\(14, 33\)"):
        runt_solver.solve_on_device(runt_pde, linearize_at=np.zeros((13, d)))
    nan = np.zeros((T, d))
    nan[7, 3] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        solver.solve_marginals(pde, linearize_at=nan)
    # a solver without a device term takes no table
    hpde, hsolver, _, _ = make_pair(33, 2, dt, T)
    with pytest.raises(TypeError, match="linearize_at needs a term"):
        hsolver.solve_on_device(hpde, linearize_at=np.zeros((T, d)))
    with pytest.raises(TypeError, match="linearize_at needs a term"):
        hsolver.solve_marginals(hpde, linearize_at=np.zeros((T, d)))
    assert calls == []
    # valid arguments reach initialize (and nothing before it touched the device)
    for call in (lambda: solver.solve_iterated(pde, start=np.zeros((T, d))), lambda: solver.solve_iterated(pde),
                 lambda: solver.solve_on_device(pde, linearize_at=np.zeros((T, d))),
                 lambda: runt_solver.solve_marginals(runt_pde, linearize_at=np.zeros((14, d)))):
        with pytest.raises(AssertionError):
            call()
    assert len(calls) == 4


# ------------------------------------------------------------------------------------ conditions on the inputs of the GPU tests
@pytest.mark.parametrize("name", list(ir.CASES))
def test_reference_iteration_converges_moves_and_forgets_its_start(name):
    """On the NumPy reference alone, for every case tests/test_gpu_iterated.py uses: (1) an increment <= 1e-9 within the cap of 10
    iterations, (2) a first increment >= 1e-4 -- the iteration visibly moves the EK1 result, well above the 1e-5 mean tolerance --
    and (3) the same fixed point from `y0` repeated T times as from the EK1 pass, to 1e-7 relative."""
    it = ir.reference(name)
    print(f"{name}: increments " + ", ".join(f"{x:.1e}" for x in it.increments))
    assert it.converged and it.num_iterations <= ir.ITERATIONS and it.increments[-1] <= ir.TOL
    assert it.increments[0] >= 1e-4
    assert np.all(np.isfinite(it.means)) and np.all(np.isfinite(it.stds))
    other = ir.reference(name, start_y0=True)
    diff = np.abs(other.means - it.means).max() / np.abs(it.means).max()
    print(f"{name}: from y0 repeated {other.num_iterations} iterations, fixed points differ by {diff:.1e}")
    assert other.converged and diff <= 1e-7
    # the table of pass 1 is the smoothed EK1 trajectory, and the runt case has its 14th row
    T = int(np.ceil(ir.CASES[name].K))
    assert it.points[0] is None and it.points[1].shape == (T, it.means.shape[1])
    assert np.array_equal(it.points[1], it.passes[0].smoothed_means[1:])


def test_reference_iteration_with_sensor_data_converges():
    it = ir.reference("fisher-neumann", observed=True)
    plain = ir.reference("fisher-neumann")
    print("observed: increments " + ", ".join(f"{x:.1e}" for x in it.increments))
    assert it.converged and it.increments[0] >= 1e-4
    assert len(it.last.solution.info["data_log_likelihoods"]) == 3
    assert np.abs(it.means - plain.means).max() > 100 * 1e-5 * np.abs(plain.means).max()        # the data matters


def test_linear_term_is_at_its_fixed_point_after_one_iteration():
    """r(u) = a u: the linearisation does not depend on the point, so pass 1 repeats pass 0 up to rounding."""
    case = ir.CASES["fisher-neumann"]
    opde, osolver = ir.oracle_side("fisher-neumann")
    opde.f = lambda _t, x: -2.0 * x
    opde.df = lambda _t, x: np.diag(np.full(x.size, -2.0))
    it = ir.iterate(osolver, opde)
    print(f"linear term: increments {it.increments}")
    assert it.num_iterations == 1 and it.converged and it.increments[0] <= 1e-12
    assert case.K == 13
