"""CPU tests of the loop's recorder and the one-call backward pass (`pnmol_filter_set_recorder`, `pnmol_smoother_steps`,
`solve_on_device`, `smooth_marginals`): the recorder's host logic (csrc/pnmol_record_plan.hpp, nothing of HIP in it) under
AddressSanitizer + UBSan -- tests/record_plan_check.cpp is a stand-alone program that includes nothing but that header and checks the
step -> slot mapping over split calls and a runt last step and every refusal --, the C ABI's new names, and the refusals of
`solve_on_device` in front of any device work.  No GPU."""

import pathlib
import re
import subprocess

import numpy as np
import pytest

import pnmol
from helpers import make_pair
from pnmol import _hip, data

ROOT = pathlib.Path(__file__).resolve().parent.parent
CLANG = pathlib.Path("/opt/rocm/lib/llvm/bin/clang++")
NAMES = ("pnmol_filter_set_recorder", "pnmol_filter_recorder_pending", "pnmol_filter_recorder_means", "pnmol_smoother_steps")


@pytest.mark.skipif(not CLANG.exists(), reason="the ROCm clang++ is not available")
def test_record_plan_host_logic_under_asan_ubsan(tmp_path):
    exe = tmp_path / "record_plan_check"
    subprocess.run([str(CLANG), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'pnmol-experiments_amd' / 'csrc'}", str(ROOT / "tests" / "record_plan_check.cpp"), "-o", str(exe)],
                   check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "record plan: ok" and "runtime error" not in run.stderr


def test_record_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "pnmol_hip.h").read_text()
    lib = _hip.load_library()
    for name in NAMES:
        assert name in _hip.SYMBOLS
        assert re.search(rf"\bint {name}\(", header)
        assert hasattr(lib, name)
    assert lib.pnmol_abi_version() == 3
    for method in ("set_recorder", "clear_recorder", "recorder_pending", "recorder_means", "smoother_steps"):
        assert method in dir(_hip.Filter)
    for cls in (pnmol.white.LinearWhiteNoiseEK1, pnmol.white.SemiLinearWhiteNoiseEK1, pnmol.latent.LinearLatentForceEK1):
        assert callable(cls.solve_on_device) and callable(cls.smooth_marginals)
    entry = (ROOT / "__graft_entry__.py").read_text()
    assert "pnmol_record.hip" in entry


def test_solve_on_device_refuses_before_any_device_work(monkeypatch):
    dt, K, N = 2.0 ** -4, 12, 16
    pde, solver, _, _ = make_pair(N, 2, dt, K)
    calls = []
    monkeypatch.setattr(type(solver), "initialize", lambda self, p: calls.append(p) or (_ for _ in ()).throw(AssertionError))
    monkeypatch.setattr(_hip.Filter, "__init__", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("device work")))
    C = data.select_nodes(N, [3])

    def ob(t, C=C, noise=1e-3):
        return data.Observation(t, C, np.zeros(C.shape[0]), noise)

    # the cases of solve_marginals, with its errors
    with pytest.raises(ValueError, match="is not a grid time"):
        solver.solve_on_device(pde, observations=[ob(4.5 * dt)])
    with pytest.raises(ValueError, match="another C"):
        solver.solve_on_device(pde, observations=[ob(4 * dt), ob(8 * dt, data.select_nodes(N, [4]))])
    with pytest.raises(ValueError, match="behind the last step taken"):
        solver.solve_on_device(pde, num_steps=6, observations=[ob(4 * dt), ob(8 * dt)])
    adaptive = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=2, steprule=pnmol.odetools.step.Adaptive())
    with pytest.raises(TypeError, match="Constant"):
        adaptive.solve_on_device(pde)
    semi = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=2, steprule=pnmol.odetools.step.Constant(dt))
    with pytest.raises(TypeError, match="linear PDE"):
        semi.solve_on_device(pde)                               # (no term the device linearises: host callables)
    latent = pnmol.latent.SemiLinearLatentForceEK1(num_derivatives=2, steprule=pnmol.odetools.step.Constant(dt))
    with pytest.raises(TypeError, match="linear PDE"):
        latent.solve_on_device(pde)
    # the recorder needs the fp64 covariance form
    sq = pnmol.sqrtform.LinearWhiteNoiseEK1(num_derivatives=2, steprule=pnmol.odetools.step.Constant(dt))
    with pytest.raises(TypeError, match="fp64 covariance-form"):
        sq.solve_on_device(pde)
    f32 = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(dt))
    f32.dtype = "f32"
    with pytest.raises(TypeError, match="fp64 covariance-form"):
        f32.solve_on_device(pde)
    assert calls == []
    # valid arguments reach initialize (and nothing before it touched the device)
    with pytest.raises(AssertionError):
        solver.solve_on_device(pde, num_steps=8, observations=[ob(4 * dt), ob(8 * dt)])
    assert len(calls) == 1


def test_smooth_marginals_has_the_refusals_of_smooth():
    dt = 2.0 ** -4
    solution = pnmol.pdefilter.PDESolution(t=np.array([0.0, dt]), mean=np.zeros((2, 3, 4)), ys=[], info={},
                                           diffusion_squared_calibrated=1.0)
    solver = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=2, steprule=pnmol.odetools.step.Constant(dt))
    with pytest.raises(TypeError, match="device-resident states"):
        solver.smooth_marginals(solution)
    for cls in (pnmol.sqrtform.LinearWhiteNoiseEK1, pnmol.latent.LinearLatentForceEK1):
        with pytest.raises(TypeError, match="white-noise"):
            cls(num_derivatives=1, steprule=pnmol.odetools.step.Constant(dt)).smooth_marginals(solution)
