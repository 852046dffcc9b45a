"""The host side of the sensor plan of the constant-step loop (csrc/pnmol_observe_plan.hpp, nothing of HIP in it) under
AddressSanitizer + UBSan: tests/observe_plan_check.cpp is a stand-alone program that includes nothing but that header, is linked with
the sanitizers and checks the entry -> step mapping (split calls, a runt last step, 16-ulp agreement), every refusal of the walk and
of the validation, and that padding C / R / y leaves zeros."""
import pathlib
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CLANG = pathlib.Path("/opt/rocm/lib/llvm/bin/clang++")


@pytest.mark.skipif(not CLANG.exists(), reason="the ROCm clang++ is not available")
def test_observe_plan_host_logic_under_asan_ubsan(tmp_path):
    exe = tmp_path / "observe_plan_check"
    subprocess.run([str(CLANG), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'pnmol-experiments_amd' / 'csrc'}", str(ROOT / "tests" / "observe_plan_check.cpp"), "-o", str(exe)],
                   check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "observe plan: ok" and "runtime error" not in run.stderr
