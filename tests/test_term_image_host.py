"""The image builder of the nonlinear terms (csrc/pnmol_term_image.hpp, host only) under AddressSanitizer + UBSan:
tests/term_image_check.cpp is a stand-alone program that includes nothing but that header, is linked with the sanitizers and checks
the invariants itself (columns ascending and packed, base values kept, added slots 0, boundary rows untouched, width, slot table,
G plane; tridiagonal base of N = 5 with two boundary rows in mp = 32; systems of 2 and 3 species, a 5-point G, G = 0)."""
import pathlib
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CLANG = pathlib.Path("/opt/rocm/lib/llvm/bin/clang++")


@pytest.mark.skipif(not CLANG.exists(), reason="the ROCm clang++ is not available")
def test_term_images_hold_their_invariants_under_asan_ubsan(tmp_path):
    exe = tmp_path / "term_image_check"
    subprocess.run([str(CLANG), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'pnmol-experiments_amd' / 'csrc'}", str(ROOT / "tests" / "term_image_check.cpp"), "-o", str(exe)],
                   check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "term image: ok" and "runtime error" not in run.stderr
