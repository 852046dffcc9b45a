"""The measurement update's kernels (pnmol_observe.hip) hold no read of an MFMA result with too few wait states behind the MFMA and no
8-byte sc1 load: the two checks of tests/test_isa_hazards.py, with the same scanner (tools/mfma_hazard_scan.py), on this
translation unit."""
import pathlib
import shutil
import subprocess
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = ROOT / "pnmol-experiments_amd" / "csrc" / "pnmol_observe.hip"


@pytest.mark.skipif(not pathlib.Path(HIPCC).exists(), reason="hipcc not available")
def test_observe_kernels_read_no_mfma_result_too_early(tmp_path):
    out = tmp_path / "pnmol_observe.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-w", f"-I{ROOT / 'include'}", "-S",
                    "--cuda-device-only", str(SRC), "-o", str(out)], check=True)
    assert "v_mfma_f64_16x16x4" in out.read_text()      # (the products really run on the fp64 MFMA)
    res = subprocess.run([sys.executable, str(ROOT / "tools" / "mfma_hazard_scan.py"), str(out), "10"],
                         check=True, capture_output=True, text=True).stdout
    lines = res.strip().splitlines()
    assert int(lines[-1].split()[0]) == 0, res
    assert int(lines[-2].split()[0]) == 0, res
