"""The conv gathers under circular padding (csrc/gemm2_stage.h, ConvGeom.circular) on the CPU:
tests/csrc/conv_circular_check.cpp compares the closed and the incremental index decode, lane by lane and K-step by
K-step, with a brute-force decode of the definition (images 1x1 / 2x2 / 3x5 / 4x6, N 2, SC 8 / 72, 3x3 at stride 1,
stride 2 and under upsample, and a pad-0 geometry whose extra output row stays zero-filled).  Run plain and once under
AddressSanitizer + UBSan (a host build; no GPU code involved)."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "csrc" / "conv_circular_check.cpp"
INC = ROOT / "onetrainer_amd" / "csrc"


@pytest.mark.parametrize("name,flags", [
    ("plain", ["-O2"]),
    ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_circular_offsets_equal_the_definition(tmp_path, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / f"conv_circular_check_{name}"
    subprocess.run([cxx, "-std=c++17", *flags, "-I", str(INC), str(SRC), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "equal the definition in both forms" in r.stdout
    assert int(r.stdout.split()[2]) > 10 ** 6   # the sweep really ran
