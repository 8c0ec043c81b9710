"""The conv gathers' incremental index decode (csrc/gemm2_stage.h offsets_step: mixed-radix counters carried from K-step
to K-step) against the closed division form, on the CPU: tests/csrc/conv_index_check.cpp walks every K-step of every
split for every lane and DMA piece of every tile width over a sweep of geometries (RW 1 / 5 / 7 / 32 / 70, RH x RW
from 3 to 700, N 1 / 3, SC 8 / 64 / 72 / 192, 1x1 and 3x3, stride 1 / 2 / 3, upsample, splits that begin inside a tap
and inside an image row) and compares every offset, zero-fill markers included.  Run plain and once under
AddressSanitizer + UBSan (a host build; no GPU code involved)."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "csrc" / "conv_index_check.cpp"
INC = ROOT / "onetrainer_amd" / "csrc"


def _run(tmp_path, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / name
    subprocess.run([cxx, "-std=c++17", *flags, "-I", str(INC), str(SRC), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "equal in both forms" in r.stdout
    return r.stdout


def test_incremental_offsets_equal_closed_form(tmp_path):
    out = _run(tmp_path, "conv_index_check", ["-O2"])
    assert int(out.split()[2]) > 10 ** 8   # the sweep really ran


def test_incremental_offsets_under_sanitizers(tmp_path):
    _run(tmp_path, "conv_index_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
