"""The deferred-reduce queue (csrc/defer.h: the host logic under otamd_gemm_defer_* and otamd_layernorm_defer_*) on the
CPU: tests/csrc/defer_queue_test.cpp instantiates it with a fake grouped launch that records (n, blocks, stream) and
walks batch rollover at MaxN, the arena wrap, a need larger than the arena, the caller-predicate flush, begin twice,
end on an unknown stream, end with a different launch stream, a failing launch and the counters.  A host build under
AddressSanitizer + UBSan; no GPU code involved."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "csrc" / "defer_queue_test.cpp"
INC = ROOT / "onetrainer_amd" / "csrc"
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_defer_queue_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, *SAN, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"{cxx} cannot link the sanitizer runtimes: {r.stderr.strip()[-300:]}")
    exe = tmp_path / "defer_queue_test"
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *SAN, "-I", str(INC), str(SRC), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "defer_queue_test: ok (17 items in 10 launches)" in r.stdout
