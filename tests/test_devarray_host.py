"""The owner of the library's device arrays (csrc/dev_array.hpp), checked on the host: tests/native/devarray_check.cpp runs
it over a stand-in HIP runtime under AddressSanitizer and UBSan (make devarray-check).  No GPU, no ROCm, no fixtures."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

PKG = Path(__file__).resolve().parents[1] / "bsmr-sddmm_amd"
SAN = "-fsanitize=address,undefined"


def _sanitizers_link(tmp_path):
    """Whether this machine's compiler finds the sanitizer runtimes (a one-line program, compiled and run)."""
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    exe = tmp_path / "probe"
    cxx = os.environ.get("CXX", "g++")
    built = subprocess.run([cxx, SAN, "-o", str(exe), str(src)], capture_output=True, text=True)
    return built.returncode == 0 and subprocess.run([str(exe)], capture_output=True).returncode == 0


def test_devarray_check(tmp_path):
    assert shutil.which("make"), "make is needed to build tests/native/devarray_check.cpp"
    sanitized = _sanitizers_link(tmp_path)
    cmd = ["make", "-C", str(PKG), "devarray-check"] + ([] if sanitized else ["DEVARRAY_SAN="])
    run = subprocess.run(cmd, capture_output=True, text=True)
    print(run.stdout)
    print(run.stderr)
    assert run.returncode == 0, f"devarray_check failed:\n{run.stdout}\n{run.stderr}"
    assert "devarray_check: ok" in run.stdout
    if not sanitized:
        pytest.skip(f"devarray_check passed, but built without {SAN}: this machine has no sanitizer runtime, "
                    "so leaks and double frees were counted by the program alone")
