"""csrc/text_math.h -- exact "%f" of a double in integer arithmetic, the digit routine of the device BVH text (csrc/text.hip) -- is
plain C++ behind a qualifier macro: tests/host/text_format_check.cpp compares it with glibc's snprintf("%f") byte for byte over
random bit patterns, degrees, float32-origin values, exact ties (k/128, k * 2^-7..-26), (k + 0.5) * 1e-6 and its neighbours,
carries (0.9999995, 9.9999995), +-0, subnormals and values up to 2^50, 2 M of each, and checks that NaN, +-inf, +-1e15 and 1e300
are reported as out of the domain while 999999999999999.9 is inside it and 24 bytes wide.  Built here with the host compiler, no
GPU and no HIP."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_text_math_equals_snprintf(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++)")
    exe = tmp_path / "text_format_check"
    b = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-o", str(exe),
                        str(ROOT / "tests" / "host" / "text_format_check.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe), "2000000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "text_format_check: ok"
