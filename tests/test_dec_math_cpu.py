"""csrc/quat_math.h and csrc/dec_math.h -- the one statement of the decoder step's pointwise math (root integration, gaze
direction, their adjoint in one piece and split in two, the GRU cell backward) -- are plain C++ behind a qualifier macro:
tests/host/dec_math_check.cpp runs them on the host against a float64 statement of the reference's formulas (ZEGGS/anim/tquat.py,
ZEGGS/modules.py:696, :739-740) that is written there and not taken from the headers, pins that statement's analytic adjoint with
central differences, and compares the split adjoint with the one-piece one -- 300 000 cases, a third in each branch of the
exponential (h < 1e-5, 1e-5 <= h < 1, h >= 1), every bound 4 x the maximum measured with this sample set and every measured maximum below
1e-6; the adjoint carry is held against the size of its summands and, where those are at most twice the result, against its own
largest entry (figures and reasoning in the program's header).  Built here with the host compiler, no GPU and no HIP."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_dec_math_equals_float64(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++)")
    exe = tmp_path / "dec_math_check"
    b = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-o", str(exe),
                        str(ROOT / "tests" / "host" / "dec_math_check.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "dec_math_check: ok"
