"""csrc/gemm_route.h -- which direct-kernel variant and grid every weight-gradient (TN) product gets, and the first-use state
machine of the variants -- is pure host code: tests/host/gemm_route_check.cpp holds the routing table (recorded from the decision
code before it moved into the header) and drives the state machine from threads with a fake check.  Built here with the host
compiler, no GPU and no HIP."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_gemm_route_table_and_first_use_state_machine(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++)")
    exe = tmp_path / "gemm_route_check"
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-pthread", "-o", str(exe),
                        str(ROOT / "tests" / "host" / "gemm_route_check.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "gemm_route_check: ok"
