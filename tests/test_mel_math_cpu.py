"""csrc/mel_math.h -- the one statement of the audio front-end's integer rules (which sample tap j of STFT frame m reads and whether
it is loaded, which STFT frames an animation frame interpolates, how many frames are ready) -- is plain C++ behind a qualifier macro:
tests/host/mel_math_check.cpp runs it on the host.  mel_first_load, the closed form that decides whether a sliding window may be
read, must equal the minimum over every tap of the frame range, enumerated through the shared index rule: centred / uncentered x
pre-emphasis on / off, n_fft / hop 800 / 200, 64 / 16, 30 / 7 and 8 / 16, signals shorter than, equal to and longer than n_fft (a
multiple of the hop and not), finished and continuing, every frame range -- those that reflect at the right end only included, and
those whose right reflection reaches further left than the first frame's start.  mel_frames_ready(n) must be exactly the number
of animation frames whose STFT frames end inside n samples.  Built here with the host compiler, no GPU and no HIP."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_mel_index_rule_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++)")
    exe = tmp_path / "mel_math_check"
    b = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-o", str(exe),
                        str(ROOT / "tests" / "host" / "mel_math_check.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "mel_math_check: ok"
