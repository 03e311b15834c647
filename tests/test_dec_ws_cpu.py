"""csrc/decoder_ws.h carves the decoder workspace; the launches of the three persistent kernels walk its per-frame operand buffers by
strides of their own.  tests/host/dec_ws_check.cpp carves over a fake base on the host and asserts, for the rigs of
tests/test_gpu_decoder_dims.py, the 75-joint rig and both sides of XD = 1152, batch sizes 1 .. 64 and T = 2 .. 64, that every such
buffer is at least as large as what is walked (extents written out in the program, not taken from the header) and that G0xf is
exactly the 201 blocks per frame the rollout walks -- the training carve had 64 + KBX + 64, short for every rig below 68 joints;
rigs with KBX > 73 keep that larger size, which tests/test_abi.py pins.  Built with hipcc in host-only mode (the header pulls in
device functions); no GPU."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_operand_buffers_cover_what_the_persistent_kernels_walk(tmp_path):
    hipcc = shutil.which("hipcc") or shutil.which("hipcc", path="/opt/rocm/bin")
    if hipcc is None:
        pytest.skip("no hipcc")
    exe = tmp_path / "dec_ws_check"
    b = subprocess.run([hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-o", str(exe), str(ROOT / "tests" / "host" / "dec_ws_check.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "dec_ws_check: ok"
