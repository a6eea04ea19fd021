"""CPU: host enumeration of decode_linear_fp8.hip's lane -> k maps and row-slab plan —
tests/csrc/decode_linear_fp8_layout_sim.cpp compiled with g++ against cambrian_amd/csrc/decode_linear_fp8_layout.h (the very
header the kernel includes): a lane's 16 weight bytes are 16 k, the weight and x operands of every product carry the same k,
every k < K is multiplied exactly once and none past K, for K from 16 to several steps past the four waves' round; every
load instruction covers whole 128-byte lines of a row; the plan is pure, covers N exactly and fills 256 CUs at N = 4096."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_linear_fp8_layout_enumeration():
    src = os.path.join(ROOT, "tests", "csrc", "decode_linear_fp8_layout_sim.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sim")
        subprocess.run(["g++", "-O1", "-std=c++17", src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK" in out.stdout
