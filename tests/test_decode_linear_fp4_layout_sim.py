"""CPU: host enumeration of decode_linear_fp4.hip's lane -> k maps and row-slab plan —
tests/csrc/decode_linear_fp4_layout_sim.cpp compiled with g++ against cambrian_amd/csrc/decode_linear_fp4_layout.h (the very
header the kernel includes), over K = 32, 224, 256, 288, 800 and more: a lane's 16 weight bytes are 32 k = one MX block, its
scale byte is byte k / 32 of the row, the weight and x operands of every product carry the same k, every (row, k < K) is
multiplied exactly once and none past K; every load instruction covers one whole 128-byte line of a row; the plan is pure,
monotone in N, covers N exactly, and a SwiGLU slab owns matching gate and up rows."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_linear_fp4_layout_enumeration():
    src = os.path.join(ROOT, "tests", "csrc", "decode_linear_fp4_layout_sim.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sim")
        subprocess.run(["g++", "-O1", "-std=c++17", src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK" in out.stdout
