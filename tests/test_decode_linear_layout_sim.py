"""CPU: host enumeration of decode_linear.hip's lane -> k maps and row-slab plan — tests/csrc/decode_linear_layout_sim.cpp
compiled with g++ against cambrian_amd/csrc/decode_linear_layout.h (the very header the kernel includes): the weight and x
operands of every product carry the same k, every k < K is multiplied exactly once and none past K, for K from one 16-byte
chunk to several steps past the four waves' round; the plan covers N exactly and fills the chip at N = 4096."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_linear_layout_enumeration():
    src = os.path.join(ROOT, "tests", "csrc", "decode_linear_layout_sim.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sim")
        subprocess.run(["g++", "-O1", "-std=c++17", src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK" in out.stdout
