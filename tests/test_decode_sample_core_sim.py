"""CPU: the arithmetic of cmb_decode_sample — tests/csrc/decode_sample_core_sim.cpp compiled with g++ under AddressSanitizer and
UBSan against cambrian_amd/csrc/decode_sample_core.h (the very header decode_sample.hip and decode_next.hip include) and run
directly: Philox4x32-10's known answers and the counter layout of a draw, the uniform strictly inside (0, 1) and the Gumbel
noise against fp64, the monotone key map with its inverse, and the fixed-point mass whose sum of 2^17 ones does not overflow."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_sample_core_arithmetic():
    src = os.path.join(ROOT, "tests", "csrc", "decode_sample_core_sim.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sim")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src,
                        "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK" in out.stdout
