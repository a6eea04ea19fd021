"""CPU: host enumeration of cmb_decode_step's workspace — tests/csrc/decode_step_layout_sim.cpp compiled with g++ under
AddressSanitizer and UBSan against cambrian_amd/csrc/decode_step_layout.h (the very header decode_step.hip includes) and run
directly: the buffers are disjoint, 16-byte aligned, wide enough and end exactly at the total; the ping-pong of the residual
stream never hands a launch its own x or residual as output, over B = 1..16 and the three model geometries."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_step_layout_enumeration():
    src = os.path.join(ROOT, "tests", "csrc", "decode_step_layout_sim.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sim")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src,
                        "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK" in out.stdout
