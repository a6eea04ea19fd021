"""CPU: host enumeration of decode_attn_multi.hip's lane maps — tests/csrc/decode_attn_multi_layout_sim.cpp compiled with g++
against cambrian_amd/csrc/decode_attn_multi_layout.h (the very header the kernel includes): for head_dim 64 / 96 / 128 and
Q * G of 1, 7, 32, 33 and 64 every (query row, key, d) product of both MFMA products is formed exactly once with operands that
carry the same index, padded rows and keys past the chunk weigh nothing, and the transposing reads of the V tile stay inside
it, deliver what the map promises and are free of bank conflicts."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_attn_multi_layout_enumeration():
    src = os.path.join(ROOT, "tests", "csrc", "decode_attn_multi_layout_sim.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sim")
        subprocess.run(["g++", "-O1", "-std=c++17", src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK" in out.stdout
