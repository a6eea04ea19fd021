"""CPU: host enumeration of extend_attn.hip's row-block map and mask rule — tests/csrc/extend_attn_layout_sim.cpp compiled with
g++ against cambrian_amd/csrc/extend_attn_layout.h (the very header the kernel includes): for G of 1, 2, 4, 7, 8 and chunks of
1, 15, 16, 17 and 33 tokens every (query row, key) pair a row may see is owned by exactly one (row block, key chunk, wave, lane,
register), a row's causal limit is t0 + its token, and the mask the kernel applies is the brute-force rule."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extend_attn_layout_enumeration():
    src = os.path.join(ROOT, "tests", "csrc", "extend_attn_layout_sim.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sim")
        subprocess.run(["g++", "-O1", "-std=c++17", src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK" in out.stdout
