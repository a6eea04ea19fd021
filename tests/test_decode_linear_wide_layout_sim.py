"""CPU: host enumeration of decode_linear_wide.hip's maps and row-slab plan — tests/csrc/decode_linear_wide_layout_sim.cpp
compiled with g++ against cambrian_amd/csrc/decode_linear_wide_layout.h (the very header the kernel includes).  It replays whole
launches for M in {1, 16, 17, 32, 33, 48, 49, 64} and K in {8, 64, 72, 264} (and two at K = 4096), both slab sizes and both
epilogues: the regrouped weight operand and the x operand of every product carry the same k, every (row, n, k) product occurs
exactly once and none past K, rows >= M are never stored, the order of a row's sum does not depend on M or on the slab, the
LDS stores stay inside the tile, and the plan is a pure function of (N, act, CU count) that covers N exactly."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_linear_wide_layout_enumeration():
    src = os.path.join(ROOT, "tests", "csrc", "decode_linear_wide_layout_sim.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sim")
        subprocess.run(["g++", "-O2", "-std=c++17", src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK" in out.stdout
