"""CPU: host-side run of ``cmb_resample_accum``'s per-cell code — tests/csrc/resample_accum_sim.cpp compiled with g++ against
cambrian_amd/csrc/resample_core.h (the very header resample_accum.hip includes): the kernel's work-item decomposition and its
base + bias + sources sum at the grids (8 -> 12), (4 -> 12), (2 -> 8), (64 -> 96), (32 -> 96), (1 -> 4), (4, 6) -> (7, 3), with
0, 1 and 2 sources, with and without base and bias, against an independent double-precision bilinear sum."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resample_accum_simulation():
    src = os.path.join(ROOT, "tests", "csrc", "resample_accum_sim.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sim")
        subprocess.run(["g++", "-O1", "-std=c++17", src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK" in out.stdout
    m = re.search(r"cases (\d+), worst rel err (\S+)", out.stdout)
    assert m and int(m.group(1)) == 7 * (2 + 4 + 4)        # n_src = 0 runs with a base only
    assert float(m.group(2)) < 1e-5


def test_the_adjoint_simulation_still_compiles_unchanged():
    """resample_core.h grew; tests/csrc/resample_sim.cpp (the adjoint's simulation) must keep compiling against it as it is."""
    src = os.path.join(ROOT, "tests", "csrc", "resample_sim.cpp")
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-c", src, "-o", os.path.join(d, "sim.o")], check=True)
