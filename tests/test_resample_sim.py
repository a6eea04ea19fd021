"""CPU: host-side run of the adjoint bilinear resample's per-axis window / weight arithmetic — tests/csrc/resample_sim.cpp
compiled with g++ against cambrian_amd/csrc/resample_core.h (the very header both resample kernels include): every
(n_in, n_out) in 1..48 x 1..48 and the release pairs; the candidate window of every input holds every output that names
it, every output's weights sum to 1, and the window stays within the trip count the kernel's loops are sized for."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resample_window_simulation():
    src = os.path.join(ROOT, "tests", "csrc", "resample_sim.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sim")
        subprocess.run(["g++", "-O1", "-std=c++17", src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK" in out.stdout
    m = re.search(r"pairs (\d+), widest window (\d+) .* widest at the release pairs (\d+)", out.stdout)
    assert m and int(m.group(1)) == 48 * 48 + 6
    assert int(m.group(3)) <= 9          # 32 -> 96: 2 / scale = 6 outputs, two end points, one widening output each side
