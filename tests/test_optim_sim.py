"""CPU: host-side run of the optimizer kernels' arithmetic — tests/csrc/optim_sim.cpp compiled with g++ against
cambrian_amd/csrc/optim_core.h (the very header optim.hip includes): the bf16 rounding over every upper half, the fixed-order
chunk sum of squares against a long double sum, the AdamW update against a double one, the clip coefficient.  Once as built
normally, once as a stand-alone binary under AddressSanitizer + UndefinedBehaviorSanitizer (host code only, no Python in the
process)."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "optim_sim.cpp")


def _run(flags):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sim")
        subprocess.run(["g++", "-std=c++17", "-Wall", *flags, SRC, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.rstrip().endswith("OK")
    return out


def test_optim_simulation():
    out = _run(["-O1"]).stdout
    assert int(re.search(r"bf16 patterns (\d+)", out).group(1)) == 65536 * 8
    m = re.search(r"sum cases (\d+), worst rel err (\S+)", out)
    # a tree over <= 2^16 non-negative terms errs by at most (16 + 3) * 2^-24 ~ 1.1e-6 relative: 1e-5 leaves ~9x
    assert int(m.group(1)) == 7 * 2 and float(m.group(2)) <= 1e-5
    rows = re.findall(r"update wd (\S+): err_core (\S+) err_float (\S+) ulp (\S+)", out)
    assert [float(r[0]) for r in rows] == [0.0, 0.1]
    for _, ec, ef, ulp in rows:
        assert float(ec) <= 2 * float(ef) + float(ulp)


def test_optim_simulation_under_sanitizers():
    out = _run(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
