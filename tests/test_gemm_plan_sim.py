"""CPU: the GEMM dispatch decisions (cambrian_amd/csrc/gemm_plan.h, the very header gemm.hip includes) compiled with g++ —
tests/csrc/gemm_plan_sim.cpp asserts the default-dispatch kernels, the tail-split table, policy / tile_hint precedence, split-K
clamping, the special kernels' eligibility and pair legality on a 256-CU device — and the whole recorded dispatch of
tests/golden/gemm_dispatch_parent.json (tools/record_gemm_dispatch.py on a GPU at the commit named in the file) replayed
through the same header without a GPU: kernel id, cmb_gemm_tail_rows and the pair flag of every case."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_plan_sim") / "sim")
    subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "csrc", "gemm_plan_sim.cpp"), "-o", exe], check=True)
    return exe


def test_plan_simulation(sim):
    out = subprocess.run([sim], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK" in out.stdout


def test_recorded_dispatch_on_the_cpu(sim):
    with open(os.path.join(ROOT, "tests", "golden", "gemm_dispatch_parent.json")) as f:
        golden = json.load(f)
    cases = golden["cases"]
    assert len(cases) >= 38
    out = subprocess.run([sim, "replay", str(golden["cus"] - golden["cus"] % 8)], input="".join(c["plan"] + "\n" for c in cases),
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    for c, line in zip(cases, lines):
        kernel, tail_rows, pair = (int(v) for v in line.split())
        assert (kernel, tail_rows, pair) == (c["kernel"], c["tail_rows"], c["pair"] or 0), (c["name"], line)
