"""GPU: every branch of the GEMM dispatch takes the kernel, and produces the bits, recorded at the commit named in
tests/golden/gemm_dispatch_parent.json.  tools/record_gemm_dispatch.py holds the case list (the smallest problems that reach
each branch of cmb_gemm / cmb_gemm_pair / cmb_gemm_tn; operands from a CPU generator seeded with the case index) and wrote the
file; here each case is launched once on the tree under test: equal cmb_gemm_last_kernel / cmb_gemm_pair_last /
cmb_gemm_tail_rows, equal SHA-256 of the output bytes.  The tail split and the pair arithmetic count in CUs: on a device with
another CU count than the recorded one the comparison does not apply."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "gemm_dispatch_parent.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def recorder(dev):
    spec = importlib.util.spec_from_file_location("record_gemm_dispatch", os.path.join(ROOT, "tools", "record_gemm_dispatch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if mod.device_cus() != GOLDEN["cus"]:
        pytest.skip(f"recorded on a device with {GOLDEN['cus']} CUs, this one has {mod.device_cus()}")
    assert [name for name, _ in mod.CASES] == [c["name"] for c in GOLDEN["cases"]]
    return mod


@pytest.mark.parametrize("index", range(len(GOLDEN["cases"])), ids=[c["name"] for c in GOLDEN["cases"]])
def test_dispatch_and_bits_as_recorded(dev, recorder, index):
    want = GOLDEN["cases"][index]
    got = recorder.run_case(index, dev)
    assert (got["kernel"], got["pair"], got["tail_rows"]) == (want["kernel"], want["pair"], want["tail_rows"]), (want["name"], got)
    if want["hash"] is not None:   # (null: the case did not reproduce its own bits at the recorded commit; ids only)
        assert got["hash"] == want["hash"], want["name"]
