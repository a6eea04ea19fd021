"""bench.py::dump_outputs on host tensors: float32 .npy files, a seeded sample that is the same from call to call, the
parameter and gradient samples at the same positions, a missing gradient as zeros, and the 64 MB bound."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_writes_a_repeatable_float32_sample(tmp_path):
    b = load_bench()
    g = torch.Generator().manual_seed(3)
    shapes, start, params = ((600, 1000), (7,), (1200, 900)), 0, []
    for s in shapes:   # value = flat position in the concatenation (exact in float32 below 2^24)
        n = int(np.prod(s))
        params.append(torch.nn.Parameter(torch.arange(start, start + n, dtype=torch.float32).reshape(s)))
        start += n
    grads = [torch.randn(p.shape, generator=g) for p in params]
    grads[1] = None
    kept = {"logits": torch.randn(b.DUMP_LOGIT_ROWS, 50, generator=g, dtype=torch.bfloat16).float(), "grads": grads}
    b.dump_outputs(str(tmp_path / "a"), torch.tensor(2.5), kept, params)
    b.dump_outputs(str(tmp_path / "b"), torch.tensor(2.5), dict(kept, logits=None), params)
    a = {n[:-4]: np.load(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a")}
    assert sorted(a) == ["grads_sample", "logits_sample", "loss", "params_sample"]
    assert sorted(os.listdir(tmp_path / "b")) == ["grads_sample.npy", "loss.npy", "params_sample.npy"]
    assert all(x.dtype == np.float32 for x in a.values()) and sum(x.nbytes for x in a.values()) <= 64 * 2 ** 20
    assert a["loss"].tolist() == [2.5] and a["logits_sample"].shape == (b.DUMP_LOGIT_ROWS, 50)
    assert a["params_sample"].shape == a["grads_sample"].shape == (b.DUMP_PARAM_SAMPLE,)
    assert np.array_equal(a["params_sample"], np.load(tmp_path / "b" / "params_sample.npy"))   # same seeded positions
    # every sampled parameter value sits at the same flat position as its gradient value
    idx = a["params_sample"].astype(np.int64)
    assert (np.diff(idx) >= 0).all() and idx[-1] < start
    flat_g = torch.cat([(x if x is not None else torch.zeros_like(p)).reshape(-1) for x, p in zip(grads, params)]).numpy()
    assert np.array_equal(flat_g[idx], a["grads_sample"]) and (a["grads_sample"][(idx >= 600000) & (idx < 600007)] == 0).all()
