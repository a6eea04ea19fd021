"""`-m gpu`: the cross-workgroup sums of the backward (bias, LayerNorm gamma / beta, position-table and newline gradients)
give the same bits on every call: each workgroup writes a partial row into a caller-allocated workspace and the rows are
added in a fixed order (common.h det_sum_kernel), where float atomics used to add them in whatever order the workgroups
finished.  Kernel by kernel, and for a whole forward + backward of the benched model."""
import pytest
import torch

from cambrian_amd import ops

pytestmark = pytest.mark.gpu


def test_colsum_is_bitwise_repeatable(dev):
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(55296, 1024, device=dev, dtype=torch.bfloat16, generator=g)
    scale = torch.rand(55296, 16, device=dev, generator=g)
    runs = [ops.k_colsum(x) for _ in range(3)]
    assert all(torch.equal(runs[0], r) for r in runs[1:])
    torch.testing.assert_close(runs[0], x.float().sum(0), rtol=1e-4, atol=5e-2)
    scaled = [ops.k_colsum(x, row_scale=scale, group=64) for _ in range(3)]
    assert all(torch.equal(scaled[0], r) for r in scaled[1:])


def test_layernorm_bwd_parameter_gradients_are_bitwise_repeatable(dev):
    g = torch.Generator(device=dev).manual_seed(1)
    side, grid_r, D = 96, 4, 1024
    x = torch.randn(2 * side * side, D, device=dev, dtype=torch.bfloat16, generator=g)
    dy = torch.randn(x.shape, device=dev, dtype=torch.bfloat16, generator=g)
    gamma = torch.rand(D, device=dev, generator=g) + 0.5
    add = torch.randn(grid_r * grid_r, D, device=dev, generator=g) * 0.1
    mean, rstd = ops.k_row_stats(x, 1e-5)
    runs = [ops.k_layernorm_bwd(dy, x, mean, rstd, gamma=gamma) for _ in range(3)]
    for _, dgamma, dbeta, _ in runs[1:]:
        assert torch.equal(dgamma, runs[0][1]) and torch.equal(dbeta, runs[0][2])
    ref = (dy.float() * ((x.float() - mean[:, None]) * rstd[:, None])).sum(0)
    torch.testing.assert_close(runs[0][1], ref, rtol=1e-3, atol=5e-2)
    dadds = [ops.k_layernorm_bwd(dy, x, mean, rstd, add=add, side=side, grid_r=grid_r)[3] for _ in range(3)]
    assert all(torch.equal(dadds[0], d) for d in dadds[1:])


def test_layernorm_bwd_multi_table_gradients_are_bitwise_repeatable(dev):
    g = torch.Generator(device=dev).manual_seed(2)
    side, grid_r, D, layers = 96, 4, 1024, 5
    x = torch.randn(2 * side * side, D, device=dev, dtype=torch.bfloat16, generator=g)
    adds = [torch.randn(grid_r * grid_r, D, device=dev, generator=g) * 0.1 for _ in range(layers)]
    dys = [torch.randn(x.shape, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(layers)]
    mean, rstd = ops.k_row_stats(x, 1e-5)

    def run():
        dadd = [torch.zeros_like(a) for a in adds]
        dx = torch.zeros(x.shape, device=dev, dtype=torch.float32)
        ops.k_layernorm_bwd_multi(x, [(dy, mean, rstd, a, i) for i, (dy, a) in enumerate(zip(dys, adds))], side, grid_r, dx,
                                  False, dadd)
        return dadd
    first = run()
    for _ in range(2):
        assert all(torch.equal(a, b) for a, b in zip(first, run()))


def test_pretraining_step_gradients_are_bitwise_repeatable(dev):
    """Forward + backward of the benched model (2 decoder layers, one image) twice on the same parameters and batch: the loss
    and EVERY trainable gradient — projectors, SVA layers, position tables, LayerNorms, biases, image newline — bit for bit."""
    import importlib.util
    import os
    os.environ.setdefault("CAMBRIAN_AMD_RANDOM_INIT", "1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_det", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from cambrian_amd.train.data_layout import synthetic_batch
    model, cfg = bench.build_model(dev, llm_layers=2)
    b = synthetic_batch(1, seed=1234, image_position=cfg.image_position)
    kw = dict(input_ids=b["input_ids"].to(dev), labels=b["labels"].to(dev), position_ids=b["position_ids"].to(dev),
              attention_mask=None, images=[i.to(dev, torch.bfloat16) for i in b["images"]],
              image_aux_attention_masks_list=[m.to(dev) for m in b["image_aux_attention_masks_list"]],
              image_sizes=b["image_sizes"])
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    runs = []
    for _ in range(2):
        out = model(**kw)
        out.loss.backward()
        runs.append((out.loss.item(), {n: p.grad.detach().clone() for n, p in named if p.grad is not None}))
        model.zero_grad(set_to_none=True)
    (l0, g0), (l1, g1) = runs
    assert l0 == l1 and set(g0) == set(g1) and len(g0) > 100
    differ = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not differ, f"{len(differ)} of {len(g0)} gradients differ between two identical backward passes: {differ[:8]}"
    del model
    torch.cuda.empty_cache()
