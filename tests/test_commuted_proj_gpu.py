"""`-m gpu`: the commuted aux projection — ``cmb_resample_accum`` (resample_accum.hip), the operator
``ops.linear_stage_maps`` built on it, and the tower -> projector boundary that hands it stage maps.

Raw kernel: against float64 torch (``F.interpolate`` on float64, sum, erf-GELU) on the very (dtype-rounded) values the kernel
reads; bounds as ``tests/test_resample_bwd_gpu.py::BOUND`` — one rounding of an fp32 sum: 1e-5 (fp32), 1e-2 (bf16).

Operator: by definition ``ops.linear(ops.resample_concat(maps, side).reshape(-1, sum C), weight, bias, act)``.  fp32: output,
the whole weight gradient, the bias gradient and the map gradients against that composition within ``TOL["fp32"]`` (CPU float32
emulation of both paths: <= 1.3e-6).  bf16: both paths against a float64 reference from the same bf16 inputs; the fused path's
error on the output and on the weight gradient must be < ``TOL["bf16"]`` and <= 2 x the unfused path's error measured in the
same test (CPU emulation: ratios 0.74-0.94 with fp32 partial products — the default — and 0.75-1.36 with bf16 ones).

Model: a small SVA model whose ConvNeXt tower is a real ``CLIPConvNextTower``; switch on against switch off."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import TOL, rel_err

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
BOUND = {"fp32": 1e-5, "bf16": 1e-2}
B = 2
GRIDS = [((8, 8), (12, 12)), ((4, 4), (12, 12)), ((4, 6), (7, 3)), ((1, 1), (4, 4))]
# (n_src, base, bias, gelu): every value of each at least twice, n_src = 0 with a base
CONFIGS = [(1, True, True, True), (2, False, False, False), (0, True, True, True), (1, False, True, False),
           (2, True, False, True), (1, True, False, False), (0, True, False, False), (2, False, True, True)]
SENTINEL = 777.0


@functools.lru_cache(maxsize=None)
def _ops():
    import __graft_entry__ as ge
    ge.build()
    from cambrian_amd import lib, ops
    from cambrian_amd.model.multimodal_encoder import vit_ops
    return ops, lib, vit_ops


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _interp64(x, gi, go):
    """x [B, hi*wi, C] (any dtype) -> float64 [B, ho*wo, C]."""
    y = x.double().view(x.shape[0], gi[0], gi[1], -1).permute(0, 3, 1, 2)
    y = F.interpolate(y, size=go, mode="bilinear", align_corners=False)
    return y.permute(0, 2, 3, 1).flatten(1, 2)


@functools.lru_cache(maxsize=None)
def _raw_inputs(gi, go, C, src_name):
    """Seeded CPU inputs in the source dtype (never written to): base, bias, two sources (the second on half the grid)."""
    gen = torch.Generator().manual_seed(1000 * gi[0] * gi[1] + 10 * go[0] * go[1] + C)
    sdt = DTYPES[src_name]
    g2 = (max(gi[0] // 2, 1), max(gi[1] // 2, 1))
    base = torch.randn(B, go[0] * go[1], C, generator=gen).to(sdt)
    bias = torch.randn(C, generator=gen)
    srcs = [(torch.randn(B, g[0] * g[1], C, generator=gen).to(sdt), g) for g in (gi, g2)]
    return base, bias, srcs


@pytest.mark.parametrize("name,src_name", [("fp32", "fp32"), ("bf16", "bf16"), ("bf16", "fp32")])
@pytest.mark.parametrize("C", [8, 72])
@pytest.mark.parametrize("gi,go", GRIDS)
def test_raw_kernel(dev, name, src_name, C, gi, go):
    ops, lib, _ = _ops()
    dt, sdt = DTYPES[name], DTYPES[src_name]
    base, bias, srcs = _raw_inputs(gi, go, C, src_name)
    P = go[0] * go[1]
    base_buf = torch.full((B, P, C + 16), SENTINEL, dtype=sdt)
    base_buf[:, :, 8:8 + C] = base
    base_buf = base_buf.to(dev)
    bias_d = bias.to(dev)
    srcs_d = [(x.to(dev), g[0], g[1]) for x, g in srcs]
    for n_src, has_base, has_bias, gelu in CONFIGS:
        pre_ref = torch.zeros(B, P, C, dtype=torch.float64)
        if has_base:
            pre_ref = pre_ref + base.double()
        if has_bias:
            pre_ref = pre_ref + bias.double()
        for x, g in srcs[:n_src]:
            pre_ref = pre_ref + _interp64(x, g, go)
        out_ref = _gelu64(pre_ref) if gelu else pre_ref
        out_buf = torch.full((B, P, C + 16), SENTINEL, dtype=dt, device=dev)
        pre_buf = torch.full((B, P, C + 8), SENTINEL, dtype=dt, device=dev)
        ops.k_resample_accum(out_buf[:, :, 8:8 + C], go[0], go[1], base=base_buf[:, :, 8:8 + C] if has_base else None,
                             bias=bias_d if has_bias else None, srcs=srcs_d[:n_src], pre_out=pre_buf[:, :, :C],
                             act=lib.ACT_GELU_ERF if gelu else lib.ACT_NONE)
        out, pre = out_buf[:, :, 8:8 + C], pre_buf[:, :, :C]
        e_out, e_pre = rel_err(out, out_ref), rel_err(pre, pre_ref)
        print(f"{gi}->{go} C={C} {name}<-{src_name} n_src={n_src} base={has_base} bias={has_bias} gelu={gelu}: "
              f"out {e_out:.3g} pre {e_pre:.3g}")
        assert e_out < BOUND[name] and e_pre < BOUND[name]
        # outside the written slices the buffers are untouched
        assert (out_buf[:, :, :8] == SENTINEL).all() and (out_buf[:, :, 8 + C:] == SENTINEL).all()
        assert (pre_buf[:, :, C:] == SENTINEL).all()
        # without pre_out the same output, bit for bit
        out2 = torch.empty(B, P, C, dtype=dt, device=dev)
        ops.k_resample_accum(out2, go[0], go[1], base=base_buf[:, :, 8:8 + C] if has_base else None,
                             bias=bias_d if has_bias else None, srcs=srcs_d[:n_src],
                             act=lib.ACT_GELU_ERF if gelu else lib.ACT_NONE)
        assert torch.equal(out2, out)
    assert (base_buf[:, :, :8] == SENTINEL).all()


def test_equal_pre_activations_give_the_gemm_epilogue_activation(dev):
    """GELU here is the GEMM epilogue's device function: a pre-activation that is exactly representable gives, bit for bit,
    the activation a fused ``ops.k_gemm(..., act=GELU)`` gives for it (bf16)."""
    ops, lib, _ = _ops()
    gen = torch.Generator().manual_seed(3)
    pre = (torch.randn(128, 64, generator=gen) * 2).to(torch.bfloat16).to(dev)
    eye = torch.eye(64, dtype=torch.bfloat16, device=dev)
    want = ops.k_gemm(pre, eye, act=lib.ACT_GELU_ERF)                  # x @ I^T: the fp32 accumulator holds pre exactly
    got = torch.empty_like(pre)
    ops.k_resample_accum(got.view(2, 64, 64), 8, 8, base=pre.view(2, 64, 64), act=lib.ACT_GELU_ERF)
    assert torch.equal(got, want)


# ---- operator ---------------------------------------------------------------------------------------------------------
N_OUT = 64
OP_CASES = {"a": ((16, 8, 4, 2), (64, 64, 128, 128), 8),          # the small tower of the model tests
            "b": ((32, 16, 8, 4), (64, 128, 256, 512), 12)}       # the release topology: two stages down-, two up-sampled


@functools.lru_cache(maxsize=None)
def _op_inputs(case, name):
    """Seeded CPU inputs (never written to): maps in the dtype of the case, fp32 master weight / bias whose values are bf16
    numbers (both paths and the reference then read the same weight), the upstream gradient."""
    grids, dims, side = OP_CASES[case]
    dt = DTYPES[name]
    gen = torch.Generator().manual_seed(41 + ord(case))
    maps = [torch.randn(B, s, s, c, generator=gen).to(dt) for s, c in zip(grids, dims)]
    w = (torch.randn(N_OUT, sum(dims), generator=gen) / math.sqrt(sum(dims))).to(torch.bfloat16).float()
    b = (0.5 * torch.randn(N_OUT, generator=gen)).to(torch.bfloat16).float()
    go = torch.randn(B * side * side, N_OUT, generator=gen).to(dt)
    return maps, w, b, go


@functools.lru_cache(maxsize=None)
def _op_ref64(case, name, gelu, with_bias):
    """float64 autograd of the definition on the CPU: (out, dW, db, [d maps])."""
    grids, dims, side = OP_CASES[case]
    maps, w, b, go = _op_inputs(case, name)
    m64 = [m.double().requires_grad_() for m in maps]
    w64 = w.double().requires_grad_()
    b64 = b.double().requires_grad_()
    x = torch.cat([_interp64(m.view(B, s * s, c), (s, s), (side, side)) for m, s, c in zip(m64, grids, dims)], -1)
    pre = x.reshape(-1, sum(dims)) @ w64.t()
    if with_bias:
        pre = pre + b64
    out = _gelu64(pre) if gelu else pre
    out.backward(go.double())
    return out.detach(), w64.grad, b64.grad if with_bias else None, [m.grad for m in m64]


def _op_run(dev, case, name, fused, gelu=True, with_bias=True, maps_grad=True, monkeypatch=None, heavy=False):
    ops, lib, _ = _ops()
    grids, dims, side = OP_CASES[case]
    maps, w, b, go = _op_inputs(case, name)
    md = [m.clone().to(dev).requires_grad_(maps_grad) for m in maps]
    wd = torch.nn.Parameter(w.clone().to(dev))
    bd = torch.nn.Parameter(b.clone().to(dev)) if with_bias else None
    act = lib.ACT_GELU_ERF if gelu else lib.ACT_NONE
    if fused:
        out = ops.linear_stage_maps(md, side, wd, bd, act, heavy=heavy, enabled=True)
    else:
        out = ops.linear(ops.resample_concat(md, side).reshape(-1, sum(dims)), wd, bd, act=act)
    assert out.shape == (B * side * side, N_OUT) and out.dtype == DTYPES[name]
    out.backward(go.to(dev))
    return out.detach(), wd.grad, None if bd is None else bd.grad, [m.grad for m in md]


@pytest.mark.parametrize("case,gelu,with_bias", [("a", True, True), ("b", True, True), ("a", False, False)])
def test_operator_fp32_equals_its_definition(dev, case, gelu, with_bias):
    grids, dims, side = OP_CASES[case]
    out_f, dw_f, db_f, dm_f = _op_run(dev, case, "fp32", True, gelu, with_bias)
    out_u, dw_u, db_u, dm_u = _op_run(dev, case, "fp32", False, gelu, with_bias)
    assert dw_f.shape == (N_OUT, sum(dims)) and dw_f.dtype == torch.float32
    errs = {"out": rel_err(out_f, out_u), "dW": rel_err(dw_f, dw_u)}
    if with_bias:
        errs["db"] = rel_err(db_f, db_u)
    for k, (a, b_) in enumerate(zip(dm_f, dm_u)):
        assert a is not None and a.shape == b_.shape
        errs[f"dmap{k}"] = rel_err(a, b_)
    # per column block of the weight gradient: a wrong column offset shows even under a small whole-matrix norm
    off = 0
    for k, c in enumerate(dims):
        errs[f"dW[:, stage {k}]"] = rel_err(dw_f[:, off:off + c], dw_u[:, off:off + c])
        off += c
    ref = _op_ref64(case, "fp32", gelu, with_bias)
    print(f"case {case}: fused vs unfused {({k: float(f'{v:.3g}') for k, v in errs.items()})}; "
          f"vs float64: fused out {rel_err(out_f, ref[0]):.3g} dW {rel_err(dw_f, ref[1]):.3g}, "
          f"unfused out {rel_err(out_u, ref[0]):.3g} dW {rel_err(dw_u, ref[1]):.3g}")
    for k, v in errs.items():
        assert v < TOL["fp32"], (k, v)


@pytest.mark.parametrize("case", ["a", "b"])
def test_operator_bf16_is_no_worse_than_the_unfused_path(dev, case):
    out_f, dw_f, db_f, dm_f = _op_run(dev, case, "bf16", True)
    out_u, dw_u, db_u, dm_u = _op_run(dev, case, "bf16", False)
    ref_out, ref_dw, ref_db, ref_dm = _op_ref64(case, "bf16", True, True)
    for what, f, u, r in (("out", out_f, out_u, ref_out), ("dW", dw_f, dw_u, ref_dw)):
        ef, eu = rel_err(f, r), rel_err(u, r)
        print(f"case {case} {what}: fused {ef:.4g} unfused {eu:.4g} ratio {ef / eu:.3f}")
        assert ef < TOL["bf16"], (what, ef)
        assert ef <= 2 * eu, (what, ef, eu)
    assert rel_err(db_f, ref_db) < TOL["bf16"]
    for a, r in zip(dm_f, ref_dm):
        assert rel_err(a, r) < TOL["bf16"]


def test_operator_is_bit_reproducible(dev):
    out_a, dw_a, db_a, dm_a = _op_run(dev, "b", "bf16", True)
    out_b, dw_b, db_b, dm_b = _op_run(dev, "b", "bf16", True)
    assert torch.equal(out_a, out_b) and torch.equal(dw_a, dw_b) and torch.equal(db_a, db_b)
    assert all(torch.equal(a, b_) for a, b_ in zip(dm_a, dm_b))


def test_frozen_maps_get_no_gradient_and_no_adjoint_gemm(dev):
    """Frozen towers: the maps carry no gradient; the weight and bias gradients are those of the trainable-maps run."""
    out_a, dw_a, db_a, dm_a = _op_run(dev, "a", "bf16", True, maps_grad=False)
    out_b, dw_b, db_b, _ = _op_run(dev, "a", "bf16", True, maps_grad=True)
    assert all(g is None for g in dm_a)
    assert torch.equal(out_a, out_b) and torch.equal(dw_a, dw_b) and torch.equal(db_a, db_b)


class _Spy:
    def __init__(self, monkeypatch, mod, attr):
        self.calls, real = [], getattr(mod, attr)
        monkeypatch.setattr(mod, attr, lambda *a, **k: (self.calls.append((a, k)), real(*a, **k))[1])


def test_switch_and_fallbacks(dev, monkeypatch):
    ops, lib, vit_ops = _ops()
    grids, dims, side = OP_CASES["a"]
    maps, w, b, _ = _op_inputs("a", "bf16")
    md = [m.to(dev) for m in maps]
    wd, bd = w.to(dev), b.to(dev)
    accum = _Spy(monkeypatch, ops, "k_resample_accum")
    resample = _Spy(monkeypatch, ops, "k_resample")
    want = ops.linear(ops.concat_stage_maps(md, side).reshape(-1, sum(dims)), wd, bd, act=lib.ACT_GELU_ERF)
    assert len(resample.calls) == 4 and not accum.calls

    def run(**kw):
        del accum.calls[:], resample.calls[:]
        return ops.linear_stage_maps(md, side, wd, bd, lib.ACT_GELU_ERF, **kw)

    # the environment is read at call time; off (the default): the unfused composition, exactly as before
    monkeypatch.delenv("CAMBRIAN_AMD_COMMUTED_PROJ", raising=False)
    assert torch.equal(run(), want) and not accum.calls and len(resample.calls) == 4
    monkeypatch.setenv("CAMBRIAN_AMD_COMMUTED_PROJ", "0")
    assert torch.equal(run(), want) and not accum.calls
    # on: one accumulate launch, the forward resample only for the two dense stages
    monkeypatch.setenv("CAMBRIAN_AMD_COMMUTED_PROJ", "1")
    got = run()
    assert len(accum.calls) == 1 and len(resample.calls) == 2
    assert [c[0][1:3] for c in resample.calls] == [(16, 16), (8, 8)]
    assert len(accum.calls[0][1]["srcs"]) == 2 and accum.calls[0][1]["base"] is not None
    assert rel_err(got, want) < TOL["bf16"]
    assert torch.equal(run(enabled=False), want) and not accum.calls            # the argument overrides the environment
    # fp8 projections active for this (heavy) projector: unfused
    with ops.fp8_projections(True):
        y = run(heavy=True)
        assert not accum.calls and len(resample.calls) == 4
        assert y.shape == want.shape and torch.isfinite(y).all()
        run(heavy=False)
        assert len(accum.calls) == 1                                            # not this projector's business
    # no stage would be commuted
    del accum.calls[:]
    big = [torch.randn(B, 8, 8, 64, device=dev, dtype=torch.bfloat16), torch.randn(B, 16, 16, 64, device=dev, dtype=torch.bfloat16)]
    y = ops.linear_stage_maps(big, 8, wd[:, :128].contiguous(), bd)
    assert not accum.calls and y.shape == (B * 64, N_OUT)
    # an input the kernels do not take (72 channels are no multiple of the GEMM's K step): unfused
    assert not ops.stage_maps_fusable([md[0], torch.zeros(B, 2, 2, 72, device=dev, dtype=torch.bfloat16)], 8,
                                      torch.zeros(64, 136, device=dev), None, lib.ACT_NONE)
    # dense stages that do not own one contiguous run of weight columns: unfused
    assert not ops.stage_maps_fusable([md[0], md[3], md[1]], 8, torch.zeros(64, 256, device=dev), None, lib.ACT_NONE)
    assert ops.stage_maps_fusable(md, side, wd, bd, lib.ACT_GELU_ERF)


def test_bf16_partial_products_switch(dev, monkeypatch):
    """CAMBRIAN_AMD_COMMUTED_PROJ_F32=0 keeps base / Y_s in bf16 (A/B runs): still within the operator's bf16 bounds."""
    monkeypatch.setenv("CAMBRIAN_AMD_COMMUTED_PROJ_F32", "0")
    ops, _, _ = _ops()
    accum = _Spy(monkeypatch, ops, "k_resample_accum")
    out_f, dw_f, _, _ = _op_run(dev, "b", "bf16", True)
    assert accum.calls[0][1]["base"].dtype == torch.bfloat16
    out_u, dw_u, _, _ = _op_run(dev, "b", "bf16", False)
    ref_out, ref_dw, _, _ = _op_ref64("b", "bf16", True, True)
    for what, f, u, r in (("out", out_f, out_u, ref_out), ("dW", dw_f, dw_u, ref_dw)):
        ef, eu = rel_err(f, r), rel_err(u, r)
        print(f"bf16 partial products, {what}: fused {ef:.4g} unfused {eu:.4g} ratio {ef / eu:.3f}")
        assert ef < TOL["bf16"] and ef <= 2 * eu


# ---- model ------------------------------------------------------------------------------------------------------------
TOWER_NAME = "clip-convnext-L-multi-stage-res64-interp64"


def _build_model(dev, dt, monkeypatch, unfreeze=False):
    """test_model_gpu._build with its ConvNeXt stand-in replaced by a real CLIPConvNextTower of the same small architecture
    (depths (1, 1, 1, 1), dims (64, 64, 128, 128), 64-pixel input, stage maps 16 / 8 / 4 / 2 -> 8 x 8, random init)."""
    _ops()
    from types import SimpleNamespace
    import test_model_gpu as M
    from cambrian_amd.model.multimodal_encoder import clip_convnext_encoder as CE
    base_name = CE.extract_res_interp(TOWER_NAME)[0]
    monkeypatch.setitem(CE.CONVNEXT_ARCH, base_name, dict(depths=(1, 1, 1, 1), dims=(64, 64, 128, 128), ln_eps=1e-5))
    small = M._SmallTower

    def make(kind, dev_, dt_, seed):
        if not kind.startswith("convnext"):
            return small(kind, dev_, dt_, seed)
        t = CE.CLIPConvNextTower(TOWER_NAME, SimpleNamespace(unfreeze_mm_vision_tower=kind.endswith("_train")), delay_load=True)
        t._compute_dtype = dt_
        t.load_model()
        assert t.offers_stage_maps and t.hidden_size == 384 and t.num_patches_per_side == 8
        t.tokens, t.res, t.trainable = 64, 64, kind.endswith("_train")
        return t

    monkeypatch.setattr(M, "_SmallTower", make)
    model, cfg, towers = M._build(dev, dt, monkeypatch, kinds=("vit", "convnext_train" if unfreeze else "convnext"))
    assert isinstance(towers[1], CE.CLIPConvNextTower)
    return model, cfg, towers


def _batch():
    from cambrian_amd.train.data_layout import synthetic_batch
    import test_model_gpu as M
    return synthetic_batch(2, seq_len=M.S, image_position=M.P0, image_token_len=M.SIDE * M.SIDE, aux_token_lens=[16, 64],
                           image_res=[56, 64], image_sizes=[(336, 336), (336, 150)], vocab_lo=1, vocab_hi=300)


def _step(model, batch, dev, dt):
    model.zero_grad(set_to_none=True)
    out = model(input_ids=batch["input_ids"].to(dev), attention_mask=batch["attention_mask"].to(dev),
                position_ids=batch["position_ids"].to(dev), labels=batch["labels"].to(dev),
                images=[i.to(dev, dt) for i in batch["images"]],
                image_aux_attention_masks_list=[m.to(dev) for m in batch["image_aux_attention_masks_list"]],
                image_sizes=batch["image_sizes"])
    logits = out.logits.detach().float().clone()        # before backward(): a fused loss reuses the logits buffer
    out.loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
    return out.loss.item(), logits, grads


def _on_off(dev, dt, monkeypatch, unfreeze, tol, via_config=False):
    ops, _, _ = _ops()
    model, cfg, towers = _build_model(dev, dt, monkeypatch, unfreeze)
    keys = [k for k in model.state_dict() if "mm_projector_aux_" in k]
    accum = _Spy(monkeypatch, ops, "k_resample_accum")
    batch = _batch()
    monkeypatch.delenv("CAMBRIAN_AMD_COMMUTED_PROJ", raising=False)
    loss_off, logits_off, grads_off = _step(model, batch, dev, dt)
    assert not accum.calls
    if via_config:
        cfg.mm_commuted_aux_projection = True
    else:
        monkeypatch.setenv("CAMBRIAN_AMD_COMMUTED_PROJ", "1")
    loss_on, logits_on, grads_on = _step(model, batch, dev, dt)
    assert len(accum.calls) == 1                        # the ConvNeXt tower's projector, and only it
    assert [k for k in model.state_dict() if "mm_projector_aux_" in k] == keys and len(keys) == 12
    e_logits = rel_err(logits_on, logits_off)
    worst = ("", 0.0)
    assert grads_on.keys() == grads_off.keys()
    for n, g_off in grads_off.items():
        e = rel_err(grads_on[n], g_off)
        if e > worst[1]:
            worst = (n, e)
    print(f"{dt} unfreeze={unfreeze}: loss {loss_on:.7g} vs {loss_off:.7g}, logits rel_err {e_logits:.3g}, "
          f"worst gradient {worst} of {len(grads_off)}")
    assert abs(loss_on - loss_off) < tol * max(1.0, abs(loss_off))
    assert e_logits < tol
    assert worst[1] < tol, worst
    return grads_off


@pytest.mark.parametrize("name", ["fp32", "bf16"])
def test_model_switch_on_equals_switch_off(dev, monkeypatch, name):
    grads = _on_off(dev, DTYPES[name], monkeypatch, False, TOL[name])
    assert any("mm_projector_aux_1.0.weight" in n for n in grads) and len(grads) > 50


def test_model_switch_through_the_config(dev, monkeypatch):
    _on_off(dev, torch.float32, monkeypatch, False, TOL["fp32"], via_config=True)


def test_model_unfrozen_tower_gradients(dev, monkeypatch):
    """Towers that train compute in bf16 only (fp32 masters), so this is the bf16 comparison with the ConvNeXt tower unfrozen:
    the loss reaches the tower through d(maps) — g_s W_s for the commuted stages, g W_dense through the adjoint resample for
    the dense ones — and every tower parameter's gradient is compared, switch on against switch off, within TOL["bf16"]."""
    grads = _on_off(dev, torch.bfloat16, monkeypatch, True, TOL["bf16"])
    tower = [n for n in grads if "vision_tower_aux_list.1." in n]
    assert len(tower) > 30, len(tower)


def test_model_generate_equal_tokens(dev, monkeypatch):
    ops, _, _ = _ops()
    from test_dynamic_gpu import _eval_batch
    model, cfg, towers = _build_model(dev, torch.float32, monkeypatch)
    model.eval()
    ids, att, sizes, images = _eval_batch(dev, torch.float32, towers)
    ids, sizes, images = ids[:1], sizes[1:2], [i[1:2] for i in images]
    kw = dict(images=[i.to(dev) for i in images], image_sizes=sizes, max_new_tokens=3)
    accum = _Spy(monkeypatch, ops, "k_resample_accum")
    monkeypatch.delenv("CAMBRIAN_AMD_COMMUTED_PROJ", raising=False)
    off = model.generate(ids.to(dev), **kw)
    assert not accum.calls
    monkeypatch.setenv("CAMBRIAN_AMD_COMMUTED_PROJ", "1")
    on = model.generate(ids.to(dev), **kw)
    assert len(accum.calls) >= 1 and off.shape == (1, 3)
    assert torch.equal(on, off)
