"""`-m gpu`: the differentiable bilinear resample — ``cmb_resample_bilinear_bwd`` (the adjoint gather kernel), the autograd
operators ``ops.resample_bilinear`` / ``ops.resample_concat`` built on it, and the call sites that now go through them.

The reference everywhere is float64 CPU autograd through ``F.interpolate(..., mode="bilinear", align_corners=False)`` on the
NCHW view, on the very (dtype-rounded) values the kernel reads; the bounds are those of
``test_kernels_gpu.py::test_resample_bilinear`` for the forward kernel: 1e-5 (fp32), 1e-2 (bf16)."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import TOL, rel_err

pytestmark = pytest.mark.gpu

DTYPES = [("fp32", torch.float32), ("bf16", torch.bfloat16)]
BOUND = {"fp32": 1e-5, "bf16": 1e-2}
B = 2
GRIDS = [((3, 3), (8, 8)), ((4, 4), (6, 6)), ((16, 16), (6, 6)), ((8, 8), (3, 3)), ((5, 5), (5, 5)), ((4, 6), (7, 3)),
         ((1, 1), (4, 4)), ((2, 2), (1, 1))]
_interpolate = F.interpolate     # the real one, whatever a test patches into torch.nn.functional


def _ref(x, gi, go, g):
    """float64 autograd: x [B, hi*wi, C], g [B, ho*wo, C] -> (out [B, ho*wo, C], dx [B, hi*wi, C]), both float64."""
    (hi, wi), (ho, wo) = gi, go
    x64 = x.detach().double().cpu().requires_grad_()
    y = _interpolate(x64.view(x.shape[0], hi, wi, -1).permute(0, 3, 1, 2), size=(ho, wo), mode="bilinear", align_corners=False)
    y = y.permute(0, 2, 3, 1).flatten(1, 2)
    y.backward(g.detach().double().cpu())
    return y.detach(), x64.grad


@functools.lru_cache(maxsize=None)
def _case(gi, go, C, name):
    """Seeded (x, g) in the dtype of the case (CPU) and their float64 reference (out, dx); computed once, never written to."""
    dt = dict(DTYPES)[name]
    gen = torch.Generator().manual_seed(1000 * gi[0] * gi[1] + 10 * go[0] * go[1] + C)
    x = torch.randn(B, gi[0] * gi[1], C, generator=gen).to(dt)
    g = torch.randn(B, go[0] * go[1], C, generator=gen).to(dt)
    return (x, g) + _ref(x, gi, go, g)


@functools.lru_cache(maxsize=None)
def _vit_ops():
    import __graft_entry__ as ge
    ge.build()
    from cambrian_amd.model.multimodal_encoder import vit_ops
    return vit_ops


def _ops():
    _vit_ops()
    from cambrian_amd import ops
    return ops


def _raw_bwd(dev, g, gi, go, C):
    """k_resample_bwd on the column slice [8, 8 + C) of a wider gradient buffer, into a NaN-filled dx."""
    vit_ops = _vit_ops()
    buf = torch.randn(B, go[0] * go[1], C + 16, generator=torch.Generator().manual_seed(3)).to(g.dtype)
    buf[:, :, 8:8 + C] = g
    buf = buf.to(dev)
    dx = torch.full((B, gi[0] * gi[1], C), float("nan"), dtype=g.dtype, device=dev)
    vit_ops.k_resample_bwd(buf, go[0], go[1], dx, gi[0], gi[1], col_offset=8)
    return dx


@pytest.mark.parametrize("name,dt", DTYPES)
@pytest.mark.parametrize("C", [8, 72])
@pytest.mark.parametrize("gi,go", GRIDS)
def test_raw_kernel(dev, name, dt, C, gi, go):
    _, g, _, dx_ref = _case(gi, go, C, name)
    dx = _raw_bwd(dev, g, gi, go, C)
    assert torch.isfinite(dx).all(), "a cell of dx was not written"
    e = rel_err(dx, dx_ref)
    print(f"{gi}->{go} C={C} {name}: rel_err {e:.3g}")
    assert e < BOUND[name]
    if (gi, go) in (((16, 16), (6, 6)), ((8, 8), (3, 3))):
        zero_ref = dx_ref == 0
        assert 0.43 < zero_ref.float().mean().item() < 0.45            # 7 of 16 cells have no output that refers to them
        assert torch.equal(dx.cpu() == 0, zero_ref)


@pytest.mark.parametrize("gi,go", [((4, 6), (7, 3)), ((16, 16), (6, 6))])
def test_adjoint_identity_fp32(dev, gi, go):
    """<R x, g> from the forward kernel against <x, R^T g> from the adjoint: any disagreement between the two kernels'
    weights shows here, whatever the reference does."""
    vit_ops = _vit_ops()
    C = 72
    x, g, _, _ = _case(gi, go, C, "fp32")
    y = torch.empty(B, go[0] * go[1], C, device=dev)
    vit_ops.k_resample(x.to(dev), gi[0], gi[1], y, go[0], go[1])
    dx = torch.empty(B, gi[0] * gi[1], C, device=dev)
    vit_ops.k_resample_bwd(g.to(dev), go[0], go[1], dx, gi[0], gi[1])
    lhs = (y.double().cpu() * g.double()).sum().item()
    rhs = (x.double() * dx.double().cpu()).sum().item()
    diff = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
    print(f"{gi}->{go}: <Rx,g> {lhs:.9g} <x,R^T g> {rhs:.9g} rel diff {diff:.3g}")
    assert diff <= 1e-5


@pytest.mark.parametrize("name,dt", DTYPES)
@pytest.mark.parametrize("C", [8, 72])
@pytest.mark.parametrize("behind_cls", [False, True])
def test_ops_resample_bilinear(dev, monkeypatch, name, dt, C, behind_cls):
    ops, vit_ops = _ops(), _vit_ops()
    gi, go = (4, 6), (7, 3)
    x, g, out_ref, dx_ref = _case(gi, go, C, name)
    seen = []
    real = ops.k_resample                                 # (where the launcher lives and ops' own callers look it up)
    monkeypatch.setattr(ops, "k_resample", lambda x_, *a, **k: (seen.append(x_.data_ptr()), real(x_, *a, **k))[1])
    if behind_cls:                                    # the tokens behind a CLS row: read in place, no copy
        parent = torch.cat([torch.ones(B, 1, C, dtype=dt), x], 1).to(dev).requires_grad_()
        xin = parent[:, 1:]
        assert not xin.is_contiguous()
    else:
        parent = x.clone().to(dev).requires_grad_()
        xin = parent
    out = ops.resample_bilinear(xin, *gi, *go)
    assert seen == [xin.data_ptr()]
    assert out.shape == out_ref.shape and out.dtype == dt and out.is_contiguous()
    assert rel_err(out, out_ref) < BOUND[name]
    out.backward(g.to(dev))
    grad = parent.grad
    if behind_cls:
        assert grad.shape == parent.shape and (grad[:, 0] == 0).all()
        grad = grad[:, 1:]
    assert rel_err(grad, dx_ref) < BOUND[name]


def test_ops_resample_bilinear_equal_grids_return_the_input(dev):
    ops = _ops()
    x = torch.randn(B, 25, 8, device=dev, requires_grad=True)
    assert ops.resample_bilinear(x, 5, 5, 5, 5) is x


@pytest.mark.parametrize("name,dt", DTYPES)
def test_ops_resample_concat(dev, monkeypatch, name, dt):
    ops, vit_ops = _ops(), _vit_ops()
    shapes, side = [(8, 8), (4, 16), (2, 24)], 6
    gen = torch.Generator().manual_seed(17)
    maps = [torch.randn(B, s, s, c, generator=gen).to(dt) for s, c in shapes]
    g = torch.randn(B, side * side, sum(c for _, c in shapes), generator=gen).to(dt)
    refs, off = [], 0
    for m, (s, c) in zip(maps, shapes):
        refs.append(_ref(m.view(B, s * s, c), (s, s), (side, side), g[:, :, off:off + c]))
        off += c
    out_ref = torch.cat([r[0] for r in refs], -1)
    calls = []
    real = ops.k_resample_bwd
    monkeypatch.setattr(ops, "k_resample_bwd", lambda *a, **k: (calls.append(a[0].data_ptr()), real(*a, **k))[1])

    leaves = [m.clone().to(dev).requires_grad_() for m in maps]
    out = ops.resample_concat(leaves, side)
    assert out.shape == out_ref.shape and out.dtype == dt and rel_err(out, out_ref) < BOUND[name]
    gd = g.to(dev)
    out.backward(gd)
    assert calls == [gd.data_ptr()] * 3                               # one launch per map, on the gradient where it lies
    for leaf, (s, c), r in zip(leaves, shapes, refs):
        assert leaf.grad.shape == leaf.shape and rel_err(leaf.grad.view(B, s * s, c), r[1]) < BOUND[name]

    # a gradient that arrives with a non-unit last stride is copied once, and the result is the same
    del calls[:]
    leaves2 = [m.clone().to(dev).requires_grad_() for m in maps]
    (ops.resample_concat(leaves2, side).transpose(1, 2) * gd.transpose(1, 2).contiguous()).sum().backward()
    assert len(calls) == 3
    for a, b in zip(leaves, leaves2):
        assert torch.equal(a.grad, b.grad)

    # a map that needs no gradient gets none, and no launch
    del calls[:]
    leaves3 = [m.clone().to(dev).requires_grad_(k != 1) for k, m in enumerate(maps)]
    ops.resample_concat(leaves3, side).backward(gd)
    assert len(calls) == 2 and leaves3[1].grad is None
    assert torch.equal(leaves3[0].grad, leaves[0].grad) and torch.equal(leaves3[2].grad, leaves[2].grad)


def test_backward_is_bit_reproducible(dev):
    gi, go, C = (8, 8), (12, 12), 72
    _, g, _, dx_ref = _case(gi, go, C, "bf16")
    a = _raw_bwd(dev, g, gi, go, C)
    b = _raw_bwd(dev, g, gi, go, C)
    assert torch.equal(a, b) and rel_err(a, dx_ref) < BOUND["bf16"]


# ---- call sites ------------------------------------------------------------------------------------------------------
class _AtenBodyReached(Exception):
    pass


def _raise(*a, **k):
    raise _AtenBodyReached()


def _convnext(dev):
    """The small tower of test_tower_block_recompute_is_the_same_function: 64-pixel input, stage maps 16 / 8 / 4 / 2 -> 8 x 8."""
    _ops()
    from cambrian_amd.model.multimodal_encoder.convnext import ConvNeXtConfig, ConvNeXtTrunk
    from cambrian_amd.model.multimodal_encoder.convnext_train import TrainableConvNeXt
    gen = torch.Generator().manual_seed(5)
    cfg = ConvNeXtConfig(depths=(2, 2, 2, 1), dims=(64, 64, 128, 128), ln_eps=1e-5)
    canon = ConvNeXtTrunk.random_canonical(cfg, gen)
    img = torch.randn(2, 3, 64, 64, generator=gen).to(dev)
    return TrainableConvNeXt(cfg, canon, dev), img


def _convnext_step(dev):
    tower, img = _convnext(dev)
    out = tower(img, 8, multi_stage=True)
    w = torch.randn(out.shape, generator=torch.Generator().manual_seed(9)).to(dev)
    (out.float() * w).sum().backward()
    return out.detach(), {k: v.grad for k, v in tower.p.items()}


def _tokens_step(dev):
    from cambrian_amd.model.multimodal_encoder.vit_train import resample_tokens_autograd
    x = torch.randn(2, 36, 64, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    xd = x.to(dev).requires_grad_()
    out = resample_tokens_autograd(xd, 16)
    out.float().square().sum().backward()
    return x, out.detach(), xd.grad


def test_call_sites_run_without_aten_interpolate(dev, monkeypatch):
    _ops()
    monkeypatch.delenv("CAMBRIAN_AMD_RESAMPLE_BWD", raising=False)
    monkeypatch.setattr(torch.nn.functional, "interpolate", _raise)
    out, grads = _convnext_step(dev)
    assert out.shape == (2, 64, 384) and all(g is not None and torch.isfinite(g).all() for g in grads.values())
    x, out, gx = _tokens_step(dev)
    assert out.shape == (2, 16, 64) and gx.shape == (2, 36, 64)
    out_ref, dx_ref = _ref(x, (6, 6), (4, 4), 2 * out)                 # d(sum out^2) = 2 out, exact in bf16
    assert rel_err(out, out_ref) < BOUND["bf16"] and rel_err(gx, dx_ref) < BOUND["bf16"]

    # the switch reaches the old body at both sites
    monkeypatch.setitem(os.environ, "CAMBRIAN_AMD_RESAMPLE_BWD", "0")
    with pytest.raises(_AtenBodyReached):
        _convnext_step(dev)
    with pytest.raises(_AtenBodyReached):
        _tokens_step(dev)


def test_old_body_against_new_at_the_convnext_tower(dev, monkeypatch):
    _ops()
    monkeypatch.setitem(os.environ, "CAMBRIAN_AMD_RESAMPLE_BWD", "1")
    out_new, grads_new = _convnext_step(dev)
    monkeypatch.setitem(os.environ, "CAMBRIAN_AMD_RESAMPLE_BWD", "0")
    out_old, grads_old = _convnext_step(dev)
    e = rel_err(out_new, out_old)
    print(f"output: rel_err {e:.3g}")
    assert e < 1e-2
    worst = ("", 0.0)
    for k, g_old in grads_old.items():
        assert g_old is not None and grads_new[k] is not None, k
        e = rel_err(grads_new[k], g_old)
        if e > worst[1]:
            worst = (k, e)
    print(f"worst parameter gradient: {worst}")
    assert len(grads_old) > 50 and worst[1] < TOL["bf16"], worst
