"""`-m gpu`: the attention kernels (flash_bwd.hip, flash2.hip) through ops.causal_attention and ops.vit_attention, judged per
block of 16 rows against an fp64 reference (tests/attn_check.py: block_err, lse_err, TOL), on the input families that move the
running maximum into late tiles (`peaked`) and put the weight on the causal edge (`diag`) as well as on Gaussian data, at the
smallest shapes at which the tiling can go wrong: one 128-row block, odd block counts through flash_items' pairing, padded
whole tiles / prefixes / single keys either side of a tile edge, token counts just before and after the 64-key and 128-row
edges.  The tolerances come from the CPU measurements of tests/test_attn_check_host.py, never from these kernels.  Every figure
is printed before it is asserted (`pytest -s`)."""
import functools

import pytest
import torch

import attn_check as A

pytestmark = pytest.mark.gpu
D = 128


def _attn_node(out):
    """The autograd node of ops.CausalAttnFn under ``out`` (vit_attention slices its output)."""
    n = out.grad_fn
    while type(n).__name__ != "CausalAttnFnBackward":
        n = n.next_functions[0][0]
    return n


def _run(q, k, v, w, key_valid=None, vit_scale=None):
    """(o, lse, dq, dk, dv) of the kernels for bf16 q, k, v and the upstream gradient w."""
    from cambrian_amd import ops
    q, k, v = (t.detach().requires_grad_() for t in (q, k, v))
    out = ops.causal_attention(q, k, v, key_valid) if vit_scale is None else ops.vit_attention(q, k, v, vit_scale)
    lse = _attn_node(out).saved_tensors[4][..., :q.shape[2]]
    out.backward(w)
    return out.detach(), lse, q.grad, k.grad, v.grad


@functools.lru_cache(maxsize=None)
def _case(dev, family, B, H, HKV, S, hd=D, mask=None, seed=0, bidir=False):
    """Inputs on the device and the fp64 reference, computed once per case and shared (never modified)."""
    scale = hd ** -0.5
    q, k, v, w = A.inputs(family, B, H, HKV, S, hd, seed=seed, scale=scale, device=dev)
    kv = None if mask is None else A.key_valid_mask(mask, B, S).to(dev)
    allow = torch.ones(1, 1, S, S, dtype=torch.bool, device=dev) if bidir else A.causal_allow(S, kv, device=dev)
    return (q, k, v, w), kv, A.reference(q, k, v, w, allow, scale)


def _judge(family, got, ref, label, zero_ok=False, skip=()):
    bad = []
    for name, a, r in zip(A.OUTPUTS, got, ref):
        if name in skip:
            continue
        err, tol = A.check(family, name, a, r, zero_ok=zero_ok and name in ("dq", "dk"))
        print(f"{label} {family} {name}: {err:.3g} (tol {tol})")
        if tol is not None and not err <= tol:
            bad.append(f"{label} {family} {name}: {err:.3g} > {tol}")
    assert not bad, bad


@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("S", A.CAUSAL_S)
@pytest.mark.parametrize("H,HKV", A.CAUSAL_HEADS)
def test_causal_tiles(dev, H, HKV, S, family):
    from cambrian_amd import ops
    (q, k, v, w), _, ref = _case(str(dev), family, 2, H, HKV, S, seed=S + H)
    assert ops.causal_attention_supported(q, k)
    _judge(family, _run(q, k, v, w), ref, f"causal S={S} H={H}/{HKV}")


@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("mask", A.MASK_NAMES)
def test_causal_key_valid_tiles(dev, mask, family):
    """causal AND key_valid with the diagonal reopened: allow = tril & key_valid | eye.  Rows that see only themselves
    (prefix70) have dq = dk = 0: those blocks get a typical block's error budget (block_errs, zero_ok)."""
    (q, k, v, w), kv, ref = _case(str(dev), family, 2, 4, 1, A.MASK_S, mask=mask, seed=7)
    _judge(family, _run(q, k, v, w, key_valid=kv), ref, f"mask {mask}", zero_ok=True)


@pytest.mark.parametrize("N", A.VIT_N)
@pytest.mark.parametrize("hd", A.VIT_HD)
def test_vit_tiles(dev, hd, N):
    """Bidirectional, kv_len = N on, just before and just after the 64-key and 128-row edges; head_dim zero-padded to 128."""
    B, H = 2, 2
    (q, k, v, w), _, ref = _case(str(dev), "gauss", B, H, H, N, hd=hd, seed=N + hd, bidir=True)
    got = _run(q, k, v, w, vit_scale=hd ** -0.5)
    assert got[0].shape == (B, H, N, hd) and got[2].shape == (B, H, N, hd) and got[3].shape == (B, H, N, hd)
    if N > 1:
        _judge("gauss", got, ref, f"vit N={N} hd={hd}")
        return
    # One token: P = 1, o = v, and dS = P (dP - D) = 0 in exact arithmetic, so dq = dk = 0 and a relative error has nothing
    # to divide by.  The kernels form dP (MFMA) and D (the prologue's loop) as two fp32 sums of the same <= 128 products
    # dO_d v_d: each is within 128 * 2^-23 * sum |dO_d v_d| of the truth (one ulp per addition, which also covers an
    # accumulator that truncates), so |dS| <= 2^-15 * sum |dO v| (P <= 1 + 2^-20), 1.01 for the bf16 rounding of dS and of
    # the result; dq = dS k scale, dk = dS q scale.
    _judge("gauss", got, ref, f"vit N=1 hd={hd}", skip=("dq", "dk"))
    ds_max = 1.01 * 2.0 ** -15 * (w.float().abs() * v.float().abs()).sum(-1, keepdim=True)
    assert bool((got[2].float().abs() <= ds_max * k.float().abs() * hd ** -0.5).all())
    assert bool((got[3].float().abs() <= ds_max * q.float().abs() * hd ** -0.5).all())


@pytest.mark.parametrize("knob", A.FLASH_KNOBS)
def test_every_shipped_variant_per_tile(dev, knob):
    """CMB_KNOB_FLASH: each variant the library ships, causal S = 384 (three blocks: the pairing of flash_items) and the
    key-padding masks, all three families."""
    from cambrian_amd import lib as L
    default = L.load().cmb_knob_get(L.KNOB_FLASH)
    try:
        L.knob_set(L.KNOB_FLASH, knob)
        for family in A.FAMILIES:
            (q, k, v, w), _, ref = _case(str(dev), family, 2, 4, 2, A.MASK_S, seed=A.MASK_S + 4)
            _judge(family, _run(q, k, v, w), ref, f"knob {knob} causal")
            for mask in A.MASK_NAMES:
                (q, k, v, w), kv, ref = _case(str(dev), family, 2, 4, 1, A.MASK_S, mask=mask, seed=7)
                _judge(family, _run(q, k, v, w, key_valid=kv), ref, f"knob {knob} mask {mask}", zero_ok=True)
    finally:
        L.knob_set(L.KNOB_FLASH, default)


@pytest.mark.parametrize("layout", ["head_major", "packed"])
def test_layouts_bit_equal_to_token_major(dev, layout):
    """ops._token_major's copy path: q, k, v given head-major contiguous, or as slices of one packed [B, S, (H + 2 HKV) D]
    tensor, give o, dq, dk, dv bit-equal to the token-major call."""
    B, H, HKV, S = 2, 4, 2, 384
    (q, k, v, w), _, _ = _case(str(dev), "peaked", B, H, HKV, S, seed=S + H)
    assert q.transpose(1, 2).is_contiguous()
    base = _run(q, k, v, w)
    if layout == "head_major":
        q2, k2, v2 = (t.contiguous() for t in (q, k, v))
        assert q2.is_contiguous() and not q2.transpose(1, 2).is_contiguous()
        w2 = w.contiguous()
    else:
        packed = torch.cat([t.transpose(1, 2).reshape(B, S, -1) for t in (q, k, v)], dim=-1)
        assert packed.shape == (B, S, (H + 2 * HKV) * D)
        q2 = packed[..., :H * D].view(B, S, H, D).transpose(1, 2)
        k2 = packed[..., H * D:(H + HKV) * D].view(B, S, HKV, D).transpose(1, 2)
        v2 = packed[..., (H + HKV) * D:].view(B, S, HKV, D).transpose(1, 2)
        assert not q2.transpose(1, 2).is_contiguous() and q2.data_ptr() == packed.data_ptr()
        w2 = w
    got = _run(q2, k2, v2, w2)
    for name, a, b in zip(A.OUTPUTS, got, base):
        assert a.shape == b.shape and torch.equal(a, b), f"{layout}: {name} differs from the token-major call"


def test_second_call_bit_equal(dev):
    (q, k, v, w), _, _ = _case(str(dev), "peaked", 2, 4, 2, 640, seed=640 + 4)
    first, second = _run(q, k, v, w), _run(q, k, v, w)
    for name, a, b in zip(A.OUTPUTS, first, second):
        assert torch.equal(a, b), f"{name}: second call differs"
