"""`-m gpu`: ``cmb_extend_attn`` (extend_attn.hip) through ``ops.extend_attention`` — a chunk of Q new tokens per cache row
against the bf16 K / V cache, under "s <= t0 + j and (key_valid[s] or s == t0 + j)".

Parity tests compare with test_decode_lookup_gpu.py's float64 CPU reference under the new mask (rotate-half RoPE, masked
softmax, grouped KV heads by indexing, from the inputs AS STORED), tolerance ``conftest.TOL["bf16"]`` through ``rel_err``.  That
metric divides by the tensor's largest element and hides a wrong late row block, so ``test_block_errors`` measures every
16-row block of the chunk against ``attn_check.reference`` with ``attn_check.TOL`` (basis: test_extend_attn_host.py, the twin
over the same cases; a row block of the kernel is at most 16 tokens, so a block of the metric never averages two of them
out)."""
import math

import pytest
import torch

import attn_check as A
from conftest import TOL, rel_err
from test_extend_attn_host import BLOCK_CHUNKS, BLOCK_HEADS, block_case

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
GEOMS = [(4, 2, 64), (4, 4, 64), (8, 2, 128), (7, 1, 128), (3, 3, 96), (32, 8, 128)]
CHUNKS = [(0, 1), (0, 17), (1, 33), (64, 16), (127, 130), (300, 50), (1031 - 40, 40)]
THETA = 10000.0
TAIL = 5          # cache slots past the chunk's own, filled with NaN


def _ops():
    from cambrian_amd import ops
    return ops


def _masks(B, t0, Q):
    """(name, bool [B, t0 + Q + TAIL], poison) — all valid; holes in the cached part (whose slots then hold NaN / 3e4); row
    B - 1 left-padded for the first Q // 3 slots of the chunk.  The tail columns stay False and are never read."""
    n = t0 + Q
    full = torch.zeros(B, n + TAIL, dtype=torch.bool)
    full[:, :n] = True
    holes = full.clone()
    for b in range(B):
        holes[b, :min(t0, 2 + b)] = False
        holes[b, 3 + b:t0:3] = False
    padded = full.clone()
    padded[B - 1, t0:t0 + Q // 3] = False
    return [("all", full, False), ("holes", holes, True), ("padded", padded, False)]


def _inputs(nh, nkv, hd, B, Q, t0, seed):
    g = torch.Generator().manual_seed(seed)
    n = t0 + Q
    q = torch.randn(B * Q, nh * hd, generator=g).to(BF)
    k = torch.randn(B * Q, nkv * hd, generator=g).to(BF)
    v = torch.randn(B * Q, nkv * hd, generator=g).to(BF)
    kc = torch.randn(B, nkv, n + TAIL, hd, generator=g).to(BF)
    vc = torch.randn(B, nkv, n + TAIL, hd, generator=g).to(BF)
    kc[:, :, t0:], vc[:, :, t0:] = float("nan"), float("nan")          # the chunk's own slots (overwritten) and the tail (never read)
    pos = torch.randint(0, 1100, (B, 1), generator=g) + torch.arange(Q)[None]          # consecutive positions per sequence
    return q, k, v, kc, vc, pos


def _reference(q, k, v, cos, sin, kc, vc, t0, Q, valid, nh, nkv, hd):
    """float64 on the CPU -> (out [B*Q, nh*hd], roped new k [B, Q, nkv, hd]): test_decode_lookup_gpu.py's, under the mask
    s <= t0 + j and (valid[b, s] or s == t0 + j) for cached and new slots alike."""
    B = kc.shape[0]
    G, n = nh // nkv, t0 + Q
    c, s = cos.double().cpu().view(B, Q, 1, hd // 2), sin.double().cpu().view(B, Q, 1, hd // 2)

    def rot(x):
        x1, x2 = x[..., :hd // 2], x[..., hd // 2:]
        return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)

    qr = rot(q.double().view(B, Q, nh, hd))
    kr = rot(k.double().view(B, Q, nkv, hd))
    K = kc.double()[:, :, :n].clone()
    V = vc.double()[:, :, :n].clone()
    K[:, :, t0:] = kr.to(BF).double().transpose(1, 2)                  # what the cache holds after the step
    V[:, :, t0:] = v.double().view(B, Q, nkv, hd).transpose(1, 2)
    slot = torch.arange(n)
    limit = t0 + torch.arange(Q)[:, None]
    m = (slot[None] <= limit)[None] & (valid[:, None, :n] | (slot[None] == limit)[None])          # [B, Q, n]
    seen = m.any(1)[:, None, :, None]                                   # a slot nobody may attend may hold NaN: it weighs 0
    K, V = torch.where(seen, K, 0.0), torch.where(seen, V, 0.0)
    head = torch.arange(nh) // G
    sc = torch.einsum("bqhd,bhjd->bhqj", qr, K[:, head]) / math.sqrt(hd)
    sc = sc.masked_fill(~m[:, None], float("-inf"))
    out = torch.einsum("bhqj,bhjd->bqhd", torch.softmax(sc, -1), V[:, head])
    return out.reshape(B * Q, nh * hd), kr


def _bits(x):
    return x.contiguous().view(torch.int16)


def _run(dev, nh, nkv, hd, B, Q, t0, valid, seed=0, splits=0, poison=False, fn=None):
    ops = _ops()
    q, k, v, kc, vc, pos = _inputs(nh, nkv, hd, B, Q, t0, seed)
    if poison:                                                          # masked cached slots hold NaN / huge values
        dead = ~valid[:, :t0]
        kc[:, :, :t0][dead[:, None].expand(B, nkv, t0)] = float("nan")
        vc[:, :, :t0][dead[:, None].expand(B, nkv, t0)] = 3.0e4
    cos, sin = ops.rope_table(pos.to(dev), hd, THETA)
    kcd, vcd = kc.to(dev), vc.to(dev)
    out = (fn or ops.extend_attention)(q.to(dev), k.to(dev), v.to(dev), cos, sin, kcd, vcd, t0, valid.to(dev), splits=splits)
    return out, (q, k, v, kc, vc, cos, sin, kcd, vcd)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel against float64, and what it stores
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("nh,nkv,hd", GEOMS)
def test_kernel_parity(dev, nh, nkv, hd, B):
    ops = _ops()
    worst, split_runs = 0.0, 0
    for t0, Q in CHUNKS:
        n = t0 + Q
        split_runs += ops.extend_attention_plan(B, nkv, t0, Q)[0] > 1
        for mname, valid, poison in _masks(B, t0, Q):
            out, (q, k, v, kc, vc, cos, sin, kcd, vcd) = _run(dev, nh, nkv, hd, B, Q, t0, valid, seed=n + Q, poison=poison)
            ref, kr = _reference(q, k, v, cos, sin, kc, vc, t0, Q, valid, nh, nkv, hd)
            e = rel_err(out, ref)
            worst = max(worst, e)
            what = f"{nh}/{nkv}/{hd} B={B} t0={t0} Q={Q} mask={mname}"
            assert torch.isfinite(out).all(), what                      # padded query rows included: they see themselves
            assert e < TOL["bf16"], f"{what}: out rel err {e}"
            new_v = vcd[:, :, t0:n].cpu()
            assert torch.equal(_bits(new_v), _bits(v.view(B, Q, nkv, hd).transpose(1, 2))), what      # raw v, bit for bit
            new_k = kcd[:, :, t0:n].transpose(1, 2)
            roped = ops.rope(k.to(dev).view(B * Q, nkv, hd), cos, sin).view(B, Q, nkv, hd)
            assert rel_err(new_k, roped) < TOL["bf16"] and rel_err(new_k, kr) < TOL["bf16"], what
            keep = torch.ones(n + TAIL, dtype=torch.bool)
            keep[t0:n] = False
            assert torch.equal(_bits(kcd.cpu()[:, :, keep]), _bits(kc[:, :, keep])), what            # NaN patterns included
            assert torch.equal(_bits(vcd.cpu()[:, :, keep]), _bits(vc[:, :, keep])), what
    assert split_runs >= 2, "no case took the split path and its merge launch"
    print(f"{nh}/{nkv}/{hd} B={B}: worst out rel err {worst:.3g}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. every 16-row block of the chunk (attn_check's metric and tolerances)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh,nkv,hd", BLOCK_HEADS)
@pytest.mark.parametrize("family", A.FAMILIES)
def test_block_errors(dev, family, nh, nkv, hd):
    """cos = 1, sin = 0, so the stored operands are the inputs: q / k / v of ``attn_check.inputs`` over S = t0 + Q slots, the
    first t0 in the cache, the last Q as the chunk; reference ``attn_check.reference`` under ``causal_allow(S, key_valid)``,
    last Q rows.  Row 0 has masked cached keys (poisoned on the device), row 1 a left-padded chunk."""
    ops = _ops()
    B = 2
    for t0, Q in BLOCK_CHUNKS:
        S = t0 + Q
        q, k, v, w, kv, ref, allow = block_case(family, nh, nkv, hd, t0, Q)
        kc = torch.zeros(B, nkv, S + TAIL, hd, dtype=BF)
        vc = torch.zeros_like(kc)
        kc[:, :, :t0], vc[:, :, :t0] = k[:, :, :t0], v[:, :, :t0]
        dead = ~kv[:, :t0]
        kc[:, :, :t0][dead[:, None].expand(B, nkv, t0)] = float("nan")
        vc[:, :, :t0][dead[:, None].expand(B, nkv, t0)] = 3.0e4
        kc[:, :, t0:], vc[:, :, t0:] = float("nan"), float("nan")
        rows = lambda x, h: x[:, :, t0:].transpose(1, 2).reshape(B * Q, h * hd).to(dev)
        cos = torch.ones(B * Q, hd // 2, dtype=torch.float32, device=dev)
        valid = torch.zeros(B, S + TAIL, dtype=torch.bool)
        valid[:, :S] = kv
        out = ops.extend_attention(rows(q, nh), rows(k, nkv), rows(v, nkv), cos, torch.zeros_like(cos), kc.to(dev), vc.to(dev),
                                   t0, valid.to(dev))
        got = out.view(B, Q, nh, hd).transpose(1, 2).cpu()
        e = A.block_err(got, ref)
        print(f"{family} {nh}/{nkv}/{hd} t0={t0} Q={Q}: block error {e:.3g} (tolerance {A.TOL[family]['o']})")
        assert e <= A.TOL[family]["o"], f"{family} {nh}/{nkv}/{hd} t0={t0} Q={Q}: block error {e}"


# ---------------------------------------------------------------------------------------------------------------------
# 3. splits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh,nkv,hd", [(8, 2, 128), (3, 3, 96), (32, 8, 128)])
def test_forced_splits_agree_and_repeat(dev, nh, nkv, hd):
    ops = _ops()
    B, t0, Q = 2, 1031 - 40, 40
    mx = ops.decode_attention_max_splits()
    assert ops.extend_attention_plan(B, nkv, t0, Q, mx)[0] > 3
    full = _masks(B, t0, Q)[0][1]
    blank = full.clone()
    c3 = ops.extend_attention_plan(B, nkv, t0, Q, 3)[1]
    blank[0, c3:2 * c3] = False                        # a whole chunk of a 3-way split
    blank[1, :t0] = False                              # every cached key of the last row
    blank[1, t0:t0 + Q // 3] = False
    for valid in (full, blank):
        outs = []
        for s in (0, 1, 2, mx):
            out, rest = _run(dev, nh, nkv, hd, B, Q, t0, valid, seed=5, splits=s)
            assert torch.isfinite(out).all(), f"splits {s}: NaN / Inf in out"
            again, rest2 = _run(dev, nh, nkv, hd, B, Q, t0, valid, seed=5, splits=s)
            assert torch.equal(again, out), f"splits {s}: a second call gave other bits"
            assert torch.equal(_bits(rest[7]), _bits(rest2[7])) and torch.equal(_bits(rest[8]), _bits(rest2[8]))
            outs.append(out)
        q, k, v, kc, vc, cos, sin = rest[:7]
        ref, _ = _reference(q, k, v, cos, sin, kc, vc, t0, Q, valid, nh, nkv, hd)
        for s, o in zip((0, 1, 2, mx), outs):
            e0, er = rel_err(o, outs[0]), rel_err(o, ref)
            print(f"{nh}/{nkv}/{hd} splits={s}: against splits=0 {e0:.3g}, against float64 {er:.3g}")
            assert e0 < TOL["bf16"] and er < TOL["bf16"], f"splits {s}"


# ---------------------------------------------------------------------------------------------------------------------
# 4. at Q <= 16 with an all-valid chunk it is cmb_decode_attn_multi's step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh,nkv,hd", GEOMS)
def test_agrees_with_decode_attention_multi(dev, nh, nkv, hd):
    ops = _ops()
    B = 2
    for Q in sorted({1, 5, min(16, 64 // (nh // nkv))}):
        for t0 in (0, 64, 300):
            valid = _masks(B, t0, Q)[1][1]             # holes in the cached part, the chunk all valid
            out, rest = _run(dev, nh, nkv, hd, B, Q, t0, valid, seed=t0 + Q, poison=True)
            old, rest_old = _run(dev, nh, nkv, hd, B, Q, t0, valid, seed=t0 + Q, poison=True, fn=ops.decode_attention_multi)
            what = f"{nh}/{nkv}/{hd} Q={Q} t0={t0}"
            assert rel_err(out, old) < TOL["bf16"], what              # bit equality is not required
            n = t0 + Q
            assert torch.equal(_bits(rest[8][:, :, t0:n]), _bits(rest_old[8][:, :, t0:n])), what      # raw v
            assert rel_err(rest[7][:, :, t0:n], rest_old[7][:, :, t0:n]) < TOL["bf16"], what
