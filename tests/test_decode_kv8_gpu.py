"""`-m gpu`: the e4m3 K / V cache of the decode steps — ``cmb_kv_quantize_e4m3`` and ``cmb_decode_attn_kv8``
(decode_attn_kv8.hip) through ``ops.kv_quantize_e4m3`` / ``ops.decode_attention_kv8``, ``cmb_decode_step_kv8`` through
``DecodeStepPlan`` and the ``generate()`` loops with ``CAMBRIAN_AMD_DECODE_KV_FP8=1``.

The quantiser is compared bit for bit with ``ops.k_quantize_fp8_rows`` (the rule it restates).  Kernel tests follow
tests/test_decode_attn_gpu.py: a float64 expression on the CPU computed from the cache AS STORED — bytes through
``torch.float8_e4m3fn`` times the stored factor, slot t as the kernel wrote it — so the only error left is the kernel's own
fp32 arithmetic and the bf16 rounding of ``out`` (``conftest.TOL["bf16"]`` through ``rel_err``).  What the e4m3 cache costs
against a bf16 cache is NOT asserted anywhere here (no bound can be derived for it); tools/bench_decode_kv8.py measures it."""
import gc
import math
import weakref

import pytest
import torch

from conftest import TOL, rel_err

pytestmark = pytest.mark.gpu

GEOMS = [(4, 2, 64), (4, 4, 64), (8, 2, 128), (7, 1, 128), (3, 3, 96), (8, 1, 128)]
LENGTHS = ["1", "2", "5", "c-1", "c", "c+1", "2*c+3", "1031", "2*m", "2*m+1"]
THETA = 10000.0
TAIL = 5          # cache slots past t: NaN bytes and NaN factors
NAN_BYTE = 0x7F
BF16_MAX = 3.3895313892515355e38


def _ops():
    from cambrian_amd import ops
    return ops


def _length(expr, B, nkv):
    ops = _ops()
    c = ops.decode_attention_plan(B, nkv, 1030)[1]
    m = 1
    while ops.decode_attention_plan(B, nkv, 2 * m - 1)[0] < 2:     # smallest m with a split at 2 * m keys
        m += 1
    return int(eval(expr, {"c": c, "m": m}))


def _masks(B, n):
    """(name, bool [B, n + TAIL]) key masks over the n cached-or-new keys; columns past n stay False."""
    full = torch.zeros(B, n + TAIL, dtype=torch.bool)
    full[:, :n] = True
    left = full.clone()
    for b in range(B):
        left[b, :min(n - 1, (3 + 7 * b) % max(n, 1))] = False          # different left padding per row
    lone = full.clone()
    lone[B - 1, :n] = False                                            # every cached key masked; slot t masked too: the
    return [("all", full), ("left", left), ("lone", lone)]             # kernel must open it by itself


def _dequant(q, inv):
    return q.view(torch.float8_e4m3fn).double() * inv.double()[..., None]


# ---------------------------------------------------------------------------------------------------------------------
# cmb_kv_quantize_e4m3
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 16])
@pytest.mark.parametrize("hd", [64, 96, 128])
def test_quantiser_equals_quantize_fp8_rows_and_touches_nothing_else(dev, hd, pad):
    ops = _ops()
    B, nkv, L, Lmax = 2, 2, 37, 42
    g = torch.Generator().manual_seed(hd + pad)
    big = (torch.randn(B, nkv, L + 7, hd, generator=g) * torch.rand(B, nkv, L + 7, 1, generator=g) * 8).to(torch.bfloat16)
    big[0, 1, 3 + 4] = 0                                               # an all-zero row (slot 4 of the slice below)
    big[1, 0, 3 + 9, ::2], big[1, 0, 3 + 9, 1::2] = BF16_MAX, -BF16_MAX  # a row of +- the largest finite bf16
    big[1, 1, 3 + 11, 5] = BF16_MAX
    src = big.to(dev)[:, :, 3:3 + L]                                   # a slice of a longer tensor: not contiguous
    assert not src.is_contiguous()
    buf = torch.full((B, nkv, Lmax, hd + pad), 0xA5, dtype=torch.uint8, device=dev)
    inv = torch.full((B, nkv, Lmax), 7.5, dtype=torch.float32, device=dev)
    cache = ops.KvCacheE4M3(buf[..., :hd], inv)
    assert cache.q.stride(2) == hd + pad
    ops.kv_quantize_e4m3(src, cache, L)
    want_q, want_inv = ops.k_quantize_fp8_rows(src.reshape(-1, hd).contiguous())
    torch.cuda.synchronize()
    assert torch.equal(buf[:, :, :L, :hd].reshape(-1, hd), want_q)
    assert torch.equal(inv[:, :, :L].reshape(-1), want_inv)
    assert float(inv[0, 1, 4]) == 1.0 and int(buf[0, 1, 4, :hd].max()) == 0                  # the zero row: factor 1, bytes 0
    assert set(buf[1, 0, 9, :hd].tolist()) == {0x7E, 0xFE}                                   # +-448, not a NaN code
    assert not ((buf[:, :, :L, :hd] & 0x7F) == 0x7F).any()
    assert bool((buf[:, :, L:] == 0xA5).all()) and bool((buf[:, :, :, hd:] == 0xA5).all())   # slots >= L and the padding
    assert bool((inv[:, :, L:] == 7.5).all())
    # a second call: the same bits
    buf2, inv2 = torch.full_like(buf, 0xA5), torch.full_like(inv, 7.5)
    ops.kv_quantize_e4m3(src, ops.KvCacheE4M3(buf2[..., :hd], inv2), L)
    assert torch.equal(buf2, buf) and torch.equal(inv2, inv)


# ---------------------------------------------------------------------------------------------------------------------
# cmb_decode_attn_kv8
# ---------------------------------------------------------------------------------------------------------------------
def _inputs(nh, nkv, hd, B, n, valid, seed):
    """bf16 q / k / v of the new token and caches of n + TAIL slots: random bytes (the NaN codes taken out at attendable
    slots only) and random positive factors at slots 0 .. n-2, NaN bytes and NaN factors at slot t = n-1 and the tail."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, nh * hd, generator=g).to(torch.bfloat16)
    k = torch.randn(B, nkv * hd, generator=g).to(torch.bfloat16)
    v = torch.randn(B, nkv * hd, generator=g).to(torch.bfloat16)
    att = valid[:, None, :, None].expand(B, nkv, n + TAIL, hd)
    caches = []
    for _ in range(2):
        by = torch.randint(0, 256, (B, nkv, n + TAIL, hd), generator=g, dtype=torch.int32).to(torch.uint8)
        nan = (by & 0x7F) == 0x7F
        by = torch.where(nan & att, by - 1, by)
        f = (0.5 + 1.5 * torch.rand(B, nkv, n + TAIL, generator=g)) / 64
        by[:, :, n - 1:] = NAN_BYTE
        f[:, :, n - 1:] = float("nan")
        caches.append((by, f))
    pos = torch.randint(0, 1100, (B, 1), generator=g)
    return q, k, v, caches[0], caches[1], pos


def _rope64(x, cos, sin, hd):
    c, s = cos.double().cpu()[:, None, :], sin.double().cpu()[:, None, :]        # [B, 1, hd/2]
    x1, x2 = x[..., :hd // 2], x[..., hd // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


def _reference(q, cos, sin, K, V, t, valid, nh, nkv, hd):
    """float64 on the CPU: K / V [B, nkv, >= t+1, hd] are the caches as stored after the step (dequantised)."""
    B = q.shape[0]
    G = nh // nkv
    qr = _rope64(q.double().view(B, nh, hd), cos, sin, hd)
    m = valid[:, :t + 1].clone()
    m[:, t] = True
    keep = m[:, None, :, None]
    K = torch.where(keep, K[:, :, :t + 1], torch.zeros((), dtype=torch.float64))    # a slot that is not attendable may hold NaN
    V = torch.where(keep, V[:, :, :t + 1], torch.zeros((), dtype=torch.float64))
    head = torch.arange(nh) // G
    sc = torch.einsum("bhd,bhjd->bhj", qr, K[:, head]) / math.sqrt(hd)
    sc = sc.masked_fill(~m[:, None, :], float("-inf"))
    return torch.einsum("bhj,bhjd->bhd", torch.softmax(sc, -1), V[:, head]).reshape(B, nh * hd)


def _run(dev, nh, nkv, hd, B, n, valid, seed=0, splits=0):
    ops = _ops()
    q, k, v, (kq, ki), (vq, vi), pos = _inputs(nh, nkv, hd, B, n, valid, seed)
    cos, sin = ops.rope_table(pos.to(dev), hd, THETA)
    kc = ops.KvCacheE4M3(kq.to(dev), ki.to(dev))
    vc = ops.KvCacheE4M3(vq.to(dev), vi.to(dev))
    out = ops.decode_attention_kv8(q.to(dev), k.to(dev), v.to(dev), cos, sin, kc, vc, n - 1, valid.to(dev), splits=splits)
    torch.cuda.synchronize()
    ref = _reference(q, cos, sin, _dequant(kc.q.cpu(), kc.inv.cpu()), _dequant(vc.q.cpu(), vc.inv.cpu()), n - 1, valid, nh, nkv, hd)
    return out, ref, dict(q=q, k=k, v=v, kq=kq, ki=ki, vq=vq, vi=vi, cos=cos, sin=sin, kc=kc, vc=vc)


def _same(a, b):
    """bit equality of two tensors that may hold NaN"""
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _untouched_but_slot_t(x, t):
    keep = torch.ones(x["kq"].shape[2], dtype=torch.bool)
    keep[t] = False
    return all(_same(x[c].q.cpu()[:, :, keep], x[q][:, :, keep]) and _same(x[c].inv.cpu()[:, :, keep], x[i][:, :, keep])
               for c, q, i in (("kc", "kq", "ki"), ("vc", "vq", "vi")))


@pytest.mark.parametrize("expr", LENGTHS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nh,nkv,hd", GEOMS)
def test_kernel_parity(dev, nh, nkv, hd, B, expr):
    n = _length(expr, B, nkv)
    t = n - 1
    for mname, valid in _masks(B, n):
        out, ref, x = _run(dev, nh, nkv, hd, B, n, valid, seed=n)
        e = rel_err(out, ref)
        print(f"{nh}/{nkv}/{hd} B={B} n={n} mask={mname}: out rel err {e:.3g}")
        assert out.dtype == torch.bfloat16 and torch.isfinite(out).all()
        assert e < TOL["bf16"], f"mask {mname}: out rel err {e}"
        assert torch.isfinite(x["kc"].inv[:, :, t]).all() and torch.isfinite(x["vc"].inv[:, :, t]).all()
        assert not ((x["kc"].q[:, :, t] & 0x7F) == 0x7F).any() and not ((x["vc"].q[:, :, t] & 0x7F) == 0x7F).any()
        assert _untouched_but_slot_t(x, t)


@pytest.mark.parametrize("nh,nkv,hd", GEOMS)
def test_slot_t_is_quantised_by_the_rule(dev, nh, nkv, hd):
    ops = _ops()
    B, n = 3, 300
    t = n - 1
    valid = _masks(B, n)[1][1]
    out, ref, x = _run(dev, nh, nkv, hd, B, n, valid, seed=17)
    # V: the raw rows through the quantiser, bit for bit
    want_q, want_inv = ops.k_quantize_fp8_rows(x["v"].to(dev).view(B * nkv, hd))
    assert torch.equal(x["vc"].q[:, :, t].reshape(B * nkv, hd), want_q)
    assert torch.equal(x["vc"].inv[:, :, t].reshape(-1), want_inv)
    # the same bytes as the prefill's quantiser gives for the same bf16 values
    pre = ops.KvCacheE4M3.empty(B, nkv, 1, hd, dev)
    ops.kv_quantize_e4m3(x["v"].to(dev).view(B, nkv, 1, hd), pre, 1)
    assert torch.equal(pre.q[:, :, 0], x["vc"].q[:, :, t]) and torch.equal(pre.inv[:, :, 0], x["vc"].inv[:, :, t])
    roped = ops.rope(x["k"].to(dev).view(B, nkv, hd), x["cos"], x["sin"])                    # bf16, as a bf16 cache holds it
    ops.kv_quantize_e4m3(roped.view(B, nkv, 1, hd), pre, 1)
    same = (pre.q[:, :, 0] == x["kc"].q[:, :, t]).float().mean().item()
    print(f"{nh}/{nkv}/{hd}: K bytes equal to the quantiser's on ops.rope's bf16 row: {same:.4f}")
    # K: the dequantised entry against the float64 roped k, element by element
    xr = _rope64(x["k"].double().view(B, nkv, hd), x["cos"], x["sin"], hd)
    inv = x["kc"].inv[:, :, t].cpu().double()
    d = x["kc"].q[:, :, t].cpu().view(torch.float8_e4m3fn).double() * inv[..., None]
    bound = xr.abs() * (2.0 ** -4 + 2.0 ** -7) + inv[..., None] * 2.0 ** -10
    worst = ((d - xr).abs() / bound).max().item()
    print(f"{nh}/{nkv}/{hd}: K slot t |d - x| / bound, worst {worst:.3f}")
    assert worst <= 1.0
    amax = xr.abs().amax(-1) / 448.0
    assert bool(((inv - amax).abs() <= amax * 2.0 ** -7).all()), "K factor further than a bf16 step from max|x| / 448"
    assert _untouched_but_slot_t(x, t)


# beside the parity geometries: every (lanes per row, heads per KV head) shape the kernel has an instantiation for at hd 96 / 64
@pytest.mark.parametrize("nh,nkv,hd", [(8, 2, 128), (3, 3, 96), (4, 2, 64), (8, 1, 96), (8, 1, 64), (4, 1, 96), (4, 1, 64)])
def test_forced_splits_agree_and_the_same_call_gives_the_same_bits(dev, nh, nkv, hd):
    ops = _ops()
    B, n = 2, 1031
    valid = _masks(B, n)[1][1]
    outs = []
    for s in (1, 2, 7, 0):
        out, ref, x = _run(dev, nh, nkv, hd, B, n, valid, seed=5, splits=s)
        assert torch.isfinite(out).all(), f"splits {s}: NaN / Inf in out"
        e = rel_err(out, ref)
        print(f"{nh}/{nkv}/{hd} splits={s}: out rel err {e:.3g}")
        assert e < TOL["bf16"], f"splits {s}: out rel err {e}"
        outs.append((out, x))
    for o, _ in outs[1:]:
        assert rel_err(o, outs[0][0]) < TOL["bf16"]
    assert ops.decode_attention_plan(B, nkv, n - 1)[0] > 1
    again, _, x2 = _run(dev, nh, nkv, hd, B, n, valid, seed=5, splits=0)
    out, x = outs[-1]
    assert torch.equal(again, out)
    for c in ("kc", "vc"):
        assert _same(x2[c].q, x[c].q) and _same(x2[c].inv, x[c].inv)


def test_packed_row_views_and_refusals(dev):
    ops = _ops()
    from cambrian_amd.lib import CambrianAmdError
    nh, nkv, hd, B, n = 8, 2, 128, 3, 300
    valid = _masks(B, n)[1][1]
    q, k, v, (kq, ki), (vq, vi), pos = _inputs(nh, nkv, hd, B, n, valid, 3)
    cos, sin = ops.rope_table(pos.to(dev), hd, THETA)
    row = torch.cat([q, k, v], 1).to(dev)
    nq, nk = nh * hd, nkv * hd
    c1 = [ops.KvCacheE4M3(a.to(dev), b.to(dev)) for a, b in ((kq, ki), (vq, vi))]
    c2 = [ops.KvCacheE4M3(a.to(dev), b.to(dev)) for a, b in ((kq, ki), (vq, vi))]
    a = ops.decode_attention_kv8(row[:, :nq], row[:, nq:nq + nk], row[:, nq + nk:], cos, sin, *c1, n - 1, valid.to(dev))
    b = ops.decode_attention_any(q.to(dev), k.to(dev), v.to(dev), cos, sin, *c2, n - 1, valid.to(dev))
    assert torch.equal(a, b) and all(_same(x.q, y.q) and _same(x.inv, y.inv) for x, y in zip(c1, c2))
    with pytest.raises(CambrianAmdError, match="unsupported geometry"):                     # fp32 activations
        ops.decode_attention_kv8(q.float().to(dev), k.float().to(dev), v.float().to(dev), cos, sin, *c1, n - 1, valid.to(dev))
    with pytest.raises(CambrianAmdError, match="no backward"):
        ops.decode_attention_kv8(q.to(dev).requires_grad_(), k.to(dev), v.to(dev), cos, sin, *c1, n - 1, valid.to(dev))


# ---------------------------------------------------------------------------------------------------------------------
# the decode step and generate() on a tiny frozen bf16 model
# ---------------------------------------------------------------------------------------------------------------------
def _lm(dev, lm="llama", hidden=256, heads=4):
    from cambrian_amd.model.language_model import cambrian_llama as CL
    geo = dict(vocab_size=512, hidden_size=hidden, intermediate_size=512, num_hidden_layers=2, num_attention_heads=heads,
               num_key_value_heads=2, rms_norm_eps=1e-5, max_position_embeddings=512)
    if lm == "phi3":
        from cambrian_amd.model.language_model import cambrian_phi3 as CP
        cfg = CP.CambrianConfig(rope_theta=10000.0, pad_token_id=0, sliding_window=None, **geo)
        cls = CP.CambrianPhi3ForCausalLM
    else:
        cfg = CL.CambrianConfig(rope_theta=500000.0, **geo)
        cls = CL.CambrianLlamaForCausalLM
    torch.manual_seed(3)
    model = cls(cfg, device=dev, llm_dtype=torch.bfloat16)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    model.requires_grad_(False)
    return model.eval()


def _prompt(dev, B=3, L=9):
    g = torch.Generator().manual_seed(B)
    ids = torch.randint(1, 512, (B, L), generator=g).to(dev)
    att = torch.ones(B, L, dtype=torch.long)
    for b in range(1, B):
        att[b, :(2 * b) % (L - 2)] = 0              # left padding: rows of different lengths
    return ids, att.to(dev)


ENV = ("CAMBRIAN_AMD_DECODE_STEP", "CAMBRIAN_AMD_DECODE_FP8", "CAMBRIAN_AMD_DECODE_FP4", "CAMBRIAN_AMD_DECODE_LINEAR",
       "CAMBRIAN_AMD_DECODE_ATTN", "CAMBRIAN_AMD_DECODE_KV_FP8", "CAMBRIAN_AMD_DECODE_SAMPLE", "CAMBRIAN_AMD_DECODE_BEAM")


@pytest.fixture()
def clean_env(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


class _Spy:
    """Counts the calls that tell the two cache formats and the two loops apart, keeps the last decode-step logits, the
    caches every plan was built on and weak references to the prefill tensors that went through the quantiser."""

    def __init__(self, monkeypatch):
        from cambrian_amd.model.language_model import cambrian_llama as CL
        ops = _ops()
        self.n = {"kv8": 0, "bf16": 0, "quant": 0, "step": 0, "beam": 0}
        self.last = None
        self.plan_caches = []
        self.prefill = []
        spy = self

        def wrap(mod, name, key, keep_last=False, before=None):
            real = getattr(mod, name)

            def counted(*a, **kw):
                if key:
                    spy.n[key] += 1
                if before:
                    before(*a, **kw)
                r = real(*a, **kw)
                if keep_last:
                    spy.last = r.clone()
                return r

            monkeypatch.setattr(mod, name, counted)

        wrap(ops, "decode_attention_kv8", "kv8")
        wrap(ops, "decode_attention", "bf16")
        wrap(ops, "kv_quantize_e4m3", "quant", before=lambda src, *a, **kw: spy.prefill.append(weakref.ref(src)))
        wrap(ops, "decode_step", "step", keep_last=True)
        wrap(ops, "decode_beam", "beam")
        wrap(CL, "_decode_logits", None, keep_last=True)
        real_build = CL.DecodeStepPlan.build.__func__

        def build(cls, lm, B, caches, *a, **kw):
            spy.plan_caches.append(caches)
            return real_build(cls, lm, B, caches, *a, **kw)

        monkeypatch.setattr(CL.DecodeStepPlan, "build", classmethod(build))

    def reset(self):
        for k in self.n:
            self.n[k] = 0
        self.last, self.plan_caches, self.prefill = None, [], []


def _generate(model, env, spy, ids, att, step, kv8, **kw):
    env.setenv("CAMBRIAN_AMD_DECODE_STEP", step)
    env.setenv("CAMBRIAN_AMD_DECODE_KV_FP8", kv8)
    spy.reset()
    toks = model.generate(ids, attention_mask=att, **kw)
    torch.cuda.synchronize()
    return toks, dict(spy.n), spy.last


NEW = 6


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
@pytest.mark.parametrize("weights", ["bf16", "fp8", "fp4"])
def test_generate_loop_equals_step_on_e4m3_caches(dev, clean_env, weights, mode):
    model = _lm(dev)
    layers = len(model.model.layers)
    if weights != "bf16":
        clean_env.setenv("CAMBRIAN_AMD_DECODE_" + weights.upper(), "1")
    spy = _Spy(clean_env)
    ids, att = _prompt(dev)
    kw = dict(max_new_tokens=NEW)
    if mode == "sampled":
        kw.update(do_sample=True, temperature=0.8, top_k=20, top_p=0.9)      # torch's warpers: device-side sampling stays off
    torch.manual_seed(123)
    loop, n_loop, logits_loop = _generate(model, clean_env, spy, ids, att, "0", "1", **kw)
    assert loop.shape == (3, NEW)
    assert n_loop["quant"] == 2 * layers and n_loop["kv8"] == (NEW - 1) * layers and n_loop["bf16"] == 0 and n_loop["step"] == 0, n_loop
    gc.collect()
    assert spy.prefill and all(r() is None for r in spy.prefill), "a bf16 prefill K / V tensor outlived the call"
    torch.manual_seed(123)
    step, n_step, logits_step = _generate(model, clean_env, spy, ids, att, "1", "1", **kw)
    assert n_step["step"] == NEW - 1 and n_step["kv8"] == 0 and n_step["bf16"] == 0 and n_step["quant"] == 2 * layers, n_step
    assert len(spy.plan_caches) == 1 and all(k.q.dtype == v.q.dtype == torch.uint8 and k.inv.dtype == torch.float32
                                             for k, v in spy.plan_caches[0])
    assert torch.equal(step, loop), (step.tolist(), loop.tolist())
    assert logits_loop.shape == logits_step.shape == (3, 512) and torch.equal(logits_loop, logits_step)
    assert len(set(loop[0].tolist())) > 1, "a constant sequence would not show a wrong step"


def test_generate_switch_off_is_the_bf16_cache_path(dev, clean_env):
    """Off (unset, "0", or the config flag absent) nothing of the e4m3 path runs and the tokens are those of the bf16
    cache; the config flag switches it on and the environment overrides the flag."""
    model = _lm(dev)
    layers = len(model.model.layers)
    spy = _Spy(clean_env)
    ids, att = _prompt(dev)
    for step in ("0", "1"):
        clean_env.setenv("CAMBRIAN_AMD_DECODE_STEP", step)
        clean_env.delenv("CAMBRIAN_AMD_DECODE_KV_FP8", raising=False)
        spy.reset()
        unset = model.generate(ids, attention_mask=att, max_new_tokens=NEW)
        assert spy.n["quant"] == 0 and spy.n["kv8"] == 0
        assert all(k.dtype == v.dtype == torch.bfloat16 for c in spy.plan_caches for k, v in c)
        off, n_off, _ = _generate(model, clean_env, spy, ids, att, step, "0", max_new_tokens=NEW)
        assert torch.equal(off, unset) and n_off["quant"] == 0 and n_off["kv8"] == 0
        assert n_off["bf16"] == (0 if step == "1" else (NEW - 1) * layers)
        model.config.decode_kv_fp8 = True
        assert torch.equal(_generate(model, clean_env, spy, ids, att, step, "0", max_new_tokens=NEW)[0], off)
        assert spy.n["quant"] == 0
        _, n_on, _ = _generate(model, clean_env, spy, ids, att, step, "", max_new_tokens=NEW)       # "" = unset: the flag decides
        assert n_on["quant"] == 2 * layers and n_on["bf16"] == 0
        del model.config.decode_kv_fp8


def test_generate_beam_search_on_e4m3_caches(dev, clean_env):
    model = _lm(dev)
    layers = len(model.model.layers)
    clean_env.setenv("CAMBRIAN_AMD_DECODE_BEAM", "1")
    spy = _Spy(clean_env)
    ids, att = _prompt(dev)
    kw = dict(max_new_tokens=NEW, num_beams=2)
    loop, n_loop, _ = _generate(model, clean_env, spy, ids, att, "0", "1", **kw)
    assert n_loop["quant"] == 2 * layers and n_loop["kv8"] > 0 and n_loop["bf16"] == 0 and n_loop["beam"] == 0, n_loop
    step, n_step, _ = _generate(model, clean_env, spy, ids, att, "1", "1", **kw)
    assert n_step["step"] > 0 and n_step["beam"] == 0 and n_step["kv8"] == 0 and n_step["bf16"] == 0, n_step   # _beam_fused is not taken
    assert spy.plan_caches and all(k.q.dtype == torch.uint8 and k.q.shape[0] == 6 for k, v in spy.plan_caches[0])
    assert torch.equal(step, loop), (step.tolist(), loop.tolist())
    # with the switch off the fused beam loop is still what runs
    _, n_off, _ = _generate(model, clean_env, spy, ids, att, "1", "0", **kw)
    assert n_off["beam"] > 0 and n_off["quant"] == 0


def test_generate_phi3_loop_equals_step(dev, clean_env):
    model = _lm(dev, "phi3")
    spy = _Spy(clean_env)
    ids, att = _prompt(dev)
    loop, n_loop, logits_loop = _generate(model, clean_env, spy, ids, att, "0", "1", max_new_tokens=NEW)
    step, n_step, logits_step = _generate(model, clean_env, spy, ids, att, "1", "1", max_new_tokens=NEW)
    assert n_loop["kv8"] == (NEW - 1) * 2 and n_loop["bf16"] == 0 and n_step["step"] == NEW - 1 and n_step["kv8"] == 0
    assert torch.equal(step, loop) and torch.equal(logits_loop, logits_step)


def test_generate_unsupported_head_dim_keeps_bf16_caches(dev, clean_env):
    model = _lm(dev, hidden=320)                       # 4 heads of 80: outside the kernel's geometries
    assert model.model.layers[0].self_attn.hd == 80
    spy = _Spy(clean_env)
    ids, att = _prompt(dev)
    off, n_off, _ = _generate(model, clean_env, spy, ids, att, "0", "0", max_new_tokens=NEW)
    on, n_on, _ = _generate(model, clean_env, spy, ids, att, "0", "1", max_new_tokens=NEW)
    assert n_on["quant"] == 0 and n_on["kv8"] == 0 and n_on == n_off
    assert torch.equal(on, off)
