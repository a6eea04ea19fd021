"""`-m gpu`: the fused decode step of generate() — ``cmb_decode_attn`` (decode_attn.hip) through ``ops.decode_attention``,
the two attention modules' ``decode`` and the generate loop.

Kernel tests compare with a plain torch expression on the CPU in float64 (rotate-half RoPE, masked softmax, grouped KV heads
by indexing), computed from the inputs AS STORED: bf16 tensors are rounded first, and the RoPE tables are the fp32 tables of
``ops.rope_table`` at the same positions — they are arguments of the kernel (an angle of ~1000 rad carries 3e-5 of fp32
rounding whoever computes it; that belongs to the table's own test, tests/test_kernels_gpu.py::test_rope).
Tolerances: ``conftest.TOL`` through ``rel_err`` (fp32 2e-5, bf16 2e-2)."""
import math

import pytest
import torch

from conftest import TOL, rel_err

pytestmark = pytest.mark.gpu

DTYPES = [("fp32", torch.float32), ("bf16", torch.bfloat16)]
GEOMS = [(4, 2, 64), (4, 4, 64), (8, 2, 128), (7, 1, 128), (3, 3, 96)]
# cache lengths t + 1; "c" is the chunk length of the library's plan for 1031 keys (resolved on the GPU box).  The last two
# are the shortest lengths the library itself splits (two chunks, the second one full / one key short).
LENGTHS = ["1", "2", "5", "c-1", "c", "c+1", "2*c+3", "1031", "2*m", "2*m+1"]
THETA = 10000.0
TAIL = 5          # cache slots past t, filled with garbage


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


def _inputs(dt, nh, nkv, hd, B, n, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, nh * hd, generator=g).to(dt)
    k = torch.randn(B, nkv * hd, generator=g).to(dt)
    v = torch.randn(B, nkv * hd, generator=g).to(dt)
    kc = torch.randn(B, nkv, n + TAIL, hd, generator=g).to(dt)
    vc = torch.randn(B, nkv, n + TAIL, hd, generator=g).to(dt)
    kc[:, :, n - 1:], vc[:, :, n - 1:] = 3.0e4, -3.0e4              # slot t (overwritten) and the tail (never read)
    pos = torch.randint(0, 1100, (B, 1), generator=g)
    return q, k, v, kc, vc, pos


def _reference(q, k, v, cos, sin, kc, vc, t, valid, nh, nkv, hd):
    """float64 on the CPU -> (out [B, nh*hd], roped new k [B, nkv, hd])."""
    B = q.shape[0]
    G = nh // nkv
    c, s = cos.double().cpu()[:, None, :], sin.double().cpu()[:, None, :]        # [B, 1, hd/2]

    def rot(x):
        x1, x2 = x[..., :hd // 2], x[..., hd // 2:]
        return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)

    qr = rot(q.double().view(B, nh, hd))
    kr = rot(k.double().view(B, nkv, hd))
    K = kc.double()[:, :, :t + 1].clone()
    V = vc.double()[:, :, :t + 1].clone()
    K[:, :, t], V[:, :, t] = kr.to(q.dtype).double(), v.double().view(B, nkv, hd)  # what the cache holds after the step
    head = torch.arange(nh) // G
    sc = torch.einsum("bhd,bhjd->bhj", qr, K[:, head]) / math.sqrt(hd)
    m = valid[:, :t + 1].clone()
    m[:, t] = True
    sc = sc.masked_fill(~m[:, None, :], float("-inf"))
    out = torch.einsum("bhj,bhjd->bhd", torch.softmax(sc, -1), V[:, head])
    return out.reshape(B, nh * hd), kr


def _run(dev, dt, nh, nkv, hd, B, n, valid, seed=0, splits=0):
    ops = _ops()
    q, k, v, kc, vc, pos = _inputs(dt, nh, nkv, hd, B, n, seed)
    cos, sin = ops.rope_table(pos.to(dev), hd, THETA)
    kcd, vcd = kc.to(dev), vc.to(dev)
    out = ops.decode_attention(q.to(dev), k.to(dev), v.to(dev), cos, sin, kcd, vcd, n - 1, valid.to(dev), splits=splits)
    ref, kr = _reference(q, k, v, cos, sin, kc, vc, n - 1, valid, nh, nkv, hd)
    return out, ref, (q, k, v, kc, vc, cos, sin, kcd, vcd, kr)


@pytest.mark.parametrize("expr", LENGTHS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nh,nkv,hd", GEOMS)
@pytest.mark.parametrize("name,dt", DTYPES)
def test_kernel_parity(dev, name, dt, nh, nkv, hd, B, expr):
    ops = _ops()
    n = _length(expr, B, nkv)
    t = n - 1
    for mname, valid in _masks(B, n):
        out, ref, (q, k, v, kc, vc, cos, sin, kcd, vcd, kr) = _run(dev, dt, nh, nkv, hd, B, n, valid, seed=n)
        e = rel_err(out, ref)
        print(f"{name} {nh}/{nkv}/{hd} B={B} n={n} mask={mname}: out rel err {e:.3g}")
        assert torch.isfinite(out).all()
        assert e < TOL[name], f"mask {mname}: out rel err {e}"
        assert torch.equal(vcd[:, :, t].cpu(), v.view(B, nkv, hd))                       # raw v, bit for bit
        roped = ops.rope(k.to(dev).view(B, nkv, hd), cos, sin)
        assert rel_err(kcd[:, :, t], roped) < TOL[name] and rel_err(kcd[:, :, t], kr) < TOL[name]
        keep = torch.ones(n + TAIL, dtype=torch.bool)
        keep[t] = False
        assert torch.equal(kcd.cpu()[:, :, keep], kc[:, :, keep]) and torch.equal(vcd.cpu()[:, :, keep], vc[:, :, keep])


@pytest.mark.parametrize("nh,nkv,hd", [(8, 2, 128), (3, 3, 96)])
@pytest.mark.parametrize("name,dt", DTYPES)
def test_forced_splits_agree(dev, name, dt, nh, nkv, hd):
    ops = _ops()
    B, n = 2, 1031
    mx = ops.decode_attention_max_splits()
    assert ops.decode_attention_plan(B, nkv, n - 1, mx)[0] > 3
    blank = torch.zeros(B, n + TAIL, dtype=torch.bool)
    blank[:, :n] = True
    c3 = ops.decode_attention_plan(B, nkv, n - 1, 3)[1]
    blank[0, c3:2 * c3] = False                        # the whole middle chunk of the 3-way split (and chunks of the finer ones)
    blank[1, :n - 1] = False                           # every chunk but the last is empty
    full = torch.zeros_like(blank)
    full[:, :n] = True
    for valid in (full, blank):
        outs = []
        for s in (1, 2, 3, mx):
            out, ref, _ = _run(dev, dt, nh, nkv, hd, B, n, valid, seed=5, splits=s)
            assert torch.isfinite(out).all(), f"splits {s}: NaN / Inf in out"
            e = rel_err(out, ref)
            print(f"{name} {nh}/{nkv}/{hd} splits={s}: out rel err {e:.3g}")
            assert e < TOL[name], f"splits {s}: out rel err {e}"
            outs.append(out)
        for o in outs[1:]:
            assert rel_err(o, outs[0]) < (1e-5 if name == "fp32" else 2e-2)


@pytest.mark.parametrize("name,dt", DTYPES)
def test_same_call_same_bits(dev, name, dt):
    valid = _masks(3, 1031)[1][1]
    a, _, _ = _run(dev, dt, 8, 2, 128, 3, 1031, valid, seed=9)
    b, _, _ = _run(dev, dt, 8, 2, 128, 3, 1031, valid, seed=9)
    assert _ops().decode_attention_plan(3, 2, 1030)[0] > 1
    assert torch.equal(a, b)


@pytest.mark.parametrize("name,dt", DTYPES)
def test_packed_row_views_equal_separate_tensors(dev, name, dt):
    ops = _ops()
    nh, nkv, hd, B, n = 8, 2, 128, 3, 300
    q, k, v, kc, vc, pos = _inputs(dt, nh, nkv, hd, B, n, 3)
    cos, sin = ops.rope_table(pos.to(dev), hd, THETA)
    valid = _masks(B, n)[1][1].to(dev)
    row = torch.cat([q, k, v], 1).to(dev)
    nq, nk = nh * hd, nkv * hd
    kc1, vc1, kc2, vc2 = kc.to(dev), vc.to(dev), kc.to(dev), vc.to(dev)
    a = ops.decode_attention(row[:, :nq], row[:, nq:nq + nk], row[:, nq + nk:], cos, sin, kc1, vc1, n - 1, valid)
    b = ops.decode_attention(q.to(dev), k.to(dev), v.to(dev), cos, sin, kc2, vc2, n - 1, valid)
    assert torch.equal(a, b) and torch.equal(kc1, kc2) and torch.equal(vc1, vc2)


def _layer(dev, dt, lm, hidden, nh, nkv, frozen=False):
    from cambrian_amd.model.language_model import cambrian_llama as CL, cambrian_phi3 as CP
    mod = CP if lm == "phi3" else CL
    cfg = mod.CambrianConfig(vocab_size=64, hidden_size=hidden, intermediate_size=2 * hidden, num_hidden_layers=1,
                             num_attention_heads=nh, num_key_value_heads=nkv, rms_norm_eps=1e-5, rope_theta=THETA,
                             max_position_embeddings=256)
    torch.manual_seed(1)
    cls = CP.Phi3DecoderLayer if lm == "phi3" else CL.LlamaDecoderLayer
    layer = cls(cfg, dev, dt)
    with torch.no_grad():
        for p in layer.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return layer.requires_grad_(not frozen)


def _decode_ab(dev, dt, layer, hidden, nkv, hd, monkeypatch, counter=None):
    """layer.decode with the kernel and with CAMBRIAN_AMD_DECODE_ATTN=0 from identical caches -> two (y, kcache, vcache)."""
    ops = _ops()
    B, n = 3, 37
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, 1, hidden, generator=g).to(dt).to(dev)
    kc = torch.randn(B, nkv, n + TAIL, hd, generator=g).to(dt).to(dev)
    vc = torch.randn(B, nkv, n + TAIL, hd, generator=g).to(dt).to(dev)
    mask = _masks(B, n)[1][1].to(dev)
    cos, sin = ops.rope_table(torch.tensor([[36], [30], [21]], device=dev), hd, THETA)
    res = []
    for env in ("1", "0"):
        monkeypatch.setenv("CAMBRIAN_AMD_DECODE_ATTN", env)
        k1, v1 = kc.clone(), vc.clone()
        before = None if counter is None else counter[0]
        with torch.no_grad():
            y = layer.decode(x, cos, sin, k1, v1, n - 1, mask)
        res.append((y, k1, v1, None if counter is None else counter[0] - before))
    return res, n - 1


@pytest.mark.parametrize("hidden,nh,nkv", [(256, 4, 4), (256, 4, 2), (512, 4, 1)])
@pytest.mark.parametrize("lm", ["llama", "phi3", "llama-frozen"])
@pytest.mark.parametrize("name,dt", DTYPES)
def test_layer_decode_kernel_vs_sdpa_branch(dev, monkeypatch, name, dt, lm, hidden, nh, nkv):
    """``llama-frozen``: the kernel arm projects with the packed [q; k; v] weight and the SDPA arm with three GEMMs, so the
    new v may differ in its last bits there — by the BLAS, not the kernel, whose store of v is checked bit for bit in
    test_kernel_parity; the other two feed both arms the same projections and the V slot is exact."""
    hd = hidden // nh
    assert _ops().decode_attention_supported(dt, nh, nkv, hd)
    frozen = lm == "llama-frozen"
    layer = _layer(dev, dt, lm.split("-")[0], hidden, nh, nkv, frozen)
    ((y1, k1, v1, _), (y0, k0, v0, _)), t = _decode_ab(dev, dt, layer, hidden, nkv, hd, monkeypatch)
    assert y1.shape == y0.shape == (3, 1, hidden)
    e = rel_err(y1, y0)
    print(f"{name} {lm} {hidden}/{nh}/{nkv}: layer out rel err {e:.3g}")
    assert e < TOL[name]
    keep = torch.ones(k1.shape[2], dtype=torch.bool)
    keep[t] = False
    assert torch.equal(v1[:, :, keep], v0[:, :, keep]) and torch.equal(k1[:, :, keep], k0[:, :, keep])
    assert rel_err(v1[:, :, t], v0[:, :, t]) < TOL[name] if frozen else torch.equal(v1[:, :, t], v0[:, :, t])
    assert rel_err(k1[:, :, t], k0[:, :, t]) < TOL[name]


@pytest.mark.parametrize("hidden,nh,nkv", [(128, 4, 2), (1024, 16, 1)])      # head_dim 32; 16 query heads per KV head
def test_unsupported_geometry_keeps_the_sdpa_branch(dev, monkeypatch, hidden, nh, nkv):
    import torch.nn.functional as F
    ops = _ops()
    hd = hidden // nh
    assert not ops.decode_attention_supported(torch.float32, nh, nkv, hd)
    calls = [0]
    real = F.scaled_dot_product_attention

    def counted(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)

    monkeypatch.setattr(F, "scaled_dot_product_attention", counted)
    layer = _layer(dev, torch.float32, "llama", hidden, nh, nkv)
    ((y1, k1, v1, n1), (y0, k0, v0, n0)), t = _decode_ab(dev, torch.float32, layer, hidden, nkv, hd, monkeypatch, calls)
    assert n1 == n0 == 1                                    # both runs went through SDPA
    assert torch.equal(y1, y0) and torch.equal(k1, k0) and torch.equal(v1, v0)
    assert torch.isfinite(y1).all()


def test_generate_decodes_on_the_kernel(dev, monkeypatch):
    """The loop really uses it: SDPA runs once per decoder layer (the prefill) and not in the decode steps; with the switch
    at 0 the decode steps call it again; the greedy tokens of the two paths are equal in fp32."""
    import torch.nn.functional as F
    from test_dynamic_gpu import _eval_batch
    from test_model_gpu import _build
    calls = [0]
    real = F.scaled_dot_product_attention

    def counted(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)

    monkeypatch.setattr(F, "scaled_dot_product_attention", counted)
    toks = {}
    for name, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        model, cfg, towers = _build(dev, dt, monkeypatch, lm="llama", nkv=2)
        model.eval()
        layers = cfg.num_hidden_layers
        ids, att, sizes, images = _eval_batch(dev, dt, towers)
        ids, sizes, images = ids[:1], sizes[1:2], [i[1:2] for i in images]
        kw = dict(images=[i.to(dev, dt) for i in images], image_sizes=sizes, max_new_tokens=4)
        for env, want in (("1", layers), ("0", layers + 3 * layers)):
            monkeypatch.setenv("CAMBRIAN_AMD_DECODE_ATTN", env)
            calls[0] = 0
            toks[name, env] = model.generate(ids.to(dev), **kw)
            assert toks[name, env].shape == (1, 4)
            assert calls[0] == want, f"{name} CAMBRIAN_AMD_DECODE_ATTN={env}: {calls[0]} SDPA calls, expected {want}"
    assert torch.equal(toks["fp32", "1"], toks["fp32", "0"])


def test_requires_grad_inputs_raise(dev):
    ops = _ops()
    from cambrian_amd.lib import CambrianAmdError
    q, k, v, kc, vc, pos = _inputs(torch.float32, 4, 2, 64, 1, 4, 0)
    cos, sin = ops.rope_table(pos.to(dev), 64, THETA)
    valid = torch.ones(1, 4 + TAIL, dtype=torch.bool, device=dev)
    with pytest.raises(CambrianAmdError, match="no backward"):
        ops.decode_attention(q.to(dev).requires_grad_(), k.to(dev), v.to(dev), cos, sin, kc.to(dev), vc.to(dev), 3, valid)


# ------------------------------------------------------------------------------------------------
# the host path that decode_attention, decode_attention_kv8 and decode_attention_multi share: message texts and the workspace
# ------------------------------------------------------------------------------------------------
ENTRIES = ["decode_attention", "decode_attention_kv8", "decode_attention_multi"]


def _entry_case(dev, entry):
    """(call(**overrides) -> out, the call's arguments by name, its workspace need at a forced split in two) on B 1, 4 / 2 heads
    of 64, 8 cache slots, bf16; ``decode_attention_multi`` with Q = 2 rows."""
    ops = _ops()
    B, nh, nkv, hd, Lmax = 1, 4, 2, 64, 8
    Q = 2 if entry == "decode_attention_multi" else 1
    g = torch.Generator().manual_seed(11)
    a = dict(q=torch.randn(B * Q, nh * hd, generator=g).bfloat16().to(dev),
             k=torch.randn(B * Q, nkv * hd, generator=g).bfloat16().to(dev),
             v=torch.randn(B * Q, nkv * hd, generator=g).bfloat16().to(dev), t=5,
             key_valid=torch.ones(B, Lmax, dtype=torch.bool, device=dev), splits=2)
    a["cos"], a["sin"] = ops.rope_table(torch.arange(5, 5 + Q, device=dev).view(B * Q, 1), hd, THETA)
    kc, vc = (torch.randn(B, nkv, Lmax, hd, generator=g).bfloat16().to(dev) for _ in range(2))
    if entry == "decode_attention_kv8":
        kc, vc = (ops.kv_quantize_e4m3(c, ops.KvCacheE4M3.empty(B, nkv, Lmax, hd, dev)) for c in (kc, vc))
    a["kc"], a["vc"] = kc, vc
    fn = getattr(ops, entry)

    def call(**kw):
        x = dict(a, **kw)
        return fn(x["q"], x["k"], x["v"], x["cos"], x["sin"], x["kc"], x["vc"], x["t"], x["key_valid"], splits=x["splits"])

    lib = ops.L.load()
    need = lib.cmb_decode_attn_multi_ws(B, nh, nkv, hd, Q, 5, 2) if Q > 1 else lib.cmb_decode_attn_ws(B, nh, nkv, hd, 5, 2)
    assert need == B * Q * nh * 2 * (hd + 2)
    return call, a, need


@pytest.mark.parametrize("entry", ENTRIES)
def test_validation_messages_of_the_three_entry_points(dev, entry):
    """One input per message, the literal texts: they name the public function, and ``decode_attention_kv8`` words two of
    them in its own way."""
    import re
    from cambrian_amd.lib import CambrianAmdError
    call, a, _ = _entry_case(dev, entry)
    multi, kv8 = entry == "decode_attention_multi", entry == "decode_attention_kv8"
    rows = 2 if multi else 1

    def raises(text, **kw):
        with pytest.raises(CambrianAmdError, match="^" + re.escape(text) + "$"):
            call(**kw)

    wide = torch.zeros(rows, 2 * 256, dtype=torch.bfloat16, device=dev)
    if kv8:
        raises("decode_attention_kv8: unsupported geometry q (1, 320) torch.bfloat16 k (1, 128) cache (1, 2, 8, 64)", q=wide[:, :320])
        raises("decode_attention_kv8: rows of q / k / v and the key mask must be contiguous, and the two caches of one layout",
               q=wide[:, ::2])
    else:
        raises(f"{entry}: unsupported geometry q ({rows}, 320) k ({rows}, 128) cache (1, 2, 8, 64) torch.bfloat16", q=wide[:, :320])
        raises(f"{entry}: rows of q / k / v, the caches and the key mask must be contiguous", q=wide[:, ::2])
    if multi:
        raises("decode_attention_multi: slots t0 .. t0 + Q - 1 outside the cache or the key mask", t=7)
        raises("decode_attention_multi: cos / sin are the contiguous fp32 [B*Q, hd/2] tables of rope_table", cos=a["cos"].double())
    else:
        raises(f"{entry}: slot t outside the cache or the key mask", t=8)
        raises(f"{entry}: cos / sin are the contiguous fp32 [B, hd/2] tables of rope_table", cos=a["cos"].double())
    raises(f"{entry}: key_valid is a bool / uint8 mask", key_valid=a["key_valid"].to(torch.int32))
    assert torch.is_grad_enabled()
    raises(f"{entry} has no backward: call it under torch.no_grad()", q=a["q"].clone().requires_grad_())


@pytest.mark.parametrize("entry", ENTRIES)
def test_split_call_takes_the_one_workspace_of_the_device(dev, entry, monkeypatch):
    """A forced split in two at t = 5: the partials go through ``ops._DECODE_WS[device]``, the entry all three functions share
    — one that is large enough is used as it is, a missing one is made with the size the library asks for — and the same
    call gives the same bits."""
    ops = _ops()
    call, a, need = _entry_case(dev, entry)
    held = torch.full((need + 64,), float("nan"), dtype=torch.float32, device=dev)
    monkeypatch.setattr(ops, "_DECODE_WS", {a["q"].device: held})
    out = call()
    assert list(ops._DECODE_WS) == [a["q"].device] and ops._DECODE_WS[a["q"].device] is held
    assert torch.isfinite(held[:need]).all() and torch.isnan(held[need:]).all()      # the partials went there, and only there
    assert out.shape == a["q"].shape and out.dtype == torch.bfloat16 and torch.isfinite(out).all()
    assert torch.equal(call(), out)
    monkeypatch.setattr(ops, "_DECODE_WS", {})
    assert torch.equal(call(), out)
    assert list(ops._DECODE_WS) == [a["q"].device] and ops._DECODE_WS[a["q"].device].numel() == need
    assert torch.equal(call(splits=2), out) and ops._DECODE_WS[a["q"].device].numel() == need
