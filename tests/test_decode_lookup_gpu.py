"""`-m gpu`: prompt-lookup speculative decoding — ``cmb_decode_attn_multi`` (decode_attn_multi.hip) through
``ops.decode_attention_multi``, the layers' ``decode_multi`` / ``lookup_step`` and ``generate(prompt_lookup_num_tokens=...)``.

Kernel tests compare with a plain torch expression on the CPU in float64 — tests/test_decode_attn_gpu.py's reference extended
to Q queries per cache row: rotate-half RoPE, masked softmax (cached slots under the key mask, the step's own slots causal),
grouped KV heads by indexing, from the inputs AS STORED (bf16 rounded first, the RoPE tables those of ``ops.rope_table``).
Tolerance: ``conftest.TOL["bf16"]`` (2e-2) through ``rel_err``."""
import math

import pytest
import torch

from conftest import TOL, rel_err
from test_decode_step_gpu import _lm, _spies

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
GEOMS = [(4, 2, 64), (4, 4, 64), (8, 2, 128), (7, 1, 128), (3, 3, 96), (32, 8, 128)]
LENGTHS = ["Q", "Q+1", "c-1", "c", "c+1", "2*c+3", "1031"]
THETA = 10000.0
TAIL = 5          # cache slots past the step's own, filled with garbage


def _ops():
    from cambrian_amd import ops
    return ops


def _qs(nh, nkv):
    return sorted({1, 2, 5, min(16, 64 // (nh // nkv))})


def _masks(B, t0, n):
    """(name, bool [B, n + TAIL]) key masks over the t0 cached keys; columns from t0 on stay False (the kernel opens the step's
    own slots by itself and must not look at the rest)."""
    full = torch.zeros(B, n + TAIL, dtype=torch.bool)
    full[:, :t0] = True
    left = full.clone()
    for b in range(B):
        left[b, :min(max(t0 - 1, 0), (3 + 7 * b) % max(t0, 1))] = False
    lone = full.clone()
    lone[B - 1, :t0] = False                                           # every cached key of the last row masked
    return [("all", full), ("left", left), ("lone", lone)]


def _inputs(nh, nkv, hd, B, Q, t0, seed):
    g = torch.Generator().manual_seed(seed)
    n = t0 + Q
    q = torch.randn(B * Q, nh * hd, generator=g).to(BF)
    k = torch.randn(B * Q, nkv * hd, generator=g).to(BF)
    v = torch.randn(B * Q, nkv * hd, generator=g).to(BF)
    kc = torch.randn(B, nkv, n + TAIL, hd, generator=g).to(BF)
    vc = torch.randn(B, nkv, n + TAIL, hd, generator=g).to(BF)
    kc[:, :, t0:], vc[:, :, t0:] = 3.0e4, float("nan")                 # the step's own slots (overwritten) and the tail (never read)
    pos = torch.randint(0, 1100, (B, 1), generator=g) + torch.arange(Q)[None]          # consecutive positions per sequence
    return q, k, v, kc, vc, pos


def _reference(q, k, v, cos, sin, kc, vc, t0, Q, valid, nh, nkv, hd):
    """float64 on the CPU -> (out [B*Q, nh*hd], roped new k [B, Q, nkv, hd])."""
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
    m = torch.zeros(B, Q, n, dtype=torch.bool)
    m[:, :, :t0] = valid[:, None, :t0]
    m[:, :, t0:] = torch.ones(Q, Q, dtype=torch.bool).tril()
    seen = m.any(1)[:, None, :, None]                                   # a slot nobody may attend may hold NaN: it weighs 0
    K, V = torch.where(seen, K, 0.0), torch.where(seen, V, 0.0)
    head = torch.arange(nh) // G
    sc = torch.einsum("bqhd,bhjd->bhqj", qr, K[:, head]) / math.sqrt(hd)
    sc = sc.masked_fill(~m[:, None], float("-inf"))
    out = torch.einsum("bhqj,bhjd->bqhd", torch.softmax(sc, -1), V[:, head])
    return out.reshape(B * Q, nh * hd), kr


def _bits(x):
    return x.contiguous().view(torch.int16)


def _run(dev, nh, nkv, hd, B, Q, t0, valid, seed=0, splits=0, poison=False):
    ops = _ops()
    q, k, v, kc, vc, pos = _inputs(nh, nkv, hd, B, Q, t0, seed)
    if poison:                                                          # masked cached slots hold NaN / huge values
        dead = ~valid[:, :t0]
        kc[:, :, :t0][dead[:, None].expand(B, nkv, t0)] = float("nan")
        vc[:, :, :t0][dead[:, None].expand(B, nkv, t0)] = 3.0e4
    cos, sin = ops.rope_table(pos.to(dev), hd, THETA)
    kcd, vcd = kc.to(dev), vc.to(dev)
    out = ops.decode_attention_multi(q.to(dev), k.to(dev), v.to(dev), cos, sin, kcd, vcd, t0, valid.to(dev), splits=splits)
    ref, kr = _reference(q, k, v, cos, sin, kc, vc, t0, Q, valid, nh, nkv, hd)
    return out, ref, (q, k, v, kc, vc, cos, sin, kcd, vcd, kr)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("nh,nkv,hd", GEOMS)
def test_kernel_parity(dev, nh, nkv, hd, B):
    ops = _ops()
    worst = 0.0
    for Q in _qs(nh, nkv):
        c = ops.decode_attention_multi_plan(B, nkv, 1031 - Q, Q)[1]
        for expr in LENGTHS:
            n = int(eval(expr, {"c": c, "Q": Q}))
            t0 = n - Q
            if t0 < 0:
                continue
            for mname, valid in _masks(B, t0, n):
                out, ref, (q, k, v, kc, vc, cos, sin, kcd, vcd, kr) = _run(dev, nh, nkv, hd, B, Q, t0, valid, seed=n + Q,
                                                                           poison=mname != "all")
                e = rel_err(out, ref)
                worst = max(worst, e)
                what = f"{nh}/{nkv}/{hd} B={B} Q={Q} n={n} mask={mname}"
                assert torch.isfinite(out).all(), what
                assert e < TOL["bf16"], f"{what}: out rel err {e}"
                new_v = vcd[:, :, t0:n].cpu()
                assert torch.equal(_bits(new_v), _bits(v.view(B, Q, nkv, hd).transpose(1, 2))), what      # raw v, bit for bit
                new_k = kcd[:, :, t0:n].transpose(1, 2)
                roped = ops.rope(k.to(dev).view(B * Q, nkv, hd), cos, sin).view(B, Q, nkv, hd)
                assert rel_err(new_k, roped) < TOL["bf16"] and rel_err(new_k, kr) < TOL["bf16"], what
                keep = torch.ones(n + TAIL, dtype=torch.bool)
                keep[t0:n] = False
                assert torch.equal(_bits(kcd.cpu()[:, :, keep]), _bits(kc[:, :, keep])), what
                assert torch.equal(_bits(vcd.cpu()[:, :, keep]), _bits(vc[:, :, keep])), what
    print(f"{nh}/{nkv}/{hd} B={B}: worst out rel err {worst:.3g}")


@pytest.mark.parametrize("nh,nkv,hd", [(8, 2, 128), (3, 3, 96), (32, 8, 128)])
def test_forced_splits_agree_and_repeat(dev, nh, nkv, hd):
    ops = _ops()
    B, n = 2, 1031
    Q = min(5, 64 // (nh // nkv))
    t0 = n - Q
    mx = ops.decode_attention_max_splits()
    assert ops.decode_attention_multi_plan(B, nkv, t0, Q, mx)[0] > 3
    full = torch.zeros(B, n + TAIL, dtype=torch.bool)
    full[:, :t0] = True
    blank = full.clone()
    c3 = ops.decode_attention_multi_plan(B, nkv, t0, Q, 3)[1]
    blank[0, c3:2 * c3] = False                        # the whole middle chunk of the 3-way split
    blank[1, :t0] = False                              # every chunk but the last is empty
    for valid in (full, blank):
        outs = []
        for s in (1, 2, 3, mx):
            out, ref, rest = _run(dev, nh, nkv, hd, B, Q, t0, valid, seed=5, splits=s)
            assert torch.isfinite(out).all(), f"splits {s}: NaN / Inf in out"
            e = rel_err(out, ref)
            print(f"{nh}/{nkv}/{hd} splits={s}: out rel err {e:.3g}")
            assert e < TOL["bf16"], f"splits {s}: out rel err {e}"
            again, _, rest2 = _run(dev, nh, nkv, hd, B, Q, t0, valid, seed=5, splits=s)
            assert torch.equal(again, out), f"splits {s}: a second call gave other bits"
            assert torch.equal(_bits(rest[7]), _bits(rest2[7])) and torch.equal(_bits(rest[8]), _bits(rest2[8]))
            outs.append(out)
        for o in outs[1:]:
            assert rel_err(o, outs[0]) < TOL["bf16"]


# ---------------------------------------------------------------------------------------------------------------------
# 2. the kernel against Q successive single-token calls
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t0", [0, 37, 700])
@pytest.mark.parametrize("nh,nkv,hd", GEOMS)
def test_kernel_equals_successive_single_token_steps(dev, nh, nkv, hd, t0):
    ops = _ops()
    B = 2
    for Q in _qs(nh, nkv):
        n = t0 + Q
        valid = _masks(B, t0, n)[1][1]
        q, k, v, kc, vc, pos = _inputs(nh, nkv, hd, B, Q, t0, seed=3 * t0 + Q)
        cos, sin = ops.rope_table(pos.to(dev), hd, THETA)
        qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
        kcm, vcm = kc.to(dev), vc.to(dev)
        out = ops.decode_attention_multi(qd, kd, vd, cos, sin, kcm, vcm, t0, valid.to(dev))
        kcs, vcs = kc.to(dev), vc.to(dev)
        mask = valid.to(dev).clone()
        rows = []
        for j in range(Q):
            sel = torch.arange(B, device=dev) * Q + j
            rows.append(ops.decode_attention(qd[sel], kd[sel], vd[sel], cos[sel].contiguous(), sin[sel].contiguous(), kcs, vcs,
                                             t0 + j, mask))
            mask[:, t0 + j] = True
        want = torch.stack(rows, 1).reshape(B * Q, nh * hd)
        e = rel_err(out, want)
        print(f"{nh}/{nkv}/{hd} t0={t0} Q={Q}: rel err against {Q} single-token calls {e:.3g}")
        assert e < TOL["bf16"]
        assert torch.equal(_bits(vcm[:, :, :n]), _bits(vcs[:, :, :n]))
        assert rel_err(kcm[:, :, t0:n], kcs[:, :, t0:n]) < TOL["bf16"] and torch.equal(_bits(kcm[:, :, :t0]), _bits(kcs[:, :, :t0]))


# ---------------------------------------------------------------------------------------------------------------------
# 3. lookup_step against Q successive per-token steps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def clean_env(monkeypatch):
    for name in ("CAMBRIAN_AMD_DECODE_STEP", "CAMBRIAN_AMD_DECODE_FP8", "CAMBRIAN_AMD_DECODE_FP4", "CAMBRIAN_AMD_DECODE_LINEAR",
                 "CAMBRIAN_AMD_DECODE_ATTN", "CAMBRIAN_AMD_DECODE_KV_FP8"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def _multi_spy(monkeypatch, calls):
    ops = _ops()
    calls["multi"] = 0
    real = ops.decode_attention_multi

    def counted(*a, **kw):
        calls["multi"] += 1
        return real(*a, **kw)

    monkeypatch.setattr(ops, "decode_attention_multi", counted)
    return calls


def _per_token_logits(model, ids, caches, t0, p0, mask, fp8, fp4):
    """The loop of test_one_step_equals_the_five_launch_loop, teacher-forced with ``ids``: fp32 logits [Q, V]."""
    from cambrian_amd.model.language_model import cambrian_llama as CL
    ops = _ops()
    cfg = model.config
    hd = model.model.layers[0].self_attn.hd
    rows = []
    mask = mask.clone()
    for j in range(ids.shape[0]):
        t = t0 + j
        mask[:, t] = True
        cos, sin = ops.rope_table(torch.tensor([[p0 + j]], device=ids.device), hd, float(cfg.rope_theta))
        h = model.model.embed_tokens(ids[j:j + 1])[:, None, :].to(model.model.llm_dtype)
        for layer, (kc, vc) in zip(model.model.layers, caches):
            h = layer.decode(h, cos, sin, kc, vc, t, mask, fp8=fp8, fp4=fp4)
        rows.append(CL._decode_logits(model, h, fp8, fp4))
    return torch.cat(rows, 0)


@pytest.mark.parametrize("t0", [36, 299])
@pytest.mark.parametrize("Q", [2, 8])
@pytest.mark.parametrize("weights", ["bf16", "fp8", "fp4"])
@pytest.mark.parametrize("lm", ["llama", "phi3"])
def test_lookup_step_equals_per_token_steps(dev, clean_env, lm, weights, Q, t0):
    from cambrian_amd.model.language_model import cambrian_llama as CL
    model = _lm(dev, lm)
    fp8, fp4 = weights == "fp8", weights == "fp4"
    a0 = model.model.layers[0].self_attn
    nkv, hd, V = a0.nkv, a0.hd, model.config.vocab_size
    n_layers = len(model.model.layers)
    gen = torch.Generator().manual_seed(7 * Q + t0)
    Lmax = t0 + Q + 3
    caches = [(torch.randn(1, nkv, Lmax, hd, generator=gen).to(BF).to(dev), torch.randn(1, nkv, Lmax, hd, generator=gen).to(BF).to(dev))
              for _ in range(n_layers)]
    mask = (torch.rand(1, Lmax, generator=gen) > 0.15)
    mask[:, t0:] = False
    mask = mask.to(dev)
    ids = torch.randint(1, V, (Q,), generator=gen).to(dev)
    p0 = t0 - 5
    calls = _multi_spy(clean_env, _spies(clean_env))

    with torch.no_grad():
        ref_caches = [(k.clone(), v.clone()) for k, v in caches]
        want = _per_token_logits(model, ids, ref_caches, t0, p0, mask, fp8, fp4)
        assert calls["attention"] == Q * n_layers and calls["multi"] == 0
        for key in calls:
            calls[key] = 0
        got_caches = [(k.clone(), v.clone()) for k, v in caches]
        got = CL.lookup_step(model, ids, got_caches, t0, p0, mask, fp8, fp4)
    torch.cuda.synchronize()
    assert calls["multi"] == n_layers and calls["attention"] == 0, calls
    lin = "linear_fp8" if fp8 else "linear"
    if not fp4:
        assert calls[lin] == 4 * n_layers + 1, calls
    assert got.shape == want.shape == (Q, V) and got.dtype == torch.float32 and torch.isfinite(got).all()
    e = rel_err(got, want)
    print(f"lookup_step {lm} {weights} Q={Q} t0={t0}: logits rel err against {Q} per-token steps {e:.3g}")
    assert e < TOL["bf16"]
    for (k1, v1), (k0, v0) in zip(got_caches, ref_caches):
        assert rel_err(k1[:, :, :t0 + Q], k0[:, :, :t0 + Q]) < TOL["bf16"] and rel_err(v1[:, :, :t0 + Q], v0[:, :, :t0 + Q]) < TOL["bf16"]
        assert torch.equal(k1[:, :, t0 + Q:], k0[:, :, t0 + Q:])

    # the plain torch body (CAMBRIAN_AMD_DECODE_ATTN=0: the modules' own bf16 projections, ops.rope, SDPA under lookup_mask)
    clean_env.setenv("CAMBRIAN_AMD_DECODE_ATTN", "0")
    for key in calls:
        calls[key] = 0
    with torch.no_grad():
        body = CL.lookup_step(model, ids, [(k.clone(), v.clone()) for k, v in caches], t0, p0, mask, fp8, fp4)
        body_ref = _per_token_logits(model, ids, [(k.clone(), v.clone()) for k, v in caches], t0, p0, mask, fp8, fp4)
    assert calls["multi"] == 0 and calls["attention"] == 0
    e_body = rel_err(body, body_ref)
    print(f"  torch body against its own per-token steps {e_body:.3g}")
    assert e_body < TOL["bf16"]
    if weights == "bf16":            # (the torch body streams no quantised weights: only bf16 compares kernel and body)
        e_kb = rel_err(got, body)
        print(f"  kernel path against the torch body {e_kb:.3g}")
        assert e_kb < TOL["bf16"]


# ---------------------------------------------------------------------------------------------------------------------
# 4. generate(), fp32 model: the tokens of the call without lookup, exactly
# ---------------------------------------------------------------------------------------------------------------------
def _lm_cpu_weights(dev, lm="llama", dt=torch.float32):
    """``_lm``'s model with weights drawn on the CPU under ``torch.manual_seed(3)`` (independent of the device's generator)."""
    cpu = _lm(torch.device("cpu"), lm, dt=dt)
    model = _lm(dev, lm, dt=dt)
    model.load_state_dict(cpu.state_dict())
    model.requires_grad_(False)
    return model.eval()


def _prompt(dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, 64, (1, 9), generator=g).to(dev)


def _replay(prompt, seq, num, max_ngram, vocab, eos, max_rows, max_new):
    """What the lookup loop must report when it emits ``seq``: a pure-Python walk with ``ngram_draft`` / ``accept``."""
    from cambrian_amd.model.language_model.lookup import accept, ngram_draft
    out = [seq[0]]
    stats = {"steps": 0, "drafted": 0, "accepted": 0}
    while len(out) < len(seq):
        room = min(num, max_rows - 1, max_new - len(out) - 1)
        draft = ngram_draft(prompt + out, room, max_ngram, vocab, eos) if room > 0 else []
        stats["steps"] += 1
        if not draft:
            out.append(seq[len(out)])
            continue
        picked = seq[len(out):len(out) + len(draft) + 1]
        a = accept(draft[:len(picked)], picked)
        a = min(a, len(picked) - 1)
        stats["drafted"] += len(draft)
        stats["accepted"] += a
        out.extend(seq[len(out):len(out) + a + 1])
    return stats


@pytest.fixture(scope="module")
def fp32_model(dev):
    return _lm_cpu_weights(dev)


@pytest.mark.parametrize("num,ngram", [(4, 2), (15, 3)])
@pytest.mark.parametrize("seed", [1, 3])
def test_generate_fp32_equals_plain_greedy(dev, clean_env, fp32_model, seed, num, ngram):
    model = fp32_model
    ids = _prompt(dev, seed)
    new = 32
    plain = model.generate(ids, max_new_tokens=new)
    got = model.generate(ids, max_new_tokens=new, prompt_lookup_num_tokens=num, max_matching_ngram_size=ngram)
    assert torch.equal(got, plain), (got.tolist(), plain.tolist())
    a0 = model.model.layers[0].self_attn
    want = _replay(ids[0].tolist(), plain[0].tolist(), num, ngram, 64, None, min(16, 64 // (a0.nh // a0.nkv)), new)
    print(f"seed {seed} ({num}, {ngram}): {model.lookup_stats}")
    assert model.lookup_stats == want, (model.lookup_stats, want)
    assert want["accepted"] >= 4, "the sequence repeats too little to show an accepted draft"
    assert want["steps"] + want["accepted"] + 1 == new


def test_generate_fp32_eos_inside_an_accepted_run(dev, clean_env, fp32_model):
    """eos is a token of the yardstick's own output at its first occurrence there.  Real drafts copy earlier text, so they never
    hold a token's first occurrence; an oracle that drafts the yardstick's continuation (and does not cut at eos, as
    ``ngram_draft`` would) puts it in the middle of an accepted run: the tokens behind it must be dropped."""
    model = fp32_model
    ids = _prompt(dev, 1)
    L, new = ids.shape[1], 32
    plain = model.generate(ids, max_new_tokens=new)[0].tolist()

    def right(seq, n, *a):
        return plain[len(seq) - L:len(seq) - L + n]

    for col in (3, 8):                                # steps of 1 + 4 drafts emit columns 1-5, 6-10: both lie inside a run
        eos = plain[col]
        assert plain.index(eos) == col, f"column {col} of {plain} is no first occurrence"
        stop = model.generate(ids, max_new_tokens=new, eos_token_id=eos)
        assert stop.shape == (1, col + 1)
        got = model.generate(ids, max_new_tokens=new, eos_token_id=eos, prompt_lookup_num_tokens=4, _draft_fn=right)
        assert torch.equal(got, stop), (got.tolist(), stop.tolist())
        assert model.lookup_stats["accepted"] >= col - 1 - (col > 5)      # the drafts before eos stood
        got = model.generate(ids, max_new_tokens=new, eos_token_id=eos, prompt_lookup_num_tokens=4)
        assert torch.equal(got, stop), (got.tolist(), stop.tolist())


@pytest.mark.parametrize("new", [1, 2, 5])
def test_generate_fp32_budget_and_cache_bound(dev, clean_env, fp32_model, new):
    """The length is exact and no slot from L + max_new_tokens - 1 on is written: the loop runs on caches with a sentinel tail."""
    from cambrian_amd.model.language_model import cambrian_llama as CL
    model = fp32_model
    ids = _prompt(dev, 3)
    L, pad, seen = ids.shape[1], 4, {}
    real = CL._lookup_loop

    def padded(self, logits, caches, key_mask, *rest):
        big = []
        for kc, vc in caches:
            assert kc.shape[2] == L + new
            tail = torch.full((1, kc.shape[1], pad, kc.shape[3]), 7.0, dtype=kc.dtype, device=kc.device)
            big.append((torch.cat([kc, tail], 2), torch.cat([vc, tail], 2)))
        km = torch.cat([key_mask, torch.zeros(1, pad, dtype=torch.bool, device=key_mask.device)], 1)
        seen["caches"], seen["mask"] = big, km
        return real(self, logits, big, km, *rest)

    clean_env.setattr(CL, "_lookup_loop", padded)
    always = lambda ids_, n, *a: [1] * n              # a drafter that always wants the whole budget
    for fn in (None, always):
        got = model.generate(ids, max_new_tokens=new, prompt_lookup_num_tokens=15, max_matching_ngram_size=3, _draft_fn=fn)
        assert got.shape == (1, new)
        assert torch.equal(got, model.generate(ids, max_new_tokens=new))
        for kc, vc in seen["caches"]:
            assert bool((kc[:, :, L + new:] == 7.0).all()) and bool((vc[:, :, L + new:] == 7.0).all())
            assert bool((kc[:, :, L + new - 1] == 0).all()) and bool((vc[:, :, L + new - 1] == 0).all())
        assert not bool(seen["mask"][:, L + new - 1:].any())


# ---------------------------------------------------------------------------------------------------------------------
# 5. generate(), bf16 kernel path
# ---------------------------------------------------------------------------------------------------------------------
def _teacher_forced_logits(model, ids, tokens, fp8):
    """Reference logits of every emitted position from the per-token loop fed with ``tokens``: generate()'s own prefill and
    decode steps, written out.  fp32 [len(tokens), V]; row i is the distribution token i was picked from."""
    from cambrian_amd.model.language_model import cambrian_llama as CL
    ops = _ops()
    m, dev = model.model, ids.device
    L, new = ids.shape[1], len(tokens)
    a0 = m.layers[0].self_attn
    theta = float(model.config.rope_theta)
    with torch.no_grad():
        kv_out = []
        pos = torch.arange(L, device=dev)[None]
        hidden = m(m.embed_tokens(ids).to(m.llm_dtype), pos, None, None, kv_out=kv_out)
        rows = [model.lm_head(hidden[:, L - 1]).float()]
        caches = []
        for k, v in kv_out:
            kc = torch.zeros(1, a0.nkv, L + new, a0.hd, dtype=k.dtype, device=dev)
            vc = torch.zeros_like(kc)
            kc[:, :, :L], vc[:, :, :L] = k, v
            caches.append((kc, vc))
        mask = torch.zeros(1, L + new, dtype=torch.bool, device=dev)
        mask[:, :L] = True
        for step in range(new - 1):
            t = L + step
            mask[:, t] = True
            cos, sin = ops.rope_table(torch.tensor([[L + step]], device=dev), a0.hd, theta)
            x = m.embed_tokens(torch.tensor([tokens[step]], device=dev))[:, None, :].to(m.llm_dtype)
            for layer, (kc, vc) in zip(m.layers, caches):
                x = layer.decode(x, cos, sin, kc, vc, t, mask, fp8=fp8)
            rows.append(CL._decode_logits(model, x, fp8))
    return torch.cat(rows, 0)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("lm", ["llama", "phi3"])
def test_generate_bf16_kernel_path(dev, clean_env, lm, fp8):
    model = _lm(dev, lm)
    if fp8:
        clean_env.setenv("CAMBRIAN_AMD_DECODE_FP8", "1")
    calls = _multi_spy(clean_env, _spies(clean_env))
    ids = _prompt(dev, 1)
    L, new = ids.shape[1], 32
    greedy = model.generate(ids, max_new_tokens=new)[0].tolist()

    def right(seq, n, *a):
        return greedy[len(seq) - L:len(seq) - L + n]

    def wrong_from_2(seq, n, *a):
        d = right(seq, n)
        return d[:1] + [(x + 1) % 64 for x in d[1:]]

    def all_wrong(seq, n, *a):
        return [(x + 1) % 64 for x in right(seq, n)]

    for name, fn in (("ngram", None), ("right", right), ("wrong from 2", wrong_from_2), ("all wrong", all_wrong)):
        for key in calls:
            calls[key] = 0
        got = model.generate(ids, max_new_tokens=new, prompt_lookup_num_tokens=7, _draft_fn=fn)
        torch.cuda.synchronize()
        stats = dict(model.lookup_stats)
        toks = got[0].tolist()
        assert got.shape == (1, new)
        ref = _teacher_forced_logits(model, ids, toks, fp8)
        top = ref.max(-1).values
        chosen = ref[torch.arange(new), torch.tensor(toks, device=dev)]
        slack = ((top - chosen) / ref.abs().max(-1).values).max().item()
        print(f"{lm} fp8={fp8} {name}: {stats}, worst (max logit - emitted logit) / max |logit| = {slack:.3g}, "
              f"equal to greedy: {toks == greedy}")
        assert slack < TOL["bf16"], f"{name}: an emitted token lies {slack} of max |logit| below the row's maximum"
        assert stats["steps"] + stats["accepted"] + 1 == new
        if name == "right":
            assert stats["accepted"] == stats["drafted"] > 0, stats
        if name == "all wrong":
            assert stats["accepted"] == 0 and stats["steps"] == new - 1, stats
        if name == "wrong from 2":
            assert stats["accepted"] <= stats["steps"], stats          # at most the first draft of a step stands
        if name != "ngram":
            assert calls["multi"] > 0
        assert calls["step"] == 0 and calls["next"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 6. off means untouched
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lm", ["llama", "phi3"])
def test_without_the_arguments_nothing_changes(dev, clean_env, lm):
    model = _lm(dev, lm)
    calls = _multi_spy(clean_env, _spies(clean_env))
    ids = _prompt(dev, 1)
    new, layers = 20, len(model.model.layers)
    outs = []
    for switch in ("0", "1"):
        clean_env.setenv("CAMBRIAN_AMD_DECODE_STEP", switch)
        for kw in (dict(), dict(prompt_lookup_num_tokens=None), dict(prompt_lookup_num_tokens=0, max_matching_ngram_size=3)):
            for key in calls:
                calls[key] = 0
            outs.append(model.generate(ids, max_new_tokens=new, **kw))
            torch.cuda.synchronize()
            assert calls["multi"] == 0
            if switch == "0":
                assert calls["step"] == 0 and calls["next"] == 0 and calls["linear"] == (new - 1) * (4 * layers + 1) \
                    and calls["attention"] == (new - 1) * layers, calls
            else:
                assert calls["step"] == new - 1 and calls["next"] == new and calls["linear"] == 0 and calls["attention"] == 0, calls
    assert all(torch.equal(o, outs[0]) for o in outs)
    assert not hasattr(model, "lookup_stats")
