"""GPU: the decode step as one library call per token (``cmb_decode_step``, decode_step.hip) and the greedy selection between
two steps (``cmb_decode_next``, decode_next.hip).

* ``cmb_decode_next`` against torch: argmax with its tie and NaN rules, the eos / done rule over consecutive calls, every
  output with ``torch.equal``, sentinels around every output, the same bits on a second call.
* one ``cmb_decode_step`` against the Python five-launch loop from cloned caches: the launchers and their arguments are the
  same, so logits and both caches must be EQUAL.
* ``generate()`` with the switch at 1 and at 0: equal tokens (greedy, greedy with an eos that stops the loop between two
  polls, sampling under one seed), and who was called how often.
* outside the conditions the switch changes nothing and no step call is made.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

THETA = 500000.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def _ops():
    from cambrian_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------------------------------
# cmb_decode_next
# ---------------------------------------------------------------------------------------------------------------------
SENT = 7


class _NextBufs:
    """Every output of ``decode_next`` as a view into the middle of a larger tensor filled with a sentinel."""

    def __init__(self, dev, B, H, hd, steps, kv_ld, eos):
        self.out_full = torch.full((B + 2, steps + 2), -SENT, dtype=torch.int64, device=dev)
        self.pos_full = torch.full((B + 2,), -SENT, dtype=torch.int64, device=dev)
        self.kv_full = torch.full((B + 2, kv_ld), SENT, dtype=torch.uint8, device=dev)
        self.x_full = torch.full((B + 2, H + 8), float(SENT), dtype=torch.bfloat16, device=dev)
        self.cos_full = torch.full((B + 2, hd // 2), float(SENT), dtype=torch.float32, device=dev)
        self.sin_full = torch.full((B + 2, hd // 2), float(SENT), dtype=torch.float32, device=dev)
        self.done_full = torch.full((B + 2,), SENT, dtype=torch.uint8, device=dev)
        self.out = self.out_full[1:B + 1, 1:steps + 1]
        self.pos, self.kv, self.x = self.pos_full[1:B + 1], self.kv_full[1:B + 1], self.x_full[1:B + 1, :H]
        self.cos, self.sin, self.done = self.cos_full[1:B + 1], self.sin_full[1:B + 1], self.done_full[1:B + 1]
        self.done.zero_()
        self.eos = eos

    def tensors(self):
        return [t.clone() for t in (self.out_full, self.pos_full, self.kv_full, self.x_full, self.cos_full, self.sin_full,
                                    self.done_full)]


def _planted_logits(gen_dev, B, V, ld, rot):
    """fp32 [B, V] as a view of [B, ld] whose columns past V hold +inf (a read past V would win), row b planted by kind
    (b + rot) % 6: maximum at 0, at V - 1, tied at three places, a row of -inf with one finite entry, a row with NaNs (the
    first wins, and it beats the +inf beside it), plain random."""
    full = torch.randn(B, ld, generator=gen_dev, device=gen_dev.device, dtype=torch.float32)
    full[:, V:] = float("inf")
    logits = full[:, :V]
    for b in range(B):
        kind = (b + rot) % 6
        if kind == 0:
            logits[b, 0] = 9.0
        elif kind == 1:
            logits[b, V - 1] = 9.0
        elif kind == 2:
            for i in (V // 3, V // 2, V - 2):
                logits[b, i] = 9.0
        elif kind == 3:
            logits[b].fill_(float("-inf"))
            logits[b, (2 * V) // 3] = -3.0e38
        elif kind == 4:
            logits[b, V // 2 + 1] = float("nan")
            logits[b, V - 1] = float("nan")
            logits[b, V // 2 + 2] = float("inf")
            logits[b, 1] = -0.0
    return logits


@pytest.mark.parametrize("V", [64, 32003, 128256])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_decode_next_against_torch(dev, B, V):
    ops = _ops()
    H, hd, steps, kv_ld, t0 = 72, 64, 8, 48, 36
    gen = torch.Generator(device=dev).manual_seed(100 * B + V % 97)
    embed = torch.randn(V + 3, H + 8, generator=gen, device=dev, dtype=torch.float32).to(torch.bfloat16)[:, :H]   # row stride H + 8
    n_tok = torch.randint(1, 30, (B,), generator=gen, device=dev)
    lds = (V, V + 5, (V + 7) // 8 * 8 + 8)                       # contiguous rows, an odd stride, lm_head's padded stride
    for rot in range(6):
        ld = lds[rot % 3]
        logits = _planted_logits(gen, B, V, ld, rot)
        want = torch.argmax(logits, -1)
        kinds = [(b + rot) % 6 for b in range(B)]
        for b, kind in enumerate(kinds):                          # the planted rows pin torch's own rules down
            if kind == 0:
                assert int(want[b]) == 0
            elif kind == 1:
                assert int(want[b]) == V - 1
            elif kind == 2:
                assert int(want[b]) == V // 3
            elif kind == 3:
                assert int(want[b]) == (2 * V) // 3
            elif kind == 4:
                assert int(want[b]) == V // 2 + 1
        bufs = _NextBufs(dev, B, H, hd, steps, kv_ld, -1)
        before = bufs.tensors()
        step, t = rot, t0 + rot
        ops.decode_next(logits, -1, None, bufs.out, step, n_tok, bufs.pos, bufs.kv, t, embed, bufs.x, hd, THETA, bufs.cos,
                        bufs.sin)
        torch.cuda.synchronize()
        assert torch.equal(bufs.out[:, step], want), (rot, bufs.out[:, step].tolist(), want.tolist())
        assert torch.equal(bufs.pos, n_tok + step)
        assert bool((bufs.kv[:, t] == 1).all())
        assert torch.equal(bufs.x, embed[want])
        cos, sin = ops.rope_table((n_tok + step)[:, None], hd, THETA)
        assert torch.equal(bufs.cos, cos) and torch.equal(bufs.sin, sin)
        # nothing else moved: put the sentinels back where the call wrote and compare the whole tensors
        after = bufs.tensors()
        bufs.out[:, step] = -SENT
        bufs.pos.fill_(-SENT)
        bufs.kv[:, t] = SENT
        bufs.x.fill_(float(SENT))
        bufs.cos.fill_(float(SENT))
        bufs.sin.fill_(float(SENT))
        for name, a, b in zip(("out_ids", "pos", "key_valid", "x", "cos", "sin", "done"), before, bufs.tensors()):
            assert torch.equal(a, b), f"{name}: bytes around the output changed"
        # the same call again: the same bits
        ops.decode_next(logits, -1, None, bufs.out, step, n_tok, bufs.pos, bufs.kv, t, embed, bufs.x, hd, THETA, bufs.cos,
                        bufs.sin)
        torch.cuda.synchronize()
        for a, b in zip(after, bufs.tensors()):
            assert torch.equal(a, b)


@pytest.mark.parametrize("B", [1, 3, 16])
def test_decode_next_eos_and_done_over_three_calls(dev, B):
    """Call 1: eos is row 0's own argmax, so row 0 is done.  Call 2: row 0 must emit eos whatever its logits say, and eos is
    planted as the argmax of the last row, which becomes done.  Call 3: both emit eos, the others their argmax."""
    ops = _ops()
    V, H, hd, steps, kv_ld, t0 = 1000, 64, 64, 4, 48, 40
    gen = torch.Generator(device=dev).manual_seed(5 + B)
    embed = torch.randn(V, H, generator=gen, device=dev).to(torch.bfloat16)
    n_tok = torch.randint(1, 30, (B,), generator=gen, device=dev)
    rounds = [torch.randn(B, V, generator=gen, device=dev) for _ in range(3)]
    eos = int(rounds[0][0].argmax())
    for r in rounds:
        r[1:B - 1 if B > 2 else B, eos] = -50.0       # the rows in between never pick eos by themselves
    rounds[1][B - 1, eos] = 50.0
    rounds[1][0, eos] = -50.0
    rounds[2][:, eos] = -50.0
    bufs = _NextBufs(dev, B, H, hd, steps, kv_ld, eos)
    done_ref = torch.zeros(B, dtype=torch.bool, device=dev)
    for step, logits in enumerate(rounds):
        nxt = logits.argmax(-1)
        nxt = torch.where(done_ref, torch.full_like(nxt, eos), nxt)
        done_ref = done_ref | (nxt == eos)
        ops.decode_next(logits, eos, bufs.done, bufs.out, step, n_tok, bufs.pos, bufs.kv, t0 + step, embed, bufs.x, hd, THETA,
                        bufs.cos, bufs.sin)
        torch.cuda.synchronize()
        assert torch.equal(bufs.out[:, step], nxt), step
        assert torch.equal(bufs.done.bool(), done_ref) and bool((bufs.done <= 1).all()), step
        assert torch.equal(bufs.x, embed[nxt])
        assert torch.equal(bufs.pos, n_tok + step) and bool((bufs.kv[:, t0 + step] == 1).all())
    assert bool(done_ref[0]) and bool(done_ref[B - 1]) and int(done_ref.sum()) == min(B, 2)
    assert int(bufs.done_full[0]) == SENT and int(bufs.done_full[-1]) == SENT
    assert bool((bufs.out_full[:, 0] == -SENT).all()) and bool((bufs.out_full[:, 4:] == -SENT).all())


# ---------------------------------------------------------------------------------------------------------------------
# a small text-only model
# ---------------------------------------------------------------------------------------------------------------------
def _lm(dev, lm="llama", dt=torch.bfloat16, inter=512, layers=2):
    from cambrian_amd.model.language_model import cambrian_llama as CL
    geo = dict(vocab_size=64, hidden_size=256, intermediate_size=inter, num_hidden_layers=layers, num_attention_heads=4,
               num_key_value_heads=2, rms_norm_eps=1e-5, max_position_embeddings=512)
    if lm == "phi3":
        from cambrian_amd.model.language_model import cambrian_phi3 as CP
        cfg = CP.CambrianConfig(rope_theta=10000.0, pad_token_id=0, sliding_window=None, **geo)
        cls = CP.CambrianPhi3ForCausalLM
    else:
        cfg = CL.CambrianConfig(rope_theta=THETA, **geo)
        cls = CL.CambrianLlamaForCausalLM
    torch.manual_seed(3)
    model = cls(cfg, device=dev, llm_dtype=dt)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    model.requires_grad_(False)
    return model.eval()


def _spies(monkeypatch):
    ops = _ops()
    calls = {"step": 0, "next": 0, "linear": 0, "linear_fp8": 0, "attention": 0}
    for key, name in (("step", "decode_step"), ("next", "decode_next"), ("linear", "decode_linear"),
                      ("linear_fp8", "decode_linear_fp8"), ("attention", "decode_attention")):
        real = getattr(ops, name)

        def counted(*a, _real=real, _key=key, **kw):
            calls[_key] += 1
            return _real(*a, **kw)

        monkeypatch.setattr(ops, name, counted)
    return calls


@pytest.fixture()
def clean_env(monkeypatch):
    for name in ("CAMBRIAN_AMD_DECODE_STEP", "CAMBRIAN_AMD_DECODE_FP8", "CAMBRIAN_AMD_DECODE_LINEAR", "CAMBRIAN_AMD_DECODE_ATTN"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


# ---------------------------------------------------------------------------------------------------------------------
# one cmb_decode_step against the five-launch loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("B,t", [(1, 36), (3, 36), (16, 36), (1, 299)])
@pytest.mark.parametrize("lm", ["llama", "phi3"])
def test_one_step_equals_the_five_launch_loop(dev, clean_env, lm, B, t, fp8):
    from cambrian_amd.model.language_model import cambrian_llama as CL
    ops = _ops()
    model = _lm(dev, lm)
    cfg = model.config
    a0 = model.model.layers[0].self_attn
    nkv, hd, H, V = a0.nkv, a0.hd, cfg.hidden_size, cfg.vocab_size
    if t == 299:
        assert ops.decode_attention_plan(B, nkv, t)[0] > 1, "this case is here for the combine launch"
    else:
        assert ops.decode_attention_plan(B, nkv, t)[0] == 1
    gen = torch.Generator().manual_seed(11 * B + t)
    Lmax = t + 5
    caches = [(torch.randn(B, nkv, Lmax, hd, generator=gen).to(torch.bfloat16).to(dev),
               torch.randn(B, nkv, Lmax, hd, generator=gen).to(torch.bfloat16).to(dev)) for _ in model.model.layers]
    x = torch.randn(B, 1, H, generator=gen).to(torch.bfloat16).to(dev)
    mask = (torch.rand(B, Lmax, generator=gen) > 0.15).to(dev)
    cos, sin = ops.rope_table(torch.randint(0, t + 1, (B, 1), generator=gen).to(dev), hd, float(cfg.rope_theta))
    calls = _spies(clean_env)
    n_layers = len(model.model.layers)

    ref_caches = [(k.clone(), v.clone()) for k, v in caches]
    with torch.no_grad():
        h = x
        for layer, (kc, vc) in zip(model.model.layers, ref_caches):
            h = layer.decode(h, cos, sin, kc, vc, t, mask, fp8=fp8)
        want = CL._decode_logits(model, h, fp8)
    torch.cuda.synchronize()
    key = "linear_fp8" if fp8 else "linear"
    assert calls[key] == 4 * n_layers + 1 and calls["attention"] == n_layers and calls["step"] == 0, calls

    got_caches = [(k.clone(), v.clone()) for k, v in caches]
    with torch.no_grad():
        plan = CL.DecodeStepPlan.build(model, B, got_caches, Lmax - 1, fp8)
        assert plan is not None
        got = plan.step(x[:, 0], cos, sin, t, mask)
    torch.cuda.synchronize()
    assert calls["step"] == 1 and calls[key] == 4 * n_layers + 1 and calls["attention"] == n_layers, calls
    assert got.shape == want.shape == (B, V) and got.dtype == torch.float32
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)
    for (k1, v1), (k0, v0), (ks, vs) in zip(got_caches, ref_caches, caches):
        assert torch.equal(k1, k0) and torch.equal(v1, v0)
        assert not torch.equal(k1[:, :, t], ks[:, :, t])          # slot t was written
    # a second step through the same plan and workspace: the same bits
    again = [(k.clone(), v.clone()) for k, v in caches]
    with torch.no_grad():
        plan2 = CL.DecodeStepPlan.build(model, B, again, Lmax - 1, fp8)
        got2 = plan2.step(x[:, 0], cos, sin, t, mask).clone()
    assert torch.equal(got2, want)


# ---------------------------------------------------------------------------------------------------------------------
# generate()
# ---------------------------------------------------------------------------------------------------------------------
def _prompt(dev, B, L=9):
    g = torch.Generator().manual_seed(B)
    ids = torch.randint(1, 64, (B, L), generator=g).to(dev)
    att = torch.ones(B, L, dtype=torch.long)
    for b in range(1, B):
        att[b, L - (2 * b) % (L - 2):] = 0          # right padding: rows of different lengths
    return ids, att.to(dev)


def _run(model, monkeypatch, calls, switch, ids, att, **kw):
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_STEP", switch)
    for k in calls:
        calls[k] = 0
    toks = model.generate(ids, attention_mask=att, **kw)
    torch.cuda.synchronize()
    return toks, dict(calls)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("lm", ["llama", "phi3"])
def test_generate_greedy_equals_the_per_token_loop(dev, clean_env, lm, B, fp8):
    model = _lm(dev, lm)
    if fp8:
        clean_env.setenv("CAMBRIAN_AMD_DECODE_FP8", "1")
    calls = _spies(clean_env)
    ids, att = _prompt(dev, B)
    new, layers = 20, len(model.model.layers)
    off, n_off = _run(model, clean_env, calls, "0", ids, att, max_new_tokens=new)
    key, other = ("linear_fp8", "linear") if fp8 else ("linear", "linear_fp8")
    assert off.shape == (B, new)
    assert n_off["step"] == 0 and n_off["next"] == 0 and n_off[key] == (new - 1) * (4 * layers + 1) and n_off[other] == 0, n_off
    on, n_on = _run(model, clean_env, calls, "1", ids, att, max_new_tokens=new)
    assert torch.equal(on, off), (on.tolist(), off.tolist())
    assert n_on["step"] == new - 1 and n_on["next"] == new, n_on
    assert n_on["linear"] == 0 and n_on["linear_fp8"] == 0 and n_on["attention"] == 0, n_on
    assert len(set(off[0].tolist())) > 1, "a constant sequence would not show a wrong step"
    # the switch from the config, and the environment over it
    clean_env.delenv("CAMBRIAN_AMD_DECODE_STEP")
    model.config.decode_step_fused = True
    for k in calls:
        calls[k] = 0
    assert torch.equal(model.generate(ids, attention_mask=att, max_new_tokens=new), off) and calls["step"] == new - 1
    assert _run(model, clean_env, calls, "0", ids, att, max_new_tokens=new)[1]["step"] == 0


@pytest.mark.parametrize("lm", ["llama", "phi3"])
def test_generate_with_eos_stops_where_the_per_token_loop_stops(dev, clean_env, lm):
    """eos is a token of the off arm's own greedy output, so the loop stops early, between two polls of ``done``."""
    model = _lm(dev, lm)
    calls = _spies(clean_env)
    new = 20
    # one row: every row is done at that row's first eos
    ids, att = _prompt(dev, 1)
    free, _ = _run(model, clean_env, calls, "0", ids, att, max_new_tokens=new)
    seq = free[0].tolist()
    # columns where a token appears for the first time, so that the loop stops right there, off a poll boundary
    cols = [c for c in range(1, new - 1) if seq.index(seq[c]) == c and (c + 1) % 8 != 0]
    assert cols, f"the greedy sequence {seq} has no usable stopping column"
    for col in {cols[0], cols[-1]}:
        eos = seq[col]
        off, n_off = _run(model, clean_env, calls, "0", ids, att, max_new_tokens=new, eos_token_id=eos)
        stop = col + 1
        assert off.shape == (1, stop) and stop < new and stop % 8 != 0 and n_off["step"] == 0
        on, n_on = _run(model, clean_env, calls, "1", ids, att, max_new_tokens=new, eos_token_id=eos)
        assert on.shape[1] < new
        assert torch.equal(on, off), (on.tolist(), off.tolist())
        # the device loop ran on to the next poll, no further
        assert n_on["next"] == min(new, -(-stop // 8) * 8) and n_on["step"] == n_on["next"] - 1, n_on
        assert n_on["linear"] == 0 and n_on["attention"] == 0
    # three rows: a row that is done keeps emitting eos while the others go on
    ids, att = _prompt(dev, 3)
    free, _ = _run(model, clean_env, calls, "0", ids, att, max_new_tokens=new)
    eos = int(free[1, 2])
    off, _ = _run(model, clean_env, calls, "0", ids, att, max_new_tokens=new, eos_token_id=eos)
    on, n_on = _run(model, clean_env, calls, "1", ids, att, max_new_tokens=new, eos_token_id=eos)
    assert torch.equal(on, off), (on.tolist(), off.tolist())
    assert bool((off[1, 2:] == eos).all()) and n_on["linear"] == 0


@pytest.mark.parametrize("lm", ["llama", "phi3"])
def test_generate_sampling_keeps_torchs_warpers(dev, clean_env, lm):
    model = _lm(dev, lm)
    calls = _spies(clean_env)
    ids, att = _prompt(dev, 3)
    new, layers = 10, len(model.model.layers)
    kw = dict(max_new_tokens=new, do_sample=True, temperature=0.8, top_k=20, top_p=0.9)
    torch.manual_seed(123)
    off, n_off = _run(model, clean_env, calls, "0", ids, att, **kw)
    torch.manual_seed(123)
    on, n_on = _run(model, clean_env, calls, "1", ids, att, **kw)
    assert torch.equal(on, off), (on.tolist(), off.tolist())
    assert n_off["step"] == 0 and n_off["linear"] == (new - 1) * (4 * layers + 1)
    assert n_on["step"] == new - 1 and n_on["next"] == 0 and n_on["linear"] == 0 and n_on["attention"] == 0, n_on
    torch.manual_seed(124)
    other, _ = _run(model, clean_env, calls, "1", ids, att, **kw)
    assert not torch.equal(other, on), "the seed does not reach the sampler"


@pytest.mark.parametrize("why", ["fp32", "batch17", "trainable", "fp8_refused"])
def test_outside_the_conditions_the_switch_changes_nothing(dev, clean_env, why):
    dt = torch.float32 if why == "fp32" else torch.bfloat16
    model = _lm(dev, "llama", dt=dt, inter=520 if why == "fp8_refused" else 512)
    if why == "trainable":
        model.model.layers[1].mlp.down_proj.weight.requires_grad_(True)
    if why == "fp8_refused":            # down_proj has K = 520: a multiple of 8 (the bf16 step takes it), not of 16
        clean_env.setenv("CAMBRIAN_AMD_DECODE_FP8", "1")
    calls = _spies(clean_env)
    ids, att = _prompt(dev, 17 if why == "batch17" else 3)
    new = 6
    for kw in (dict(), dict(do_sample=True, temperature=0.7)):
        torch.manual_seed(9)
        off, n_off = _run(model, clean_env, calls, "0", ids, att, max_new_tokens=new, **kw)
        torch.manual_seed(9)
        on, n_on = _run(model, clean_env, calls, "1", ids, att, max_new_tokens=new, **kw)
        assert n_on["step"] == 0 and n_on["next"] == 0 and n_off["step"] == 0, (why, n_on)
        assert torch.equal(on, off)
        assert n_on == n_off, (why, n_on, n_off)
    if why == "fp8_refused":            # the layers ran on the bf16 five-launch loop; the lm_head alone takes its e4m3 copy
        assert n_on["linear"] == (new - 1) * 4 * len(model.model.layers) and n_on["linear_fp8"] == new - 1, n_on
