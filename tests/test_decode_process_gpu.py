"""GPU: the logits processors of ``generate()`` on the device (``cmb_decode_process``, decode_process.hip).

* the kernel against ``processors.apply_torch`` bit for bit: 1, 3, 16 and 17 rows; V = 1000 in rows of 1011 that start off a
  16-byte boundary, V = 32064, V = 128256; histories of 0, 1, 2, 3, 37 and 1500 ids (more ids than the workgroup has threads)
  drawn from 5 to 40 symbols; every processor on and off; sentinel columns behind every row; ids V + 3 and -1 in the history
  and in every list; the done flags; the same bits on a second run.
* ``generate()`` on the tiny random model of test_decode_step_gpu.py with the switch on: the fused loops return the ids and the
  width of the per-launch loop, the outputs have the properties the processors promise, an fp32 model on the per-launch loop
  equals a loop that applies the transformers classes step by step, rows of 17 take the kernel too.
* without the switch nothing changes and ``ops.decode_process`` is not called.
"""
import pytest
import torch

from test_decode_process_host import hf_chain
from test_decode_step_gpu import _lm, _prompt, _spies, clean_env as _step_clean_env  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

SENT = 12345.0
NINF = float("-inf")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


@pytest.fixture()
def clean_env(_step_clean_env):
    for name in ("CAMBRIAN_AMD_DECODE_PROCESS", "CAMBRIAN_AMD_DECODE_SAMPLE", "CAMBRIAN_AMD_DECODE_BEAM"):
        _step_clean_env.delenv(name, raising=False)
    return _step_clean_env


def _mods():
    from cambrian_amd import ops
    from cambrian_amd.model.language_model import processors as P
    return ops, P


def _bits(t):
    return t.contiguous().view(torch.int32)


def _values(dev, B, V, gen):
    vals = torch.randn(B, V, generator=gen) * 3
    vals[torch.rand(B, V, generator=gen) < 0.02] = NINF
    vals[:, 0::97] = 0.0
    vals[:, 5::97] = -0.0
    vals[:, 11::97] = float("inf")
    return vals.to(dev)


def _rows(vals, ld):
    """(the whole buffer, logits [B, V] as a view of it): rows of ``ld`` floats that start one float past the allocation, so
    off a 16-byte boundary for most rows; everything outside the view holds the sentinel."""
    B, V = vals.shape
    buf = torch.full((B * ld + 8,), SENT, dtype=torch.float32, device=vals.device)
    logits = buf[1:1 + B * ld].view(B, ld)[:, :V]
    logits.copy_(vals)
    return buf, logits


def _specs(P, symbols, h0, n, V, outside):
    """The parameter combinations for one history: every processor alone, on and off values, and everything together.  ``h0``:
    row 0's history, from which the words and eos ids that are sure to match are taken."""
    s = [int(i) for i in symbols]
    last = int(h0[n - 1]) if n else s[0]
    tail2 = [int(i) for i in h0[max(n - 2, 0):n]]
    tail3 = [int(i) for i in h0[max(n - 3, 0):n]]
    extra = [V + 3, -1] if outside else []
    words = [[s[1]], tail2 + [s[2]], tail3 + [s[3]], [s[0], s[1], s[2], s[4]], [last, s[3]]]
    words = [w for w in words if len(w) >= 2] + ([[V + 3, s[2]], [last, V + 3]] if outside else [])
    return [
        P.ProcessSpec(penalty=1.3), P.ProcessSpec(penalty=0.8, ngram=1), P.ProcessSpec(ngram=2), P.ProcessSpec(ngram=3, penalty=1.3),
        P.ProcessSpec(min_new=n + 1, eos=[s[2]] + extra), P.ProcessSpec(min_new=0, eos=[s[4], last]),
        P.ProcessSpec(words=words, bans=[s[1]] + extra), P.ProcessSpec(bans=[s[0], s[3], V - 1, 0] + extra),
        P.ProcessSpec(penalty=1.3, ngram=2, min_new=n + 5, eos=[s[3], last, s[0]] + extra, bans=[s[4], V - 1] + extra, words=words),
        P.ProcessSpec(penalty=0.8, ngram=3, min_new=n, eos=extra + [last], words=words),
    ]


@pytest.mark.parametrize("V,ld", [(1000, 1011), (32064, 32072), (128256, 128264)])
@pytest.mark.parametrize("B", [1, 3, 16, 17])
def test_kernel_equals_apply_torch_bit_for_bit(dev, B, V, ld):
    ops, P = _mods()
    gen = torch.Generator().manual_seed(B * 7 + V)
    assert ld >= V + 4, "the sentinel columns must reach past V + 3"
    vals = _values(dev, B, V, gen)
    seen = dict(penalised=0, banned=0, done=0)
    # ids V + 3 and -1 in the history and in every list: at the smallest and at the largest shape, on the long histories
    lengths = [(n, False) for n in (0, 1, 2, 3, 37, 1500)] + ([(37, True), (1500, True)] if (B, V) in ((3, 1000), (17, 128256)) else [])
    for n, outside in lengths:
        n_sym = 5 + (n * 7 + B) % 36                                       # 5 .. 40 symbols
        symbols = torch.randperm(V, generator=gen)[:n_sym]
        if outside:
            symbols = torch.cat([symbols[:-2], torch.tensor([V + 3, -1])])
        hist_full = torch.full((B, n + 3), -7, dtype=torch.int64)
        hist_full[:, :n] = symbols[torch.randint(0, n_sym, (B, n), generator=gen)]
        if n >= 2 and B > 1:
            hist_full[1, n - 1] = hist_full[0, n - 1]                      # a second row that ends as row 0 does
        hist = hist_full.to(dev)
        for spec in _specs(P, symbols[:5].tolist(), hist_full[0], n, V, outside):
            spec.penalty = float(torch.tensor(spec.penalty, dtype=torch.float32))
            proc = ops.DecodeProcess(spec, dev)
            buf, logits = _rows(vals, ld)
            before = buf.clone()
            ref_buf = buf.clone()
            ref = ref_buf[1:1 + B * ld].view(B, ld)[:, :V]
            done = torch.full((B,), 5, dtype=torch.uint8, device=dev)
            P.apply_torch(ref, hist, n, spec)
            ops.decode_process(logits, hist if n else None, n, proc, done)
            torch.cuda.synchronize()
            what = (n, spec)
            assert torch.equal(_bits(buf), _bits(ref_buf)), what          # the rows, and every sentinel in and around them
            again = before.clone()
            ops.decode_process(again[1:1 + B * ld].view(B, ld)[:, :V], hist, n, proc, None)
            assert torch.equal(_bits(again), _bits(buf)), what
            want_done = torch.full((B,), 5, dtype=torch.uint8)
            if spec.eos and n >= 1:
                want_done[torch.isin(hist_full[:, n - 1], torch.tensor(spec.eos))] = 1
            assert torch.equal(done.cpu(), want_done), what
            changed = (_bits(buf) != _bits(before))
            seen["banned"] += int(bool(((buf == NINF) & changed).any()))
            seen["penalised"] += int(bool((torch.isfinite(buf) & changed).any()))
            seen["done"] += int(bool((want_done == 1).any()))
    assert all(v >= 8 for v in seen.values()), seen


def test_unaligned_rows_and_layout_assumptions(dev):
    """The V = 1000 case really has rows off a 16-byte boundary, and a history wider than the workgroup."""
    buf, logits = _rows(_values(dev, 3, 1000, torch.Generator().manual_seed(0)), 1011)
    assert [logits[b].data_ptr() % 16 for b in range(3)] == [4, 0, 12] and logits.stride(0) == 1011
    assert 1500 > 1024


# ---------------------------------------------------------------------------------------------------------------------
# generate()
# ---------------------------------------------------------------------------------------------------------------------
def _proc_spy(monkeypatch, calls):
    ops, _ = _mods()
    calls["process"] = 0
    real = ops.decode_process

    def counted(*a, **kw):
        calls["process"] += 1
        return real(*a, **kw)

    monkeypatch.setattr(ops, "decode_process", counted)
    return calls


def _gen(model, env, calls, step, ids, att, **kw):
    env.setenv("CAMBRIAN_AMD_DECODE_STEP", step)
    for k in calls:
        calls[k] = 0
    out = model.generate(ids, attention_mask=att, **kw)
    torch.cuda.synchronize()
    return out, dict(calls)


def _bigrams_repeat(row):
    pairs = list(zip(row[:-1], row[1:]))
    return len(pairs) != len(set(pairs))


def _contains(row, word):
    return any(row[i:i + len(word)] == word for i in range(len(row) - len(word) + 1))


def test_generate_fused_greedy_equals_the_per_launch_loop(dev, clean_env):
    model = _lm(dev)
    calls = _proc_spy(clean_env, _spies(clean_env))
    ids, att = _prompt(dev, 3)
    new = 20
    plain, n_plain = _gen(model, clean_env, calls, "0", ids, att, max_new_tokens=new)
    assert n_plain["process"] == 0
    clean_env.setenv("CAMBRIAN_AMD_DECODE_PROCESS", "1")
    rows = plain.tolist()
    early = rows[0][1]                                   # an id row 0 emits at column 1
    word = rows[1][3:5]
    assert any(_bigrams_repeat(r) for r in rows), "the plain output repeats no bigram: the n-gram case would show nothing"
    free = sorted(set(range(1, 64)) - set(sum(rows, [])))[0]                 # an id the plain run never emits
    second = rows[2][4]
    cases = dict(penalty=dict(repetition_penalty=1.3), ngram=dict(no_repeat_ngram_size=2),
                 min_len=dict(min_new_tokens=6, eos_token_id=early), eos_list=dict(eos_token_id=[free, second]),
                 word=dict(bad_words_ids=[word]))
    for name, kw in cases.items():
        off, n_off = _gen(model, clean_env, calls, "0", ids, att, max_new_tokens=new, **kw)
        on, n_on = _gen(model, clean_env, calls, "1", ids, att, max_new_tokens=new, **kw)
        assert on.shape == off.shape and torch.equal(on, off), (name, on.tolist(), off.tolist())
        assert n_off["process"] == off.shape[1] and n_off["step"] == 0 and n_off["next"] == 0, (name, n_off)
        assert n_on["process"] == n_on["next"] == n_on["step"] + 1 and n_on["linear"] == 0, (name, n_on)
        got = on.tolist()
        if name == "penalty":
            assert not torch.equal(on, plain), "the penalty changed no token: the case shows nothing"
        if name == "ngram":
            assert not any(_bigrams_repeat(r) for r in got)
        if name == "min_len":
            assert all(early not in r[:6] for r in got) and on.shape[1] >= 6
            assert early in rows[0][:6], "the plain run does not emit the eos early"
        if name == "eos_list":
            c = got[2].index(second)
            assert free not in got[2][:c] and all(t == free for t in got[2][c + 1:]), got[2]      # after a secondary eos: eos[0]
        if name == "word":
            assert _contains(rows[1], word) and not any(_contains(r, word) for r in got)
    # one row that ends on the secondary eos between two polls: the width is the per-launch loop's
    ids1, att1 = _prompt(dev, 1)
    seq = _gen(model, clean_env, calls, "0", ids1, att1, max_new_tokens=new)[0][0].tolist()
    col = [c for c in range(1, new - 1) if seq.index(seq[c]) == c and (c + 1) % 8 != 0][0]
    kw = dict(max_new_tokens=new, eos_token_id=[free, seq[col]])
    off, _ = _gen(model, clean_env, calls, "0", ids1, att1, **kw)
    on, _ = _gen(model, clean_env, calls, "1", ids1, att1, **kw)
    assert off.shape == (1, col + 1) and torch.equal(on, off), (on.tolist(), off.tolist())


def test_generate_fp32_per_launch_loop_equals_the_hf_classes(dev, clean_env):
    """The per-launch loop of an fp32 model twice: once with the kernel, once with the transformers classes applied to the
    model's logits in the kernel's place at every step (``ops.decode_process`` replaced for that run, so both runs see logits
    from the same decode path and no rounding difference between a cached step and a full forward can flip an argmax)."""
    pytest.importorskip("transformers")
    model = _lm(dev, dt=torch.float32)
    clean_env.setenv("CAMBRIAN_AMD_DECODE_PROCESS", "1")
    clean_env.setenv("CAMBRIAN_AMD_DECODE_STEP", "0")
    ops, _ = _mods()
    ids, att = _prompt(dev, 3)
    new = 16
    seen = dict(kernel=0, hf=0)
    real = ops.decode_process

    def counted(*a, **k):
        seen["kernel"] += 1
        return real(*a, **k)

    def by_hf(chain, logits, hist, n):
        seen["hf"] += 1
        logits.copy_(chain(hist[:, :n].clone(), logits.clone()))
        return logits

    clean_env.setattr(ops, "decode_process", counted)
    plain = model.generate(ids, attention_mask=att, max_new_tokens=new).tolist()
    assert seen["kernel"] == 0
    word = plain[0][2:4]
    for kw, hf in ((dict(repetition_penalty=1.3), dict(penalty=1.3)), (dict(no_repeat_ngram_size=2), dict(ngram=2)),
                   (dict(min_new_tokens=6, eos_token_id=plain[0][1]), dict(min_new=6, eos=[plain[0][1]])),
                   (dict(bad_words_ids=[word, [plain[1][0]]], suppress_tokens=[plain[2][0]], repetition_penalty=0.8),
                    dict(bad_words=[word, [plain[1][0]]], suppress=[plain[2][0]], penalty=0.8))):
        got = model.generate(ids, attention_mask=att, max_new_tokens=new, **kw)
        torch.cuda.synchronize()
        assert seen["kernel"] == got.shape[1] and seen["hf"] == 0
        # the same loop over the same logits, the transformers classes in the kernel's place at every step
        chain = hf_chain(device=dev, **hf)
        clean_env.setattr(ops, "decode_process", lambda logits, hist, n, proc, done=None: by_hf(chain, logits, hist, n))
        out = model.generate(ids, attention_mask=att, max_new_tokens=new, **kw)
        clean_env.setattr(ops, "decode_process", counted)
        assert seen["hf"] == out.shape[1]
        seen.update(kernel=0, hf=0)
        assert got.shape == out.shape and torch.equal(got, out), (kw, got.tolist(), out.tolist())
        if "min_new_tokens" in kw or "suppress_tokens" in kw:          # these forbid a token the plain run emits
            assert got.tolist() != plain, kw


def test_generate_sample_fused_respects_the_processors(dev, clean_env):
    model = _lm(dev)
    calls = _proc_spy(clean_env, _spies(clean_env))
    clean_env.setenv("CAMBRIAN_AMD_DECODE_PROCESS", "1")
    clean_env.setenv("CAMBRIAN_AMD_DECODE_SAMPLE", "1")
    ids, att = _prompt(dev, 3)
    new = 24
    kw = dict(max_new_tokens=new, do_sample=True, temperature=1.5, top_k=8)
    torch.manual_seed(5)
    free, _ = _gen(model, clean_env, calls, "1", ids, att, **kw)
    common = max(range(64), key=lambda t: sum(r.count(t) for r in free.tolist()))
    torch.manual_seed(5)
    got, n = _gen(model, clean_env, calls, "1", ids, att, no_repeat_ngram_size=2, suppress_tokens=[common, 3], **kw)
    assert n["process"] == new and n["step"] == new - 1 and n["next"] == 0 and n["linear"] == 0, n
    assert got.shape == (3, new)
    for r in got.tolist():
        assert not _bigrams_repeat(r) and common not in r and 3 not in r, r
    assert any(common in r for r in free.tolist())


def test_rows_of_17_take_the_kernel_on_the_per_launch_loop(dev, clean_env):
    model = _lm(dev)
    calls = _proc_spy(clean_env, _spies(clean_env))
    clean_env.setenv("CAMBRIAN_AMD_DECODE_PROCESS", "1")
    ids, att = _prompt(dev, 17)
    new = 12
    for step in ("0", "1"):
        got, n = _gen(model, clean_env, calls, step, ids, att, max_new_tokens=new, no_repeat_ngram_size=2, repetition_penalty=1.2)
        assert got.shape == (17, new) and n["process"] == new and n["step"] == 0 and n["next"] == 0, n
        assert not any(_bigrams_repeat(r) for r in got.tolist())


def test_without_the_switch_nothing_changes(dev, clean_env):
    model = _lm(dev)
    calls = _proc_spy(clean_env, _spies(clean_env))
    ids, att = _prompt(dev, 3)
    new, layers = 12, len(model.model.layers)
    outs = {}
    for step in ("0", "1"):
        for kw in (dict(), dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, bad_words_ids=None, suppress_tokens=None)):
            for sample in (False, True):
                torch.manual_seed(21)
                extra = dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9) if sample else {}
                got, n = _gen(model, clean_env, calls, step, ids, att, max_new_tokens=new, **extra, **kw)
                assert n["process"] == 0, n
                if step == "0":
                    assert n["step"] == 0 and n["next"] == 0 and n["linear"] == (new - 1) * (4 * layers + 1), n
                else:
                    assert n["step"] == new - 1 and n["next"] == (0 if sample else new) and n["linear"] == 0, n
                outs.setdefault(sample, []).append(got)
    for sample, group in outs.items():
        assert all(torch.equal(o, group[0]) for o in group), sample
    # the switch on and every argument off: still no call, and the same ids
    clean_env.setenv("CAMBRIAN_AMD_DECODE_PROCESS", "1")
    got, n = _gen(model, clean_env, calls, "1", ids, att, max_new_tokens=new, repetition_penalty=1.0, eos_token_id=None)
    assert n["process"] == 0 and torch.equal(got, outs[False][0])
