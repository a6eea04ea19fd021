"""CPU: the host side of the logits processors of ``generate()`` (``cmb_decode_process``).

* ``processors.apply_torch`` against the five transformers classes chained in HF's order, bit for bit, on random cases (small
  alphabets so that ids and n-grams repeat, ``-inf`` entries, penalties 1.3 and 0.8, n-gram sizes 0..4, words of 1..4 ids) and on
  targeted ones.  tests/test_decode_process_gpu.py imports ``hf_chain``.
* the argument rules of ``generate()`` with the switch off and on, all with ``self=None``: they are checked before the model is
  touched.
* the symbol is declared, exported and bound; the entry point's argument checks return before any launch, on pointers that
  are never dereferenced.
"""
import ctypes as C
import os
import random
import re

import pytest
import torch

from cambrian_amd.model.language_model import processors as P
from cambrian_amd.model.language_model.cambrian_llama import _generate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, ALIGNMENT = 0, -1, -2
NINF = float("-inf")


def hf_chain(penalty=1.0, ngram=0, min_new=0, eos=None, bad_words=None, suppress=None, device="cpu"):
    """HF's processors for these arguments in the order GenerationMixin builds them, as one callable
    ``(ids [B, n] int64, scores [B, V] fp32) -> scores``."""
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, NoBadWordsLogitsProcessor,
                                                        NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                                                        SuppressTokensLogitsProcessor)
    chain = []
    if penalty != 1.0:
        chain.append(RepetitionPenaltyLogitsProcessor(penalty=penalty))
    if ngram > 0:
        chain.append(NoRepeatNGramLogitsProcessor(ngram))
    # (HF's class refuses to be built when dropping the words that are one eos id leaves none; it is handed the full list)
    if bad_words and any(not (len(w) == 1 and w[0] in (eos or [])) for w in bad_words):
        chain.append(NoBadWordsLogitsProcessor(bad_words, eos))
    if min_new > 0 and eos:
        chain.append(MinNewTokensLengthLogitsProcessor(0, min_new, eos, device=device))
    if suppress:
        chain.append(SuppressTokensLogitsProcessor(suppress, device=device))

    def run(ids, scores):
        for proc in chain:
            scores = proc(ids, scores)
        return scores
    return run


def _bits(t):
    return t.contiguous().view(torch.int32)


def _spec(**kw):
    return P.parse(True, kw.pop("eos", None), kw.pop("penalty", None), kw.pop("ngram", None), kw.pop("min_new", None),
                   kw.pop("bad_words", None), kw.pop("suppress", None)) or P.ProcessSpec()


def _both(logits, hist, n, **kw):
    """(apply_torch's result, HF's result) on clones."""
    pytest.importorskip("transformers")
    spec = _spec(**dict(kw))
    got = P.apply_torch(logits.clone(), hist, n, spec)
    want = hf_chain(penalty=kw.get("penalty") or 1.0, ngram=kw.get("ngram") or 0, min_new=kw.get("min_new") or 0,
                    eos=P.eos_list(kw.get("eos")), bad_words=kw.get("bad_words"), suppress=kw.get("suppress"))(
        hist[:, :n].clone(), logits.clone())
    return got, want


def test_apply_torch_equals_the_hf_chain_on_random_cases():
    pytest.importorskip("transformers")
    rng = random.Random(5)
    g = torch.Generator().manual_seed(5)
    seen = dict(penalised=0, ngram_ban=0, word_ban=0, min_len=0)
    for case in range(400):
        V = rng.choice((5, 8, 13, 40))
        B = rng.randint(1, 3)
        n = rng.randint(0, 12)
        alphabet = rng.randint(2, min(V, 6))
        hist = torch.randint(0, alphabet, (B, 14), generator=g)
        logits = torch.randn(B, V, generator=g) * 3
        logits[torch.rand(B, V, generator=g) < 0.1] = NINF
        kw = dict(penalty=rng.choice((None, 1.0, 1.3, 0.8)), ngram=rng.choice((None, 0, 1, 2, 3, 4)),
                  min_new=rng.choice((None, 0, 3, 20)), eos=rng.choice((None, rng.randrange(V), [rng.randrange(V), rng.randrange(V)])),
                  suppress=rng.choice((None, [rng.randrange(V)], [rng.randrange(V), rng.randrange(V)])))
        if rng.random() < 0.7:
            kw["bad_words"] = [[rng.randrange(alphabet) for _ in range(rng.randint(1, 4))] for _ in range(rng.randint(1, 4))]
        got, want = _both(logits, hist, n, **kw)
        assert torch.equal(_bits(got), _bits(want)), (case, kw, n, hist[:, :n].tolist())
        spec = _spec(**dict(kw))
        seen["penalised"] += int(spec.penalty != 1.0 and n > 0)
        seen["ngram_ban"] += int(spec.ngram > 1 and bool(((got == NINF) & (logits != NINF)).any()))
        seen["word_ban"] += int(bool(spec.words) and n >= 2)
        seen["min_len"] += int(bool(spec.eos) and n < spec.min_new)
    assert all(v > 20 for v in seen.values()), seen


def test_empty_history_and_the_ngram_threshold():
    V = 9
    logits = torch.arange(V, dtype=torch.float32)[None] - 4
    hist = torch.tensor([[1, 2, 1, 2, 1, 2, 1]])
    got, want = _both(logits, hist, 0, penalty=1.3, ngram=2, bad_words=[[1, 2]], suppress=[7], eos=3, min_new=1)
    assert torch.equal(_bits(got), _bits(want))
    assert (got == NINF)[0].nonzero()[:, 0].tolist() == [3, 7]                      # min length and the suppressed id only
    for hist in (hist, torch.full((1, 7), 3)):
        for g in (2, 3, 4):
            for n in (g - 2, g - 1, g):
                got, want = _both(logits, hist, n, ngram=g)
                assert torch.equal(_bits(got), _bits(want)), (g, n)
                banned = (got == NINF)[0].nonzero()[:, 0].tolist()
                # n = g - 2: the rule does not look; n = g - 1: it looks and finds no window; n = g: one window, which hits
                # iff it starts with the history's last g - 1 ids (the constant history: always)
                assert banned == ([3] if n == g and int(hist[0, 0]) == 3 else []), (g, n)
    got, want = _both(logits, torch.tensor([[5, 5, 1]]), 3, ngram=3)                  # 5 5 | 5 1: the window 5 5 1 starts with the tail 5 1? no
    assert torch.equal(_bits(got), _bits(want)) and not bool((got == NINF).any())
    got, want = _both(logits, torch.tensor([[5, 1, 7, 5, 1]]), 5, ngram=3)
    assert torch.equal(_bits(got), _bits(want)) and (got == NINF)[0].nonzero()[:, 0].tolist() == [7]


def test_ngram_of_one_bans_every_id_of_the_history():
    logits = torch.zeros(2, 6)
    hist = torch.tensor([[4, 4, 2, 0], [1, 1, 1, 5]])
    got, want = _both(logits, hist, 3, ngram=1)
    assert torch.equal(_bits(got), _bits(want))
    assert (got == NINF).tolist() == [[False, False, True, False, True, False], [False, True, False, False, False, False]]


def test_word_of_m_ids_bans_at_n_equal_m_not_before():
    logits = torch.zeros(1, 8)
    for m in (2, 3, 4):
        word = list(range(1, m + 1))                                 # 1 2 .. m
        prefix = word[:-1]
        hist = torch.tensor([prefix + [0] * 6])
        got, want = _both(logits, hist, m - 1, bad_words=[word])     # the history IS the prefix, but m <= n fails: HF bans nothing
        assert torch.equal(_bits(got), _bits(want)) and not bool((got == NINF).any()), m
        hist = torch.tensor([[6] + prefix + [0] * 5])
        got, want = _both(logits, hist, m, bad_words=[word])
        assert torch.equal(_bits(got), _bits(want)) and (got == NINF)[0].nonzero()[:, 0].tolist() == [m], m
        got, want = _both(logits, torch.tensor([[6] + prefix[::-1] + [0] * 5]), m, bad_words=[word])
        assert torch.equal(_bits(got), _bits(want)) and (bool((got == NINF).any()) is (m == 2)), m


def test_duplicate_id_is_penalised_once_and_special_values():
    inf = float("inf")
    logits = torch.tensor([[2.7, -2.7, inf, NINF, 0.0, -0.0, 1e-38, -3e38]])
    hist = torch.tensor([[0, 0, 1, 1, 1, 2, 3, 4, 5, 6, 7, 0]])
    for p in (1.3, 0.8):
        got, want = _both(logits, hist, 12, penalty=p)
        assert torch.equal(_bits(got), _bits(want)), p
        p32 = torch.tensor(p, dtype=torch.float32)
        once = torch.where(logits < 0, logits * p32, logits / p32)
        assert torch.equal(_bits(got), _bits(once)), "an id that occurs three times was not penalised exactly once"
        assert got[0, 2] == inf and got[0, 3] == NINF and _bits(got)[0, 4] == 0 and _bits(got)[0, 5] == -2 ** 31
    # a penalised id that is also banned ends at -inf; an untouched element keeps its bits
    got, want = _both(logits, hist, 2, penalty=1.3, ngram=1)
    assert torch.equal(_bits(got), _bits(want)) and got[0, 0] == NINF and torch.equal(_bits(got)[0, 1:], _bits(logits)[0, 1:])


def test_an_eos_id_that_is_also_a_bad_word():
    logits = torch.zeros(1, 6)
    hist = torch.tensor([[1, 2, 3]])
    spec = _spec(eos=[4, 5], bad_words=[[4], [5], [3], [2, 4]])
    assert spec.bans == [3] and spec.words == [[2, 4]] and spec.eos == [4, 5]       # [4] and [5] are dropped, as HF drops them
    got, want = _both(logits, hist, 3, eos=[4, 5], bad_words=[[4], [5], [3], [2, 4]])
    assert torch.equal(_bits(got), _bits(want)) and (got == NINF)[0].tolist() == [False, False, False, True, False, False]
    got, want = _both(logits, hist, 2, eos=[4, 5], bad_words=[[4], [5], [3], [2, 4]], min_new=3)
    assert torch.equal(_bits(got), _bits(want)) and (got == NINF)[0].tolist() == [False, False, False, True, True, True]


def test_ids_outside_the_vocabulary_match_but_never_index():
    V = 6
    logits = torch.zeros(1, V)
    hist = torch.tensor([[V + 3, 2, V + 3, -1, 2, V + 3]])
    spec = P.ProcessSpec(penalty=1.3, ngram=2, min_new=99, eos=[V + 3, 1], bans=[-1, V, 4], words=[[V + 3, 5], [2, V + 3]])
    got = P.apply_torch(logits - 1.0, hist, 6, spec)
    # bigram (V+3, 2) would repeat: 2 banned; the word (V+3, 5) ends the history on V+3: 5 banned; eos 1 (min length), ban 4
    assert (got == NINF)[0].tolist() == [False, True, True, False, True, True]
    assert got[0, 0] == -1.0 and got[0, 3] == -1.0
    done = torch.zeros(1, dtype=torch.bool)
    P.apply_torch(logits.clone(), hist, 6, spec, done)
    assert bool(done[0])                                              # the last id is in the set, though it has no column
    done = torch.zeros(1, dtype=torch.uint8)
    P.apply_torch(logits.clone(), hist, 5, spec, done)
    assert not bool(done[0])


def test_trim_for_an_eos_set():
    from cambrian_amd import ops
    ids = torch.tensor([[3, 9, 7, 7, 7, 7], [3, 4, 5, 8, 7, 7]])
    assert ops.trim_after_all_done_set(ids, [7, 9, 8]).tolist() == [[3, 9, 7, 7], [3, 4, 5, 8]]
    assert ops.trim_after_all_done_set(ids, [7]).shape == (2, 5) and ops.trim_after_all_done_set(ids, [1]).shape == (2, 6)
    assert ops.trim_after_all_done(ids, 7).shape == (2, 5)              # the single-id helper is what it was
    assert ops.trim_after_all_done_set(ids[:, :0], [7]).shape == (2, 0)


# ---------------------------------------------------------------------------------------------------------------------
# the argument rules of generate()
# ---------------------------------------------------------------------------------------------------------------------
ONE = torch.zeros(1, 4, dtype=torch.long)


def test_switch_resolution(monkeypatch):
    from cambrian_amd import ops
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_PROCESS", raising=False)
    assert ops.decode_process_enabled() is False and ops.decode_process_enabled(True) is True
    for value, flag, want in (("1", False, True), ("0", True, False), ("", True, True), ("", False, False)):
        monkeypatch.setenv("CAMBRIAN_AMD_DECODE_PROCESS", value)
        assert ops.decode_process_enabled(flag) is want, (value, flag)
    for value in ("yes", "2", "on"):
        monkeypatch.setenv("CAMBRIAN_AMD_DECODE_PROCESS", value)
        with pytest.raises(ValueError, match="CAMBRIAN_AMD_DECODE_PROCESS"):
            ops.decode_process_enabled()


def test_switched_off_every_call_behaves_as_before(monkeypatch):
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_PROCESS", raising=False)
    with pytest.raises(ValueError, match=r"unsupported argument repetition_penalty=1.3"):
        _generate(None, ONE, repetition_penalty=1.3)
    for kw in (dict(no_repeat_ngram_size=2), dict(min_new_tokens=3), dict(bad_words_ids=[[1, 2]]), dict(suppress_tokens=[1]),
               dict(eos_token_id=[1, 2]), dict(eos_token_id=[1])):
        with pytest.raises(ValueError, match="CAMBRIAN_AMD_DECODE_PROCESS=1") as e:
            _generate(None, ONE, **kw)
        assert next(iter(kw)) in str(e.value)
    # at their off values the new keywords are no-ops: the call gets past the argument rules and dies on the missing model
    with pytest.raises(AttributeError):
        _generate(None, ONE, no_repeat_ngram_size=0, min_new_tokens=0, bad_words_ids=None, suppress_tokens=None,
                  repetition_penalty=1.0, eos_token_id=3)
    with pytest.raises(AttributeError):
        _generate(None, ONE, no_repeat_ngram_size=None, min_new_tokens=None)
    with pytest.raises(ValueError, match="penalty_alpha"):
        _generate(None, ONE, no_repeat_ngram_size=2, penalty_alpha=0.6)          # an unknown keyword is still rejected first
    assert P.parse(False, 3) is None and P.parse(False, None, None, 0, 0, None, None) is None


def test_switched_on_the_values_are_validated_before_the_model(monkeypatch):
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_PROCESS", "1")
    for kw, match in ((dict(repetition_penalty=0.0), "strictly positive"), (dict(repetition_penalty=-1.0), "strictly positive"),
                      (dict(repetition_penalty=float("inf")), "strictly positive"), (dict(repetition_penalty="1.2"), "strictly positive"),
                      (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"), (dict(no_repeat_ngram_size=1.5), "no_repeat_ngram_size"),
                      (dict(min_new_tokens=-2), "min_new_tokens"), (dict(bad_words_ids=[]), "non-empty list"),
                      (dict(bad_words_ids=[3]), "list of lists"), (dict(bad_words_ids=[[]]), "non-negative"),
                      (dict(bad_words_ids=[[1, -2]]), "non-negative"), (dict(suppress_tokens=3), "suppress_tokens"),
                      (dict(eos_token_id=[]), "eos_token_id"), (dict(eos_token_id=[1, "a"]), "eos_token_id")):
        with pytest.raises(ValueError, match=match):
            _generate(None, ONE, **kw)
    with pytest.raises(ValueError, match="penalty_alpha"):
        _generate(None, ONE, repetition_penalty=1.3, penalty_alpha=0.6)
    # accepted: the call gets past the argument rules and dies on the missing model
    for kw in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=3, min_new_tokens=2, eos_token_id=[5, 6]),
               dict(bad_words_ids=[[1], [2, 3]], suppress_tokens=[4]), dict(eos_token_id=[7]), dict(repetition_penalty=1.0)):
        with pytest.raises(AttributeError):
            _generate(None, ONE, **kw)


def test_refused_combinations(monkeypatch):
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_PROCESS", "1")
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_BEAM", "1")
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_KV_FP8", raising=False)
    args = (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(min_new_tokens=2, eos_token_id=1),
            dict(bad_words_ids=[[1, 2]]), dict(suppress_tokens=[3]), dict(eos_token_id=[1, 2]))
    for kw in args:
        with pytest.raises(NotImplementedError, match="num_beams=3") as e:
            _generate(None, ONE, num_beams=3, **kw)
        assert "beam search" in str(e.value)
        with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens") as e:
            _generate(None, ONE, prompt_lookup_num_tokens=4, **kw)
        assert "logits processors" in str(e.value)
    # at their off values both modes go on to the model
    with pytest.raises(AttributeError):
        _generate(None, ONE, num_beams=3, repetition_penalty=1.0, no_repeat_ngram_size=0, eos_token_id=[4])
    with pytest.raises(AttributeError):
        _generate(None, ONE, prompt_lookup_num_tokens=4, min_new_tokens=0, eos_token_id=4)


def test_spec_and_its_lists():
    spec = P.parse(True, [9, 4, 9], 1.3, 3, 5, [[7], [1, 2, 3], [4], [5, 6]], [11, 12])
    assert (spec.ngram, spec.min_new, spec.eos, spec.bans, spec.words) == (3, 5, [9, 4], [11, 12, 7], [[1, 2, 3], [5, 6]])
    assert spec.penalty == float(torch.tensor(1.3, dtype=torch.float32)) and spec.active and spec.edits
    eos, bans, ids, off = spec.device_lists("cpu")
    assert eos.tolist() == [9, 4] and bans.tolist() == [11, 12, 7] and ids.tolist() == [1, 2, 3, 5, 6] and off.tolist() == [0, 3, 5]
    assert all(t.dtype == torch.int64 for t in (eos, bans, ids, off))
    assert P.parse(True, 5) is None and P.parse(True, [5]) is None and P.parse(True, None, 1.0, 0, 0) is None
    assert P.parse(True, None, None, None, 4) is None                   # a minimum length without an eos id changes nothing
    only_set = P.parse(True, [5, 6])
    assert only_set.active and not only_set.edits and only_set.device_lists("cpu")[1:] == (None, None, None)


# ---------------------------------------------------------------------------------------------------------------------
# header / ABI / host-side checks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cambrian_amd import lib
    return lib


def test_symbol_is_declared_exported_and_bound(built):
    text = open(os.path.join(ROOT, "include", "cambrian_amd.h")).read()
    name = "cmb_decode_process"
    lib = built.load()
    assert re.search(r"\b%s\s*\(" % name, text), "not declared in the header"
    assert name in built.SIGNATURES
    assert getattr(lib, name).argtypes == built.SIGNATURES[name][1]           # resolves: the symbol left the library
    assert name in text[text.index("ABI revision"):text.index("#define CMB_ABI_VERSION")]
    assert built.ABI_VERSION == lib.cmb_abi_version()
    assert "decode_process.hip" in open(os.path.join(ROOT, "cambrian_amd", "csrc", "Makefile")).read()
    decl = re.search(r"\b%s\s*\((.*?)\);" % name, text, re.S).group(1)
    assert len(decl.split(",")) == len(built.SIGNATURES[name][1])
    src = open(os.path.join(ROOT, "cambrian_amd", "csrc", "decode_process.hip")).read()
    assert '#include "decode_process_core.h"' in src                          # the header the CPU simulator compiles


def test_rejects_bad_arguments_before_any_launch(built):
    lib = built.load()
    raw = (C.c_char * 272)()
    p = (C.addressof(raw) + 15) & ~15

    def call(logits=p, ld=1011, B=3, V=1000, hist=p, hist_ld=40, n=37, penalty=1.3, ngram=3, min_new=0, eos=p, n_eos=2, bans=p,
             n_bans=2, ids=p, n_ids=5, off=p, n_words=2, done=p):
        return lib.cmb_decode_process(logits, ld, B, V, hist, hist_ld, n, penalty, ngram, min_new, eos, n_eos, bans, n_bans, ids,
                                      n_ids, off, n_words, done, None)

    assert call(logits=None) == BAD_ARG and call(hist=None) == BAD_ARG and call(eos=None) == BAD_ARG
    assert call(bans=None) == BAD_ARG and call(ids=None) == BAD_ARG and call(off=None) == BAD_ARG
    assert call(n_eos=-1) == BAD_ARG and call(n_bans=-1) == BAD_ARG and call(n_words=-1) == BAD_ARG and call(n=-1) == BAD_ARG
    assert call(n_ids=1) == BAD_ARG and call(n_ids=-1) == BAD_ARG           # fewer ids than words
    assert call(B=0) == BAD_ARG and call(B=-2) == BAD_ARG
    assert call(V=0) == BAD_ARG and call(V=2 ** 31, ld=2 ** 31) == BAD_ARG and call(ld=999) == BAD_ARG
    assert call(hist_ld=36) == BAD_ARG
    for bad in (0.0, -1.3, float("inf"), float("nan")):
        assert call(penalty=bad) == BAD_ARG, bad
    assert call(ngram=-1) == BAD_ARG and call(min_new=-1) == BAD_ARG
    # a bad argument is reported before a bad alignment
    assert call(logits=p + 2, ngram=-1) == BAD_ARG
    assert call(logits=p + 2) == ALIGNMENT
    for name in ("hist", "eos", "bans", "ids", "off"):
        assert call(**{name: p + 4}) == ALIGNMENT, name
