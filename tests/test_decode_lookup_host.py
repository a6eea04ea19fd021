"""CPU: host side of prompt-lookup decoding — ``lookup.ngram_draft`` against transformers' ``PromptLookupCandidateGenerator``,
``lookup.accept``, the argument rules of ``generate(prompt_lookup_num_tokens=...)`` (checked before the model is touched, so
``self=None`` reaches them), and the symbols, bindings, plan and host-side argument checks of ``cmb_decode_attn_multi``.  No
kernel is launched: every library call below returns from the host-side checks, on pointers that are never dereferenced."""
import ctypes as C
import os
import random
import re

import pytest
import torch

from cambrian_amd.model.language_model.cambrian_llama import _generate
from cambrian_amd.model.language_model.lookup import accept, ngram_draft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cmb_decode_attn_multi", "cmb_decode_attn_multi_ws", "cmb_decode_attn_multi_plan")
OK, BAD_ARG, ALIGNMENT = 0, -1, -2


# ---------------------------------------------------------------------------------------------------------------------
# drafting and acceptance
# ---------------------------------------------------------------------------------------------------------------------
def test_ngram_draft_equals_hf_candidate_generator():
    pytest.importorskip("transformers")
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    rng = random.Random(7)
    hits = 0
    for case in range(200):
        n = rng.randint(2, 40)
        seq = [rng.randrange(6) for _ in range(n)]
        for num in (1, 4, 15):
            for ngram in (1, 2, 3):
                for eos in (None, rng.randrange(6)):
                    gen = PromptLookupCandidateGenerator(eos_token_id=None if eos is None else torch.tensor([eos]),
                                                         num_output_tokens=num, max_matching_ngram_size=ngram, max_length=10 ** 6)
                    cand, _ = gen.get_candidates(torch.tensor([seq]))
                    want = cand[0, n:].tolist()
                    got = ngram_draft(seq, num, ngram, 6, eos)
                    assert got == want, (seq, num, ngram, eos, got, want)
                    hits += bool(want)
    assert hits > 1000, "the random sequences produced too few drafts to compare"


def test_ngram_draft_cuts_at_ids_outside_the_vocabulary():
    # the leftmost match of the last id (5) is at index 0; its continuation runs into the image placeholder
    seq = [5, 1, 2, -200, 3, 4, 5]
    assert ngram_draft(seq, 4, 1, 64) == [1, 2]
    assert ngram_draft([5, -200, 7, 5], 4, 1, 64) == []                # nothing before the cut: no second match is tried (HF's eos rule)
    assert ngram_draft([5, 1, 70, 2, 5], 4, 1, 64) == [1]              # ids >= vocab too
    assert ngram_draft([5, 1, 63, 2, 5], 4, 1, 64) == [1, 63, 2, 5]
    assert ngram_draft([5, 1, 9, 2, 5], 4, 1, 64, eos=9) == [1]
    assert ngram_draft([5, 1, 9, 2, 5], 2, 1, 64) == [1, 9]            # at most num_tokens
    assert ngram_draft([1, 2, 3], 4, 2, 64) == [] and ngram_draft([4], 4, 2, 64) == [] and ngram_draft([], 4, 2, 64) == []
    assert ngram_draft([1, 2, 1, 2], 0, 2, 64) == []
    # the longest n-gram first, the leftmost match of it
    assert ngram_draft([1, 2, 7, 9, 2, 8, 1, 2], 1, 2, 64) == [7] and ngram_draft([1, 2, 7, 9, 2, 8, 1, 2], 1, 1, 64) == [7]
    assert ngram_draft([3, 2, 7, 9, 2, 8, 1, 2], 1, 2, 64) == [7] and ngram_draft([9, 2, 7, 1, 2, 8, 1, 2], 1, 2, 64) == [8]


def test_accept_counts_leading_agreement():
    assert accept([4, 5, 6], [9, 5, 6, 1]) == 0
    assert accept([4, 5, 6], [4, 5, 7, 1]) == 2
    assert accept([4, 5, 6], [4, 5, 6, 1]) == 3
    assert accept([4, 5, 6], [4, 9, 6, 1]) == 1                        # a later agreement does not count
    assert accept([], [3]) == 0
    assert accept([4], torch.tensor([4, 2])) == 1


# ---------------------------------------------------------------------------------------------------------------------
# generate()'s argument rules
# ---------------------------------------------------------------------------------------------------------------------
def test_generate_checks_the_lookup_arguments_before_the_model(monkeypatch):
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_KV_FP8", raising=False)
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_BEAM", raising=False)
    one = torch.zeros(1, 4, dtype=torch.long)
    for bad in (-1, 16, 100, 2.5, True):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
            _generate(None, one, prompt_lookup_num_tokens=bad)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match="max_matching_ngram_size"):
            _generate(None, one, prompt_lookup_num_tokens=4, max_matching_ngram_size=bad)
    with pytest.raises(ValueError, match="batch size 1"):
        _generate(None, torch.zeros(2, 4, dtype=torch.long), prompt_lookup_num_tokens=4)
    with pytest.raises(NotImplementedError, match="greedy only"):
        _generate(None, one, prompt_lookup_num_tokens=4, do_sample=True, temperature=0.7)
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_BEAM", "1")
    with pytest.raises(NotImplementedError, match="beam search"):
        _generate(None, one, prompt_lookup_num_tokens=4, num_beams=3)
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_KV_FP8", "1")
    with pytest.raises(NotImplementedError, match="e4m3 K / V cache"):
        _generate(None, one, prompt_lookup_num_tokens=4)
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_KV_FP8")
    # a legal set passes the rules and reaches the model (None has none); so do "off" and do_sample at temperature 0
    for kw in (dict(prompt_lookup_num_tokens=1), dict(prompt_lookup_num_tokens=15, max_matching_ngram_size=5),
               dict(prompt_lookup_num_tokens=4, do_sample=True, temperature=0.0), dict(prompt_lookup_num_tokens=None),
               dict(prompt_lookup_num_tokens=0)):
        with pytest.raises(AttributeError):
            _generate(None, one, **kw)
    # an unknown keyword is still rejected first
    with pytest.raises(ValueError, match="penalty_alpha"):
        _generate(None, one, prompt_lookup_num_tokens=4, penalty_alpha=0.6)


# ---------------------------------------------------------------------------------------------------------------------
# header / ABI / host-side checks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cambrian_amd import lib
    return lib


def _aligned(nbytes=256):
    raw = (C.c_char * (nbytes + 16))()
    return raw, (C.addressof(raw) + 15) & ~15


def test_symbols_are_declared_exported_and_bound(built):
    text = open(os.path.join(ROOT, "include", "cambrian_amd.h")).read()
    lib = built.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in the header"
        assert name in built.SIGNATURES
        assert getattr(lib, name).argtypes == built.SIGNATURES[name][1]       # resolves: the symbol left the library
        assert name in text[text.index("ABI revision"):text.index("#define CMB_ABI_VERSION")]
    assert built.ABI_VERSION == 13 == lib.cmb_abi_version()
    mk = open(os.path.join(ROOT, "cambrian_amd", "csrc", "Makefile")).read()
    assert "decode_attn_multi.hip" in mk
    # the C declaration and the binding have the same number of arguments
    for name in NAMES:
        decl = re.search(r"\b%s\s*\((.*?)\);" % name, text, re.S).group(1)
        assert len(decl.split(",")) == len(built.SIGNATURES[name][1]), name


def test_supported_geometries_and_rows(built):
    from cambrian_amd import ops
    bf = torch.bfloat16
    assert ops.DECODE_LOOKUP_MAX_ROWS == 16
    for nh, nkv, hd, Q in ((32, 8, 128, 16), (56, 8, 128, 9), (32, 32, 96, 16), (4, 2, 64, 1), (8, 1, 128, 8)):
        assert ops.decode_attention_multi_supported(bf, nh, nkv, hd, Q)
        assert not ops.decode_attention_multi_supported(torch.float32, nh, nkv, hd, Q)      # bf16 only
    assert not ops.decode_attention_multi_supported(bf, 32, 8, 128, 17) and not ops.decode_attention_multi_supported(bf, 32, 8, 128, 0)
    assert not ops.decode_attention_multi_supported(bf, 56, 8, 128, 10)       # 70 rows
    assert not ops.decode_attention_multi_supported(bf, 8, 1, 128, 9)         # 72 rows
    assert not ops.decode_attention_multi_supported(bf, 32, 8, 80, 4) and not ops.decode_attention_multi_supported(bf, 9, 1, 128, 2)


def test_plan_is_the_single_token_plan_over_all_slots(built):
    from cambrian_amd import ops
    for B, nkv, t0, Q in ((1, 8, 2047, 16), (1, 8, 0, 1), (2, 2, 1026, 5), (1, 1, 100, 4), (16, 8, 8000, 2)):
        for forced in (0, 1, 3, 64):
            s, ch = ops.decode_attention_multi_plan(B, nkv, t0, Q, forced)
            assert (s, ch) == ops.decode_attention_plan(B, nkv, t0 + Q - 1, forced)
            assert s * ch >= t0 + Q > (s - 1) * ch
    lib = built.load()
    assert lib.cmb_decode_attn_multi_plan(1, 8, 10, 0, 0, None, None, None) == BAD_ARG
    assert lib.cmb_decode_attn_multi_plan(1, 8, 10, 17, 0, None, None, None) == BAD_ARG
    assert lib.cmb_decode_attn_multi_plan(1, 8, -1, 4, 0, None, None, None) == BAD_ARG
    assert lib.cmb_decode_attn_multi_ws(2, 8, 2, 128, 5, 1026, 1) == 0
    assert lib.cmb_decode_attn_multi_ws(2, 8, 2, 128, 5, 1026, 3) == 2 * 5 * 8 * 3 * 130
    assert lib.cmb_decode_attn_multi_ws(2, 8, 1, 128, 9, 1026, 3) == BAD_ARG       # 72 rows


def test_rejects_bad_arguments_before_any_launch(built):
    lib = built.load()
    keep, p = _aligned()

    def call(q=p, k=p, v=p, cos=p, sin=p, kc=p, vc=p, c_sb=1 << 20, c_sh=1 << 18, c_st=128, B=2, nh=8, nkv=2, hd=128, Q=5,
             t0=1026, kvalid=p, kv_ld=2048, splits=2, ws=p, ws_floats=1 << 30, out=p, q_ld=2048):
        return lib.cmb_decode_attn_multi(q, q_ld, k, 2048, v, 2048, cos, sin, kc, vc, c_sb, c_sh, c_st, B, nh, nkv, hd, Q, t0,
                                         kvalid, kv_ld, 0.088, splits, ws, ws_floats, out, None)

    for name in ("q", "k", "v", "cos", "sin", "kc", "vc", "kvalid", "out"):
        assert call(**{name: None}) == BAD_ARG, f"NULL {name}"
    assert call(ws=None) == BAD_ARG                                     # split run without a workspace
    for hd in (0, 32, 80, 256):
        assert call(hd=hd) == BAD_ARG, hd
    assert call(nh=9, nkv=1) == BAD_ARG and call(nh=7, nkv=2) == BAD_ARG
    assert call(Q=0) == BAD_ARG and call(Q=17) == BAD_ARG and call(Q=-3) == BAD_ARG
    assert call(nh=16, Q=9) == BAD_ARG                                  # 8 heads per group x 9 tokens = 72 rows
    assert call(t0=-1) == BAD_ARG
    assert call(kv_ld=1030) == BAD_ARG                                  # the mask row is shorter than t0 + Q
    assert call(B=65536) == BAD_ARG and call(nkv=65536, nh=65536) == BAD_ARG
    need = lib.cmb_decode_attn_multi_ws(2, 8, 2, 128, 5, 1026, 2)
    assert need > 0 and call(ws_floats=need - 1) == BAD_ARG             # one float short
    assert call(splits=-1) == BAD_ARG and call(splits=10 ** 6) == BAD_ARG
    # a bad argument is reported before a bad alignment (cmb_decode_attn's order)
    assert call(q=p + 8, t0=-1) == BAD_ARG and call(q=p + 8, ws_floats=need - 1) == BAD_ARG
    assert call(c_st=132) == ALIGNMENT and call(c_sh=(1 << 18) + 4) == ALIGNMENT and call(c_sb=(1 << 20) + 4) == ALIGNMENT
    for name in ("q", "k", "v", "kc", "vc", "out"):
        assert call(**{name: p + 8}) == ALIGNMENT, name
    assert call(q_ld=2052) == ALIGNMENT
    assert call(B=0) == OK and call(B=0, ws=None, ws_floats=0) == OK    # B == 0 is a no-op
