"""CPU: the beam-search restatement (cambrian_amd/model/language_model/beam.py) against HF's ``GenerationMixin._beam_search`` on a
random tiny ``LlamaForCausalLM`` — tokens equal, sequence scores within 1e-5 — and the argument rules of ``generate()`` around
the ``CAMBRIAN_AMD_DECODE_BEAM`` switch."""
import pytest
import torch

from cambrian_amd.model.language_model import beam as BM

PROMPT = 5


def tiny_hf_llama(seed: int, vocab: int = 97, scale: float = 4.0):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.LlamaConfig(vocab_size=vocab, hidden_size=32, intermediate_size=64, num_hidden_layers=2,
                                   num_attention_heads=2, num_key_value_heads=1, max_position_embeddings=64,
                                   tie_word_embeddings=False)
    torch.manual_seed(seed)
    model = transformers.LlamaForCausalLM(cfg).eval()
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(scale if p.dim() > 1 else 1.0)
    return model


def decision_gap(trace: dict, nb: int) -> float:
    """The smallest gap of any comparison of one ``beam_update`` that decided something (``trace`` as that function fills
    it), over all prompts: adjacent scores among the top K + 1 candidates, among the first num_beams + 1 running scores, among
    the first num_beams + 1 merged hypothesis scores, and the flag's comparison.  Exactly equal values are ordered by index on
    every implementation and the -1e9 markers (anything below -5e8) stand for "none": neither is a decision."""
    gaps = [float("inf")]
    for name, upto in (("cand", None), ("run", nb + 1), ("merged", nb + 1)):
        v = trace[name][:, :upto].double()
        hi, lo = v[:, :-1], v[:, 1:]
        d = (hi - lo)[(hi > -5e8) & (lo > -5e8) & (hi != lo) & torch.isfinite(lo)]
        gaps.append(float(d.min()) if d.numel() else float("inf"))
    best, worst = trace["flag"]
    d = (best.double() - worst.double()).abs()[trace["fin_ok"] & (worst > -5e8)]
    gaps.append(float(d.min()) if d.numel() else float("inf"))
    return min(gaps)


def drive_restatement(next_logits, B: int, nb: int, max_new: int, eos, fill: int, extra: int = 0):
    """The restatement around ``next_logits(run_ids [B * nb, s]) -> fp32 [B * nb, V]``; returns (tokens, score of slot 0,
    steps taken).  ``extra``: steps to run on after the stopping point (never past ``max_new``)."""
    st = BM.BeamState(B, nb, max_new)
    steps, over = 0, 0
    for s in range(max_new):
        logits = next_logits(st.run_ids.reshape(B * nb, max_new)[:, :s])
        BM.beam_update(st, logits, s, eos, s + 1 == max_new)
        steps = s + 1
        if BM.beam_done(st):
            if over == extra:
                break
            over += 1
    return BM.beam_result(st, fill), st.fin_score[:, 0].clone(), steps, st


def hf_case(model, prompts, nb, max_new, eos):
    out = model.generate(prompts, attention_mask=torch.ones_like(prompts), num_beams=nb, max_new_tokens=max_new, do_sample=False,
                         eos_token_id=eos, pad_token_id=0, length_penalty=1.0, early_stopping=False, num_return_sequences=1,
                         output_scores=True, return_dict_in_generate=True)
    return out.sequences[:, prompts.shape[1]:], out.sequences_scores


def model_logits(model, prompts, nb):
    rep = prompts.repeat_interleave(nb, dim=0)

    def f(run):
        with torch.no_grad():
            return model(torch.cat((rep, run), dim=1)).logits[:, -1].float()
    return f


@pytest.mark.parametrize("nb", [2, 3, 4, 8])
def test_restatement_equals_hf_beam_search(nb):
    model = tiny_hf_llama(100 + nb)
    gen = torch.Generator().manual_seed(7 * nb)
    with torch.no_grad():
        freq = model(torch.randint(1, 97, (8, PROMPT), generator=gen)).logits[:, -1].softmax(-1).mean(0)
    frequent = [int(i) for i in freq.topk(3).indices]
    early = 0
    for eos in [None] + frequent:
        for max_new in (1, 2, 9, 12):
            for B in (1, 2):
                prompts = torch.randint(1, 97, (B, PROMPT), generator=gen)
                want, want_s = hf_case(model, prompts, nb, max_new, eos)
                got, got_s, steps, st = drive_restatement(model_logits(model, prompts, nb), B, nb, max_new, eos,
                                                          BM.beam_fill(0, eos))
                what = (nb, eos, max_new, B)
                assert got.tolist() == want.tolist(), what
                assert torch.allclose(got_s, want_s, atol=1e-5, rtol=0), (what, got_s, want_s)
                early += steps < max_new
                # running on after the stopping point leaves the kept hypotheses as they are
                if steps < max_new:
                    more, more_s, steps3, st3 = drive_restatement(model_logits(model, prompts, nb), B, nb, max_new, eos,
                                                                  BM.beam_fill(0, eos), extra=3)
                    assert steps3 > steps or steps == max_new
                    assert more.tolist() == got.tolist() and torch.equal(more_s, got_s), what
                    assert torch.equal(st3.fin_score, st.fin_score) and torch.equal(st3.fin_len, st.fin_len)
    print(f"num_beams {nb}: {early} cases stopped before max_new_tokens")


def test_first_step_sees_beam_zero_only_and_ties_go_to_the_lowest_index():
    B, nb, V = 1, 3, 7
    st = BM.BeamState(B, nb, 4)
    logits = torch.zeros(nb, V)                                   # every score equal: the order is the flat index
    parent, tok = BM.beam_update(st, logits, 0, None, False)
    assert parent.tolist() == [[0, 0, 0]] and tok.tolist() == [[0, 1, 2]]
    parent, tok = BM.beam_update(st, logits, 1, None, False)
    assert parent.tolist() == [[0, 0, 0]] and tok.tolist() == [[0, 1, 2]]
    assert st.run_ids[0, :, :2].tolist() == [[0, 0], [0, 1], [0, 2]]
    assert not bool(st.fin_ok.any()) and bool(st.unsat.all())
    BM.beam_update(st, logits, 2, None, True)                     # the last step finishes the top num_beams candidates
    assert bool(st.fin_ok.all()) and st.fin_len.tolist() == [[3, 3, 3]] and bool(st.all_hit.all())
    assert BM.beam_done(st)
    assert BM.beam_result(st, -1).tolist() == [[0, 0, 0]]


def test_result_pads_shorter_rows_with_the_fill():
    st = BM.BeamState(2, 2, 5)
    st.fin_ids[0, 0] = torch.tensor([4, 5, 6, 0, 0])
    st.fin_ids[1, 0] = torch.tensor([7, 9, 0, 0, 0])
    st.fin_len[:, 0] = torch.tensor([3, 2], dtype=torch.int32)
    assert BM.beam_result(st, 9).tolist() == [[4, 5, 6], [7, 9, 9]]
    assert BM.beam_fill(0, 9) == 9 and BM.beam_fill(3, 9) == 3 and BM.beam_fill(None, None) == -1


def load_beam_fixture():
    """tests/golden/beam_cases.pt (tests/golden/make_beam_golden.py): a tiny Llama's weights and HF's recorded beam searches."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beam_cases.pt")
    return torch.load(path, map_location="cpu", weights_only=True)


def test_restatement_equals_the_recorded_hf_results():
    """The committed fixture: HF's tokens and scores on cases whose every decision is at least 1e-3 wide; every cell of
    num_beams 2 / 4 / 8 x eos none / present is filled and at least three cases with an eos stop before max_new_tokens."""
    transformers = pytest.importorskip("transformers")
    fx = load_beam_fixture()
    model = transformers.LlamaForCausalLM(transformers.LlamaConfig(**fx["config"]))
    model.load_state_dict({k: v.float() for k, v in fx["state"].items()}, strict=True)
    model.eval()
    cells, early = set(), 0
    for c in fx["cases"]:
        nb, eos, new, prompts = c["num_beams"], c["eos"], c["max_new"], c["prompts"]
        assert c["gap"] >= 1e-3
        got, got_s, steps, _ = drive_restatement(model_logits(model, prompts, nb), prompts.shape[0], nb, new, eos,
                                                 BM.beam_fill(0, eos))
        assert got.tolist() == c["tokens"].tolist(), (nb, eos)
        assert torch.allclose(got_s, c["scores"], atol=1e-5, rtol=0) and steps == c["steps"]
        cells.add((nb, eos is not None))
        early += eos is not None and steps < new
    assert cells == {(nb, e) for nb in (2, 4, 8) for e in (False, True)} and early >= 3, (cells, early)


# ---------------------------------------------------------------------------------------------------------------------
# the switch and the argument rules of generate()
# ---------------------------------------------------------------------------------------------------------------------
def test_switch_reads_the_environment_over_the_config(monkeypatch):
    from cambrian_amd import ops
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_BEAM", raising=False)
    assert ops.decode_beam_enabled() is False and ops.decode_beam_enabled(True) is True
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_BEAM", "1")
    assert ops.decode_beam_enabled(False) is True
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_BEAM", "0")
    assert ops.decode_beam_enabled(True) is False
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_BEAM", "")
    assert ops.decode_beam_enabled(True) is True
    for bad in ("2", "yes", "on", "-1", " 1"):
        monkeypatch.setenv("CAMBRIAN_AMD_DECODE_BEAM", bad)
        with pytest.raises(ValueError, match="CAMBRIAN_AMD_DECODE_BEAM"):
            ops.decode_beam_enabled(True)


def test_switch_off_keeps_the_raise_also_without_self(monkeypatch):
    from cambrian_amd.model.language_model.cambrian_llama import _generate
    for value in (None, "0"):
        if value is None:
            monkeypatch.delenv("CAMBRIAN_AMD_DECODE_BEAM", raising=False)
        else:
            monkeypatch.setenv("CAMBRIAN_AMD_DECODE_BEAM", value)
        with pytest.raises(NotImplementedError, match="num_beams"):
            _generate(None, torch.zeros(1, 4, dtype=torch.long), num_beams=5)


def test_switch_on_refuses_beam_sampling_and_no_new_tokens(monkeypatch):
    from cambrian_amd.model.language_model.cambrian_llama import _generate
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_BEAM", "1")
    ids = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="num_beams"):
        _generate(None, ids, num_beams=3, do_sample=True)
    with pytest.raises(ValueError, match="max_new_tokens"):
        _generate(None, ids, num_beams=3, max_new_tokens=0)
    for beams in (1, None):                                         # not beam search: the switch is not even read
        monkeypatch.setenv("CAMBRIAN_AMD_DECODE_BEAM", "bogus")
        with pytest.raises(ValueError, match="unsupported argument"):
            _generate(None, ids, num_beams=beams, no_such_argument=1)
