"""Writes tests/golden/beam_cases.pt: beam search of HF transformers (``GenerationMixin._beam_search``) on a tiny random
``LlamaForCausalLM``, recorded for tests/test_decode_beam_host.py (the restatement on the CPU) and tests/test_decode_beam_gpu.py
(``generate()`` on the device).  Recorded results only:

* ``config`` / ``state``: the model (H 128, 2 heads of 64, 1 kv head, intermediate 128, 2 layers, V 64), every weight a bf16
  number so that it is stored in two bytes and is the same number in fp32;
* ``cases``: prompts, ``num_beams``, the eos id, ``max_new_tokens``, HF's new tokens and sequence scores, how many steps the
  search took, and the smallest gap of any comparison that decided something (``decision_gap``: adjacent scores among the top
  K + 1, the hypotheses' merge, the early-stop flag) when the restatement is driven by the same logits.

Only cases whose gap is >= 1e-3 are kept, so that an implementation whose logits differ in the last bits takes the same
decisions.  Seeds are searched until every cell (num_beams 2 / 4 / 8 x eos none / present) holds CASES_PER_CELL cases and at
least three cases with an eos stop before max_new_tokens.

    PYTHONPATH=. python tests/golden/make_beam_golden.py
"""
import os
import sys

import torch
import transformers

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_decode_beam_host import decision_gap, hf_case, model_logits  # noqa: E402

from cambrian_amd.model.language_model import beam as BM  # noqa: E402

CONFIG = dict(vocab_size=64, hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
              num_key_value_heads=1, max_position_embeddings=64, rms_norm_eps=1e-5, rope_theta=10000.0, tie_word_embeddings=False)
MIN_GAP, MAX_NEW, PROMPT, CASES_PER_CELL, MAX_SEEDS = 1e-3, 12, 5, 2, 6000


def build_model(state=None):
    cfg = transformers.LlamaConfig(**CONFIG)
    if state is None:
        torch.manual_seed(1234)
        model = transformers.LlamaForCausalLM(cfg)
        with torch.no_grad():
            for p in model.parameters():
                if p.dim() > 1:
                    p.mul_(4.0)
                p.copy_(p.to(torch.bfloat16).float())
        return model.eval()
    model = transformers.LlamaForCausalLM(cfg)
    model.load_state_dict({k: v.float() for k, v in state.items()}, strict=True)
    return model.eval()


def restatement_with_gap(model, prompts, nb, max_new, eos):
    """(tokens, score of the best hypothesis, steps, smallest decision gap) of beam.py around the model's logits."""
    B = prompts.shape[0]
    st = BM.BeamState(B, nb, max_new)
    logits_of = model_logits(model, prompts, nb)
    gap, steps = float("inf"), 0
    for s in range(max_new):
        trace = {}
        BM.beam_update(st, logits_of(st.run_ids.reshape(B * nb, max_new)[:, :s]), s, eos, s + 1 == max_new, trace)
        gap, steps = min(gap, decision_gap(trace, nb)), s + 1
        if BM.beam_done(st):
            break
    return BM.beam_result(st, BM.beam_fill(0, eos)), st.fin_score[:, 0].clone(), steps, gap


def main():
    model = build_model()
    gen = torch.Generator().manual_seed(99)
    with torch.no_grad():
        freq = model(torch.randint(1, 64, (16, PROMPT), generator=gen)).logits[:, -1].softmax(-1).mean(0)
    eos_id = int(freq.topk(2).indices[1])
    cases, tried, early = [], 0, 0
    for nb in (2, 4, 8):
        for eos in (None, eos_id):
            kept = 0
            for seed in range(MAX_SEEDS):
                need_early = eos is not None and nb == 8 and early < 3
                if kept >= CASES_PER_CELL and not need_early:
                    break
                g = torch.Generator().manual_seed(10000 * nb + 2 * seed + (eos is not None))
                prompts = torch.randint(1, 64, (1 if nb == 8 else 2, PROMPT), generator=g)   # 8 beams: few seeds qualify
                tried += 1
                toks, score, steps, gap = restatement_with_gap(model, prompts, nb, MAX_NEW, eos)
                if gap < MIN_GAP or (kept >= CASES_PER_CELL and steps == MAX_NEW):
                    continue
                want, want_s = hf_case(model, prompts, nb, MAX_NEW, eos)
                assert toks.tolist() == want.tolist(), (nb, eos, seed)
                assert torch.allclose(score, want_s, atol=1e-5, rtol=0)
                kept += 1
                early += eos is not None and steps < MAX_NEW
                cases.append(dict(num_beams=nb, eos=eos, max_new=MAX_NEW, prompts=prompts, tokens=want, scores=want_s, steps=steps,
                                  gap=gap))
            assert kept >= CASES_PER_CELL, (nb, eos, "no seed qualified")
    assert early >= 3, f"only {early} cases with an eos stop before max_new_tokens"
    assert all(c["gap"] >= MIN_GAP for c in cases)
    state = {k: v.to(torch.bfloat16) for k, v in model.state_dict().items()}
    path = os.path.join(HERE, "beam_cases.pt")
    torch.save(dict(config=CONFIG, state=state, cases=cases, transformers=transformers.__version__), path)
    print(f"{len(cases)} cases of {tried} tried, {early} stop early; {os.path.getsize(path)} bytes -> {path}")
    for c in cases:
        print(c["num_beams"], c["eos"], c["steps"], f"{c['gap']:.2e}", c["tokens"].tolist())


if __name__ == "__main__":
    main()
