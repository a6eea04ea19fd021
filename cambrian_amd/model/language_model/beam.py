"""Beam search of ``generate()``: the selection step restated once in plain torch.

The semantics are those of ``GenerationMixin._beam_search`` of transformers 5.x (the vectorised form) under ``do_sample=False``,
``length_penalty=1.0``, ``early_stopping=False``, ``num_return_sequences=1`` and no logits processor, with one refinement: where
HF's ``topk`` leaves the order of equal scores undefined, equal scores are ordered by the lowest index (a stable descending
sort).  Per step ``s`` (0-based) and per prompt, with ``K = 2 * num_beams``:

1. ``score[beam, tok] = run_score[beam] + log_softmax(logits[beam])[tok]`` on fp32 logits; ``run_score`` starts at
   ``[0, -1e9, -1e9, ...]`` so that the first step sees beam 0 only.
2. the ``K`` largest of the flattened ``[num_beams * V]``, descending, equal scores by the lowest flat index ``beam * V + tok``.
3. a candidate *hits* when its token is ``eos`` or when this is the last step (``s + 1 == max_new_tokens``).
4. the running beams are the top ``num_beams`` of ``score - 1e9 * hit``; child ``i`` inherits the sequence (and the K/V rows) of its
   parent beam.
5. candidates ranked ``< num_beams`` that hit become hypotheses with score ``score / (s + 1)`` (minus ``1e9`` once the prompt's
   early-stop flag is satisfied); every other candidate takes part with ``- 1e9`` and is not finished.  They are merged behind the
   ``num_beams`` kept hypotheses (initial score ``-1e9``, not finished) and the top ``num_beams`` are kept, earlier entries first
   among equals.
6. ``unsat &= any(run_score[0] / (s + 1) > where(fin_ok, min(fin_score), -1e9))`` — sticky.
7. the search is over after a step when no prompt is ``unsat`` or every candidate of every prompt hit (``beam_done``).

This module is device-agnostic and calls no kernel.  It is the selection of the per-launch loop of ``generate()`` and the
reference ``cmb_decode_beam`` (csrc/decode_beam.hip, whose arithmetic is csrc/decode_beam_core.h) is tested against.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

NEG = -1.0e9


class BeamState:
    """What beam search carries from step to step, per prompt ``b`` and slot ``i < num_beams``:
    ``run_ids`` int64 [B, nb, max_new] / ``run_score`` fp32 [B, nb]: the running beams, best first;
    ``fin_ids`` int64 [B, nb, max_new] / ``fin_len`` int32 / ``fin_score`` fp32 / ``fin_ok`` bool [B, nb]: the kept hypotheses,
    best first (``fin_len`` counts the generated tokens, the eos included);
    ``unsat`` bool [B]: the early-stop flag; ``all_hit`` bool [B]: whether every candidate of the last step hit."""

    def __init__(self, B: int, num_beams: int, max_new: int, device=None):
        kw = dict(device=device)
        self.run_ids = torch.zeros(B, num_beams, max_new, dtype=torch.int64, **kw)
        self.run_score = torch.zeros(B, num_beams, dtype=torch.float32, **kw)
        self.run_score[:, 1:] = NEG
        self.fin_ids = torch.zeros(B, num_beams, max_new, dtype=torch.int64, **kw)
        self.fin_len = torch.zeros(B, num_beams, dtype=torch.int32, **kw)
        self.fin_score = torch.full((B, num_beams), NEG, dtype=torch.float32, **kw)
        self.fin_ok = torch.zeros(B, num_beams, dtype=torch.bool, **kw)
        self.unsat = torch.ones(B, dtype=torch.bool, **kw)
        self.all_hit = torch.zeros(B, dtype=torch.bool, **kw)


def _top(values: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k largest of every row, descending, the lowest index first among equals."""
    srt = torch.sort(values, dim=1, descending=True, stable=True)
    return srt.values[:, :k], srt.indices[:, :k]


def beam_update(state: BeamState, logits: torch.Tensor, step: int, eos: Optional[int], last: bool, trace: Optional[dict] = None):
    """One step: ``logits`` fp32 [B * num_beams, V] of the running beams (row ``b * num_beams + i``).  Updates ``state`` and
    returns ``(parent, tok)``, int64 [B, num_beams]: the beam every new running beam continues and the token it appends.
    ``trace``: a dict that receives what the step compared, sorted descending per prompt — ``cand`` the top K + 1 scores,
    ``run`` the K running scores, ``merged`` the num_beams + K hypothesis scores, ``flag`` (best running, worst kept) — so that
    a caller can tell how close any decision was."""
    B, nb, M = state.run_ids.shape
    V = logits.shape[-1]
    if V < 2:
        raise ValueError("beam search needs a vocabulary of at least 2")
    K = 2 * nb
    score = torch.log_softmax(logits.float(), dim=-1).view(B, nb, V) + state.run_score[:, :, None]
    more_s, more_i = _top(score.reshape(B, nb * V), K + 1)
    top_s, top_i = more_s[:, :K], more_i[:, :K]
    beam, tok = top_i // V, top_i % V
    hit = torch.ones_like(tok, dtype=torch.bool) if last else \
        (tok == int(eos) if eos is not None else torch.zeros_like(tok, dtype=torch.bool))
    cand_ids = state.run_ids.gather(1, beam[:, :, None].expand(B, K, M)).clone()
    cand_ids[:, :, step] = tok

    # the running beams of the next step
    run_s = top_s + hit.to(torch.float32) * NEG
    new_s, pick = _top(run_s, nb)
    parent, new_tok = beam.gather(1, pick), tok.gather(1, pick)
    state.run_ids = cand_ids.gather(1, pick[:, :, None].expand(B, nb, M))
    state.run_score = new_s

    # the kept hypotheses
    just = hit & (torch.arange(K, device=tok.device) < nb)[None, :]
    fin_s = top_s / float(step + 1)
    fin_s = fin_s + (~state.unsat)[:, None].to(torch.float32) * NEG
    fin_s = fin_s + (~just).to(torch.float32) * NEG
    merged_s = torch.cat((state.fin_score, fin_s), dim=1)
    _, keep = _top(merged_s, nb)
    state.fin_score = merged_s.gather(1, keep)
    state.fin_ok = torch.cat((state.fin_ok, just), dim=1).gather(1, keep)
    state.fin_len = torch.cat((state.fin_len, torch.full_like(tok, step + 1, dtype=torch.int32)), dim=1).gather(1, keep)
    state.fin_ids = torch.cat((state.fin_ids, cand_ids), dim=1).gather(1, keep[:, :, None].expand(B, nb, M))

    # the early-stop flag
    best = state.run_score[:, :1] / float(step + 1)
    worst = torch.where(state.fin_ok, state.fin_score.min(dim=1, keepdim=True).values,
                        torch.full_like(state.fin_score, NEG))
    state.unsat = state.unsat & (best > worst).any(dim=1)
    state.all_hit = hit.all(dim=1)
    if trace is not None:
        trace.update(cand=more_s, run=_top(run_s, K)[0], merged=_top(merged_s, nb + K)[0], flag=(best, worst), fin_ok=state.fin_ok)
    return parent, new_tok


def beam_done(state: BeamState) -> bool:
    """Whether the search ends after the step that left ``state`` (reads the device)."""
    return not bool(state.unsat.any() & ~state.all_hit.all())


def beam_result(state: BeamState, fill: int) -> torch.Tensor:
    """The generated tokens of the best hypothesis of every prompt, int64 [B, n] with n the longest of them; shorter rows are
    padded with ``fill`` (HF: ``pad_token_id or eos_token_id``)."""
    n_each = state.fin_len[:, 0].to(torch.int64)
    n = int(n_each.max())
    ids = state.fin_ids[:, 0, :n].clone()
    ids[torch.arange(n, device=ids.device)[None, :] >= n_each[:, None]] = int(fill)
    return ids


def beam_fill(pad_token_id, eos_token_id) -> int:
    """HF's ``pad_token_id or eos_token_id`` (so a pad id of 0 pads with eos), -1 without an eos id."""
    if eos_token_id is None:
        return -1
    return int(pad_token_id or eos_token_id)
