"""Prompt-lookup drafting for ``generate(prompt_lookup_num_tokens=...)``: HF's assisted decoding with a
``PromptLookupCandidateGenerator`` (transformers/generation/candidate_generator.py), restated on Python lists.  Pure host code:
nothing here touches a device.

The verify step (``lookup_step`` in cambrian_llama.py) runs [last token, drafts] as one multi-token decode step; ``accept``
counts the leading drafts the model reproduced."""
from __future__ import annotations

from typing import List, Optional, Sequence


def ngram_draft(ids: Sequence[int], num_tokens: int, max_ngram: int, vocab: int, eos: Optional[int] = None) -> List[int]:
    """``PromptLookupCandidateGenerator.get_candidates`` on one sequence: for n-gram sizes from ``min(max_ngram, len - 1)`` down
    to 1, the LEFTMOST earlier occurrence of the sequence's last n ids that has a continuation; its continuation, at most
    ``num_tokens`` ids, is the draft.  The first such match decides (also when the cuts below leave nothing of it).  The draft
    is cut before an ``eos`` id, as HF does, and before the first id outside ``[0, vocab)`` — the image placeholder (-200) of
    a multimodal prompt is no token the model can be fed."""
    ids = list(ids)
    n_ids = len(ids)
    if num_tokens < 1 or max_ngram < 1:
        return []
    for n in range(min(max_ngram, n_ids - 1), 0, -1):
        tail = ids[n_ids - n:]
        for i in range(n_ids - n + 1):
            if ids[i:i + n] != tail:
                continue
            start = i + n
            end = min(start + num_tokens, n_ids)
            if start >= end:
                continue
            draft = ids[start:end]
            for j, tok in enumerate(draft):
                if (eos is not None and tok == eos) or not 0 <= tok < vocab:
                    return draft[:j]
            return draft
    return []


def accept(draft: Sequence[int], picked: Sequence[int]) -> int:
    """How many leading drafts the model reproduced: ``picked[j]`` is the model's token after [last token, draft[:j]], so
    draft[j] stands iff every earlier draft stood and ``picked[j] == draft[j]``.  ``picked`` has ``len(draft) + 1`` entries;
    the step emits ``draft[:a] + [picked[a]]``."""
    a = 0
    while a < len(draft) and int(picked[a]) == int(draft[a]):
        a += 1
    return a
