"""The logits processors of ``generate()`` that read the ids produced so far: ``repetition_penalty``,
``no_repeat_ngram_size``, ``bad_words_ids``, ``min_new_tokens``, ``suppress_tokens``, and an ``eos_token_id`` that is a set.

``parse`` turns the arguments into one ``ProcessSpec`` (or refuses them) before the model is touched; ``apply_torch`` restates in
torch the rule that ``cmb_decode_process`` (csrc/decode_process.hip, declared in include/cambrian_amd.h) applies on the
device.  It is the oracle of the kernel's tests and the host arm of tools/bench_decode_process.py; ``generate()`` itself runs
the kernel.

The rule.  The reference calls ``super().generate(inputs_embeds=...)``, so HF's processors see the GENERATED ids only, never the
prompt.  For a row with generated ids ``h[0..n)`` at the step that selects token ``n`` HF chains RepetitionPenalty,
NoRepeatNGram, NoBadWords, MinNewTokensLength(0, ...) and SuppressTokens, which equals one pass:

* penalty ``p != 1``: for every DISTINCT id of ``h``: ``l = logits[id]; logits[id] = l * p if l < 0 else l / p`` (fp32);
* then ``-inf`` at: every ``h[i + g - 1]`` with ``h[i .. i+g-1) == h[n-g+1 .. n)`` when ``g = no_repeat_ngram_size > 0`` and
  ``n + 1 >= g``; every bad word of one id; the last id of a bad word of ``m > 1`` ids when ``m <= n`` (HF's rule, not
  ``m - 1 <= n``) and ``h`` ends with its first ``m - 1`` ids; every suppressed token; every eos id while ``n < min_new_tokens``.

An id outside ``[0, V)`` is never used as an index and still takes part in the matching.  Checked bit for bit against the five
classes of transformers 5.x (tests/test_decode_process_host.py); equality with the transformers 4.37.0 the reference pins is
NOT verified.
"""
from __future__ import annotations

import math
import numbers
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import torch

SWITCH = "config.decode_logits_processors / CAMBRIAN_AMD_DECODE_PROCESS=1"
ARGUMENTS = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "bad_words_ids", "suppress_tokens")


@dataclass
class ProcessSpec:
    """What one ``generate()`` call asks of ``cmb_decode_process``.  ``eos``: the eos set, ``eos[0]`` is what a done row
    emits; ``bans``: suppressed tokens and bad words of one id; ``words``: bad words of two or more ids."""
    penalty: float = 1.0
    ngram: int = 0
    min_new: int = 0
    eos: List[int] = field(default_factory=list)
    bans: List[int] = field(default_factory=list)
    words: List[List[int]] = field(default_factory=list)

    @property
    def edits(self) -> bool:
        """Whether any logit can change."""
        return self.penalty != 1.0 or self.ngram > 0 or bool(self.bans) or bool(self.words) or (self.min_new > 0 and bool(self.eos))

    @property
    def active(self) -> bool:
        """Whether ``generate()`` needs the kernel: a logit can change, or the eos id is a set of more than one."""
        return self.edits or len(self.eos) > 1

    def device_lists(self, device):
        """(eos, bans, word_ids, word_off) as int64 device tensors, None for an empty list: uploaded once per call."""
        def up(values):
            return torch.tensor(values, dtype=torch.int64, device=device) if len(values) else None
        off = [0]
        for w in self.words:
            off.append(off[-1] + len(w))
        return up(self.eos), up(self.bans), up([i for w in self.words for i in w]), up(off if self.words else [])


def _is_int(v) -> bool:
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def eos_list(eos_token_id) -> Optional[List[int]]:
    """None, or the ids of ``eos_token_id`` (an int, or a non-empty list / tuple / 1-d tensor of ints) in their order without
    repeats."""
    if eos_token_id is None:
        return None
    if isinstance(eos_token_id, torch.Tensor):
        eos_token_id = eos_token_id.tolist()
    if _is_int(eos_token_id):
        return [int(eos_token_id)]
    if not isinstance(eos_token_id, (list, tuple)) or not len(eos_token_id) or not all(_is_int(e) for e in eos_token_id):
        raise ValueError(f"generate(eos_token_id={eos_token_id!r}): has to be an int or a non-empty list of ints")
    out: List[int] = []
    for e in eos_token_id:
        if int(e) not in out:
            out.append(int(e))
    return out


def parse(enabled: bool, eos_token_id=None, repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None,
          bad_words_ids=None, suppress_tokens=None, beams: int = 1, lookup: bool = False) -> Optional[ProcessSpec]:
    """The processor arguments of ``generate()``, checked before the model is touched.  Returns None when the call needs no
    kernel (every argument at its off value and at most one eos id), else the ``ProcessSpec``.

    Switch off (``enabled`` False): the four new keywords are accepted at their off values only and a list ``eos_token_id`` is
    refused, each with a ValueError that names the switch (``repetition_penalty`` is left to the caller's rule for keywords
    it accepts at one value).  Switch on: the values are validated as HF validates them; beam search and prompt-lookup decoding
    do not combine with any of them (NotImplementedError)."""
    is_set = isinstance(eos_token_id, (list, tuple)) or (isinstance(eos_token_id, torch.Tensor) and eos_token_id.dim() > 0)
    if not enabled:
        for name, value, off in (("no_repeat_ngram_size", no_repeat_ngram_size, (None, 0)), ("min_new_tokens", min_new_tokens, (None, 0)),
                                 ("bad_words_ids", bad_words_ids, (None,)), ("suppress_tokens", suppress_tokens, (None,))):
            if not any(value is o or (o is not None and _is_int(value) and value == o) for o in off):
                raise ValueError(f"generate({name}={value!r}): the logits processors are switched off; switch them on with {SWITCH}")
        if is_set:
            raise ValueError(f"generate(eos_token_id={eos_token_id!r}): a list of eos ids needs the logits processors; switch them on "
                             f"with {SWITCH}, or pass one int")
        return None
    spec = ProcessSpec()
    if repetition_penalty is not None:
        if isinstance(repetition_penalty, bool) or not isinstance(repetition_penalty, (int, float)) \
                or not math.isfinite(repetition_penalty) or not repetition_penalty > 0:
            raise ValueError(f"`repetition_penalty` has to be a strictly positive float, but is {repetition_penalty!r}")
        spec.penalty = float(torch.tensor(float(repetition_penalty), dtype=torch.float32))       # the fp32 the kernel is handed
    if no_repeat_ngram_size is not None:
        if not _is_int(no_repeat_ngram_size) or no_repeat_ngram_size < 0:
            raise ValueError(f"`no_repeat_ngram_size` has to be an integer >= 0 (0: off), but is {no_repeat_ngram_size!r}")
        spec.ngram = int(no_repeat_ngram_size)
    if min_new_tokens is not None:
        if not _is_int(min_new_tokens) or min_new_tokens < 0:
            raise ValueError(f"`min_new_tokens` has to be an integer >= 0, but is {min_new_tokens!r}")
        spec.min_new = int(min_new_tokens)
    spec.eos = eos_list(eos_token_id) or []
    if suppress_tokens is not None:
        if isinstance(suppress_tokens, torch.Tensor):
            suppress_tokens = suppress_tokens.tolist()
        if not isinstance(suppress_tokens, (list, tuple)) or not all(_is_int(i) for i in suppress_tokens):
            raise ValueError(f"`suppress_tokens` has to be a list of integers, but is {suppress_tokens!r}")
        spec.bans = [int(i) for i in suppress_tokens]
    if bad_words_ids is not None:
        if not isinstance(bad_words_ids, (list, tuple)) or len(bad_words_ids) == 0:
            raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bad_words_ids!r}.")
        if any(not isinstance(w, (list, tuple)) for w in bad_words_ids):
            raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bad_words_ids!r}.")
        if any(len(w) == 0 or any(not _is_int(i) or i < 0 for i in w) for w in bad_words_ids):
            raise ValueError(f"Each list in `bad_words_ids` has to be a non-empty list of non-negative integers, but is "
                             f"{bad_words_ids!r}.")
        for w in bad_words_ids:
            w = [int(i) for i in w]
            if len(w) == 1 and w[0] in spec.eos:               # HF drops the words that are exactly one eos id
                continue
            if len(w) == 1:
                spec.bans.append(w[0])
            else:
                spec.words.append(w)
    named = [n for n, on in (("repetition_penalty", spec.penalty != 1.0), ("no_repeat_ngram_size", spec.ngram > 0),
                             ("min_new_tokens", spec.min_new > 0), ("bad_words_ids", bad_words_ids is not None),
                             ("suppress_tokens", bool(suppress_tokens)), ("eos_token_id as a list", len(spec.eos) > 1)) if on]
    if named and beams > 1:
        raise NotImplementedError(f"generate(num_beams={beams}, {named[0]}=...): beam search applies the logits processors to "
                                  "log-softmax scores, a rule that is not implemented; use num_beams=1")
    if named and lookup:
        raise NotImplementedError(f"generate(prompt_lookup_num_tokens=..., {named[0]}=...): prompt-lookup decoding does not "
                                  "combine with the logits processors (every verify row would need its own history)")
    return spec if spec.active else None


def apply_torch(logits: torch.Tensor, hist: torch.Tensor, n: int, spec: ProcessSpec, done: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The rule of the module's docstring on fp32 ``logits`` [B, V] (any strides), IN PLACE, from ``hist`` [B, >= n] int64 of
    which the first ``n`` columns are valid; with ``done`` (bool / uint8 [B]) and an eos set, ``done[b]`` is set where
    ``hist[b, n - 1]`` is in the set.  Plain torch: the gathers, scatters and compares the kernel replaces.  Returns ``logits``."""
    B, V = logits.shape
    dev = logits.device
    h = hist[:, :n]
    ninf = float("-inf")

    def columns(ids: torch.Tensor, on: Optional[torch.Tensor] = None) -> torch.Tensor:
        """bool [B, V]: the columns ``ids`` [B, k] name (where ``on``); an id outside [0, V) names none."""
        ok = (ids >= 0) & (ids < V)
        if on is not None:
            ok = ok & on
        mask = torch.zeros(B, V + 1, dtype=torch.bool, device=dev)
        mask.scatter_(1, torch.where(ok, ids, torch.full_like(ids, V)), True)
        return mask[:, :V]

    if spec.penalty != 1.0 and n > 0:
        p = torch.tensor(spec.penalty, dtype=torch.float32, device=dev)
        logits.copy_(torch.where(columns(h), torch.where(logits < 0, logits * p, logits / p), logits))
    ban = torch.zeros(B, V, dtype=torch.bool, device=dev)
    g = spec.ngram
    if g > 0 and n + 1 >= g and n >= g:
        win = h.unfold(1, g, 1)                                          # [B, n - g + 1, g]
        hit = (win[:, :, :g - 1] == h[:, None, n - g + 1:n]).all(-1)     # g = 1: nothing to compare, every window hits
        ban |= columns(win[:, :, g - 1], hit)
    single = [i for i in spec.bans if 0 <= i < V]
    if single:
        ban[:, torch.tensor(single, dtype=torch.int64, device=dev)] = True
    for w in spec.words:
        m = len(w)
        if m <= n and 0 <= w[-1] < V:
            ban[:, w[-1]] |= (h[:, n - m + 1:n] == torch.tensor(w[:-1], dtype=torch.int64, device=dev)).all(-1)
    if n < spec.min_new:
        for e in spec.eos:
            if 0 <= e < V:
                ban[:, e] = True
    logits.masked_fill_(ban, ninf)
    if done is not None and spec.eos and n >= 1:
        hit = torch.isin(h[:, n - 1], torch.tensor(spec.eos, dtype=torch.int64, device=dev))
        done.copy_(done | hit.to(done.dtype))
    return logits


def first_in_set(ids: torch.Tensor, eos: Sequence[int]) -> torch.Tensor:
    """bool [B, n]: the columns from each row's first id that is in ``eos`` on."""
    return torch.isin(ids, torch.tensor(list(eos), dtype=torch.int64, device=ids.device)).long().cumsum(dim=1) > 0
