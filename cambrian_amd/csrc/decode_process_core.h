// decode_process_core.h — the rules of the logits processors of generate() (cmb_decode_process, decode_process.hip), written as
// host+device functions so tests/csrc/decode_process_core_sim.cpp runs the very same code on the CPU
// (tests/test_decode_process_core_sim.py): which ids may index a row, the repetition penalty, the no-repeat n-gram predicate,
// the bad-word predicate, membership in a small id list, and the argument rules of the entry point.  The definition they
// implement is restated in torch in cambrian_amd/model/language_model/processors.py (HF's RepetitionPenalty, NoRepeatNGram,
// NoBadWords, MinNewTokensLength and SuppressTokens logits processors chained in that order, over the generated ids only).
#pragma once
#include <stdint.h>

#include "../../include/cambrian_amd.h"

#if !defined(CMB_PHD)
#if defined(__HIPCC__)
#define CMB_PHD __host__ __device__ __forceinline__
#else
#define CMB_PHD static inline
#endif
#endif

// The column of `id` in a row of V logits, or -1 when the id names none (an eos id in the embedding table's padding, an image
// placeholder): such an id is never used as an index, but it still takes part in n-gram and word matching.  V <= 2^31 - 1.
CMB_PHD int32_t cmb_dp_index(int64_t id, int64_t V) { return id >= 0 && id < V ? (int32_t)id : -1; }

// HF's RepetitionPenaltyLogitsProcessor on one logit: torch.where(l < 0, l * p, l / p), one IEEE-rounded fp32 operation
// (-0.0 and NaN take the division, -inf stays -inf).
CMB_PHD float cmb_dp_penalise(float l, float p) { return l < 0.f ? l * p : l / p; }

// Position j holds the first occurrence of its id: the lane there, and no other, penalises it, so every distinct id is
// penalised once whatever order the lanes run in.  (The kernel evaluates this predicate on 32-bit columns staged through LDS.)
CMB_PHD bool cmb_dp_first_occurrence(const int64_t* h, int64_t j) {
  for (int64_t i = 0; i < j; ++i)
    if (h[i] == h[j]) return false;
  return true;
}

// Whether the no-repeat rule of size g looks at a history of n ids at all (HF: cur_len + 1 >= ngram_size).
CMB_PHD bool cmb_dp_ngram_active(int64_t n, int64_t g) { return g > 0 && n + 1 >= g; }

// The n-gram that starts at h[i] (0 <= i <= n - g) begins with the last g - 1 ids of the history: h[i + g - 1] would repeat it.
// With g = 1 there is nothing to compare and every id of h is banned.
CMB_PHD bool cmb_dp_ngram_hits(const int64_t* h, int64_t n, int64_t g, int64_t i) {
  const int64_t* tail = h + (n - g + 1);
  for (int64_t k = 0; k + 1 < g; ++k)
    if (h[i + k] != tail[k]) return false;
  return true;
}

// Whether the last id of the word w[0 .. m) is banned after a history of n ids.  A word of one id always is.  A longer word is
// when m <= n and the history ends with w[0 .. m - 1): HF's NoBadWordsLogitsProcessor compares the lengths as m <= n, not
// m - 1 <= n, so a history of exactly m - 1 ids that equals the prefix bans nothing.
CMB_PHD bool cmb_dp_word_hits(const int64_t* h, int64_t n, const int64_t* w, int64_t m) {
  if (m < 1) return false;
  if (m == 1) return true;
  if (m > n) return false;
  const int64_t* tail = h + (n - m + 1);
  for (int64_t k = 0; k + 1 < m; ++k)
    if (tail[k] != w[k]) return false;
  return true;
}

// Word number w of the table (ids [n_ids], off [n_words + 1]): its first id and its length, or 0 when the offsets do not
// describe a piece of `ids` — a table out of rule bans nothing instead of being read out of bounds.
CMB_PHD int64_t cmb_dp_word_at(const int64_t* off, int64_t w, int64_t n_ids, int64_t* first) {
  const int64_t o0 = off[w], o1 = off[w + 1];
  if (o0 < 0 || o1 <= o0 || o1 > n_ids) return 0;
  *first = o0;
  return o1 - o0;
}

CMB_PHD bool cmb_dp_in_set(int64_t id, const int64_t* set, int64_t n_set) {
  for (int64_t k = 0; k < n_set; ++k)
    if (set[k] == id) return true;
  return false;
}

// The argument rules of cmb_decode_process, checked before any launch: NULL pointers, then sizes and strides, then the
// parameters (CMB_ERR_BAD_ARG); then alignment (CMB_ERR_ALIGNMENT).  A list of no entries may be NULL; `done` may be NULL.
CMB_PHD bool cmb_dp_finite(float x) { return x - x == 0.f; }

CMB_PHD int cmb_dp_check_args(const float* logits, int64_t logits_ld, int32_t B, int64_t V, const int64_t* hist, int64_t hist_ld,
                              int64_t n_hist, float penalty, int64_t ngram, int64_t min_new, const int64_t* eos, int32_t n_eos,
                              const int64_t* bans, int32_t n_bans, const int64_t* word_ids, int64_t n_word_ids,
                              const int64_t* word_off, int32_t n_words, const uint8_t* done) {
  (void)done;
  if (!logits || n_eos < 0 || n_bans < 0 || n_words < 0 || n_word_ids < 0 || n_hist < 0) return CMB_ERR_BAD_ARG;
  if ((n_hist > 0 && !hist) || (n_eos > 0 && !eos) || (n_bans > 0 && !bans)) return CMB_ERR_BAD_ARG;
  if (n_words > 0 && (!word_ids || !word_off || n_word_ids < n_words)) return CMB_ERR_BAD_ARG;
  if (B < 1 || V < 1 || V > 0x7FFFFFFFll || logits_ld < V || (n_hist > 0 && hist_ld < n_hist)) return CMB_ERR_BAD_ARG;
  if (!cmb_dp_finite(penalty) || !(penalty > 0.f) || ngram < 0 || min_new < 0) return CMB_ERR_BAD_ARG;
  if (((uintptr_t)logits & 3u) || ((uintptr_t)hist & 7u) || ((uintptr_t)eos & 7u) || ((uintptr_t)bans & 7u) ||
      ((uintptr_t)word_ids & 7u) || ((uintptr_t)word_off & 7u))
    return CMB_ERR_ALIGNMENT;
  return CMB_OK;
}
