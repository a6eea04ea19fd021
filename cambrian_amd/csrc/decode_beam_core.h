// decode_beam_core.h — arithmetic and bookkeeping of beam search (cmb_decode_beam, decode_beam.hip), written as host+device
// functions so tests/csrc/decode_beam_core_sim.cpp runs the very same code on the CPU (tests/test_decode_beam_core_sim.py):
// the byte layout of the state block, the ordering key of a candidate, and one prompt's step — which candidates run on, which
// become hypotheses, the merge with the kept hypotheses and the early-stop flag.  The definition it implements is restated in
// torch in cambrian_amd/model/language_model/beam.py (HF's GenerationMixin._beam_search with equal scores ordered by index).
#pragma once
#include "decode_sample_core.h"

#define CMB_BEAM_MAX 16                    /* beams of one prompt (rows of a decode step) */
#define CMB_BEAM_MAXK (2 * CMB_BEAM_MAX)   /* candidates kept per prompt and step: K = 2 * num_beams */
#define CMB_BEAM_NEG (-1.0e9f)

// ---- the state block ----------------------------------------------------------------------------------------------------------
// One allocation per generate() call, zero-initialised by the caller: step 0 reads none of it (it starts from run_score =
// [0, -1e9, ...], fin_score = -1e9, fin_ok = 0, unsat = 1).  R = prompts * num_beams rows, K = 2 * num_beams, M = max_new;
// row r = prompt * num_beams + slot.  Every section starts at a multiple of 16 bytes, in this order:
enum cmb_beam_section {
  CMB_BEAM_RUN_SCORE = 0,   /* float   [R]        score of running beam r, best first inside a prompt */
  CMB_BEAM_FIN_SCORE,       /* float   [R]        score of kept hypothesis r, best first */
  CMB_BEAM_FIN_LEN,         /* int32   [R]        its generated tokens, the eos included */
  CMB_BEAM_PARENT,          /* int32   [R]        the last step: the slot (0 .. num_beams - 1) running beam r continues */
  CMB_BEAM_TOK,             /* int32   [R]        the last step: the token it appended */
  CMB_BEAM_CAND_LP,         /* float   [R][K]     the last step: log-probabilities of row r's min(K, V) largest logits, descending */
  CMB_BEAM_CAND_TOK,        /* int32   [R][K]     their token ids */
  CMB_BEAM_FIN_OK,          /* uint8   [R]        hypothesis r is a finished sequence */
  CMB_BEAM_UNSAT,           /* uint8   [prompts]  the early-stop flag (1: a running beam may still beat a kept hypothesis) */
  CMB_BEAM_ALL_HIT,         /* uint8   [prompts]  the last step: every candidate hit the stopping criterion */
  CMB_BEAM_RUN_IDS,         /* int64   [2][R][M]  the running sequences; step s reads half s & 1 and writes half (s + 1) & 1 */
  CMB_BEAM_FIN_IDS,         /* int64   [R][M]     the kept hypotheses' sequences */
  CMB_BEAM_SECTIONS
};

typedef struct cmb_beam_layout {
  int64_t off[CMB_BEAM_SECTIONS];
  int64_t total;
} cmb_beam_layout;

CMB_PHD cmb_beam_layout cmb_beam_make_layout(int64_t prompts, int64_t num_beams, int64_t max_new) {
  const int64_t R = prompts * num_beams, K = 2 * num_beams;
  const int64_t bytes[CMB_BEAM_SECTIONS] = {4 * R, 4 * R, 4 * R, 4 * R, 4 * R, 4 * R * K, 4 * R * K, R, prompts, prompts,
                                            16 * R * max_new, 8 * R * max_new};
  cmb_beam_layout L;
  int64_t at = 0;
  for (int i = 0; i < CMB_BEAM_SECTIONS; ++i) {
    L.off[i] = at;
    at += (bytes[i] + 15) / 16 * 16;
  }
  L.total = at;
  return L;
}

// ---- the ordering key ---------------------------------------------------------------------------------------------------------
// unsigned order of the keys = descending order of the candidates: the larger score first, among equal scores (-0 == +0) the
// LOWER index first.  Distinct indices give distinct keys.
CMB_PHD uint64_t cmb_beam_key(float score, uint32_t index) { return ((uint64_t)cmb_ds_key32(score) << 32) | (uint32_t)~index; }

// the score of a hypothesis of `len` generated tokens (length_penalty = 1)
CMB_PHD float cmb_beam_hyp_score(float score, int64_t len) { return score / (float)len; }

// ---- one prompt's step --------------------------------------------------------------------------------------------------------
typedef struct cmb_beam_cand {
  float score;             /* run_score[beam] + log_softmax(logits[beam])[tok] */
  int32_t beam, tok;
} cmb_beam_cand;

// One prompt's state (in) and what the step makes of it (out); everything the step needs lives here, so that on the device the
// whole struct sits in LDS and no array is indexed in registers.
typedef struct cmb_beam_prompt {
  /* in / out */
  float run_score[CMB_BEAM_MAX], fin_score[CMB_BEAM_MAX];
  int32_t fin_len[CMB_BEAM_MAX];
  uint8_t fin_ok[CMB_BEAM_MAX];
  uint8_t unsat;
  /* out */
  int32_t parent[CMB_BEAM_MAX], tok[CMB_BEAM_MAX];   /* running beam i continues slot parent[i] with tok[i] */
  int32_t run_src[CMB_BEAM_MAX];                     /* ... and is candidate run_src[i] */
  int32_t fin_src[CMB_BEAM_MAX];                     /* kept hypothesis i was: m < num_beams hypothesis m, else candidate m - num_beams */
  uint8_t all_hit, fin_moved;                        /* fin_moved: some fin_src[i] != i */
  /* scratch */
  float s[CMB_BEAM_MAX + CMB_BEAM_MAXK], new_score[CMB_BEAM_MAX];
  int32_t new_len[CMB_BEAM_MAX];
  uint8_t hit[CMB_BEAM_MAXK], taken[CMB_BEAM_MAX + CMB_BEAM_MAXK], ok[CMB_BEAM_MAX + CMB_BEAM_MAXK], new_ok[CMB_BEAM_MAX];
} cmb_beam_prompt;

CMB_PHD void cmb_beam_init(cmb_beam_prompt* p, int nb) {
  for (int i = 0; i < nb; ++i) {
    p->run_score[i] = i ? CMB_BEAM_NEG : 0.f;
    p->fin_score[i] = CMB_BEAM_NEG;
    p->fin_len[i] = 0;
    p->fin_ok[i] = 0;
  }
  p->unsat = 1;
}

// the position of the largest s[0 .. n) not yet taken, the first among equals; marks it taken
CMB_PHD int cmb_beam_take(cmb_beam_prompt* p, int n) {
  int best = -1;
  uint32_t best_key = 0;
  for (int c = 0; c < n; ++c) {
    if (p->taken[c]) continue;
    const uint32_t k = cmb_ds_key32(p->s[c]);
    if (best < 0 || k > best_key) {
      best = c;
      best_key = k;
    }
  }
  p->taken[best] = 1;
  return best;
}

// top[0 .. 2 nb): the prompt's candidates in cmb_beam_key order.  step: 0-based; eos: -1 = none; last: step + 1 == max_new.
CMB_PHD void cmb_beam_step(cmb_beam_prompt* p, const cmb_beam_cand* top, int nb, int64_t step, int64_t eos, int last) {
  const int K = 2 * nb;
  uint8_t all_hit = 1;
  // the running beams: the top nb of score - 1e9 * hit
  for (int c = 0; c < K; ++c) {
    p->hit[c] = (uint8_t)(last || (eos >= 0 && (int64_t)top[c].tok == eos));
    all_hit &= p->hit[c];
    p->s[c] = p->hit[c] ? top[c].score + CMB_BEAM_NEG : top[c].score;
    p->taken[c] = 0;
  }
  for (int i = 0; i < nb; ++i) {
    const int c = cmb_beam_take(p, K);
    p->run_src[i] = c;
    p->parent[i] = top[c].beam;
    p->tok[i] = top[c].tok;
    p->run_score[i] = p->s[c];
  }
  // the kept hypotheses: the old ones, then the candidates (those of the first nb that hit: score / length, behind everything
  // once the flag is satisfied; the others 1e9 lower and not finished); the top nb, earlier entries first among equals
  for (int m = 0; m < nb; ++m) {
    p->s[m] = p->fin_score[m];
    p->ok[m] = p->fin_ok[m];
    p->taken[m] = 0;
  }
  for (int c = 0; c < K; ++c) {
    const uint8_t just = (uint8_t)(p->hit[c] && c < nb);
    float f = cmb_beam_hyp_score(top[c].score, step + 1);
    if (!p->unsat) f += CMB_BEAM_NEG;
    if (!just) f += CMB_BEAM_NEG;
    p->s[nb + c] = f;
    p->ok[nb + c] = just;
    p->taken[nb + c] = 0;
  }
  uint8_t moved = 0;
  for (int i = 0; i < nb; ++i) {
    const int m = cmb_beam_take(p, nb + K);
    p->fin_src[i] = m;
    moved |= (uint8_t)(m != i);
    p->new_score[i] = p->s[m];
    p->new_ok[i] = p->ok[m];
    p->new_len[i] = m < nb ? p->fin_len[m] : (int32_t)(step + 1);
  }
  float worst = p->new_score[0];
  for (int i = 0; i < nb; ++i) {
    p->fin_score[i] = p->new_score[i];
    p->fin_ok[i] = p->new_ok[i];
    p->fin_len[i] = p->new_len[i];
    if (p->new_score[i] < worst) worst = p->new_score[i];
  }
  // the flag: can the best running beam still beat the worst kept hypothesis (an open slot counts as -1e9)?
  const float best = cmb_beam_hyp_score(p->run_score[0], step + 1);
  uint8_t any = 0;
  for (int i = 0; i < nb; ++i) any |= (uint8_t)(best > (p->fin_ok[i] ? worst : CMB_BEAM_NEG));
  p->unsat = (uint8_t)(p->unsat && any);
  p->all_hit = all_hit;
  p->fin_moved = moved;
}
