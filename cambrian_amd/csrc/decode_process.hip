// decode_process.hip — the logits processors of generate() that read the ids produced so far (cmb_decode_process): repetition
// penalty, no-repeat n-gram, bad words, suppressed tokens, minimum length, and the done flag of an eos SET, applied to a step's
// fp32 logits in place, in one launch, before cmb_decode_next / cmb_decode_sample select from them.
// Roofline class: launch-bound (a row of logits is read and written at a few indices only; the history is a few KB).
//
// One workgroup of DP_THREADS per row, two phases with a workgroup barrier between them:
//   1. penalty: every DISTINCT id of the history is penalised exactly once.  The lane that holds position j applies the penalty
//      iff no earlier position holds the same id (a first-occurrence test), so the winner is a property of the history and not of
//      the order the lanes ran in.  The other way — a bitmap over V in LDS, the old value of an atomic-or picking the winner —
//      needs V bits: 16 KB at V = 128256, but the contract is V <= 2^31 - 1, 256 MiB of bits against 160 KiB of LDS per CU, so
//      it would need this test as a second path anyway.  The test is quadratic in the history; the ids are staged through LDS
//      as 32-bit columns (an id that names no column is -1 and never compared), DP_THREADS at a time, and read back 16 bytes
//      per load at an address the whole wave shares.
//   2. bans: -inf at every id the n-gram rule, the word table, the single-id list and the minimum length name.  Lanes may store
//      the same -inf to one address; a penalised id that is also banned ends at -inf because of the barrier.
// Plain stores only, no atomics: the same bits on every run.  The rules live in decode_process_core.h, which
// tests/csrc/decode_process_core_sim.cpp runs on the CPU.
#include <math.h>

#include "common.h"
#include "decode_process_core.h"

#define DP_THREADS 1024

namespace {

struct DpParams {
  float* logits; int64_t logits_ld; int64_t V;
  const int64_t* hist; int64_t hist_ld; int64_t n;
  float penalty; int64_t ngram; int64_t min_new;
  const int64_t* eos; int32_t n_eos;
  const int64_t* bans; int32_t n_bans;
  const int64_t* word_ids; int64_t n_word_ids; const int64_t* word_off; int32_t n_words;
  uint8_t* done;
};

__device__ __forceinline__ void dp_ban(float* row, int64_t id, int64_t V) {
  const int32_t c = cmb_dp_index(id, V);
  if (c >= 0) row[c] = -INFINITY;
}

__global__ void __launch_bounds__(DP_THREADS) decode_process_kernel(DpParams p) {
  __shared__ __attribute__((aligned(16))) int32_t tile[DP_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  float* row = p.logits + (int64_t)b * p.logits_ld;
  const int64_t n = p.n;
  const int64_t* h = n > 0 ? p.hist + (int64_t)b * p.hist_ld : nullptr;

  // ---- 1. the penalty, once per distinct id ----
  if (p.penalty != 1.0f) {
    for (int64_t c0 = 0; c0 < n; c0 += DP_THREADS) {            // this lane holds position c0 + tid
      const int32_t mine = c0 + tid < n ? cmb_dp_index(h[c0 + tid], p.V) : -1;
      bool dup = mine < 0;                                        // nothing to penalise
      for (int64_t t0 = 0; t0 <= c0; t0 += DP_THREADS) {          // the positions before it, DP_THREADS at a time
        __syncthreads();                                          // the previous tile has been read
        tile[tid] = t0 == c0 ? mine : cmb_dp_index(h[t0 + tid], p.V);      // t0 < c0: t0 + tid < c0 < n
        __syncthreads();
        const int lim = t0 == c0 ? tid : DP_THREADS;              // only positions before this lane's
        for (int i = 0; i < lim && !dup; i += 4) {
          const int4 q = *reinterpret_cast<const int4*>(&tile[i]);
          dup = (q.x == mine) | ((i + 1 < lim) & (q.y == mine)) | ((i + 2 < lim) & (q.z == mine)) | ((i + 3 < lim) & (q.w == mine));
        }
      }
      if (!dup) row[mine] = cmb_dp_penalise(row[mine], p.penalty);
    }
  }
  __syncthreads();

  // ---- 2. the bans ----
  const int64_t g = p.ngram;
  if (cmb_dp_ngram_active(n, g))
    for (int64_t i = tid; i <= n - g; i += DP_THREADS)
      if (cmb_dp_ngram_hits(h, n, g, i)) dp_ban(row, h[i + g - 1], p.V);
  for (int k = tid; k < p.n_bans; k += DP_THREADS) dp_ban(row, p.bans[k], p.V);
  for (int w = tid; w < p.n_words; w += DP_THREADS) {
    int64_t first = 0;
    const int64_t m = cmb_dp_word_at(p.word_off, w, p.n_word_ids, &first);
    if (m > 0 && cmb_dp_word_hits(h, n, p.word_ids + first, m)) dp_ban(row, p.word_ids[first + m - 1], p.V);
  }
  if (n < p.min_new)
    for (int k = tid; k < p.n_eos; k += DP_THREADS) dp_ban(row, p.eos[k], p.V);
  // the row produced an id of the eos set at the last step: the selection that follows emits eos[0] for it from now on
  if (tid == 0 && p.done && p.n_eos > 0 && n >= 1 && cmb_dp_in_set(h[n - 1], p.eos, p.n_eos)) p.done[b] = 1;
}

}  // namespace

extern "C" int cmb_decode_process(float* logits, int64_t logits_ld, int32_t B, int64_t V, const int64_t* hist, int64_t hist_ld,
                                  int64_t n_hist, float penalty, int64_t ngram, int64_t min_new, const int64_t* eos, int32_t n_eos,
                                  const int64_t* bans, int32_t n_bans, const int64_t* word_ids, int64_t n_word_ids,
                                  const int64_t* word_off, int32_t n_words, uint8_t* done, void* stream) {
  const int rc = cmb_dp_check_args(logits, logits_ld, B, V, hist, hist_ld, n_hist, penalty, ngram, min_new, eos, n_eos, bans, n_bans,
                                   word_ids, n_word_ids, word_off, n_words, done);
  if (rc != CMB_OK) return rc;

  DpParams p;
  p.logits = logits; p.logits_ld = logits_ld; p.V = V;
  p.hist = hist; p.hist_ld = hist_ld; p.n = n_hist;
  p.penalty = penalty; p.ngram = ngram; p.min_new = min_new;
  p.eos = eos; p.n_eos = n_eos;
  p.bans = bans; p.n_bans = n_bans;
  p.word_ids = word_ids; p.n_word_ids = n_word_ids; p.word_off = word_off; p.n_words = n_words;
  p.done = done;
  hipLaunchKernelGGL(decode_process_kernel, dim3((unsigned)B), dim3(DP_THREADS), 0, (hipStream_t)stream, p);
  CMB_CHECK_LAUNCH();
  return CMB_OK;
}
