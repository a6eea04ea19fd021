// decode_beam.hip — beam search between two decode steps of generate() (cmb_decode_beam): what the host did with a log_softmax,
// two topk's, a dozen gathers and an index_select of every layer's whole cache per token.  num_beams beams of a prompt are
// num_beams rows of the decode step; three launches (+ the RoPE-table launch), ordered by the stream alone:
//
//   rows     one workgroup of DN_THREADS per row, on decode_select.h's walk, keys and radix select: the row maximum, the
//            log-sum-exp from cmb_ds_mass fixed-point masses (integer sums: the same bits in any order), and the row's
//            min(K, V) largest logits (K = 2 num_beams) with their indices, equal logits at the cut resolved to the LOWEST
//            indices — the select runs over the 64-bit (value, ~index) key, its three index digits only when equal values
//            straddle the cut.  Written as log-probabilities, descending, into the state block.
//            Roofline class: L2 (a row of fp32 logits is swept four times by ONE workgroup, seven with a tie at the cut:
//            513 KB at V = 128256; HBM sees it once).
//   group    one workgroup per prompt: score = run_score + log-probability for the <= 512 candidates, their rank under
//            cmb_beam_key by counting, then ONE thread runs cmb_beam_step (decode_beam_core.h: running beams, hypotheses, the
//            merge, the flag) on the top K; the workgroup writes the sequences (the running ones double-buffered: a child
//            copies its parent's prefix from the other half, no walk over the steps) and does decode_next's tail for its
//            rows: pos, the key-mask byte, the embedding row.
//   reorder  every layer's K and V cache in place, generated columns L0 .. t-1 only (the prompt's columns are the same in
//            every beam of a prompt): row i takes row parent[i]'s values.  A thread owns one 16-byte piece of all num_beams
//            rows of a prompt and loads every child's source before it stores any, so swaps and a parent with several children
//            need no second buffer; a prompt whose parents are the identity is skipped.  Its first thread also folds the
//            prompts' flags into the `unfinished` byte.  Roofline class: HBM / L2 (2 x generated columns x layers x 2 x nkv
//            x hd x num_beams x 2 bytes).
// No floating-point atomics, no global scratch beyond the state block; the result has the same bits on every run and a
// prompt's result does not depend on the other prompts.
//
// A row's candidates are chosen by logit, the prompt's by score: within a row the score is a monotone function of the logit,
// so the prompt's top K are among the rows' top K — except where two DIFFERENT logits at a row's cut round to the SAME score
// and the dropped one has the lower index (the restatement would then order them by index).
#include "decode_select.h"
#include "decode_beam_core.h"

#define DB_GROUP_THREADS 512      /* >= CMB_BEAM_MAX * CMB_BEAM_MAXK candidates of a prompt */
#define DB_REORDER_THREADS 256
#define DB_REORDER_LAYERS 64      /* cache pointers of one reorder launch (a kernel argument) */

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// rows
// ---------------------------------------------------------------------------------------------------------------------
struct DbRowParams {
  const float* logits; int64_t logits_ld; int64_t V;
  int32_t K;
  float* cand_lp; int32_t* cand_tok;
};

__global__ void __launch_bounds__(DN_THREADS) decode_beam_rows_kernel(DbRowParams p) {
  __shared__ uint32_t hist[DS_BINS];
  __shared__ unsigned long long red[DN_WAVES], wsum[DN_WAVES], found[2];
  __shared__ unsigned long long list[CMB_BEAM_MAXK];
  __shared__ uint32_t n_list;
  const int r = blockIdx.x, tid = threadIdx.x;
  const float* row = p.logits + (int64_t)r * p.logits_ld;
  const int64_t V = p.V;
  const int K = p.K, Kr = V < K ? (int)V : K;

  // ---- sweep 1: the maximum and the count histogram of the top 11 key bits
  hist[tid] = 0;
  hist[tid + DN_THREADS] = 0;
  if (tid == 0) n_list = 0;
  __syncthreads();
  unsigned long long best = 0;
  dn_walk<false>(row, V, tid, [&](float v, uint32_t i) {
    best = dn_max(best, dn_key(v, i));
    atomicAdd(&hist[cmb_ds_key32(v) >> 21], 1u);
  });
  const unsigned long long m = dn_block_max(best, red, tid);
  const float v_max = cmb_ds_key32_value((uint32_t)(m >> 32));

  // ---- the Kr-th largest key32, 11 + 11 + 10 bits; the masses ride on the second sweep
  DsFound f = ds_find<uint32_t, true>(hist, (unsigned long long)Kr, -1.f, tid, wsum, found);
  uint32_t prefix = f.bin;
  unsigned long long rem = (unsigned long long)Kr - f.before;
  unsigned long long mass = 0;
#pragma unroll
  for (int pass = 1; pass < 3; ++pass) {
    const int have = pass == 1 ? 21 : 10, shift = pass == 1 ? 10 : 0;
    hist[tid] = 0;
    hist[tid + DN_THREADS] = 0;
    __syncthreads();
    dn_walk<false>(row, V, tid, [&](float v, uint32_t) {
      const uint32_t key = cmb_ds_key32(v);
      if (pass == 1) mass += cmb_ds_mass(v, v_max);
      if ((key >> have) == prefix) atomicAdd(&hist[(key >> shift) & (pass == 1 ? 2047u : 1023u)], 1u);
    });
    __syncthreads();
    f = ds_find<uint32_t, true>(hist, rem, -1.f, tid, wsum, found);
    prefix = (prefix << (pass == 1 ? 11 : 10)) | f.bin;
    rem -= f.before;
  }
  // rem of the elements equal to the cut value are taken: all of them, or those with the lowest indices = the largest ~index
  uint32_t low = 0;
  if ((unsigned long long)hist[f.bin] != rem) {
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
      const int have = pass == 1 ? 21 : 10, shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
      __syncthreads();                                 // every thread has read hist[f.bin] / finished ds_find
      hist[tid] = 0;
      hist[tid + DN_THREADS] = 0;
      __syncthreads();
      dn_walk<false>(row, V, tid, [&](float v, uint32_t i) {
        const uint32_t u = ~i;
        if (cmb_ds_key32(v) == prefix && (pass == 0 || (u >> have) == low))
          atomicAdd(&hist[(u >> shift) & (pass == 2 ? 1023u : 2047u)], 1u);
      });
      __syncthreads();
      f = ds_find<uint32_t, true>(hist, rem, -1.f, tid, wsum, found);
      low = pass == 0 ? f.bin : (low << (pass == 1 ? 11 : 10)) | f.bin;
      rem -= f.before;
    }
  }
  const unsigned long long cut = ((unsigned long long)prefix << 32) | low;

  // ---- the row's log-sum-exp: integer sums, any order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mass += __shfl_xor(mass, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = mass;         // dn_block_max's reads of red lie before ds_find's barriers

  // ---- the Kr elements at or above the cut, then their order by counting
  dn_walk<false>(row, V, tid, [&](float v, uint32_t i) {
    const unsigned long long k = dn_key(v, i);
    if (k >= cut) {
      const uint32_t at = atomicAdd(&n_list, 1u);
      if (at < CMB_BEAM_MAXK) list[at] = k;
    }
  });
  __syncthreads();
  const int n = n_list < (uint32_t)Kr ? (int)n_list : Kr;
  if (tid < K) {
    float lp = __builtin_nanf("");
    int32_t tok = -1;
    int at = tid;
    if (tid < n) {
      unsigned long long total = 0;
#pragma unroll
      for (int w = 0; w < DN_WAVES; ++w) total += red[w];
      const float log_z = logf((float)((double)total * (1.0 / 1099511627776.0)));
      const unsigned long long k = list[tid];
      int rank = 0;
      for (int j = 0; j < n; ++j) rank += list[j] > k;
      lp = (cmb_ds_key32_value((uint32_t)(k >> 32)) - v_max) - log_z;
      tok = (int32_t)(uint32_t)~(uint32_t)k;
      at = rank;
    }
    p.cand_lp[(int64_t)r * K + at] = lp;               // slots n .. K-1 (a row shorter than K) are marked empty
    p.cand_tok[(int64_t)r * K + at] = tok;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// group
// ---------------------------------------------------------------------------------------------------------------------
struct DbGroupParams {
  int32_t nb, last;
  int64_t V, eos, step, M;
  uint8_t* state;
  cmb_beam_layout lay;
  const int64_t* n_tok; int64_t* pos;
  uint8_t* key_valid; int64_t kv_ld; int64_t t;
  const bf16_t* embed; int64_t embed_ld; int64_t H;
  bf16_t* x; int64_t x_ld;
};

template <typename T>
__device__ __forceinline__ T* db_section(const DbGroupParams& p, int which) {
  return reinterpret_cast<T*>(p.state + p.lay.off[which]);
}

__global__ void __launch_bounds__(DB_GROUP_THREADS) decode_beam_group_kernel(DbGroupParams p) {
  __shared__ unsigned long long keys[CMB_BEAM_MAX * CMB_BEAM_MAXK];
  __shared__ cmb_beam_cand top[CMB_BEAM_MAXK];
  __shared__ cmb_beam_prompt P;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nb = p.nb, K = 2 * nb, Kr = p.V < K ? (int)p.V : K, n = nb * Kr;
  const int64_t M = p.M, step = p.step, row0 = (int64_t)b * nb;
  float* run_score = db_section<float>(p, CMB_BEAM_RUN_SCORE) + row0;
  float* fin_score = db_section<float>(p, CMB_BEAM_FIN_SCORE) + row0;
  int32_t* fin_len = db_section<int32_t>(p, CMB_BEAM_FIN_LEN) + row0;
  uint8_t* fin_ok = db_section<uint8_t>(p, CMB_BEAM_FIN_OK) + row0;
  uint8_t* unsat = db_section<uint8_t>(p, CMB_BEAM_UNSAT) + b;
  const float* cand_lp = db_section<float>(p, CMB_BEAM_CAND_LP) + row0 * K;
  const int32_t* cand_tok = db_section<int32_t>(p, CMB_BEAM_CAND_TOK) + row0 * K;
  const int64_t* run_old = db_section<int64_t>(p, CMB_BEAM_RUN_IDS) + ((step & 1) * gridDim.x * nb + row0) * M;
  int64_t* run_new = db_section<int64_t>(p, CMB_BEAM_RUN_IDS) + (((step + 1) & 1) * gridDim.x * nb + row0) * M;
  int64_t* fin_ids = db_section<int64_t>(p, CMB_BEAM_FIN_IDS) + row0 * M;

  // ---- the prompt's state (step 0 starts from the initial one, whatever the block holds)
  if (tid == 0) {
    if (step == 0) {
      cmb_beam_init(&P, nb);
    } else {
      for (int i = 0; i < nb; ++i) {
        P.run_score[i] = run_score[i];
        P.fin_score[i] = fin_score[i];
        P.fin_len[i] = fin_len[i];
        P.fin_ok[i] = fin_ok[i];
      }
      P.unsat = *unsat;
    }
  }
  __syncthreads();

  // ---- candidates: score, key, rank by counting; the top K in order
  cmb_beam_cand mine;
  unsigned long long key = 0;
  if (tid < n) {
    const int beam = tid / Kr, c = tid - beam * Kr;
    mine.beam = beam;
    mine.tok = cand_tok[beam * K + c];
    if ((uint32_t)mine.tok >= (uint32_t)p.V) mine.tok = 0;        // an empty slot cannot be among the first Kr; stay in range
    mine.score = P.run_score[beam] + cand_lp[beam * K + c];
    key = cmb_beam_key(mine.score, (uint32_t)((int64_t)beam * p.V + mine.tok));
    keys[tid] = key;
  }
  __syncthreads();
  if (tid < n) {
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += keys[j] > key;
    if (rank < K) top[rank] = mine;
  }
  __syncthreads();
  if (tid == 0) {
    cmb_beam_step(&P, top, nb, step, p.eos, p.last);
    for (int i = 0; i < nb; ++i) {
      run_score[i] = P.run_score[i];
      fin_score[i] = P.fin_score[i];
      fin_len[i] = P.fin_len[i];
      fin_ok[i] = P.fin_ok[i];
      db_section<int32_t>(p, CMB_BEAM_PARENT)[row0 + i] = P.parent[i];
      db_section<int32_t>(p, CMB_BEAM_TOK)[row0 + i] = P.tok[i];
    }
    *unsat = P.unsat;
    db_section<uint8_t>(p, CMB_BEAM_ALL_HIT)[b] = P.all_hit;
  }
  __syncthreads();

  // ---- the running sequences: child i = its parent's prefix from the other half + its token
  const int64_t cols = step + 1;
  for (int64_t at = tid; at < nb * cols; at += DB_GROUP_THREADS) {
    const int i = (int)(at / cols);
    const int64_t c = at - i * cols;
    run_new[i * M + c] = c < step ? run_old[P.parent[i] * M + c] : (int64_t)P.tok[i];
  }
  // ---- the kept hypotheses: a thread owns a column and reads all of it before it writes
  if (P.fin_moved)
    for (int64_t c = tid; c < cols; c += DB_GROUP_THREADS) {
      int64_t val[CMB_BEAM_MAX];
#pragma unroll
      for (int i = 0; i < CMB_BEAM_MAX; ++i)
        if (i < nb) {
          const int src = P.fin_src[i];
          if (src < nb) {
            val[i] = fin_ids[src * M + c];
          } else {
            const cmb_beam_cand cand = top[src - nb];
            val[i] = c < step ? run_old[cand.beam * M + c] : (int64_t)cand.tok;
          }
        }
#pragma unroll
      for (int i = 0; i < CMB_BEAM_MAX; ++i)
        if (i < nb) fin_ids[i * M + c] = val[i];
    }
  // ---- decode_next's tail for the prompt's rows
  if (tid < nb) {
    p.pos[row0 + tid] = p.n_tok[row0 + tid] + step;
    p.key_valid[(row0 + tid) * p.kv_ld + p.t] = 1;
  }
  const int64_t pieces = p.H >> 3;
  for (int64_t at = tid; at < nb * pieces; at += DB_GROUP_THREADS) {
    const int i = (int)(at / pieces);
    const int64_t piece = at - i * pieces;
    reinterpret_cast<bf16x8_t*>(p.x + (row0 + i) * p.x_ld)[piece] =
        reinterpret_cast<const bf16x8_t*>(p.embed + (int64_t)P.tok[i] * p.embed_ld)[piece];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// reorder
// ---------------------------------------------------------------------------------------------------------------------
struct DbReorderParams {
  bf16_t* cache[2 * DB_REORDER_LAYERS];     // launch-local layer l: K at 2 l, V at 2 l + 1
  int32_t nb, prompts, nkv, pieces;         // pieces: hd / 8
  int64_t L0, G;                            // generated columns L0 .. L0 + G - 1
  int64_t c_sb, c_sh, c_st;
  const int32_t* parent;
  const uint8_t* unsat; const uint8_t* all_hit; uint8_t* unfinished;   // unfinished NULL: not written
};

__global__ void __launch_bounds__(DB_REORDER_THREADS) decode_beam_reorder_kernel(DbReorderParams p) {
  if (p.unfinished && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    bool any_unsat = false, all_hit = true;
    for (int b = 0; b < p.prompts; ++b) {
      any_unsat |= p.unsat[b] != 0;
      all_hit &= p.all_hit[b] != 0;
    }
    *p.unfinished = (uint8_t)(any_unsat && !all_hit);
  }
  const int64_t items = (int64_t)p.prompts * p.nkv * p.G * p.pieces;
  const int64_t at = (int64_t)blockIdx.x * DB_REORDER_THREADS + threadIdx.x;
  if (at >= items) return;
  const int piece = (int)(at % p.pieces);
  int64_t rest = at / p.pieces;
  const int64_t c = rest % p.G;
  rest /= p.G;
  const int h = (int)(rest % p.nkv), b = (int)(rest / p.nkv);
  const int nb = p.nb;
  int par[CMB_BEAM_MAX];
  bool identity = true;
#pragma unroll
  for (int i = 0; i < CMB_BEAM_MAX; ++i)
    if (i < nb) {
      par[i] = p.parent[b * nb + i];
      if ((unsigned)par[i] >= (unsigned)nb) par[i] = i;      // not a slot of this prompt: the row stays
      identity &= par[i] == i;
    }
  if (identity) return;
  bf16_t* base = p.cache[blockIdx.y] + (int64_t)b * nb * p.c_sb + h * p.c_sh + (p.L0 + c) * p.c_st + piece * 8;
  bf16x8_t val[CMB_BEAM_MAX];
#pragma unroll
  for (int i = 0; i < CMB_BEAM_MAX; ++i)
    if (i < nb) val[i] = *reinterpret_cast<const bf16x8_t*>(base + par[i] * p.c_sb);
#pragma unroll
  for (int i = 0; i < CMB_BEAM_MAX; ++i)
    if (i < nb && par[i] != i) *reinterpret_cast<bf16x8_t*>(base + i * p.c_sb) = val[i];
}

// the rules of the cache description, in order: BAD_ARG (pointers, geometry, strides, the column range), then ALIGNMENT
int db_check_caches(const cmb_decode_step_desc* d, const cmb_decode_layer* layers, int32_t rows, int64_t L0, int64_t t) {
  if (d->layers < 1 || d->B != rows || d->nkv < 1 || d->hd < 8 || d->hd % 8) return CMB_ERR_BAD_ARG;
  if (d->c_sb < 0 || d->c_sh < 0 || d->c_st < d->hd || L0 < 0 || L0 > t) return CMB_ERR_BAD_ARG;
  for (int l = 0; l < d->layers; ++l)
    if (!layers[l].kcache || !layers[l].vcache) return CMB_ERR_BAD_ARG;
  if (d->c_sb % 8 || d->c_sh % 8 || d->c_st % 8) return CMB_ERR_ALIGNMENT;
  for (int l = 0; l < d->layers; ++l)
    if (!cmb_aligned16(layers[l].kcache) || !cmb_aligned16(layers[l].vcache)) return CMB_ERR_ALIGNMENT;
  return CMB_OK;
}

// d NULL: no caches, one workgroup for the `unfinished` byte
int db_reorder(const cmb_decode_step_desc* d, const cmb_decode_layer* layers, const int32_t* parent, int32_t prompts, int32_t nb,
               int64_t L0, int64_t t, const uint8_t* unsat, const uint8_t* all_hit, uint8_t* unfinished, hipStream_t stream) {
  DbReorderParams p;
  p.nb = nb; p.prompts = prompts;
  p.nkv = d ? d->nkv : 0; p.pieces = d ? d->hd / 8 : 0;
  p.L0 = L0; p.G = d ? t - L0 : 0;
  p.c_sb = d ? d->c_sb : 0; p.c_sh = d ? d->c_sh : 0; p.c_st = d ? d->c_st : 0;
  p.parent = parent; p.unsat = unsat; p.all_hit = all_hit; p.unfinished = unfinished;
  const int64_t items = (int64_t)prompts * p.nkv * p.G * p.pieces;
  const int n_layers = items > 0 ? d->layers : 0;
  if (!n_layers && !unfinished) return CMB_OK;
  int l0 = 0;
  do {
    const int n = n_layers - l0 < DB_REORDER_LAYERS ? n_layers - l0 : DB_REORDER_LAYERS;
    for (int l = 0; l < n; ++l) {
      p.cache[2 * l] = (bf16_t*)layers[l0 + l].kcache;
      p.cache[2 * l + 1] = (bf16_t*)layers[l0 + l].vcache;
    }
    const unsigned gx = n ? (unsigned)((items + DB_REORDER_THREADS - 1) / DB_REORDER_THREADS) : 1u;
    hipLaunchKernelGGL(decode_beam_reorder_kernel, dim3(gx, n ? 2u * n : 1u), dim3(DB_REORDER_THREADS), 0, stream, p);
    CMB_CHECK_LAUNCH();
    p.unfinished = nullptr;
    l0 += n;
  } while (l0 < n_layers);
  return CMB_OK;
}

}  // namespace

extern "C" int64_t cmb_decode_beam_state_bytes(int32_t prompts, int32_t num_beams, int64_t max_new) {
  if (prompts < 1 || num_beams < 2 || num_beams > CMB_BEAM_MAX || (int64_t)prompts * num_beams > DN_MAX_B || max_new < 1 ||
      max_new > 0x7FFFFFFFll)
    return CMB_ERR_BAD_ARG;
  return cmb_beam_make_layout(prompts, num_beams, max_new).total;
}

extern "C" int cmb_decode_beam_reorder(const cmb_decode_step_desc* d, const cmb_decode_layer* layers, const int32_t* parent,
                                       int32_t num_beams, int64_t L0, int64_t t, void* stream) {
  if (!d || !layers || !parent) return CMB_ERR_BAD_ARG;
  if (d->B < 1 || d->B > DN_MAX_B || num_beams < 2 || num_beams > CMB_BEAM_MAX || d->B % num_beams) return CMB_ERR_BAD_ARG;
  int rc = db_check_caches(d, layers, d->B, L0, t);
  if (rc != CMB_OK) return rc;
  if ((uintptr_t)parent & 3u) return CMB_ERR_ALIGNMENT;
  return db_reorder(d, layers, parent, d->B / num_beams, num_beams, L0, t, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int cmb_decode_beam(const float* logits, int64_t logits_ld, int32_t rows, int32_t num_beams, int64_t V, int64_t eos,
                               void* state, int64_t state_bytes, int64_t step, int64_t max_new, const int64_t* n_tok,
                               int64_t* pos, uint8_t* key_valid, int64_t kv_ld, int64_t t, const void* embed, int64_t embed_ld,
                               int64_t embed_rows, int64_t H, void* x, int64_t x_ld, int32_t hd, float rope_base, float* cos_t,
                               float* sin_t, const cmb_decode_step_desc* d, const cmb_decode_layer* layers, int64_t L0,
                               uint8_t* unfinished, void* stream) {
  if (!state || !unfinished || (d == nullptr) != (layers == nullptr)) return CMB_ERR_BAD_ARG;
  // cmb_decode_next's rules in its order; the state block stands in for `done` and `out_ids` (max_new columns)
  int rc = dn_check_args(logits, logits_ld, rows, V, eos, (const uint8_t*)state, (const int64_t*)state, max_new, step, n_tok, pos,
                         key_valid, kv_ld, t, embed, embed_ld, embed_rows, H, x, x_ld, hd, cos_t, sin_t);
  if (rc != CMB_OK) return rc;
  if (num_beams < 2 || num_beams > CMB_BEAM_MAX || rows % num_beams || V < 2 || V * num_beams >= 0x80000000ll ||
      max_new > 0x7FFFFFFFll)
    return CMB_ERR_BAD_ARG;
  const int32_t prompts = rows / num_beams;
  const cmb_beam_layout lay = cmb_beam_make_layout(prompts, num_beams, max_new);
  if (state_bytes < lay.total) return CMB_ERR_WORKSPACE;
  if (d) {
    rc = db_check_caches(d, layers, rows, L0, t);
    if (rc == CMB_ERR_BAD_ARG) return rc;
  }
  int align = dn_check_align(logits, (const int64_t*)state, n_tok, pos, embed, x);
  if (align == CMB_OK && !cmb_aligned16(state)) align = CMB_ERR_ALIGNMENT;
  if (align != CMB_OK) return align;
  if (rc != CMB_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  uint8_t* st = (uint8_t*)state;

  DbRowParams rp;
  rp.logits = logits; rp.logits_ld = logits_ld; rp.V = V; rp.K = 2 * num_beams;
  rp.cand_lp = (float*)(st + lay.off[CMB_BEAM_CAND_LP]);
  rp.cand_tok = (int32_t*)(st + lay.off[CMB_BEAM_CAND_TOK]);
  hipLaunchKernelGGL(decode_beam_rows_kernel, dim3((unsigned)rows), dim3(DN_THREADS), 0, s, rp);
  CMB_CHECK_LAUNCH();

  DbGroupParams gp;
  gp.nb = num_beams; gp.last = step + 1 == max_new;
  gp.V = V; gp.eos = eos; gp.step = step; gp.M = max_new;
  gp.state = st; gp.lay = lay;
  gp.n_tok = n_tok; gp.pos = pos;
  gp.key_valid = key_valid; gp.kv_ld = kv_ld; gp.t = t;
  gp.embed = (const bf16_t*)embed; gp.embed_ld = embed_ld; gp.H = H;
  gp.x = (bf16_t*)x; gp.x_ld = x_ld;
  hipLaunchKernelGGL(decode_beam_group_kernel, dim3((unsigned)prompts), dim3(DB_GROUP_THREADS), 0, s, gp);
  CMB_CHECK_LAUNCH();

  rc = db_reorder(d, layers, (const int32_t*)(st + lay.off[CMB_BEAM_PARENT]), prompts, num_beams, L0, t,
                  st + lay.off[CMB_BEAM_UNSAT], st + lay.off[CMB_BEAM_ALL_HIT], unfinished, s);
  if (rc != CMB_OK) return rc;
  return cmb_rope_table(pos, rows, hd, rope_base, cos_t, sin_t, stream);
}
