// decode_select.h — what the two token selection kernels share (decode_next.hip: greedy, decode_sample.hip: a filtered random
// draw): the 64-bit (value, index) key and its workgroup maximum, the walk over a row of fp32 logits of any alignment, and the
// tail that turns the chosen id into the next decode step's inputs.  One workgroup of DN_THREADS per row.
#pragma once
#include "common.h"
#include "decode_sample_core.h"

#define DN_THREADS 1024
#define DN_WAVES (DN_THREADS / 64)
#define DN_MAX_B 16

namespace {

struct DnParams {
  const float* logits; int64_t logits_ld; int64_t V;
  int64_t eos; uint8_t* done;
  int64_t* out_ids; int64_t out_ld; int64_t step;
  const int64_t* n_tok; int64_t* pos;
  uint8_t* key_valid; int64_t kv_ld; int64_t t;
  const bf16_t* embed; int64_t embed_ld; int64_t H;
  bf16_t* x; int64_t x_ld;
};

// high 32 bits: cmb_ds_key32 of the value; low 32 bits: ~index, so among equal values (and among NaNs) the LOWEST index is the
// largest key.  0 is below every key.
__device__ __forceinline__ unsigned long long dn_key(float v, uint32_t idx) {
  return ((unsigned long long)cmb_ds_key32(v) << 32) | (uint32_t)~idx;
}

__device__ __forceinline__ unsigned long long dn_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// f(value, index) for every element of the row, strided over the lanes: the floats before the first 16-byte boundary of the row
// (0..3) one by one, then whole 16-byte pieces, then the tail.  NT: the row is read once (a non-temporal load).
template <bool NT, typename F>
__device__ __forceinline__ void dn_walk(const float* row, int64_t V, int tid, F f) {
  int64_t head = (int64_t)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) >> 2);
  if (head > V) head = V;
  const int64_t pieces = (V - head) >> 2;
  const int64_t tail0 = head + (pieces << 2);
  if (tid < head) f(row[tid], (uint32_t)tid);
  const f32x4_t* vrow = reinterpret_cast<const f32x4_t*>(row + head);
#pragma unroll 4
  for (int64_t i = tid; i < pieces; i += DN_THREADS) {
    const f32x4_t v = NT ? __builtin_nontemporal_load(vrow + i) : vrow[i];
    const uint32_t at = (uint32_t)(head + (i << 2));
    f(v[0], at);
    f(v[1], at + 1);
    f(v[2], at + 2);
    f(v[3], at + 3);
  }
  if (tail0 + tid < V) f(row[tail0 + tid], (uint32_t)(tail0 + tid));
}

// the maximum of `best` over the workgroup, in every thread.  max over keys is associative and commutative, so the order of
// the reduction (xor shuffles inside a wave, then LDS across the waves) cannot change the result.  red: DN_WAVES entries.
__device__ __forceinline__ unsigned long long dn_block_max(unsigned long long best, unsigned long long* red, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = dn_max(best, __shfl_xor(best, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = best;
  __syncthreads();
  unsigned long long m = red[0];
#pragma unroll
  for (int w = 1; w < DN_WAVES; ++w) m = dn_max(m, red[w]);
  return m;
}

// ---- the radix select both filtered selections share (decode_sample.hip: top-k / top-p, decode_beam.hip: a row's K largest) ----
#define DS_BINS 2048

struct DsFound {
  uint32_t bin;
  unsigned long long before, total;
};

// The bin of h[0 .. DS_BINS) at which the running sum reaches `target` (1 <= target <= total), and the sum before that bin;
// REV: the running sum starts at the last bin.  top_p >= 0: the target is the nucleus target of the total.  Thread t owns two
// bins that follow each other in scan order; an inclusive scan by shuffles inside a wave, the wave totals through LDS.
// The caller has a barrier between the last atomic on h and this call.
template <typename T, bool REV>
__device__ __forceinline__ DsFound ds_find(const T* h, unsigned long long target, float top_p, int tid, unsigned long long* wsum,
                                           unsigned long long* found) {
  const int lane = tid & 63, wave = tid >> 6;
  const int i0 = REV ? DS_BINS - 1 - 2 * tid : 2 * tid, i1 = REV ? i0 - 1 : i0 + 1;
  const unsigned long long a = h[i0], s = a + h[i1];
  unsigned long long inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  unsigned long long off = 0, total = 0;
#pragma unroll
  for (int w = 0; w < DN_WAVES; ++w) {
    const unsigned long long ws = wsum[w];
    if (w < wave) off += ws;
    total += ws;
  }
  if (top_p >= 0.f) target = cmb_ds_nucleus_target(top_p, total) + 1;
  inc += off;
  const unsigned long long exc = inc - s;
  if (exc < target && target <= inc) {
    const bool first = exc + a >= target;
    found[0] = (unsigned long long)(first ? i0 : i1);
    found[1] = first ? exc : exc + a;
  }
  __syncthreads();
  DsFound r;
  r.bin = (uint32_t)found[0];
  r.before = found[1];
  r.total = total;
  return r;
}

// thread 0 applies the eos rule to the id it was given and writes the id, the position and the key-mask byte; the whole
// workgroup copies the embedding row in 16-byte pieces.  `chosen`: one int64 of LDS.
__device__ __forceinline__ void dn_tail(const DnParams& p, int b, int tid, int64_t nxt, int64_t* chosen) {
  if (tid == 0) {
    if (p.eos >= 0) {
      if (p.done[b]) nxt = p.eos;
      if (nxt == p.eos) p.done[b] = 1;
    }
    p.out_ids[(int64_t)b * p.out_ld + p.step] = nxt;
    p.pos[b] = p.n_tok[b] + p.step;
    p.key_valid[(int64_t)b * p.kv_ld + p.t] = 1;
    *chosen = nxt;
  }
  __syncthreads();
  const bf16x8_t* src = reinterpret_cast<const bf16x8_t*>(p.embed + *chosen * p.embed_ld);
  bf16x8_t* dst = reinterpret_cast<bf16x8_t*>(p.x + (int64_t)b * p.x_ld);
  for (int64_t i = tid; i < (p.H >> 3); i += DN_THREADS) dst[i] = src[i];
}

// the argument rules both entry points share, in cmb_decode_next's order: dn_check_args (NULL pointers, then sizes and strides;
// CMB_ERR_BAD_ARG), then dn_check_align (CMB_ERR_ALIGNMENT)
static inline int dn_check_args(const float* logits, int64_t logits_ld, int32_t B, int64_t V, int64_t eos, const uint8_t* done,
                                const int64_t* out_ids, int64_t out_ld, int64_t step, const int64_t* n_tok, const int64_t* pos,
                                const uint8_t* key_valid, int64_t kv_ld, int64_t t, const void* embed, int64_t embed_ld,
                                int64_t embed_rows, int64_t H, const void* x, int64_t x_ld, int32_t hd, const float* cos_t,
                                const float* sin_t) {
  if (!logits || !out_ids || !n_tok || !pos || !key_valid || !embed || !x || !cos_t || !sin_t) return CMB_ERR_BAD_ARG;
  if (B < 1 || B > DN_MAX_B || V < 1 || V > 0x7FFFFFFFll || logits_ld < V || embed_rows < V) return CMB_ERR_BAD_ARG;
  if (eos < -1 || eos >= embed_rows || (eos >= 0 && !done)) return CMB_ERR_BAD_ARG;
  if (step < 0 || step >= out_ld || t < 0 || t >= kv_ld) return CMB_ERR_BAD_ARG;
  if (H < 8 || H % 8 || embed_ld < H || embed_ld % 8 || x_ld < H || x_ld % 8 || hd <= 0 || (hd & 1)) return CMB_ERR_BAD_ARG;
  return CMB_OK;
}

static inline int dn_check_align(const float* logits, const int64_t* out_ids, const int64_t* n_tok, const int64_t* pos,
                                 const void* embed, const void* x) {
  if (((uintptr_t)logits & 3u) || ((uintptr_t)out_ids & 7u) || ((uintptr_t)n_tok & 7u) || ((uintptr_t)pos & 7u) ||
      !cmb_aligned16(embed) || !cmb_aligned16(x))
    return CMB_ERR_ALIGNMENT;
  return CMB_OK;
}

}  // namespace
