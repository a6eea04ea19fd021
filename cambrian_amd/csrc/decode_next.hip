// decode_next.hip — greedy token selection of generate() and the next decode step's inputs in one launch (cmb_decode_next):
// what the host loop did with about ten small ATen launches between two steps (argmax, where, ==, |, the key-mask write, the
// position add, the embedding lookup and its cast) and, with an eos id, a blocking read of `done` per token.
// Roofline class: HBM / L2 (a row of fp32 logits is read once: 513 KB at V = 128256; everything else is a few KB).
//
// One workgroup of DN_THREADS per row.  The row is strided over the lanes in 16-byte pieces (a scalar head up to the first
// 16-byte boundary and a scalar tail, so any row stride is taken); every lane keeps the best (value, index) it has seen as ONE
// 64-bit key whose unsigned order is torch.argmax's order:
//   high 32 bits: the float's bits mapped monotonically (negative: all bits flipped, else the sign bit set), -0 read as +0,
//                 any NaN as 0xFFFFFFFF — above +inf;
//   low 32 bits:  ~index, so among equal values (and among NaNs) the LOWEST index is the largest key.
// max over keys is associative and commutative, so the order of the reduction (xor shuffles inside a wave, then LDS across
// the waves) cannot change the result: the same bits on every run, no atomics.  Thread 0 then applies the eos rule and
// writes the id, the position and the key-mask byte; the whole workgroup copies the embedding row in 16-byte pieces.
#include "common.h"

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

__device__ __forceinline__ unsigned long long dn_key(float v, uint32_t idx) {
  uint32_t b = __builtin_bit_cast(uint32_t, v);
  uint32_t k;
  if (v != v) k = 0xFFFFFFFFu;
  else if (v == 0.f) k = 0x80000000u;
  else k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((unsigned long long)k << 32) | (uint32_t)~idx;
}

__device__ __forceinline__ unsigned long long dn_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

__global__ void __launch_bounds__(DN_THREADS) decode_next_kernel(DnParams p) {
  __shared__ unsigned long long red[DN_WAVES];
  __shared__ int64_t chosen;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = p.logits + (int64_t)b * p.logits_ld;
  const int64_t V = p.V;

  // floats before the first 16-byte boundary of the row (0..3), then whole pieces, then the tail
  int64_t head = (int64_t)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) >> 2);
  if (head > V) head = V;
  const int64_t pieces = (V - head) >> 2;
  const int64_t tail0 = head + (pieces << 2);

  unsigned long long best = 0;       // below every key: the smallest high word is -inf's, 0x007FFFFF
  if (tid < head) best = dn_key(row[tid], (uint32_t)tid);
  const f32x4_t* vrow = reinterpret_cast<const f32x4_t*>(row + head);
#pragma unroll 4
  for (int64_t i = tid; i < pieces; i += DN_THREADS) {
    const f32x4_t v = __builtin_nontemporal_load(vrow + i);
    const uint32_t at = (uint32_t)(head + (i << 2));
    best = dn_max(best, dn_max(dn_max(dn_key(v[0], at), dn_key(v[1], at + 1)), dn_max(dn_key(v[2], at + 2), dn_key(v[3], at + 3))));
  }
  if (tail0 + tid < V) best = dn_max(best, dn_key(row[tail0 + tid], (uint32_t)(tail0 + tid)));

#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = dn_max(best, __shfl_xor(best, o, 64));
  if (lane == 0) red[wave] = best;
  __syncthreads();
  if (tid == 0) {
    unsigned long long m = red[0];
#pragma unroll
    for (int w = 1; w < DN_WAVES; ++w) m = dn_max(m, red[w]);
    int64_t nxt = (int64_t)(uint32_t)~(uint32_t)m;
    if (p.eos >= 0) {
      if (p.done[b]) nxt = p.eos;
      if (nxt == p.eos) p.done[b] = 1;
    }
    p.out_ids[(int64_t)b * p.out_ld + p.step] = nxt;
    p.pos[b] = p.n_tok[b] + p.step;
    p.key_valid[(int64_t)b * p.kv_ld + p.t] = 1;
    chosen = nxt;
  }
  __syncthreads();
  const bf16x8_t* src = reinterpret_cast<const bf16x8_t*>(p.embed + chosen * p.embed_ld);
  bf16x8_t* dst = reinterpret_cast<bf16x8_t*>(p.x + (int64_t)b * p.x_ld);
  for (int64_t i = tid; i < (p.H >> 3); i += DN_THREADS) dst[i] = src[i];
}

}  // namespace

extern "C" int cmb_decode_next(const float* logits, int64_t logits_ld, int32_t B, int64_t V, int64_t eos, uint8_t* done,
                               int64_t* out_ids, int64_t out_ld, int64_t step, const int64_t* n_tok, int64_t* pos,
                               uint8_t* key_valid, int64_t kv_ld, int64_t t, const void* embed, int64_t embed_ld,
                               int64_t embed_rows, int64_t H, void* x, int64_t x_ld, int32_t hd, float rope_base, float* cos_t,
                               float* sin_t, void* stream) {
  if (!logits || !out_ids || !n_tok || !pos || !key_valid || !embed || !x || !cos_t || !sin_t) return CMB_ERR_BAD_ARG;
  if (B < 1 || B > DN_MAX_B || V < 1 || V > 0x7FFFFFFFll || logits_ld < V || embed_rows < V) return CMB_ERR_BAD_ARG;
  if (eos < -1 || eos >= embed_rows || (eos >= 0 && !done)) return CMB_ERR_BAD_ARG;
  if (step < 0 || step >= out_ld || t < 0 || t >= kv_ld) return CMB_ERR_BAD_ARG;
  if (H < 8 || H % 8 || embed_ld < H || embed_ld % 8 || x_ld < H || x_ld % 8 || hd <= 0 || (hd & 1)) return CMB_ERR_BAD_ARG;
  if (((uintptr_t)logits & 3u) || ((uintptr_t)out_ids & 7u) || ((uintptr_t)n_tok & 7u) || ((uintptr_t)pos & 7u) ||
      !cmb_aligned16(embed) || !cmb_aligned16(x))
    return CMB_ERR_ALIGNMENT;

  DnParams p;
  p.logits = logits; p.logits_ld = logits_ld; p.V = V;
  p.eos = eos; p.done = done;
  p.out_ids = out_ids; p.out_ld = out_ld; p.step = step;
  p.n_tok = n_tok; p.pos = pos;
  p.key_valid = key_valid; p.kv_ld = kv_ld; p.t = t;
  p.embed = (const bf16_t*)embed; p.embed_ld = embed_ld; p.H = H;
  p.x = (bf16_t*)x; p.x_ld = x_ld;
  hipLaunchKernelGGL(decode_next_kernel, dim3((unsigned)B), dim3(DN_THREADS), 0, (hipStream_t)stream, p);
  CMB_CHECK_LAUNCH();
  return cmb_rope_table(pos, B, hd, rope_base, cos_t, sin_t, stream);
}
