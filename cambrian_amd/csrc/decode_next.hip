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
// The key, the row walk, the reduction, the tail and the argument rules live in decode_select.h, which decode_sample.hip shares.
#include "decode_select.h"

namespace {

__global__ void __launch_bounds__(DN_THREADS) decode_next_kernel(DnParams p) {
  __shared__ unsigned long long red[DN_WAVES];
  __shared__ int64_t chosen;
  const int b = blockIdx.x, tid = threadIdx.x;
  unsigned long long best = 0;       // below every key: the smallest high word is -inf's, 0x007FFFFF
  dn_walk<true>(p.logits + (int64_t)b * p.logits_ld, p.V, tid, [&](float v, uint32_t i) { best = dn_max(best, dn_key(v, i)); });
  const unsigned long long m = dn_block_max(best, red, tid);
  dn_tail(p, b, tid, (int64_t)(uint32_t)~(uint32_t)m, &chosen);
}

}  // namespace

extern "C" int cmb_decode_next(const float* logits, int64_t logits_ld, int32_t B, int64_t V, int64_t eos, uint8_t* done,
                               int64_t* out_ids, int64_t out_ld, int64_t step, const int64_t* n_tok, int64_t* pos,
                               uint8_t* key_valid, int64_t kv_ld, int64_t t, const void* embed, int64_t embed_ld,
                               int64_t embed_rows, int64_t H, void* x, int64_t x_ld, int32_t hd, float rope_base, float* cos_t,
                               float* sin_t, void* stream) {
  int rc = dn_check_args(logits, logits_ld, B, V, eos, done, out_ids, out_ld, step, n_tok, pos, key_valid, kv_ld, t, embed, embed_ld,
                         embed_rows, H, x, x_ld, hd, cos_t, sin_t);
  if (rc == CMB_OK) rc = dn_check_align(logits, out_ids, n_tok, pos, embed, x);
  if (rc != CMB_OK) return rc;

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
