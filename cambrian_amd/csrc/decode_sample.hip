// decode_sample.hip — sampled token selection of generate() and the next decode step's inputs in one launch (cmb_decode_sample):
// cmb_decode_next's contract with the argmax replaced by temperature -> top-k -> top-p -> a random draw, which the host loop
// did with about twenty ATen launches (a topk and a full sort of the vocabulary among them) and, with an eos id, a blocking read
// of `done` per token.
// Roofline class: L2 (a row of fp32 logits is read up to seven times by ONE workgroup: 513 KB at V = 128256, which neither the
// 128 VGPRs a 1024-thread workgroup leaves per lane nor the LDS hold; HBM sees it once).
//
// One workgroup of DN_THREADS per row b, z_i = logits[b, i] * inv_temperature:
//   sweep 1   decode_next's argmax of the row (64-bit keys) and, with top-k, the count histogram of the top 11 bits of key32(z).
//             A maximum that is not finite (a NaN, +inf, every logit -inf, or a z_max that overflowed) ends here: the id is the
//             argmax.
//   top-k     radix select of the k-th largest key32(z), 11 + 11 + 10 bits: sweeps 1..3, integer LDS histograms of DS_BINS bins;
//             after each, a workgroup scan from the top finds the bin that holds the k-th element.  Exact; ties at the k-th
//             value are kept.
//   top-p     the same select from the bottom over fixed-point masses (cmb_ds_mass: exp(z - z_max) in units of 2^-40, uint64
//             LDS atomics, so the sums are exact integers in any order) of the elements top-k kept: sweeps 4..6.  The first
//             histogram's total is Z; the cut is the smallest value whose cumulative mass from below exceeds (1 - top_p) * Z.
//   draw      Gumbel-max over the elements with key32(z) >= the threshold key: s = z + g, g from Philox4x32-10 with counter
//             (i / 4, b, step, 0) and the seed as key, the largest s by decode_next's key reduction (lowest index among equals).
//             Random words are generated only for groups of four that hold a kept element within the largest possible noise
//             (CMB_DS_GUMBEL_MAX) of the wave's best score so far, and the accurate logarithms are
//             taken only where a cheap upper bound of the score (cmb_ds_gumbel_bound) reaches the wave's best so far: which
//             elements are spared changes nothing, they could neither win nor tie.
// No floating-point atomics, no global scratch; integer sums and the key maximum do not depend on the order of their terms, so
// the result has the same bits on every run and does not depend on B.  Then decode_next's tail.
#include "decode_select.h"

namespace {

struct DsParams {
  DnParams n;
  float inv_t; int64_t top_k; float top_p;
  const uint64_t* seed;
  float* thr; int32_t* n_keep;
};

__global__ void __launch_bounds__(DN_THREADS) decode_sample_kernel(DsParams q) {
  __shared__ unsigned long long hist[DS_BINS];      // the count passes use its first half as uint32 bins
  __shared__ unsigned long long red[DN_WAVES], wsum[DN_WAVES], found[2];
  __shared__ int64_t chosen;
  const DnParams& p = q.n;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* row = p.logits + (int64_t)b * p.logits_ld;
  const int64_t V = p.V;
  const float inv_t = q.inv_t;
  uint32_t* hist32 = reinterpret_cast<uint32_t*>(hist);
  const unsigned long long k = (unsigned long long)(q.top_k < V ? q.top_k : V);   // 0: off
  const bool use_p = q.top_p < 1.f;

  // ---- sweep 1
  hist[tid] = 0;
  hist[tid + DN_THREADS] = 0;
  __syncthreads();
  unsigned long long best = 0;
  if (k)
    dn_walk<false>(row, V, tid, [&](float v, uint32_t i) {
      best = dn_max(best, dn_key(v, i));
      atomicAdd(&hist32[cmb_ds_key32(v * inv_t) >> 21], 1u);
    });
  else
    dn_walk<false>(row, V, tid, [&](float v, uint32_t i) { best = dn_max(best, dn_key(v, i)); });
  const unsigned long long m = dn_block_max(best, red, tid);
  __syncthreads();                                   // red is written again by the draw
  int64_t nxt = (int64_t)(uint32_t)~(uint32_t)m;
  const uint32_t kmax = (uint32_t)(m >> 32);
  const float z_max = cmb_ds_key32_value(kmax) * inv_t;
  // +inf is 0xFF800000 and a NaN 0xFFFFFFFF; -inf is the smallest key
  const bool finite = kmax < 0xFF800000u && kmax > 0x007FFFFFu && cmb_ds_key32(z_max) < 0xFF800000u;
  float thr = __builtin_nanf("");
  unsigned long long kept = 0;

  if (finite) {
    // ---- top-k: the k-th largest key
    uint32_t thr_key = 0;                            // keep iff key32(z) >= thr_key; no key is below 0x007FFFFF
    if (k) {
      DsFound f = ds_find<uint32_t, true>(hist32, k, -1.f, tid, wsum, found);
      uint32_t prefix = f.bin;
      unsigned long long rem = k - f.before;
#pragma unroll
      for (int pass = 1; pass < 3; ++pass) {
        const int have = pass == 1 ? 21 : 10, shift = pass == 1 ? 10 : 0;   // bits below the prefix; where this digit starts
        hist[tid] = 0;
        __syncthreads();
        dn_walk<false>(row, V, tid, [&](float v, uint32_t) {
          const uint32_t key = cmb_ds_key32(v * inv_t);
          if ((key >> have) == prefix) atomicAdd(&hist32[(key >> shift) & (pass == 1 ? 2047u : 1023u)], 1u);
        });
        __syncthreads();
        f = ds_find<uint32_t, true>(hist32, rem, -1.f, tid, wsum, found);
        prefix = (prefix << (pass == 1 ? 11 : 10)) | f.bin;
        rem -= f.before;
      }
      thr_key = prefix;
    }
    // ---- top-p over what top-k kept: the smallest key whose cumulative mass from below exceeds (1 - top_p) * Z
    if (use_p) {
      const uint32_t k_key = thr_key;
      uint32_t prefix = 0;
      unsigned long long target = 0;
#pragma unroll
      for (int pass = 0; pass < 3; ++pass) {
        const int have = pass == 1 ? 21 : 10, shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
        hist[tid] = 0;
        hist[tid + DN_THREADS] = 0;
        __syncthreads();
        dn_walk<false>(row, V, tid, [&](float v, uint32_t) {
          const float z = v * inv_t;
          const uint32_t key = cmb_ds_key32(z);
          if (key >= k_key && (pass == 0 || (key >> have) == prefix)) {
            const unsigned long long w = cmb_ds_mass(z, z_max);
            if (w) atomicAdd(&hist[(key >> shift) & (pass == 2 ? 1023u : 2047u)], w);
          }
        });
        __syncthreads();
        const DsFound f = ds_find<unsigned long long, false>(hist, target, pass == 0 ? q.top_p : -1.f, tid, wsum, found);
        if (pass == 0) target = cmb_ds_nucleus_target(q.top_p, f.total) + 1;
        prefix = pass == 0 ? f.bin : (prefix << (pass == 1 ? 11 : 10)) | f.bin;
        target -= f.before;
      }
      thr_key = prefix;
    }
    thr = thr_key ? cmb_ds_key32_value(thr_key) : -__builtin_inff();

    // ---- the draw, over index-aligned groups of four (one Philox call each)
    const uint64_t seed = *q.seed;
    const bool aligned = ((uintptr_t)row & 15u) == 0;
    const int64_t groups = (V + 3) >> 2;
    best = 0;
    uint32_t cnt = 0;
    // the best score this wave has computed so far: an element whose cheap upper bound is strictly below it can neither win
    // nor tie, and is spared the accurate logarithms.  Shared across the wave before every group (the trip count is uniform).
    float floor_s = -__builtin_inff();
    const int64_t iters = (groups + DN_THREADS - 1) / DN_THREADS;
    for (int64_t it = 0; it < iters; ++it) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) floor_s = fmaxf(floor_s, __shfl_xor(floor_s, o, 64));
      const int64_t g = it * DN_THREADS + tid;
      if (g >= groups) continue;
      const int64_t base = g << 2;
      const int n = V - base < 4 ? (int)(V - base) : 4;
      float z[4];
      if (aligned && n == 4) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(row + base);
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = v[j] * inv_t;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = j < n ? row[base + j] * inv_t : 0.f;
      }
      bool in[4], any = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool kept_j = j < n && cmb_ds_key32(z[j]) >= thr_key;
        cnt += kept_j;
        in[j] = kept_j && !(z[j] + (CMB_DS_GUMBEL_MAX + CMB_DS_GUMBEL_SLACK) < floor_s);   // no noise lifts the others that far
        any |= in[j];
      }
      if (!any) continue;
      const cmb_philox4 w = cmb_ds_words(seed, (uint32_t)g, (uint32_t)b, (uint32_t)p.step);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (in[j]) {
          if (z[j] + cmb_ds_gumbel_bound(w.w[j]) < floor_s) continue;
          const float sc = z[j] + cmb_ds_gumbel(w.w[j]);
          best = dn_max(best, dn_key(sc, (uint32_t)(base + j)));
          floor_s = fmaxf(floor_s, sc);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = cnt;
    const unsigned long long top = dn_block_max(best, red, tid);      // its barrier publishes wsum too
    nxt = (int64_t)(uint32_t)~(uint32_t)top;
    if (tid == 0)
      for (int w = 0; w < DN_WAVES; ++w) kept += wsum[w];
  }
  if (tid == 0) {
    if (q.thr) q.thr[b] = thr;
    if (q.n_keep) q.n_keep[b] = (int32_t)kept;
  }
  dn_tail(p, b, tid, nxt, &chosen);
}

}  // namespace

extern "C" int cmb_decode_sample(const float* logits, int64_t logits_ld, int32_t B, int64_t V, float inv_temperature, int64_t top_k,
                                 float top_p, const uint64_t* seed, int64_t eos, uint8_t* done, int64_t* out_ids, int64_t out_ld,
                                 int64_t step, const int64_t* n_tok, int64_t* pos, uint8_t* key_valid, int64_t kv_ld, int64_t t,
                                 const void* embed, int64_t embed_ld, int64_t embed_rows, int64_t H, void* x, int64_t x_ld,
                                 int32_t hd, float rope_base, float* cos_t, float* sin_t, float* thr, int32_t* n_keep,
                                 void* stream) {
  if (!seed) return CMB_ERR_BAD_ARG;
  int rc = dn_check_args(logits, logits_ld, B, V, eos, done, out_ids, out_ld, step, n_tok, pos, key_valid, kv_ld, t, embed, embed_ld,
                         embed_rows, H, x, x_ld, hd, cos_t, sin_t);
  if (rc != CMB_OK) return rc;
  if (!(inv_temperature > 0.f) || inv_temperature > 3.4028234e38f || !(top_p > 0.f) || !(top_p <= 1.f) || top_k < 0)
    return CMB_ERR_BAD_ARG;
  rc = dn_check_align(logits, out_ids, n_tok, pos, embed, x);
  if (rc != CMB_OK) return rc;
  if (((uintptr_t)seed & 7u) || ((uintptr_t)thr & 3u) || ((uintptr_t)n_keep & 3u)) return CMB_ERR_ALIGNMENT;

  DsParams q;
  DnParams& p = q.n;
  p.logits = logits; p.logits_ld = logits_ld; p.V = V;
  p.eos = eos; p.done = done;
  p.out_ids = out_ids; p.out_ld = out_ld; p.step = step;
  p.n_tok = n_tok; p.pos = pos;
  p.key_valid = key_valid; p.kv_ld = kv_ld; p.t = t;
  p.embed = (const bf16_t*)embed; p.embed_ld = embed_ld; p.H = H;
  p.x = (bf16_t*)x; p.x_ld = x_ld;
  q.inv_t = inv_temperature; q.top_k = top_k; q.top_p = top_p;
  q.seed = seed; q.thr = thr; q.n_keep = n_keep;
  hipLaunchKernelGGL(decode_sample_kernel, dim3((unsigned)B), dim3(DN_THREADS), 0, (hipStream_t)stream, q);
  CMB_CHECK_LAUNCH();
  return cmb_rope_table(pos, B, hd, rope_base, cos_t, sin_t, stream);
}
