// decode_attn_multi.hip — cmb_decode_attn's step for Q consecutive new tokens per cache row (the verify step of prompt-lookup
// speculative decoding in generate(): HF's assisted decoding with a PromptLookupCandidateGenerator, whose forward over the
// candidate tokens is LlamaAttention / Phi3Attention with use_cache on Q new positions):
//   * RoPE (rotate-half, the fp32 tables of cmb_rope_table, one row per new token) on the q and k heads of all Q tokens,
//   * roped k and raw v of token j written into cache slot t0 + j,
//   * softmax(scale * q.K^T).V of every query head of token j over cache slots 0 .. t0 + j: cached slots under the key-padding
//     mask, the step's own slots t0 .. t0 + j always open.
// Roofline class: HBM (the K / V cache is read once per step, whatever Q is).
//
// Layout (decode_attn_multi_layout.h has the lane maps; tests/csrc/decode_attn_multi_layout_sim.cpp enumerates them).  One
// workgroup (4 waves) per (batch row, KV head, chunk of keys) holds all R = Q * G query rows of the KV head, row r = token
// r / G, head r % G, padded to RT tiles of 16 — up to 64 rows, past what a VALU dot product per row can carry, so both
// products run on the bf16 MFMA.  A wave takes 16 keys per iteration: the K rows go from the cache straight into registers in
// the A-operand layout of v_mfma_f32_16x16x32_bf16 (S^T = K . Q^T, q roped, rounded to bf16 and held as B operands for the
// whole kernel; the scale is applied to the fp32 scores), the V rows through a wave-private LDS tile that is read back
// transposed (ds_read_b64_tr_b16) as the A operand of v_mfma_f32_16x16x16_bf16 (O^T = V^T . P^T), whose B operand is the score
// registers converted in place: a lane owns ONE query row, its online softmax (fp32 max / sum / accumulators, base-2
// exponent) needs two shuffles per tile.  P is rounded to bf16; a key that is not attendable has its V rows zeroed on the way
// into LDS and its score replaced by -inf, so whatever the slot holds (NaN included) stays out.  No barrier inside the loop:
// every wave owns its tile.  The four waves are merged through LDS in wave order.
// Split over keys as decode_attn.hip: chunk c of `splits` (over slots 0 .. t0 + Q - 1) reads the cached slots of its range
// and writes an un-normalised partial to the workspace, a second launch merges them in chunk order; no atomics, the same bits
// on every run.  The workgroup of the last chunk owns the step's own slots: one wave ropes the new k rows in registers (rounded
// to bf16, the value later steps read), takes the new v rows from the arguments, stores both and attends to them under the
// causal rule — no workgroup reads a slot that the launch writes.
#include "decode_attn_common.h"
#include "decode_attn_host.h"
#include "tile_ops.h"
#include "decode_attn_multi_layout.h"

namespace {

struct DamParams {
  const bf16_t *q, *k, *v;
  int64_t q_ld, k_ld, v_ld;
  const float *cos_t, *sin_t;
  bf16_t *kc, *vc;
  int64_t c_sb, c_sh, c_st;
  int32_t G, nkv, Q, R;
  int64_t t0;
  const uint8_t* key_valid;
  int64_t kv_ld;
  float scale_log2;      // scale * log2(e): scores live in the base-2 exponent domain
  int32_t splits;
  int64_t chunk;
  float* ws;
  bf16_t* out;
  int64_t out_ld;        // nh * hd
};

template <int HD, int RT>
__global__ void __launch_bounds__(DEC_THREADS) decode_attn_multi_kernel(const DamParams p) {
  constexpr int KS = HD / 32, DT = HD / 16, HALF = HD / 2;
  constexpr int VTILE = DAM_KEYS * (HD * 2 + 32);
  constexpr int OLD = HD + 4;          // floats per row of the merge buffer: 16 rows' float4 stores on 16 different slots
  constexpr int STEP = DEC_WAVES * DAM_KEYS;

  __shared__ __attribute__((aligned(16))) char sm_v[DEC_WAVES * VTILE];
  __shared__ __attribute__((aligned(16))) float sm_o[RT * 16 * OLD];
  __shared__ float sm_m[DEC_WAVES][RT * 16], sm_l[RT * 16];

  const int c = blockIdx.x, kvh = blockIdx.y;
  const int64_t b = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lg = lane >> 4, li = lane & 15;
  const int G = p.G, Q = p.Q, R = p.R;
  const bf16x8_t zero8 = cvt8_bf16(0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f);

  // roped row `row` of the step (q or k head at x), the lane's 8 columns of k-step ks, rounded to bf16
  auto rope8 = [&](const bf16_t* x, int64_t row, int ks) {
    const int d0 = dam_qk_d(ks, lane, 0);
    const int dr = d0 >= HALF ? d0 - HALF : d0;
    float cs[8], sn[8], o[8];
    load8f(p.cos_t + row * HALF + dr, cs);
    load8f(p.sin_t + row * HALF + dr, sn);
    rope_slice<bf16_t, HD>(x, d0, cs, sn, o);
    return Row16<bf16_t>::from_f32(o);
  };

  // ---- the query rows: B operands of the score product, kept for the whole kernel ----
  bf16x8_t qf[RT][KS];
  int jrow[RT];                        // token of the lane's row in tile rt (padded rows: 0, never stored)
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int r = dam_q_row(rt, lane);
    const bool live = r < R;
    const int j = live ? dam_row_token(r, G) : 0, g = live ? r - j * G : 0;
    jrow[rt] = j;
    const int64_t row = b * Q + j;
    const bf16_t* qp = p.q + row * p.q_ld + (int64_t)(kvh * G + g) * HD;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const bf16x8_t x = rope8(qp, row, ks);
      qf[rt][ks] = live ? x : zero8;
    }
  }

  float m[RT], l[RT];                  // l: the lane's own keys only, summed over the four lane groups at the end
  f32x4_t acc[RT][DT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    m[rt] = -INFINITY;
    l[rt] = 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[rt][dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }

  char* vt = sm_v + wave * VTILE;
  int tro[DT], wro[KS];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) tro[dt] = dam_v_tr_off(HD, dt, lane);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) wro[ks] = dam_v_write_off(HD, ks, lane);

  // one key tile: kr the 16 K rows as A operands, the V rows in the wave's LDS tile (rows of keys that are not open: zero),
  // open bit kk = key kk of the tile is attendable; own = the step's own slots, where row r sees keys 0 .. token(r)
  auto absorb = [&](const bf16x8_t (&kr)[KS], uint32_t open, bool own) {
    s16x4_t pf[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      f32x4_t s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kr[ks], qf[rt][ks], s, 0, 0, 0);
      const int last = own ? jrow[rt] : DAM_KEYS - 1;
      float sv[4];
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int kk = dam_s_key(lane, i);
        const bool on = ((open >> kk) & 1u) != 0 && kk <= last;
        sv[i] = on ? s[i] * p.scale_log2 : -INFINITY;      // a select: a NaN score of a closed key goes no further
        mx = fmaxf(mx, sv[i]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = fmaxf(m[rt], mx);
      const float mref = mn == -INFINITY ? 0.f : mn;       // nothing attendable so far: every weight below is exp2(-inf) = 0
      const float alpha = __builtin_amdgcn_exp2f(m[rt] - mref);
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) { sv[i] = __builtin_amdgcn_exp2f(sv[i] - mref); ps += sv[i]; }
      l[rt] = l[rt] * alpha + ps;
      m[rt] = mn;
      const uint32_t p01 = cvt2_bf16(sv[0], sv[1]), p23 = cvt2_bf16(sv[2], sv[3]);
      pf[rt] = __builtin_bit_cast(s16x4_t, (uint64_t)p01 | ((uint64_t)p23 << 32));
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) acc[rt][dt] *= alpha;
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const s16x4_t vf = lds_read_tr16(vt + tro[dt]);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[rt][dt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(vf, pf[rt], acc[rt][dt], 0, 0, 0);
    }
  };
  // the lane's pieces of the V rows into the wave's tile; the tile's previous reads were issued before (LDS runs a wave's
  // accesses in order), the compiler is kept from moving either across
  auto stage_v = [&](const bf16x8_t (&rv)[KS], bool on) {
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) *reinterpret_cast<bf16x8_t*>(vt + wro[ks]) = on ? rv[ks] : zero8;
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  };

  // ---- cached keys [c0, c1) of this chunk: slots >= t0 are never read back ----
  const int64_t c0 = (int64_t)c * p.chunk;
  const int64_t c1 = (c0 + p.chunk < p.t0) ? c0 + p.chunk : p.t0;
  const int64_t coff = b * p.c_sb + (int64_t)kvh * p.c_sh + 8 * lg;
  const bf16_t* kb = p.kc + coff;
  const bf16_t* vb = p.vc + coff;
  const uint8_t* kvp = p.key_valid + b * p.kv_ld;

  bf16x8_t kr[KS], vr[KS], nkr[KS], nvr[KS];
  bool ok = false, nok = false;
  auto fetch = [&](int64_t base, bf16x8_t (&rk)[KS], bf16x8_t (&rv)[KS], bool& o) {
    const int64_t j = base + li;
    const bool in = j < c1;
    const int64_t jj = in ? j : c0;            // past the chunk: re-read its first row (c0 < c1 here), closed
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      rk[ks] = *reinterpret_cast<const bf16x8_t*>(kb + jj * p.c_st + 32 * ks);
      rv[ks] = *reinterpret_cast<const bf16x8_t*>(vb + jj * p.c_st + 32 * ks);
    }
    o = in & (kvp[jj] != 0);
  };
  int64_t base = c0 + wave * DAM_KEYS;         // wave-uniform: every branch below is taken by whole waves
  if (base < c1) fetch(base, kr, vr, ok);
  for (; base < c1; base += STEP) {
    const bool more = base + STEP < c1;
    if (more) fetch(base + STEP, nkr, nvr, nok);
    stage_v(vr, ok);
    const uint32_t open = (uint32_t)(__ballot(ok) & 0xFFFFu);    // lanes 0..15 hold keys 0..15 (every lane group the same)
    absorb(kr, open, false);
    if (more) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) { kr[ks] = nkr[ks]; vr[ks] = nvr[ks]; }
      ok = nok;
    }
  }

  // ---- the step's own slots t0 .. t0 + Q - 1, in one wave of the last chunk's workgroup ----
  if (c == p.splits - 1 && wave == DEC_WAVES - 1) {
    const bool live = li < Q;
    const int64_t row = b * Q + (live ? li : 0);
    const int64_t soff = b * p.c_sb + (int64_t)kvh * p.c_sh + (p.t0 + li) * p.c_st;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int d0 = dam_qk_d(ks, lane, 0);
      kr[ks] = rope8(p.k + row * p.k_ld + (int64_t)kvh * HD, row, ks);      // attend to what the cache will hold
      vr[ks] = *reinterpret_cast<const bf16x8_t*>(p.v + row * p.v_ld + (int64_t)kvh * HD + d0);
      if (live) {
        *reinterpret_cast<bf16x8_t*>(p.kc + soff + d0) = kr[ks];
        *reinterpret_cast<bf16x8_t*>(p.vc + soff + d0) = vr[ks];
      }
    }
    stage_v(vr, live);
    absorb(kr, (1u << Q) - 1u, true);
  }

  // ---- merge the four waves through LDS, in wave order ----
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    l[rt] += __shfl_xor(l[rt], 16, 64);
    l[rt] += __shfl_xor(l[rt], 32, 64);
    if (lg == 0) sm_m[wave][16 * rt + li] = m[rt];
  }
  __syncthreads();
  float wt[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    float M = sm_m[0][16 * rt + li];
#pragma unroll
    for (int w = 1; w < DEC_WAVES; ++w) M = fmaxf(M, sm_m[w][16 * rt + li]);
    wt[rt] = dec_weight(m[rt], M);
  }
#pragma unroll
  for (int w = 0; w < DEC_WAVES; ++w) {
    if (wave == w) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          f32x4_t* dst = reinterpret_cast<f32x4_t*>(sm_o + (16 * rt + li) * OLD + dam_o_d(dt, lane, 0));
          const f32x4_t x = acc[rt][dt] * wt[rt];
          *dst = w == 0 ? x : *dst + x;
        }
        if (lg == 0) sm_l[16 * rt + li] = (w == 0 ? 0.f : sm_l[16 * rt + li]) + l[rt] * wt[rt];
      }
    }
    __syncthreads();
  }

  float* part = p.ws ? p.ws + (((b * p.nkv + kvh) * p.splits + c) * (int64_t)R) * (HD + 2) : nullptr;   // [R*HD] acc, [R] m, [R] l
  for (int idx = threadIdx.x; idx < R * HD; idx += DEC_THREADS) {
    const int r = idx / HD, d = idx - r * HD;
    const float num = sm_o[r * OLD + d], den = sm_l[r];
    if (p.splits == 1) {
      const int j = dam_row_token(r, G), g = r - j * G;
      p.out[(b * Q + j) * p.out_ld + (int64_t)(kvh * G + g) * HD + d] = (bf16_t)(num / den);   // den > 0: the row's own slot is open
    } else {
      part[idx] = num;
      if (d == 0) {
        float M = sm_m[0][r];
#pragma unroll
        for (int w = 1; w < DEC_WAVES; ++w) M = fmaxf(M, sm_m[w][r]);
        part[R * HD + r] = M;
        part[R * HD + R + r] = den;
      }
    }
  }
}

// out[b * Q + j, head, :] = sum_c acc_c * 2^(m_c - M) / sum_c l_c * 2^(m_c - M), chunks in order; an empty chunk (m = -inf)
// weighs 0.  Grid (R, nkv, B).
__global__ void __launch_bounds__(128) decode_multi_combine_kernel(const float* __restrict__ ws, int G, int Q, int nkv, int hd,
                                                                   int splits, bf16_t* __restrict__ out) {
  const int r = blockIdx.x, kvh = blockIdx.y, R = gridDim.x;
  const int64_t b = blockIdx.z;
  const int d = threadIdx.x;
  if (d >= hd) return;
  const int64_t ps = (int64_t)R * (hd + 2);
  const float* base = ws + (b * nkv + kvh) * splits * ps;
  float M = -INFINITY;
  for (int c = 0; c < splits; ++c) M = fmaxf(M, base[c * ps + R * hd + r]);
  float num = 0.f, den = 0.f;
  for (int c = 0; c < splits; ++c) {
    const float* pc = base + c * ps;
    const float wt = dec_weight(pc[R * hd + r], M);
    num += pc[r * hd + d] * wt;
    den += pc[R * hd + R + r] * wt;
  }
  const int j = r / G, g = r - j * G;
  out[((b * Q + j) * (int64_t)nkv * G + (int64_t)kvh * G + g) * hd + d] = (bf16_t)(num / den);
}

// cmb_decode_attn's geometry rule in bf16, 1 .. DAM_MAX_Q tokens and at most DAM_MAX_ROWS query rows per KV head.  The plan is
// cmb_decode_attn's over slots 0 .. t0 + Q - 1 (dec_plan_slots): the last chunk holds the step's own slots.
bool dam_geometry_ok(int32_t nh, int32_t nkv, int32_t hd, int32_t Q) {
  return dec_geometry_ok(CMB_BF16, nh, nkv, hd) && Q >= 1 && Q <= DAM_MAX_Q && Q * (nh / nkv) <= DAM_MAX_ROWS;
}

}  // namespace

extern "C" int cmb_decode_attn_multi_plan(int64_t B, int32_t nkv, int64_t t0, int32_t Q, int32_t splits, int32_t* splits_out,
                                          int64_t* chunk_out, int32_t* max_splits_out) {
  // more than DAM_MAX_Q tokens are planned as none, which is rejected
  return dec_plan_slots(B, nkv, t0, Q > DAM_MAX_Q ? 0 : Q, splits, splits_out, chunk_out, max_splits_out);
}

extern "C" int64_t cmb_decode_attn_multi_ws(int64_t B, int32_t nh, int32_t nkv, int32_t hd, int32_t Q, int64_t t0,
                                            int32_t splits) {
  int32_t s = 0;
  if (!dam_geometry_ok(nh, nkv, hd, Q) || dec_plan_slots(B, nkv, t0, Q, splits, &s, nullptr, nullptr) != CMB_OK)
    return CMB_ERR_BAD_ARG;
  return dec_ws_need(B * Q * nh, s, hd);
}

extern "C" int cmb_decode_attn_multi(const void* q, int64_t q_ld, const void* k, int64_t k_ld, const void* v, int64_t v_ld,
                                     const float* cos_t, const float* sin_t, void* kcache, void* vcache, int64_t c_sb,
                                     int64_t c_sh, int64_t c_st, int64_t B, int32_t nh, int32_t nkv, int32_t hd, int32_t Q,
                                     int64_t t0, const uint8_t* key_valid, int64_t kv_ld, float scale, int32_t splits, float* ws,
                                     int64_t ws_floats, void* out, void* stream) {
  if (!dec_all_set({q, k, v, cos_t, sin_t, kcache, vcache, key_valid, out})) return CMB_ERR_BAD_ARG;
  if (!dam_geometry_ok(nh, nkv, hd, Q) || !dec_range_ok(B, nkv, t0, Q, kv_ld)) return CMB_ERR_BAD_ARG;
  if (B == 0) return CMB_OK;
  int32_t s = 0;
  int64_t chunk = 0;
  if (dec_plan_slots(B, nkv, t0, Q, splits, &s, &chunk, nullptr) != CMB_OK) return CMB_ERR_BAD_ARG;
  const int64_t need = dec_ws_need(B * Q * nh, s, hd);
  if (need > 0 && (!ws || ws_floats < need)) return CMB_ERR_BAD_ARG;
  if (!dec_aligned16({q, k, v, kcache, vcache, out}, {q_ld, k_ld, v_ld, c_sb, c_sh, c_st}, 2)) return CMB_ERR_ALIGNMENT;

  DamParams p;
  p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v;
  p.q_ld = q_ld; p.k_ld = k_ld; p.v_ld = v_ld;
  p.cos_t = cos_t; p.sin_t = sin_t;
  p.kc = (bf16_t*)kcache; p.vc = (bf16_t*)vcache;
  p.c_sb = c_sb; p.c_sh = c_sh; p.c_st = c_st;
  p.G = nh / nkv; p.nkv = nkv; p.Q = Q; p.R = Q * p.G;
  p.t0 = t0;
  p.key_valid = key_valid; p.kv_ld = kv_ld;
  p.scale_log2 = scale * DEC_LOG2E;
  p.splits = s; p.chunk = chunk;
  p.ws = s == 1 ? nullptr : ws;
  p.out = (bf16_t*)out;
  p.out_ld = (int64_t)nh * hd;

  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)s, (unsigned)nkv, (unsigned)B);
  const int RT = dam_row_tiles(p.R);
#define DAM_LAUNCH(HD, RTV) hipLaunchKernelGGL((decode_attn_multi_kernel<HD, RTV>), grid, dim3(DEC_THREADS), 0, st, p)
#define DAM_ROWS(HD)                               \
  do {                                             \
    if (RT == 1) DAM_LAUNCH(HD, 1);                \
    else if (RT == 2) DAM_LAUNCH(HD, 2);           \
    else if (RT == 3) DAM_LAUNCH(HD, 3);           \
    else DAM_LAUNCH(HD, 4);                        \
  } while (0)
  if (hd == 64) DAM_ROWS(64);
  else if (hd == 96) DAM_ROWS(96);
  else DAM_ROWS(128);
#undef DAM_ROWS
#undef DAM_LAUNCH
  CMB_CHECK_LAUNCH();
  if (s > 1) {
    hipLaunchKernelGGL(decode_multi_combine_kernel, dim3((unsigned)p.R, (unsigned)nkv, (unsigned)B), dim3(128), 0, st,
                       (const float*)ws, p.G, (int)Q, (int)nkv, (int)hd, (int)s, (bf16_t*)out);
    CMB_CHECK_LAUNCH();
  }
  return CMB_OK;
}
