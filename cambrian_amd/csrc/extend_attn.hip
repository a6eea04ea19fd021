// extend_attn.hip — cmb_extend_attn: attention of a CHUNK of Q consecutive new tokens per cache row against the bf16 K/V cache
// (the suffix of a prompt whose head is already cached: generate(prefix=...), the next turn of a chat).  It is
// cmb_decode_attn_multi's step without its limit of 16 tokens / 64 query rows, and with ONE mask rule for cached and new
// slots: query (b, j) sees slot s iff s <= t0 + j and (key_valid[b][s] != 0 or s == t0 + j) — cmb_flash_attn_fwd's "causal AND
// key padding, diagonal open", so a batch whose suffixes are left-padded inside the chunk is legal.
//   launch 1  extend_store_kernel: RoPE (rotate-half, fp32 tables, one row per new token) on the k heads of the Q tokens,
//             rounded to bf16 once; roped k and raw v of token j into cache slot t0 + j.
//   launch 2  extend_attn_kernel<HD, RT>: grid (row block x key chunk, KV head, batch row).  A row block is TB = min(16, 64 / G)
//             consecutive tokens, TB * G <= 64 query rows (extend_attn_layout.h); the workgroup is decode_attn_multi.hip's:
//             four waves, each 16 keys per iteration, K rows from the cache straight into the A operand of
//             v_mfma_f32_16x16x32_bf16 (S^T = K . Q^T, q roped and rounded to bf16), V rows through the wave-private skewed LDS
//             tile and ds_read_b64_tr_b16 into v_mfma_f32_16x16x16_bf16 (O^T = V^T . P^T), one query row per lane, online
//             softmax in fp32 / base 2, waves merged through LDS in wave order.  Every row carries its own causal limit
//             t0 + token; the new slots are read from the cache like any other (launch 1 of the same call wrote them).
//   launch 3  extend_combine_kernel, when the keys are split: chunk c of `splits` writes an un-normalised fp32 partial to the
//             workspace, merged in chunk order; no atomics, the same bits on every run.  A row block skips the chunks past its
//             last token and the merge reads only the chunks a row can see.
// Roofline class: L2 / MFMA for chunks past a few row blocks, HBM for one row block (then it is cmb_decode_attn_multi's stream).
// Known limit: the cache of a KV head is read once per ROW BLOCK, ceil(Q / TB) times per call.  The re-reads hit L2 (a head's
// cache is t0 * hd * 4 bytes), but for chunks of hundreds of tokens that traffic, and a score tile of only 16 keys x 64 rows
// per wave, is well short of what a 128-row flash tile with K / V staged once per workgroup reaches; such a kernel is not here.
#include "decode_attn_common.h"
#include "decode_attn_host.h"
#include "tile_ops.h"
#include "extend_attn_layout.h"

namespace {

struct ExaParams {
  const bf16_t *q, *k, *v;
  int64_t q_ld, k_ld, v_ld;
  const float *cos_t, *sin_t;
  bf16_t *kc, *vc;
  int64_t c_sb, c_sh, c_st;
  int32_t G, nkv, Q;
  int64_t rows;          // B * Q
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

constexpr int EXA_STORE_TOKENS = 8;   // tokens per workgroup of extend_store_kernel: 32 lanes each, 16 pieces of k and 16 of v

// roped k and raw v of the Q new tokens into their slots.  Grid (ceil(B * Q / 8), nkv).
template <int HD>
__global__ void __launch_bounds__(DEC_THREADS) extend_store_kernel(const ExaParams p) {
  constexpr int HALF = HD / 2;
  const int64_t row = (int64_t)blockIdx.x * EXA_STORE_TOKENS + (threadIdx.x >> 5);
  const int kvh = blockIdx.y;
  const int piece = threadIdx.x & 15;
  const bool is_v = (threadIdx.x & 16) != 0;
  if (row >= p.rows || piece >= HD / 8) return;
  const int64_t b = row / p.Q;
  const int64_t slot = p.t0 + (row - b * p.Q);
  const int d0 = 8 * piece;
  const int64_t dst = b * p.c_sb + (int64_t)kvh * p.c_sh + slot * p.c_st + d0;
  if (is_v) {
    *reinterpret_cast<bf16x8_t*>(p.vc + dst) = *reinterpret_cast<const bf16x8_t*>(p.v + row * p.v_ld + (int64_t)kvh * HD + d0);
  } else {
    const int dr = d0 >= HALF ? d0 - HALF : d0;
    float cs[8], sn[8], o[8];
    load8f(p.cos_t + row * HALF + dr, cs);
    load8f(p.sin_t + row * HALF + dr, sn);
    rope_slice<bf16_t, HD>(p.k + row * p.k_ld + (int64_t)kvh * HD, d0, cs, sn, o);
    *reinterpret_cast<bf16x8_t*>(p.kc + dst) = Row16<bf16_t>::from_f32(o);
  }
}

template <int HD, int RT>
__global__ void __launch_bounds__(DEC_THREADS) extend_attn_kernel(const ExaParams p) {
  constexpr int KS = HD / 32, DT = HD / 16, HALF = HD / 2;
  constexpr int VTILE = DAM_KEYS * (HD * 2 + 32);
  constexpr int OLD = HD + 4;          // floats per row of the merge buffer: 16 rows' float4 stores on 16 different slots
  constexpr int STEP = DEC_WAVES * DAM_KEYS;

  __shared__ __attribute__((aligned(16))) char sm_v[DEC_WAVES * VTILE];
  __shared__ __attribute__((aligned(16))) float sm_o[RT * 16 * OLD];
  __shared__ float sm_m[DEC_WAVES][RT * 16], sm_l[RT * 16];

  const int G = p.G, Q = p.Q;
  const int rb = blockIdx.x / p.splits, c = blockIdx.x - rb * p.splits;
  const int kvh = blockIdx.y;
  const int64_t b = blockIdx.z;
  // keys [c0, c1) of this chunk that the row block can see at all; a chunk past the block's last token has no work, and the
  // merge does not read its partial
  const int64_t kend = exa_block_key_end(p.t0, rb, Q, G);
  const int64_t c0 = (int64_t)c * p.chunk;
  if (c0 >= kend) return;
  const int64_t c1 = c0 + p.chunk < kend ? c0 + p.chunk : kend;
  const int R = exa_block_rows(rb, Q, G);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lg = lane >> 4, li = lane & 15;
  const bf16x8_t zero8 = cvt8_bf16(0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f);

  // ---- the query rows, roped and rounded to bf16: B operands of the score product, kept for the whole kernel ----
  bf16x8_t qf[RT][KS];
  int jrow[RT];                        // token (in the chunk) of the lane's row in tile rt; padded rows: the block's first
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int r = dam_q_row(rt, lane);
    const bool live = r < R;
    const int j = exa_row_token(rb, live ? r : 0, G), g = live ? exa_row_head(r, G) : 0;
    jrow[rt] = j;
    const int64_t row = b * Q + j;
    const bf16_t* qp = p.q + row * p.q_ld + (int64_t)(kvh * G + g) * HD;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int d0 = dam_qk_d(ks, lane, 0);
      const int dr = d0 >= HALF ? d0 - HALF : d0;
      float cs[8], sn[8], o[8];
      load8f(p.cos_t + row * HALF + dr, cs);
      load8f(p.sin_t + row * HALF + dr, sn);
      rope_slice<bf16_t, HD>(qp, d0, cs, sn, o);
      qf[rt][ks] = live ? Row16<bf16_t>::from_f32(o) : zero8;
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

  // one key tile: kr the 16 K rows as A operands, the V rows in the wave's LDS tile.  Bit kk of `in`: key kk lies in the
  // chunk; of `valid`: its key_valid byte is set; rel0 = (slot of key 0) - t0, so key kk is kk + rel0 - token(r) past row r's limit
  auto absorb = [&](const bf16x8_t (&kr)[KS], uint32_t in, uint32_t valid, int rel0) {
    s16x4_t pf[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      f32x4_t s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kr[ks], qf[rt][ks], s, 0, 0, 0);
      const int past = rel0 - jrow[rt];
      float sv[4];
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int kk = dam_s_key(lane, i);
        const bool on = ((in >> kk) & 1u) != 0 && exa_key_open(kk + past, ((valid >> kk) & 1u) != 0);
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

  const int64_t coff = b * p.c_sb + (int64_t)kvh * p.c_sh + 8 * lg;
  const bf16_t* kb = p.kc + coff;
  const bf16_t* vb = p.vc + coff;
  const uint8_t* kvp = p.key_valid + b * p.kv_ld;

  bf16x8_t kr[KS], vr[KS], nkr[KS], nvr[KS];
  bool in = false, ok = false, nin = false, nok = false;
  auto fetch = [&](int64_t base, bf16x8_t (&rk)[KS], bf16x8_t (&rv)[KS], bool& i, bool& o) {
    const int64_t j = base + li;
    i = j < c1;
    const int64_t jj = i ? j : c0;             // past the chunk: re-read its first row (c0 < c1 here), closed
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      rk[ks] = *reinterpret_cast<const bf16x8_t*>(kb + jj * p.c_st + 32 * ks);
      rv[ks] = *reinterpret_cast<const bf16x8_t*>(vb + jj * p.c_st + 32 * ks);
    }
    o = kvp[jj] != 0;
  };
  int64_t base = exa_tile_base(c0, wave, 0);   // wave-uniform: every branch below is taken by whole waves
  if (base < c1) fetch(base, kr, vr, in, ok);
  for (; base < c1; base += STEP) {
    const bool more = base + STEP < c1;
    if (more) fetch(base + STEP, nkr, nvr, nin, nok);
    stage_v(vr, in && exa_v_keep(base + li, p.t0, ok));
    // lanes 0..15 hold keys 0..15 (every lane group the same)
    const uint32_t inb = (uint32_t)(__ballot(in) & 0xFFFFu), okb = (uint32_t)(__ballot(ok) & 0xFFFFu);
    absorb(kr, inb, okb, (int)(base - p.t0));  // |base - t0| < 2^31: the host checks t0 + Q
    if (more) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) { kr[ks] = nkr[ks]; vr[ks] = nvr[ks]; }
      in = nin;
      ok = nok;
    }
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

  // partials of the (sequence, KV head, chunk): [Q*G * HD] acc, [Q*G] m, [Q*G] l, rows in the order token-major, head-minor
  const int64_t RQ = (int64_t)Q * G;
  float* part = p.ws ? p.ws + (((b * p.nkv + kvh) * p.splits + c) * RQ) * (HD + 2) : nullptr;
  for (int idx = threadIdx.x; idx < R * HD; idx += DEC_THREADS) {
    const int r = idx / HD, d = idx - r * HD;
    const float num = sm_o[r * OLD + d], den = sm_l[r];
    if (p.splits == 1) {
      const int j = exa_row_token(rb, r, G), g = exa_row_head(r, G);
      p.out[(b * Q + j) * p.out_ld + (int64_t)(kvh * G + g) * HD + d] = (bf16_t)(num / den);   // den > 0: the row's own slot is open
    } else {
      const int64_t rg = exa_row_global(rb, r, G);
      part[rg * HD + d] = num;
      if (d == 0) {
        float M = sm_m[0][r];
#pragma unroll
        for (int w = 1; w < DEC_WAVES; ++w) M = fmaxf(M, sm_m[w][r]);
        part[RQ * HD + rg] = M;
        part[RQ * HD + RQ + rg] = den;
      }
    }
  }
}

// out[b * Q + j, head, :] = sum_c acc_c * 2^(m_c - M) / sum_c l_c * 2^(m_c - M) over the chunks that hold a slot <= t0 + j, in
// order; a chunk in which the row saw nothing (m = -inf) weighs 0.  Grid (Q * G, nkv, B).
__global__ void __launch_bounds__(128) extend_combine_kernel(const float* __restrict__ ws, int G, int Q, int nkv, int hd,
                                                             int splits, int64_t t0, int64_t chunk, bf16_t* __restrict__ out) {
  const int r = blockIdx.x, kvh = blockIdx.y;
  const int64_t RQ = gridDim.x;
  const int64_t b = blockIdx.z;
  const int d = threadIdx.x;
  if (d >= hd) return;
  const int j = r / G, g = r - j * G;
  const int seen = (int)((t0 + j) / chunk) + 1;          // <= splits: splits * chunk >= t0 + Q
  const int64_t ps = RQ * (hd + 2);
  const float* base = ws + (b * nkv + kvh) * splits * ps;
  float M = -INFINITY;
  for (int c = 0; c < seen; ++c) M = fmaxf(M, base[c * ps + RQ * hd + r]);
  float num = 0.f, den = 0.f;
  for (int c = 0; c < seen; ++c) {
    const float* pc = base + c * ps;
    const float wt = dec_weight(pc[RQ * hd + r], M);
    num += pc[(int64_t)r * hd + d] * wt;
    den += pc[RQ * hd + RQ + r] * wt;
  }
  out[((b * Q + j) * (int64_t)nkv * G + (int64_t)kvh * G + g) * hd + d] = (bf16_t)(num / den);
}

// cmb_decode_attn's geometry rule in bf16 and 1 .. EXA_MAX_Q tokens
bool exa_geometry_ok(int32_t nh, int32_t nkv, int32_t hd, int32_t Q) {
  return dec_geometry_ok(CMB_BF16, nh, nkv, hd) && Q >= 1 && Q <= EXA_MAX_Q;
}

// cmb_decode_attn's plan over slots 0 .. t0 + Q - 1 for B * ceil(Q / 16) * nkv workgroups per chunk (a function of the call's
// B, nkv, t0, Q alone; groups past 4 heads have more row blocks than counted): the row blocks already fill the machine for
// long chunks, which then split little or not at all.  t0 + Q stays below 2^31 (the kernel's slot differences are ints).
int exa_plan(int64_t B, int32_t nkv, int64_t t0, int32_t Q, int32_t splits, int32_t* splits_out, int64_t* chunk_out,
             int32_t* max_splits_out) {
  if (Q > EXA_MAX_Q || t0 > INT32_MAX - EXA_MAX_Q) Q = 0;       // planned as no token, which is rejected
  const int64_t blocks = Q >= 1 ? (Q + DAM_MAX_Q - 1) / DAM_MAX_Q : 1;
  return dec_plan_slots(B >= 1 ? B * blocks : B, nkv, t0, Q, splits, splits_out, chunk_out, max_splits_out);
}

}  // namespace

extern "C" int cmb_extend_attn_plan(int64_t B, int32_t nkv, int64_t t0, int32_t Q, int32_t splits, int32_t* splits_out,
                                    int64_t* chunk_out, int32_t* max_splits_out) {
  return exa_plan(B, nkv, t0, Q, splits, splits_out, chunk_out, max_splits_out);
}

extern "C" int64_t cmb_extend_attn_ws(int64_t B, int32_t nh, int32_t nkv, int32_t hd, int32_t Q, int64_t t0, int32_t splits) {
  int32_t s = 0;
  if (!exa_geometry_ok(nh, nkv, hd, Q) || exa_plan(B, nkv, t0, Q, splits, &s, nullptr, nullptr) != CMB_OK)
    return CMB_ERR_BAD_ARG;
  return dec_ws_need(B * Q * nh, s, hd);
}

extern "C" int cmb_extend_attn(const void* q, int64_t q_ld, const void* k, int64_t k_ld, const void* v, int64_t v_ld,
                               const float* cos_t, const float* sin_t, void* kcache, void* vcache, int64_t c_sb, int64_t c_sh,
                               int64_t c_st, int64_t B, int32_t nh, int32_t nkv, int32_t hd, int32_t Q, int64_t t0,
                               const uint8_t* key_valid, int64_t kv_ld, float scale, int32_t splits, float* ws,
                               int64_t ws_floats, void* out, void* stream) {
  if (!dec_all_set({q, k, v, cos_t, sin_t, kcache, vcache, key_valid, out})) return CMB_ERR_BAD_ARG;
  if (!exa_geometry_ok(nh, nkv, hd, Q) || !dec_range_ok(B, nkv, t0, Q, kv_ld)) return CMB_ERR_BAD_ARG;
  if (B == 0) return CMB_OK;
  const int G = nh / nkv;
  int32_t s = 0;
  int64_t chunk = 0;
  if (exa_plan(B, nkv, t0, Q, splits, &s, &chunk, nullptr) != CMB_OK) return CMB_ERR_BAD_ARG;
  const int64_t need = dec_ws_need(B * Q * nh, s, hd);
  if (need > 0 && (!ws || ws_floats < need)) return CMB_ERR_BAD_ARG;
  if (!dec_aligned16({q, k, v, kcache, vcache, out}, {q_ld, k_ld, v_ld, c_sb, c_sh, c_st}, 2)) return CMB_ERR_ALIGNMENT;

  ExaParams p;
  p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v;
  p.q_ld = q_ld; p.k_ld = k_ld; p.v_ld = v_ld;
  p.cos_t = cos_t; p.sin_t = sin_t;
  p.kc = (bf16_t*)kcache; p.vc = (bf16_t*)vcache;
  p.c_sb = c_sb; p.c_sh = c_sh; p.c_st = c_st;
  p.G = G; p.nkv = nkv; p.Q = Q;
  p.rows = B * Q;
  p.t0 = t0;
  p.key_valid = key_valid; p.kv_ld = kv_ld;
  p.scale_log2 = scale * DEC_LOG2E;
  p.splits = s; p.chunk = chunk;
  p.ws = s == 1 ? nullptr : ws;
  p.out = (bf16_t*)out;
  p.out_ld = (int64_t)nh * hd;

  // grid sizes: B, nkv <= 65535 (dec_range_ok); B * Q / 8 < 2^28; row blocks * splits <= 512 * 64; Q * G <= 32768
  hipStream_t st = (hipStream_t)stream;
  const dim3 sgrid((unsigned)((p.rows + EXA_STORE_TOKENS - 1) / EXA_STORE_TOKENS), (unsigned)nkv);
  if (hd == 64) hipLaunchKernelGGL(extend_store_kernel<64>, sgrid, dim3(DEC_THREADS), 0, st, p);
  else if (hd == 96) hipLaunchKernelGGL(extend_store_kernel<96>, sgrid, dim3(DEC_THREADS), 0, st, p);
  else hipLaunchKernelGGL(extend_store_kernel<128>, sgrid, dim3(DEC_THREADS), 0, st, p);
  CMB_CHECK_LAUNCH();

  const dim3 grid((unsigned)(exa_blocks(Q, G) * s), (unsigned)nkv, (unsigned)B);
  const int RT = dam_row_tiles(exa_block_rows(0, Q, G));       // the first row block is the largest
#define EXA_LAUNCH(HD, RTV) hipLaunchKernelGGL((extend_attn_kernel<HD, RTV>), grid, dim3(DEC_THREADS), 0, st, p)
#define EXA_ROWS(HD)                               \
  do {                                             \
    if (RT == 1) EXA_LAUNCH(HD, 1);                \
    else if (RT == 2) EXA_LAUNCH(HD, 2);           \
    else if (RT == 3) EXA_LAUNCH(HD, 3);           \
    else EXA_LAUNCH(HD, 4);                        \
  } while (0)
  if (hd == 64) EXA_ROWS(64);
  else if (hd == 96) EXA_ROWS(96);
  else EXA_ROWS(128);
#undef EXA_ROWS
#undef EXA_LAUNCH
  CMB_CHECK_LAUNCH();
  if (s > 1) {
    hipLaunchKernelGGL(extend_combine_kernel, dim3((unsigned)(Q * G), (unsigned)nkv, (unsigned)B), dim3(128), 0, st,
                       (const float*)ws, G, (int)Q, (int)nkv, (int)hd, (int)s, t0, chunk, (bf16_t*)out);
    CMB_CHECK_LAUNCH();
  }
  return CMB_OK;
}
