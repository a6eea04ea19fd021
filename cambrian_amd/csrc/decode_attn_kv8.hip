// decode_attn_kv8.hip — cmb_decode_attn's step (decode_attn.hip: RoPE on the new q / k, slot t written, softmax(scale * q.K^T).V
// over cache keys 0..t, grouped KV heads, key-padding mask with slot t open) on a 1-byte K / V cache, and the kernel that puts
// the prefill's K / V into that cache.
// Roofline class: HBM (the cache is read once per step: 2 * nkv * (hd + 4) bytes per cached key, row and layer, against
// 2 * nkv * hd * 2 of the bf16 cache).
//
// Format.  A cache row (one key's hd values of one KV head) is hd OCP e4m3fn bytes plus one fp32 factor, by
// cmb_quantize_fp8_rows' rule (fp8.hip), expression for expression: amax = max |x|, s = 448 / amax (1 for a zero row), byte =
// v_cvt_pk_fp8_f32(clamp(x * s, +-448)), factor = amax / 448 (1 for a zero row).  kv8_scale / kv8_inv / kv8_pack4 below are those
// expressions; both kernels of this file use them, so a token's bytes do not depend on whether it came in through the prefill
// or through a decode step.
//
// cmb_decode_attn_kv8 keeps decode_attn_kernel's structure: one workgroup (4 waves) per (batch row, KV head, chunk of keys) with
// all G query heads in it, rows straight to VGPRs with the next iteration's in flight, one online softmax per lane group in
// the base-2 domain, groups merged by shuffles and then through LDS, partials in the (acc[G][hd], m[G], l[G]) layout that
// decode_combine_kernel merges.
// Bytes per lane and load: 16 (= 16 elements) where a KV head has up to 4 query heads (GP 1 / 2 / 4), 8 at GP = 8.  With 16,
// an hd-128 row lies in 8 lanes, an hd-64 row in 4 and an hd-96 row in 6 of 8, so a load instruction brings twice the keys, the
// DPP reduction is one step shorter and the per-key softmax arithmetic, which every lane of a group repeats, is repeated by
// half as many lanes; q and the accumulators are 16 fp32 per lane and head, which at GP = 8 would be 256 registers before
// anything else — there the kernel keeps the bf16 kernel's lane shape (8 elements per lane, 16 lanes per hd-128 row).  The
// RoPE table of the lane's piece is loaded where it is used, not held across the key loop: that is what keeps GP = 4 within
// 256 registers (two waves per SIMD) without spilling.
// At one byte per element the step is bound by VALU issue rather than by the cache stream, so q.k and the weighted sum of V
// run on packed fp32 multiply-adds (v_pk_fma_f32) over the pairs v_cvt_pk_f32_fp8 delivers.  Both choices were A/B'd on an
// MI355X while the kernel was written (Llama-3-8B geometry, one call at 16 rows x 8192 keys; a development timing loop, its
// figures are not in the profile note): 8 bytes per lane with scalar multiply-adds did not beat the bf16 kernel on a whole
// decode step, and 16 bytes per lane with scalar multiply-adds at one wave per SIMD was slower than the bf16 kernel on the
// call alone.  The final form's rows are in profiles/decode_kv8.md (that call: 81.8 us against the bf16 kernel's 114.5).
// Bytes become fp32 with v_cvt_pk_f32_fp8 (exact).  K's factor multiplies the score after the group reduction (one multiply
// per key and head); V's factor is folded into the weight that multiplies the row, the denominator l takes the unscaled
// weight.  A key's two factors are one 4-byte load each, the same address across its lane group.  A key that is not
// attendable may hold any bytes and factors (NaN included): its score is replaced, its row and its V factor are zeroed.
// The workgroup of the last chunk owns slot t: it ropes the new k in registers, rounds it to bf16 as the bf16 kernel does,
// quantises that row and the raw v row (amax over the lane group by DPP), attends to the dequantised values and is the only
// one that stores the slot's bytes and factors.
//
// cmb_kv_quantize_e4m3: a streaming kernel, a row across a lane group of 8 (hd <= 64: 4) lanes of 16 elements each (two
// 16-byte loads, one 16-byte store), 8 or 16 rows per wave, amax by shuffles inside the group.  No workspace, no atomics.
#include "decode_attn_common.h"
#include "decode_attn_host.h"

namespace {

__device__ __forceinline__ float kv8_scale(float amax) { return amax > 0.0f ? 448.0f / amax : 1.0f; }
__device__ __forceinline__ float kv8_inv(float amax) { return amax > 0.0f ? amax / 448.0f : 1.0f; }
// four values -> four e4m3fn bytes (element e in byte e), clamped so that the cast cannot produce a NaN code
__device__ __forceinline__ uint32_t kv8_pack4(const float* v, float scale) {
  float c[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) c[e] = fminf(fmaxf(v[e] * scale, -448.0f), 448.0f);
  int packed = 0;
  packed = __builtin_amdgcn_cvt_pk_fp8_f32(c[0], c[1], packed, false);
  packed = __builtin_amdgcn_cvt_pk_fp8_f32(c[2], c[3], packed, true);
  return (uint32_t)packed;
}
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
template <int E> struct Kv8Raw;                      // a lane's E cache bytes
template <> struct Kv8Raw<8> { typedef u32x2_t raw; };
template <> struct Kv8Raw<16> { typedef u32x4_t raw; };
// E e4m3fn bytes -> E fp32, exactly, as the E / 2 pairs v_cvt_pk_f32_fp8 delivers: the operands of the packed multiply-adds
template <int E>
__device__ __forceinline__ void kv8_to_f32x2(const typename Kv8Raw<E>::raw r, f32x2_t (&v)[E / 2]) {
#pragma unroll
  for (int w = 0; w < E / 4; ++w) {
    v[2 * w] = __builtin_amdgcn_cvt_pk_f32_fp8(r[w], false);
    v[2 * w + 1] = __builtin_amdgcn_cvt_pk_f32_fp8(r[w], true);
  }
}
template <int E>
__device__ __forceinline__ typename Kv8Raw<E>::raw kv8_pack(const float (&v)[E], float scale) {
  typename Kv8Raw<E>::raw r;
#pragma unroll
  for (int w = 0; w < E / 4; ++w) r[w] = kv8_pack4(v + 4 * w, scale);
  return r;
}

// new-token row `x`, bf16: E (8 or 16) roped elements at d0; a piece never straddles HD / 2 (HD / 2 is a multiple of 16)
template <int HD, int E>
__device__ __forceinline__ void rope_piece(const bf16_t* x, int d0, const float (&cs)[E], const float (&sn)[E], float (&o)[E]) {
#pragma unroll
  for (int h = 0; h < E / 8; ++h) {
    float c8[8], s8[8], o8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { c8[e] = cs[8 * h + e]; s8[e] = sn[8 * h + e]; }
    rope_slice<bf16_t, HD>(x, d0 + 8 * h, c8, s8, o8);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[8 * h + e] = o8[e];
  }
}
// E fp32 -> bf16 -> fp32: the value a bf16 cache would hold
template <int E>
__device__ __forceinline__ void round_bf16(float (&v)[E]) {
#pragma unroll
  for (int h = 0; h < E / 8; ++h) {
    float t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = v[8 * h + e];
    Row16<bf16_t>::to_f32(Row16<bf16_t>::from_f32(t), t);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[8 * h + e] = t[e];
  }
}
template <int E>
__device__ __forceinline__ void load_bf16(const bf16_t* p, float (&v)[E]) {
#pragma unroll
  for (int h = 0; h < E / 8; ++h) {
    float t[8];
    Vec8<bf16_t>::load(p + 8 * h, t);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[8 * h + e] = t[e];
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// prefill K / V -> cache
// ------------------------------------------------------------------------------------------------------------------------
constexpr int KVQ_THREADS = 256;

// LPR lanes per row, 16 elements per lane; row r = (b * nkv + h) * L + tok
template <int LPR>
__global__ void __launch_bounds__(KVQ_THREADS) kv_quantize_kernel(const bf16_t* __restrict__ src, int64_t s_sb, int64_t s_sh,
                                                                  int64_t s_st, int64_t rows, int32_t nkv, int64_t L, int32_t hd,
                                                                  uint8_t* __restrict__ dst, int64_t c_sb, int64_t c_sh,
                                                                  int64_t c_st, float* __restrict__ inv, int64_t i_sb,
                                                                  int64_t i_sh) {
  constexpr int RPB = KVQ_THREADS / LPR;
  const int li = threadIdx.x % LPR;
  const int64_t r0 = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR;
  const bool live = r0 < rows;
  const int64_t r = live ? r0 : rows - 1;          // a group past the end shadows the last row (every lane shuffles) and stores nothing
  const int64_t bh = r / L, tok = r - bh * L;
  const int64_t b = bh / nkv, h = bh - b * nkv;
  const int d0 = li * 16;
  const bool active = d0 < hd;                      // hd 96: lanes 6 and 7 of 8 hold nothing
  float v[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = 0.0f;
  if (active) {
    const bf16_t* p = src + b * s_sb + h * s_sh + tok * s_st + d0;
    float a[8], c[8];
    Vec8<bf16_t>::load(p, a);
    Vec8<bf16_t>::load(p + 8, c);
#pragma unroll
    for (int i = 0; i < 8; ++i) { v[i] = a[i]; v[8 + i] = c[i]; }
  }
  float amax = 0.0f;
#pragma unroll
  for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(v[i]));
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off, 64));
  const float scale = kv8_scale(amax);
  if (live && active) {
    const u32x4_t w = {kv8_pack4(v, scale), kv8_pack4(v + 4, scale), kv8_pack4(v + 8, scale), kv8_pack4(v + 12, scale)};
    *reinterpret_cast<u32x4_t*>(dst + b * c_sb + h * c_sh + tok * c_st + d0) = w;
    if (li == 0) inv[b * i_sb + h * i_sh + tok] = kv8_inv(amax);
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// the decode step
// ------------------------------------------------------------------------------------------------------------------------
struct Dec8Params {
  const bf16_t *q, *k, *v;
  int64_t q_ld, k_ld, v_ld;
  const float *cos_t, *sin_t;
  uint8_t *kc, *vc;
  int64_t c_sb, c_sh, c_st;          // bytes
  float *k_inv, *v_inv;
  int64_t i_sb, i_sh;                // elements; the slot stride is 1
  int32_t G, nkv;
  int64_t t;
  const uint8_t* key_valid;
  int64_t kv_ld;
  float scale_log2;
  int32_t splits;
  int64_t chunk;
  float* ws;
  bf16_t* out;
};

// E: elements (= cache bytes) per lane, 16 for GP <= 4 and 8 for GP = 8 (the file header says why)
template <int HD, int GP, int E>
__global__ void __launch_bounds__(DEC_THREADS) decode_attn_kv8_kernel(const Dec8Params p) {
  typedef bf16_t T;
  constexpr int LPKA = HD / E;                                    // lanes that hold a piece of a row
  constexpr int LPK = LPKA <= 4 ? 4 : (LPKA <= 8 ? 8 : 16);       // lanes per key (power of two)
  constexpr int KPW = 64 / LPK;                                   // keys per wave and load instruction
  constexpr int DEC_U = (GP > 4 || (E == 16 && GP > 2)) ? 2 : 4;  // rows of K (and of V) per lane and iteration
  constexpr int STEP = DEC_U * DEC_WAVES * KPW;                   // keys per workgroup iteration
  constexpr int HALF = HD / 2;
  typedef typename Kv8Raw<E>::raw raw;
  static_assert((E == 8 || E == 16) && HD % E == 0 && HALF % E == 0, "a lane's piece lies in one half of the head");

  __shared__ float sm_acc[DEC_WAVES][GP * HD];
  __shared__ float sm_m[DEC_WAVES][GP], sm_l[DEC_WAVES][GP];

  const int c = blockIdx.x, kvh = blockIdx.y;
  const int64_t b = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & (LPK - 1), kg = lane / LPK;
  const bool active = li < LPKA;
  const int d0 = active ? li * E : 0;         // idle lanes (hd 96) shadow piece 0 with q = 0; they never store
  const int G = p.G;

  // this lane's piece of the row's RoPE table; loaded where it is used (here and for slot t), not held across the key loop
  auto rope_table = [&](float (&cs)[E], float (&sn)[E]) {
    const int dr = d0 >= HALF ? d0 - HALF : d0;
    const float* ct = p.cos_t + b * HALF + dr;
    const float* st = p.sin_t + b * HALF + dr;
#pragma unroll
    for (int e = 0; e < E; ++e) { cs[e] = ct[e]; sn[e] = st[e]; }
  };
  // q and the accumulators as pairs: q.k and the weighted sum of V run on packed fp32 multiply-adds (v_pk_fma_f32), two
  // elements per instruction — at one byte per element the step is bound by VALU issue, not by the cache stream
  constexpr int EP = E / 2;
  f32x2_t q[GP][EP];
#pragma unroll
  for (int g = 0; g < GP; ++g) {
    if (g < G && active) {
      float cs[E], sn[E], qf[E];
      rope_table(cs, sn);
      rope_piece<HD, E>(p.q + b * p.q_ld + (int64_t)(kvh * G + g) * HD, d0, cs, sn, qf);
#pragma unroll
      for (int j = 0; j < EP; ++j) q[g][j] = (f32x2_t){qf[2 * j] * p.scale_log2, qf[2 * j + 1] * p.scale_log2};
    } else {
#pragma unroll
      for (int j = 0; j < EP; ++j) q[g][j] = (f32x2_t){0.f, 0.f};
    }
  }

  float m[GP], l[GP];
  f32x2_t acc[GP][EP];
#pragma unroll
  for (int g = 0; g < GP; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int j = 0; j < EP; ++j) acc[g][j] = (f32x2_t){0.f, 0.f};
  }
  // q . k of this lane's piece, summed over the lane group
  auto score = [&](const f32x2_t (&qg)[EP], const f32x2_t (&kf)[EP]) {
    f32x2_t d = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < EP; ++j) d = __builtin_elementwise_fma(qg[j], kf[j], d);
    return group_sum<LPK>(d[0] + d[1]);
  };

  // one online-softmax step over U scored rows: s[u][g] (-inf = not attendable; overwritten with the weights), rv[u] the
  // rows of V as loaded and vi[u] their factors (a row that is not attendable may hold anything, NaN included, in both:
  // neither is multiplied in)
  auto absorb = [&](float (&s)[DEC_U][GP], const raw (&rv)[DEC_U], const float (&vi)[DEC_U], const bool (&o)[DEC_U]) {
#pragma unroll
    for (int g = 0; g < GP; ++g) {
      float mn = m[g];
#pragma unroll
      for (int u = 0; u < DEC_U; ++u) mn = fmaxf(mn, s[u][g]);
      const float mref = mn == -INFINITY ? 0.f : mn;      // nothing attendable so far: every weight below is exp2(-inf) = 0
      const float alpha = __builtin_amdgcn_exp2f(m[g] - mref);
      float ps = 0.f;
#pragma unroll
      for (int u = 0; u < DEC_U; ++u) { s[u][g] = __builtin_amdgcn_exp2f(s[u][g] - mref); ps += s[u][g]; }
      l[g] = l[g] * alpha + ps;
      m[g] = mn;
#pragma unroll
      for (int j = 0; j < EP; ++j) acc[g][j] *= (f32x2_t){alpha, alpha};
    }
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
      raw r = rv[u];
#pragma unroll
      for (int w = 0; w < E / 4; ++w) r[w] = o[u] ? r[w] : 0u;      // byte 0 is +0: a row that is not attendable adds nothing
      f32x2_t vf[EP];
      kv8_to_f32x2<E>(r, vf);
      const float f = o[u] ? vi[u] : 0.f;
#pragma unroll
      for (int g = 0; g < GP; ++g) {
        const float w = s[u][g] * f;
#pragma unroll
        for (int j = 0; j < EP; ++j) acc[g][j] = __builtin_elementwise_fma((f32x2_t){w, w}, vf[j], acc[g][j]);
      }
    }
  };

  // ---- cached keys [c0, c1) of this chunk (slot t is never read back) ----
  const int64_t c0 = (int64_t)c * p.chunk;
  const int64_t c1 = (c0 + p.chunk < p.t) ? c0 + p.chunk : p.t;
  const int64_t rowb = b * p.c_sb + (int64_t)kvh * p.c_sh + d0;
  const uint8_t* kb = p.kc + rowb;
  const uint8_t* vb = p.vc + rowb;
  const int64_t invb = b * p.i_sb + (int64_t)kvh * p.i_sh;
  const float* kib = p.k_inv + invb;
  const float* vib = p.v_inv + invb;
  const uint8_t* kvp = p.key_valid + b * p.kv_ld;

  raw kr[DEC_U], vr[DEC_U], nkr[DEC_U], nvr[DEC_U];
  float ki[DEC_U], vi[DEC_U], nki[DEC_U], nvi[DEC_U];
  bool ok[DEC_U], nok[DEC_U];
  auto fetch = [&](int64_t base, raw (&rk)[DEC_U], raw (&rv)[DEC_U], float (&fk)[DEC_U], float (&fv)[DEC_U], bool (&o)[DEC_U]) {
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
      const int64_t j = base + (u * DEC_WAVES + wave) * KPW + kg;
      const bool in = j < c1;
      const int64_t jj = in ? j : c0;          // past the chunk: re-read its first row (c0 < c1 here), weight 0
      rk[u] = *reinterpret_cast<const raw*>(kb + jj * p.c_st);
      rv[u] = *reinterpret_cast<const raw*>(vb + jj * p.c_st);
      fk[u] = kib[jj];
      fv[u] = vib[jj];
      o[u] = in & (kvp[jj] != 0);              // jj is in range either way: no branch around the loads
    }
  };
  if (c0 < c1) fetch(c0, kr, vr, ki, vi, ok);
  for (int64_t base = c0; base < c1; base += STEP) {
    const bool more = base + STEP < c1;
    if (more) fetch(base + STEP, nkr, nvr, nki, nvi, nok);
    float s[DEC_U][GP];
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
      f32x2_t kf[EP];
      kv8_to_f32x2<E>(kr[u], kf);
#pragma unroll
      for (int g = 0; g < GP; ++g) {
        const float d = score(q[g], kf) * ki[u];
        s[u][g] = ok[u] ? d : -INFINITY;
      }
    }
    absorb(s, vr, vi, ok);
    if (more) {
#pragma unroll
      for (int u = 0; u < DEC_U; ++u) { kr[u] = nkr[u]; vr[u] = nvr[u]; ki[u] = nki[u]; vi[u] = nvi[u]; ok[u] = nok[u]; }
    }
  }

  // ---- the new token (slot t), in the workgroup of the last chunk ----
  if (c == p.splits - 1) {
    float kn[E], vn[E];
    {
      float cs[E], sn[E];
      rope_table(cs, sn);
      rope_piece<HD, E>(p.k + b * p.k_ld + (int64_t)kvh * HD, d0, cs, sn, kn);
    }
    round_bf16<E>(kn);                                            // the bf16 value a bf16 cache would hold
    load_bf16<E>(p.v + b * p.v_ld + (int64_t)kvh * HD + d0, vn);
    float ka = 0.f, va = 0.f;                 // idle lanes shadow piece 0: the group's maximum is the row's
#pragma unroll
    for (int e = 0; e < E; ++e) { ka = fmaxf(ka, fabsf(kn[e])); va = fmaxf(va, fabsf(vn[e])); }
    ka = group_max<LPK>(ka);
    va = group_max<LPK>(va);
    const float ksc = kv8_scale(ka), vsc = kv8_scale(va);
    const raw kraw = kv8_pack<E>(kn, ksc), vraw = kv8_pack<E>(vn, vsc);
    const float kinv = kv8_inv(ka), vinv = kv8_inv(va);
    f32x2_t kd[EP];
    kv8_to_f32x2<E>(kraw, kd);                // attend to what the cache will hold
    const bool mine = wave == 0 && kg == 0;   // one lane group scores it; group_sum needs every lane, so all compute
    float s[DEC_U][GP];
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
      vr[u] = vraw;
      vi[u] = vinv;
      ok[u] = u == 0 && mine;
#pragma unroll
      for (int g = 0; g < GP; ++g) s[u][g] = -INFINITY;
    }
#pragma unroll
    for (int g = 0; g < GP; ++g) {
      const float d = score(q[g], kd) * kinv;
      s[0][g] = mine ? d : -INFINITY;
    }
    absorb(s, vr, vi, ok);
    if (mine && active) {
      const int64_t off = rowb + p.t * p.c_st;
      *reinterpret_cast<raw*>(p.kc + off) = kraw;
      *reinterpret_cast<raw*>(p.vc + off) = vraw;
      if (li == 0) {
        p.k_inv[invb + p.t] = kinv;
        p.v_inv[invb + p.t] = vinv;
      }
    }
  }

  // ---- merge the lane groups of a wave ----
#pragma unroll
  for (int o = LPK; o < 64; o <<= 1) {
#pragma unroll
    for (int g = 0; g < GP; ++g) {
      const float mo = __shfl_xor(m[g], o, 64), lo = __shfl_xor(l[g], o, 64);
      const float mn = fmaxf(m[g], mo);
      const float wa = dec_weight(m[g], mn), wb = dec_weight(mo, mn);
      l[g] = l[g] * wa + lo * wb;
      m[g] = mn;
#pragma unroll
      for (int e = 0; e < E; ++e) acc[g][e >> 1][e & 1] = acc[g][e >> 1][e & 1] * wa + __shfl_xor(acc[g][e >> 1][e & 1], o, 64) * wb;
    }
  }
  // ---- and the four waves through LDS ----
  if (kg == 0 && active) {
#pragma unroll
    for (int g = 0; g < GP; ++g) {
#pragma unroll
      for (int e = 0; e < E; ++e) sm_acc[wave][g * HD + d0 + e] = acc[g][e >> 1][e & 1];
      if (li == 0) { sm_m[wave][g] = m[g]; sm_l[wave][g] = l[g]; }
    }
  }
  __syncthreads();
  const int64_t head0 = (b * p.nkv + kvh) * G;     // first query head of this KV head, counted over the batch
  float* part = p.ws ? p.ws + (head0 * p.splits + (int64_t)c * G) * (HD + 2) : nullptr;   // [G*HD] acc, [G] m, [G] l
  for (int idx = threadIdx.x; idx < G * HD; idx += DEC_THREADS) {
    const int g = idx / HD, d = idx - g * HD;
    float M = sm_m[0][g];
#pragma unroll
    for (int w = 1; w < DEC_WAVES; ++w) M = fmaxf(M, sm_m[w][g]);
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int w = 0; w < DEC_WAVES; ++w) {
      const float wt = dec_weight(sm_m[w][g], M);
      num += sm_acc[w][idx] * wt;
      den += sm_l[w][g] * wt;
    }
    if (p.splits == 1) {
      p.out[(head0 + g) * HD + d] = (T)(num / den);    // den > 0: slot t is always attendable
    } else {
      part[idx] = num;
      if (d == 0) { part[G * HD + g] = M; part[G * HD + G + g] = den; }
    }
  }
}

inline bool aligned4(const void* p) { return (((uintptr_t)p) & 3u) == 0; }

}  // namespace

extern "C" int cmb_kv_quantize_e4m3(const void* src, int64_t s_sb, int64_t s_sh, int64_t s_st, int64_t B, int32_t nkv, int64_t L,
                                    int32_t hd, void* cache, int64_t c_sb, int64_t c_sh, int64_t c_st, float* inv, int64_t i_sb,
                                    int64_t i_sh, void* stream) {
  if (B < 0 || nkv < 0 || L < 0 || hd < 16 || hd > 128 || hd % 16) return CMB_ERR_BAD_ARG;
  if (B == 0 || nkv == 0 || L == 0) return CMB_OK;
  if (!src || !cache || !inv) return CMB_ERR_BAD_ARG;
  if (s_sb < 0 || s_sh < 0 || s_st < hd || c_sb < 0 || c_sh < 0 || c_st < hd || i_sb < 0 || i_sh < 0) return CMB_ERR_BAD_ARG;
  const int64_t rows = B * nkv * L;
  if (rows / L / nkv != B || rows > ((int64_t)1 << 34)) return CMB_ERR_BAD_ARG;
  if (!cmb_aligned16(src) || !cmb_aligned16(cache) || !aligned4(inv) || s_sb % 8 || s_sh % 8 || s_st % 8 || c_sb % 16 ||
      c_sh % 16 || c_st % 16)
    return CMB_ERR_ALIGNMENT;
  hipStream_t st = (hipStream_t)stream;
#define KVQ_LAUNCH(LPR)                                                                                                       \
  hipLaunchKernelGGL(kv_quantize_kernel<LPR>, dim3((unsigned)((rows + KVQ_THREADS / LPR - 1) / (KVQ_THREADS / LPR))),          \
                     dim3(KVQ_THREADS), 0, st, (const bf16_t*)src, s_sb, s_sh, s_st, rows, nkv, L, hd, (uint8_t*)cache, c_sb, \
                     c_sh, c_st, inv, i_sb, i_sh)
  if (hd <= 64) KVQ_LAUNCH(4); else KVQ_LAUNCH(8);
#undef KVQ_LAUNCH
  CMB_CHECK_LAUNCH();
  return CMB_OK;
}

extern "C" int cmb_decode_attn_kv8(const void* q, int64_t q_ld, const void* k, int64_t k_ld, const void* v, int64_t v_ld,
                                   const float* cos_t, const float* sin_t, void* kcache, void* vcache, int64_t c_sb,
                                   int64_t c_sh, int64_t c_st, float* k_inv, float* v_inv, int64_t i_sb, int64_t i_sh, int64_t B,
                                   int32_t nh, int32_t nkv, int32_t hd, int64_t t, const uint8_t* key_valid, int64_t kv_ld,
                                   float scale, int32_t splits, float* ws, int64_t ws_floats, void* out, void* stream) {
  if (!dec_all_set({q, k, v, cos_t, sin_t, kcache, vcache, k_inv, v_inv, key_valid, out})) return CMB_ERR_BAD_ARG;
  if (!dec_range_ok(B, nkv, t, 1, kv_ld)) return CMB_ERR_BAD_ARG;
  // the geometry rule, the plan and the workspace need are cmb_decode_attn's.  Unlike it, this entry point has always looked at
  // `splits` and the cache strides before it returns from B == 0, so an empty batch is planned as a batch of one.
  int32_t s = 0;
  int64_t chunk = 0;
  if (!dec_geometry_ok(CMB_BF16, nh, nkv, hd) || dec_plan_slots(B > 0 ? B : 1, nkv, t, 1, splits, &s, &chunk, nullptr) != CMB_OK)
    return CMB_ERR_BAD_ARG;
  if (c_sb < 0 || c_sh < 0 || c_st < hd || i_sb < 0 || i_sh < 0) return CMB_ERR_BAD_ARG;
  if (B == 0) return CMB_OK;
  const int64_t need = dec_ws_need(B * nh, s, hd);
  if (need > 0 && (!ws || ws_floats < need)) return CMB_ERR_BAD_ARG;
  if (!dec_aligned16({q, k, v, kcache, vcache, out}, {q_ld, k_ld, v_ld}, 2) || !dec_aligned16({}, {c_sb, c_sh, c_st}, 1) ||
      !aligned4(k_inv) || !aligned4(v_inv))
    return CMB_ERR_ALIGNMENT;

  Dec8Params p;
  p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v;
  p.q_ld = q_ld; p.k_ld = k_ld; p.v_ld = v_ld;
  p.cos_t = cos_t; p.sin_t = sin_t;
  p.kc = (uint8_t*)kcache; p.vc = (uint8_t*)vcache;
  p.c_sb = c_sb; p.c_sh = c_sh; p.c_st = c_st;
  p.k_inv = k_inv; p.v_inv = v_inv;
  p.i_sb = i_sb; p.i_sh = i_sh;
  p.G = nh / nkv; p.nkv = nkv;
  p.t = t;
  p.key_valid = key_valid; p.kv_ld = kv_ld;
  p.scale_log2 = scale * DEC_LOG2E;
  p.splits = s; p.chunk = chunk;
  p.ws = s == 1 ? nullptr : ws;
  p.out = (bf16_t*)out;

  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)s, (unsigned)nkv, (unsigned)B);
  const int G = p.G;
#define DEC8_LAUNCH(HD, GP, E) hipLaunchKernelGGL((decode_attn_kv8_kernel<HD, GP, E>), grid, dim3(DEC_THREADS), 0, st, p)
#define DEC8_GROUP(HD)                           \
  do {                                           \
    if (G == 1) DEC8_LAUNCH(HD, 1, 16);          \
    else if (G == 2) DEC8_LAUNCH(HD, 2, 16);     \
    else if (G <= 4) DEC8_LAUNCH(HD, 4, 16);     \
    else DEC8_LAUNCH(HD, 8, 8);                  \
  } while (0)
  if (hd == 64) DEC8_GROUP(64);
  else if (hd == 96) DEC8_GROUP(96);
  else DEC8_GROUP(128);
#undef DEC8_GROUP
#undef DEC8_LAUNCH
  CMB_CHECK_LAUNCH();
  if (s > 1) {
    dec_launch_combine<bf16_t>(B * nh, ws, G, hd, s, out, st);
    CMB_CHECK_LAUNCH();
  }
  return CMB_OK;
}
