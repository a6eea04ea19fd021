// decode_attn.hip — one decode step of a decoder layer's attention, everything between the QKV projection and o_proj
// (the per-token body of generate(); HF LlamaAttention / Phi3Attention with a K/V cache, reached from
// cambrian_llama.py:157-166 with use_cache):
//   * RoPE (rotate-half, the fp32 tables of cmb_rope_table) on the new token's q and k heads,
//   * roped k and raw v written into cache slot t,
//   * softmax(scale * q.K^T).V of every query head over cache keys 0..t, grouped KV heads, key-padding mask with slot t open.
// Roofline class: HBM (the K / V cache is read once per step; everything else is a few KB).
//
// Layout.  One workgroup (4 waves) per (batch row, KV head, chunk of keys); all G = nh / nkv query heads of the KV head
// live in that workgroup, so a cache row is fetched once, not G times.  A K / V row is spread over LPK lanes of 16 bytes
// each (bf16 hd 128: 16 lanes, a wave covers 4 keys per load instruction; hd 96 idles 4 of 16), straight into VGPRs, U = 4
// rows of K and of V in flight per lane (2 at 5-8 heads per group, whose q and accumulators fill the register file) plus the
// next iteration's, no LDS staging.  Every lane group runs its own online
// softmax (fp32 scores / max / sum / accumulators, base-2 exponent) over the keys it is dealt; q.k is VALU plus a DPP
// reduction over the group.  Groups are merged by shuffles inside a wave and through LDS across the four waves.
// Split over keys: chunk c of `splits` writes an un-normalised partial (acc[G][hd], m[G], l[G]) to the workspace and
// decode_combine_kernel merges the chunks in chunk order — two plain launches, no atomics or flags, the same bits on
// every run.  splits == 1 writes `out` directly.  The workgroup of the last chunk owns slot t: it takes the new k / v from
// the arguments (k roped in registers, rounded to the cache dtype as later steps will read it) and is the only one that
// stores them.
#include "decode_attn_common.h"
#include "decode_attn_host.h"

namespace {

struct DecParams {
  const void *q, *k, *v;
  int64_t q_ld, k_ld, v_ld;
  const float *cos_t, *sin_t;
  void *kc, *vc;
  int64_t c_sb, c_sh, c_st;
  int32_t G, nkv;
  int64_t t;
  const uint8_t* key_valid;
  int64_t kv_ld;
  float scale_log2;      // scale * log2(e): scores live in the base-2 exponent domain
  int32_t splits;
  int64_t chunk;
  float* ws;
  void* out;
};

template <typename T, int HD, int GP>
__global__ void __launch_bounds__(DEC_THREADS) decode_attn_kernel(const DecParams p) {
  constexpr int E = Row16<T>::E;
  constexpr int LPKA = HD / E;                                    // lanes that hold a piece of a row
  constexpr int LPK = LPKA <= 8 ? 8 : (LPKA <= 16 ? 16 : 32);     // lanes per key (power of two)
  constexpr int KPW = 64 / LPK;                                   // keys per wave and load instruction
  constexpr int DEC_U = GP > 4 ? 2 : 4;                           // rows of K (and of V) per lane and iteration
  constexpr int STEP = DEC_U * DEC_WAVES * KPW;                   // keys per workgroup iteration
  constexpr int HALF = HD / 2;
  typedef typename Row16<T>::raw raw;

  __shared__ float sm_acc[DEC_WAVES][GP * HD];
  __shared__ float sm_m[DEC_WAVES][GP], sm_l[DEC_WAVES][GP];

  const int c = blockIdx.x, kvh = blockIdx.y;
  const int64_t b = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & (LPK - 1), kg = lane / LPK;
  const bool active = li < LPKA;
  const int d0 = active ? li * E : 0;         // idle lanes (hd 96) shadow piece 0 with q = 0; they never store
  const int G = p.G;

  float cs[E], sn[E];
  {
    const int dr = d0 >= HALF ? d0 - HALF : d0;
    const float* ct = p.cos_t + b * HALF + dr;
    const float* st = p.sin_t + b * HALF + dr;
#pragma unroll
    for (int e = 0; e < E; ++e) { cs[e] = ct[e]; sn[e] = st[e]; }
  }
  float q[GP][E];
#pragma unroll
  for (int g = 0; g < GP; ++g) {
    if (g < G && active) {
      rope_slice<T, HD>((const T*)p.q + b * p.q_ld + (int64_t)(kvh * G + g) * HD, d0, cs, sn, q[g]);
#pragma unroll
      for (int e = 0; e < E; ++e) q[g][e] *= p.scale_log2;
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) q[g][e] = 0.f;
    }
  }

  float m[GP], l[GP], acc[GP][E];
#pragma unroll
  for (int g = 0; g < GP; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) acc[g][e] = 0.f;
  }

  // one online-softmax step over U scored rows: s[u][g] (-inf = not attendable; overwritten with the weights), rv[u] the
  // rows of V as loaded (a row that is not attendable may hold anything, NaN included: it is not multiplied in)
  auto absorb = [&](float (&s)[DEC_U][GP], const raw (&rv)[DEC_U], const bool (&o)[DEC_U]) {
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
      for (int e = 0; e < E; ++e) acc[g][e] *= alpha;
    }
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
      float vf[E];
      Row16<T>::to_f32(rv[u], vf);
#pragma unroll
      for (int e = 0; e < E; ++e) vf[e] = o[u] ? vf[e] : 0.f;
#pragma unroll
      for (int g = 0; g < GP; ++g) {
#pragma unroll
        for (int e = 0; e < E; ++e) acc[g][e] += s[u][g] * vf[e];
      }
    }
  };

  // ---- cached keys [c0, c1) of this chunk (slot t is never read back) ----
  const int64_t c0 = (int64_t)c * p.chunk;
  const int64_t c1 = (c0 + p.chunk < p.t) ? c0 + p.chunk : p.t;
  const T* kb = (const T*)p.kc + b * p.c_sb + (int64_t)kvh * p.c_sh + d0;
  const T* vb = (const T*)p.vc + b * p.c_sb + (int64_t)kvh * p.c_sh + d0;
  const uint8_t* kvp = p.key_valid + b * p.kv_ld;

  raw kr[DEC_U], vr[DEC_U], nkr[DEC_U], nvr[DEC_U];
  bool ok[DEC_U], nok[DEC_U];
  auto fetch = [&](int64_t base, raw (&rk)[DEC_U], raw (&rv)[DEC_U], bool (&o)[DEC_U]) {
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
      const int64_t j = base + (u * DEC_WAVES + wave) * KPW + kg;
      const bool in = j < c1;
      const int64_t jj = in ? j : c0;          // past the chunk: re-read its first row (c0 < c1 here), weight 0
      rk[u] = *reinterpret_cast<const raw*>(kb + jj * p.c_st);
      rv[u] = *reinterpret_cast<const raw*>(vb + jj * p.c_st);
      o[u] = in & (kvp[jj] != 0);              // jj is in range either way: no branch around the byte load
    }
  };
  if (c0 < c1) fetch(c0, kr, vr, ok);
  for (int64_t base = c0; base < c1; base += STEP) {
    const bool more = base + STEP < c1;
    if (more) fetch(base + STEP, nkr, nvr, nok);
    float s[DEC_U][GP];
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
      float kf[E];
      Row16<T>::to_f32(kr[u], kf);
#pragma unroll
      for (int g = 0; g < GP; ++g) {
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < E; ++e) d += q[g][e] * kf[e];
        d = group_sum<LPK>(d);
        s[u][g] = ok[u] ? d : -INFINITY;
      }
    }
    absorb(s, vr, ok);
    if (more) {
#pragma unroll
      for (int u = 0; u < DEC_U; ++u) { kr[u] = nkr[u]; vr[u] = nvr[u]; ok[u] = nok[u]; }
    }
  }

  // ---- the new token (slot t), in the workgroup of the last chunk ----
  if (c == p.splits - 1) {
    float kn[E];
    rope_slice<T, HD>((const T*)p.k + b * p.k_ld + (int64_t)kvh * HD, d0, cs, sn, kn);
    const raw kraw = Row16<T>::from_f32(kn);
    const raw vraw = *reinterpret_cast<const raw*>((const T*)p.v + b * p.v_ld + (int64_t)kvh * HD + d0);
    Row16<T>::to_f32(kraw, kn);               // attend to what the cache will hold
    const bool mine = wave == 0 && kg == 0;   // one lane group scores it; group_sum needs every lane, so all compute
    float s[DEC_U][GP];
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
      vr[u] = vraw;
      ok[u] = u == 0 && mine;
#pragma unroll
      for (int g = 0; g < GP; ++g) s[u][g] = -INFINITY;
    }
#pragma unroll
    for (int g = 0; g < GP; ++g) {
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) d += q[g][e] * kn[e];
      d = group_sum<LPK>(d);
      s[0][g] = mine ? d : -INFINITY;
    }
    absorb(s, vr, ok);
    if (mine && active) {
      const int64_t off = b * p.c_sb + (int64_t)kvh * p.c_sh + p.t * p.c_st + d0;
      *reinterpret_cast<raw*>((T*)p.kc + off) = kraw;
      *reinterpret_cast<raw*>((T*)p.vc + off) = vraw;
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
      for (int e = 0; e < E; ++e) acc[g][e] = acc[g][e] * wa + __shfl_xor(acc[g][e], o, 64) * wb;
    }
  }
  // ---- and the four waves through LDS ----
  if (kg == 0 && active) {
#pragma unroll
    for (int g = 0; g < GP; ++g) {
#pragma unroll
      for (int e = 0; e < E; ++e) sm_acc[wave][g * HD + d0 + e] = acc[g][e];
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
      ((T*)p.out)[(head0 + g) * HD + d] = (T)(num / den);    // den > 0: slot t is always attendable
    } else {
      part[idx] = num;
      if (d == 0) { part[G * HD + g] = M; part[G * HD + G + g] = den; }
    }
  }
}

int dec_cu_count() {
  static std::atomic<int> cached{0};
  int n = cached.load(std::memory_order_relaxed);
  if (n > 0) return n;
  int dev = 0;
  n = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    return 256;          // no device (host-side queries): an MI355X's count; not cached
  }
  cached.store(n, std::memory_order_relaxed);
  return n;
}

// splits * chunk >= t + 1 > (splits - 1) * chunk: no chunk is empty and the last one holds slot t
bool dec_plan(int64_t B, int32_t nkv, int64_t t, int32_t forced, int32_t* splits, int64_t* chunk) {
  if (B <= 0 || nkv <= 0 || t < 0 || forced < 0 || forced > DEC_MAX_SPLITS) return false;
  const int64_t len = t + 1;
  int64_t s = forced;
  if (s == 0) {          // about two workgroups per CU, never chunks under DEC_MIN_CHUNK keys
    const int64_t want = 2 * (int64_t)dec_cu_count(), rows = B * nkv;
    s = (want + rows - 1) / rows;
    if (s > len / DEC_MIN_CHUNK) s = len / DEC_MIN_CHUNK;
    if (s > DEC_MAX_SPLITS) s = DEC_MAX_SPLITS;
    if (s < 1) s = 1;
  }
  if (s > len) s = len;
  *chunk = (len + s - 1) / s;
  *splits = (int32_t)((len + *chunk - 1) / *chunk);
  return true;
}

}  // namespace

// dec_geometry_ok and the plan query, declared in decode_attn_host.h for the other two files
bool dec_geometry_ok(int dtype, int32_t nh, int32_t nkv, int32_t hd) {
  if (dtype != CMB_BF16 && dtype != CMB_F32) return false;
  if (hd != 64 && hd != 96 && hd != 128) return false;
  if (nh <= 0 || nkv <= 0 || nh % nkv != 0 || nh / nkv > DEC_MAX_GROUP) return false;
  return true;
}

int dec_plan_slots(int64_t B, int32_t nkv, int64_t t0, int64_t n, int32_t forced, int32_t* splits_out, int64_t* chunk_out,
                   int32_t* max_splits_out) {
  if (max_splits_out) *max_splits_out = DEC_MAX_SPLITS;
  int32_t s = 0;
  int64_t ch = 0;
  if (t0 < 0 || n < 1 || !dec_plan(B, nkv, t0 + n - 1, forced, &s, &ch)) return CMB_ERR_BAD_ARG;
  if (splits_out) *splits_out = s;
  if (chunk_out) *chunk_out = ch;
  return CMB_OK;
}

extern "C" int cmb_decode_attn_plan(int64_t B, int32_t nkv, int64_t t, int32_t splits, int32_t* splits_out,
                                    int64_t* chunk_out, int32_t* max_splits_out) {
  return dec_plan_slots(B, nkv, t, 1, splits, splits_out, chunk_out, max_splits_out);
}

extern "C" int64_t cmb_decode_attn_ws(int64_t B, int32_t nh, int32_t nkv, int32_t hd, int64_t t, int32_t splits) {
  int32_t s = 0;
  int64_t ch = 0;
  if (!dec_geometry_ok(CMB_F32, nh, nkv, hd) || !dec_plan(B, nkv, t, splits, &s, &ch)) return CMB_ERR_BAD_ARG;
  return dec_ws_need(B * nh, s, hd);
}

extern "C" int cmb_decode_attn(int dtype, const void* q, int64_t q_ld, const void* k, int64_t k_ld, const void* v,
                               int64_t v_ld, const float* cos_t, const float* sin_t, void* kcache, void* vcache,
                               int64_t c_sb, int64_t c_sh, int64_t c_st, int64_t B, int32_t nh, int32_t nkv, int32_t hd,
                               int64_t t, const uint8_t* key_valid, int64_t kv_ld, float scale, int32_t splits, float* ws,
                               int64_t ws_floats, void* out, void* stream) {
  if (!dec_all_set({q, k, v, cos_t, sin_t, kcache, vcache, key_valid, out})) return CMB_ERR_BAD_ARG;
  if (!dec_geometry_ok(dtype, nh, nkv, hd) || !dec_range_ok(B, nkv, t, 1, kv_ld)) return CMB_ERR_BAD_ARG;
  if (B == 0) return CMB_OK;
  int32_t s = 0;
  int64_t chunk = 0;
  if (!dec_plan(B, nkv, t, splits, &s, &chunk)) return CMB_ERR_BAD_ARG;
  const int64_t need = dec_ws_need(B * nh, s, hd);
  if (need > 0 && (!ws || ws_floats < need)) return CMB_ERR_BAD_ARG;
  if (!dec_aligned16({q, k, v, kcache, vcache, out}, {q_ld, k_ld, v_ld, c_sb, c_sh, c_st}, dtype == CMB_BF16 ? 2 : 4))
    return CMB_ERR_ALIGNMENT;

  DecParams p;
  p.q = q; p.k = k; p.v = v;
  p.q_ld = q_ld; p.k_ld = k_ld; p.v_ld = v_ld;
  p.cos_t = cos_t; p.sin_t = sin_t;
  p.kc = kcache; p.vc = vcache;
  p.c_sb = c_sb; p.c_sh = c_sh; p.c_st = c_st;
  p.G = nh / nkv; p.nkv = nkv;
  p.t = t;
  p.key_valid = key_valid; p.kv_ld = kv_ld;
  p.scale_log2 = scale * DEC_LOG2E;
  p.splits = s; p.chunk = chunk;
  p.ws = s == 1 ? nullptr : ws;
  p.out = out;

  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)s, (unsigned)nkv, (unsigned)B);
  const int G = p.G;
#define DEC_LAUNCH(T, HD, GP) hipLaunchKernelGGL((decode_attn_kernel<T, HD, GP>), grid, dim3(DEC_THREADS), 0, st, p)
#define DEC_GROUP(T, HD)                           \
  do {                                             \
    if (G == 1) DEC_LAUNCH(T, HD, 1);              \
    else if (G == 2) DEC_LAUNCH(T, HD, 2);         \
    else if (G <= 4) DEC_LAUNCH(T, HD, 4);         \
    else DEC_LAUNCH(T, HD, 8);                     \
  } while (0)
#define DEC_HD(T)                                  \
  do {                                             \
    if (hd == 64) DEC_GROUP(T, 64);                \
    else if (hd == 96) DEC_GROUP(T, 96);           \
    else DEC_GROUP(T, 128);                        \
  } while (0)
  if (dtype == CMB_BF16) DEC_HD(bf16_t); else DEC_HD(float);
#undef DEC_HD
#undef DEC_GROUP
#undef DEC_LAUNCH
  CMB_CHECK_LAUNCH();
  if (s > 1) {
    if (dtype == CMB_BF16) dec_launch_combine<bf16_t>(B * nh, ws, G, hd, s, out, st);
    else dec_launch_combine<float>(B * nh, ws, G, hd, s, out, st);
    CMB_CHECK_LAUNCH();
  }
  return CMB_OK;
}
