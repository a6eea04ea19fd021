// decode_attn_common.h — what the decode-attention kernels share (decode_attn.hip on bf16 / fp32 caches, decode_attn_kv8.hip on
// e4m3 caches, decode_attn_multi.hip for Q tokens per step): the workgroup shape and the limits of the plan, the 16-byte row
// pieces, the DPP lane-group reductions, RoPE of a new-token slice, the weight of a partial and the kernel that merges the
// chunks' partials of the two single-token files.  Constants and device code; what the three launchers share on the host is in
// decode_attn_host.h, and the plan and the geometry rule stay in decode_attn.hip (reached through that header).
#pragma once
#include "common.h"

namespace {

constexpr int DEC_THREADS = 256, DEC_WAVES = 4;
constexpr int DEC_MAX_SPLITS = 64;    // cmb_decode_attn_plan reports it
constexpr int DEC_MIN_CHUNK = 128;    // keys per chunk below which the library does not split further
constexpr int DEC_MAX_GROUP = 8;

template <typename T> struct Row16;   // 16 bytes of a row: E elements
template <> struct Row16<bf16_t> {
  static constexpr int E = 8;
  typedef bf16x8_t raw;
  static __device__ __forceinline__ void to_f32(const raw& r, float (&v)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)r[i];
  }
  static __device__ __forceinline__ raw from_f32(const float (&v)[8]) {
    return cvt8_bf16(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
  }
};
template <> struct Row16<float> {
  static constexpr int E = 4;
  typedef f32x4_t raw;
  static __device__ __forceinline__ void to_f32(const raw& r, float (&v)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = r[i];
  }
  static __device__ __forceinline__ raw from_f32(const float (&v)[4]) { return (raw){v[0], v[1], v[2], v[3]}; }
};

// v + / max (v of the lane the DPP control names); controls used: quad_perm [1,0,3,2] / [2,3,0,1], row_half_mirror, row_mirror
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  const int o = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true);
  return v + __builtin_bit_cast(float, o);
}
template <int CTRL>
__device__ __forceinline__ float dpp_max(float v) {
  const int o = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true);
  return fmaxf(v, __builtin_bit_cast(float, o));
}
// sum over an aligned group of LPK (4 / 8 / 16 / 32) lanes, result in every lane of the group; all 64 lanes must be active
template <int LPK>
__device__ __forceinline__ float group_sum(float v) {
  static_assert(LPK == 4 || LPK == 8 || LPK == 16 || LPK == 32, "lane groups of 4, 8, 16 or 32");
  v = dpp_add<0xB1>(v);
  v = dpp_add<0x4E>(v);
  if (LPK >= 8) v = dpp_add<0x141>(v);        // quads hold equal sums: the mirrored lane is in the other quad
  if (LPK >= 16) v = dpp_add<0x140>(v);
  if (LPK >= 32) v += __shfl_xor(v, 16, 64);
  return v;
}
// the maximum likewise, over 4 / 8 / 16 lanes
template <int LPK>
__device__ __forceinline__ float group_max(float v) {
  static_assert(LPK == 4 || LPK == 8 || LPK == 16, "lane groups of 4, 8 or 16");
  v = dpp_max<0xB1>(v);
  v = dpp_max<0x4E>(v);
  if (LPK >= 8) v = dpp_max<0x141>(v);
  if (LPK >= 16) v = dpp_max<0x140>(v);
  return v;
}

__device__ __forceinline__ float dec_weight(float m, float mref) {   // exp2(m - mref), 0 for an empty partial (m = -inf)
  return m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m - mref);
}

// new-token row `x` (E elements at d0 and the E at the rotate-half partner position) -> roped E elements at d0
template <typename T, int HD>
__device__ __forceinline__ void rope_slice(const T* x, int d0, const float (&cs)[Row16<T>::E], const float (&sn)[Row16<T>::E],
                                           float (&o)[Row16<T>::E]) {
  constexpr int E = Row16<T>::E, HALF = HD / 2;
  typedef typename Row16<T>::raw raw;
  const bool hi = d0 >= HALF;
  float a[E], b[E];
  Row16<T>::to_f32(*reinterpret_cast<const raw*>(x + d0), a);
  Row16<T>::to_f32(*reinterpret_cast<const raw*>(x + (hi ? d0 - HALF : d0 + HALF)), b);
#pragma unroll
  for (int e = 0; e < E; ++e) o[e] = hi ? a[e] * cs[e] + b[e] * sn[e] : a[e] * cs[e] - b[e] * sn[e];
}

// out[b, h, :] = sum_c acc_c * 2^(m_c - M) / sum_c l_c * 2^(m_c - M), chunks in order; an empty chunk (m = -inf) weighs 0
template <typename T>
__global__ void __launch_bounds__(128) decode_combine_kernel(const float* __restrict__ ws, int G, int hd, int splits,
                                                             T* __restrict__ out) {
  const int64_t h = blockIdx.x;                 // query head counted over the batch
  const int64_t hk = h / G;
  const int g = (int)(h - hk * G);
  const int d = threadIdx.x;
  if (d >= hd) return;
  const int64_t ps = (int64_t)G * (hd + 2);
  const float* base = ws + hk * splits * ps;
  float M = -INFINITY;
  for (int c = 0; c < splits; ++c) M = fmaxf(M, base[c * ps + G * hd + g]);
  float num = 0.f, den = 0.f;
  for (int c = 0; c < splits; ++c) {
    const float* pc = base + c * ps;
    const float wt = dec_weight(pc[G * hd + g], M);
    num += pc[g * hd + d] * wt;
    den += pc[G * hd + G + g] * wt;
  }
  out[h * hd + d] = (T)(num / den);
}

}  // namespace
