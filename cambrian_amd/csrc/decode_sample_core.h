// decode_sample_core.h — arithmetic of the token selection kernels (decode_next.hip, decode_sample.hip), written as host+device
// functions so tests/csrc/decode_sample_core_sim.cpp runs the very same code on the CPU (tests/test_decode_sample_core_sim.py):
// the monotone 32-bit key of a float and its inverse, Philox4x32-10, the uniform of a random word and its negated logarithm,
// the Gumbel noise, and the fixed-point probability mass whose integer sums do not depend on the order of the additions.
#pragma once
#include <math.h>
#include <stdint.h>

#if !defined(CMB_PHD)
#if defined(__HIPCC__)
#define CMB_PHD __host__ __device__ __forceinline__
#else
#define CMB_PHD static inline
#endif
#endif

CMB_PHD uint32_t cmb_ds_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}
CMB_PHD float cmb_ds_float(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

// ---- the key: unsigned order of the keys = order of the floats -----------------------------------------------------------------
// negative: all bits flipped, else the sign bit set; -0 is read as +0, any NaN as 0xFFFFFFFF (above +inf, torch.argmax's rule).
// -inf is 0x007FFFFF, the smallest key there is; no float maps below it.
CMB_PHD uint32_t cmb_ds_key32(float v) {
  const uint32_t b = cmb_ds_bits(v);
  if (v != v) return 0xFFFFFFFFu;
  if (v == 0.f) return 0x80000000u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// the float of a key that cmb_ds_key32 gave for a number (not a NaN)
CMB_PHD float cmb_ds_key32_value(uint32_t k) { return cmb_ds_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// ---- Philox4x32-10 (Salmon et al., SC'11) -------------------------------------------------------------------------------------
typedef struct cmb_philox4 {
  uint32_t w[4];
} cmb_philox4;

CMB_PHD cmb_philox4 cmb_ds_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  cmb_philox4 out;
  out.w[0] = c0; out.w[1] = c1; out.w[2] = c2; out.w[3] = c3;
  return out;
}

// the words of elements 4g .. 4g + 3 of row b at draw `step` under `seed`: counter (g, b, step, 0), key (seed low, seed high)
CMB_PHD cmb_philox4 cmb_ds_words(uint64_t seed, uint32_t group, uint32_t b, uint32_t step) {
  return cmb_ds_philox(group, b, step, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// ---- the uniform and the Gumbel noise -----------------------------------------------------------------------------------------
// u = ((word >> 8) + 0.5) * 2^-24 = (2n + 1) * 2^-25 with n < 2^24: strictly inside (0, 1).  2n + 1 has up to 25 bits, one more
// than an fp32 holds, so u is an fp32 number only for n < 2^23 (u < 1/2); for the other half 1 - u = (2 (2^24 - n) - 1) * 2^-25
// is one.  -log u is therefore taken as -logf(u) below one half and as -log1pf(-(1 - u)) above: both arguments are exact, and
// u never rounds to 1 (which would make the noise infinite).
CMB_PHD double cmb_ds_u(uint32_t word) { return ((double)(word >> 8) + 0.5) * (1.0 / 16777216.0); }   // exact, for host checks
CMB_PHD float cmb_ds_neg_log_u(uint32_t word) {
  const uint32_t n = word >> 8;
  if (n < 0x800000u) return -logf((float)(2u * n + 1u) * (1.0f / 33554432.0f));
  return -log1pf(-((float)(2u * (0x1000000u - n) - 1u) * (1.0f / 33554432.0f)));
}
// g = -log(-log u): between -2.86 (u = 2^-25) and 17.33 (1 - u = 2^-25)
CMB_PHD float cmb_ds_gumbel(uint32_t word) { return -logf(cmb_ds_neg_log_u(word)); }
#define CMB_DS_GUMBEL_MAX 17.33f   /* 25 ln 2 = 17.3287 */

// A cheap upper bound of cmb_ds_gumbel(word) for the draw: most elements cannot reach the best score seen so far, and this
// tells without the accurate logarithms.  It takes the hardware's log2 (1 ulp) where the device has one:
//   below one half  u is exact, t' = -log2(u) ln 2 lies in [0.69, 17.4] with a relative error of a few 1e-7;
//   above           u' = 1 - (1 - u) rounds once (6e-8), so t' is off by at most about 3e-7 ABSOLUTE; t' < 0.01 (u within 1 % of
//                   1: the largest noise there is, and where that error would matter) answers +inf, "ask the accurate form";
//                   otherwise the relative error of t' is at most 3e-5;
// so -log2(t') ln 2 is within 4e-5 of g.  CMB_DS_GUMBEL_SLACK on top of it covers that more than twice over and the rounding of
// a sum of magnitude <= 128 as well (an ulp of 8e-6).
#define CMB_DS_GUMBEL_SLACK 1e-4f
#if defined(__HIP_DEVICE_COMPILE__)
#define CMB_DS_LOG2(x) __log2f(x)
#else
#define CMB_DS_LOG2(x) log2f(x)
#endif
CMB_PHD float cmb_ds_gumbel_bound(uint32_t word) {
  const uint32_t n = word >> 8;
  const bool low = n < 0x800000u;
  const float m = (float)(low ? 2u * n + 1u : 2u * (0x1000000u - n) - 1u) * (1.0f / 33554432.0f);   // u, or 1 - u
  const float t = -CMB_DS_LOG2(low ? m : 1.0f - m) * 0.69314718f;
  if (!low && t < 1e-2f) return INFINITY;
  return -CMB_DS_LOG2(t) * 0.69314718f + CMB_DS_GUMBEL_SLACK;
}

// ---- fixed-point probability mass ---------------------------------------------------------------------------------------------
// w = exp(z - z_max) in (0, 1] as an integer multiple of 2^-40: at most 2^40 per term, so 2^17 terms stay below 2^58 and a sum in
// uint64 is exact, whatever its order.  A weight below 2^-40 counts as nothing.
#define CMB_DS_MASS_ONE 1099511627776.0f   /* 2^40 */
CMB_PHD uint64_t cmb_ds_mass(float z, float z_max) { return (uint64_t)(expf(z - z_max) * CMB_DS_MASS_ONE); }

// the nucleus target: the largest integer T with T <= (1 - top_p) * Z, clamped below Z so that the maximum is always kept;
// "mass > (1 - top_p) * Z" for an integer mass is "mass >= T + 1"
CMB_PHD uint64_t cmb_ds_nucleus_target(float top_p, uint64_t Z) {
  const double t = (1.0 - (double)top_p) * (double)Z;
  uint64_t T = t <= 0.0 ? 0u : (uint64_t)t;
  if (Z && T > Z - 1) T = Z - 1;
  return T;
}
