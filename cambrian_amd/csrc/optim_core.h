// optim_core.h — arithmetic of the optimizer kernels (optim.hip: cmb_grad_sqnorm, cmb_adamw_step), written as host+device
// functions so tests/csrc/optim_sim.cpp runs the very same code on the CPU (tests/test_optim_sim.py) before anything is
// launched on a GPU: the bf16 widening / rounding, the fixed summation order of one chunk's sum of squares, the in-order fp64
// sum of the chunk partials, the clip coefficient and the per-element AdamW update.
//
// A CHUNK is CMB_OPTIM_CHUNK consecutive elements of one tensor, the unit of work of a workgroup of CMB_OPTIM_THREADS threads.
// Element i of a chunk belongs to slot (i / 8) % CMB_OPTIM_THREADS, sub-element i % 8, round i / (8 * CMB_OPTIM_THREADS); the
// chunk's sum of squares is formed as
//   acc[slot][e] = fma(g, g, acc[slot][e])          over the rounds, ascending              (cmb_optim_sq_accum)
//   s[slot]      = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7))                         (cmb_optim_sum8)
//   halving tree over the slots: for o = THREADS / 2 .. 1: s[l] += s[l + o] for l < o        (cmb_optim_tree_lane)
// which names every addition, so the result does not depend on how the elements were loaded (16-byte vectors or one by one)
// nor on the grid.  Elements past the end of the tensor contribute nothing (their accumulators stay +0).
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

#define CMB_OPTIM_THREADS 256
#define CMB_OPTIM_CHUNK 65536   /* a power of two <= 65536: 32 rounds of 256 threads x 8 elements */
#define CMB_OPTIM_ROUND (8 * CMB_OPTIM_THREADS)

CMB_PHD int64_t cmb_optim_chunks_of(int64_t n) { return n <= 0 ? 0 : (n + CMB_OPTIM_CHUNK - 1) / CMB_OPTIM_CHUNK; }

// ---- bf16 <-> fp32 ------------------------------------------------------------------------------------------------------------
CMB_PHD uint32_t cmb_f32_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}
CMB_PHD float cmb_bits_f32(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}
// exact: a bf16 is the upper half of an fp32
CMB_PHD float cmb_bf16_widen(uint16_t h) { return cmb_bits_f32((uint32_t)h << 16); }
// round to nearest, ties to even; a NaN becomes the quiet NaN 0x7fc0 (what torch's fp32 -> bf16 cast gives), so that the
// carry of the rounding increment can never turn a NaN into an infinity or a zero
CMB_PHD uint16_t cmb_bf16_rne(float f) {
  const uint32_t u = cmb_f32_bits(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// ---- sum of squares of one chunk ------------------------------------------------------------------------------------------------
CMB_PHD void cmb_optim_sq_accum(float& acc, float g) { acc = fmaf(g, g, acc); }
CMB_PHD float cmb_optim_sum8(const float (&a)[8]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}
// one lane's part of one level of the halving tree over s[0 .. 2 * o); the levels are separated by a barrier on the device
CMB_PHD void cmb_optim_tree_lane(float* s, int lane, int o) {
  if (lane < o) s[lane] = s[lane] + s[lane + o];
}

// sum of the chunk partials in index order, in fp64, rounded once (the second stage of cmb_grad_sqnorm; the device walks the
// same order 64 partials at a time)
CMB_PHD double cmb_optim_final_add(double s, float partial) { return s + (double)partial; }

// ---- clipping ---------------------------------------------------------------------------------------------------------------------
// torch.nn.utils.clip_grad_norm_'s coefficient for gradients that still carry the factor 1 / grad_scale:
//   min(1, max_norm / (grad_scale * sqrt(sumsq) + 1e-6)).
// A NaN norm fails the comparison and gives 1 (the NaN gradients that produced it then reach the update as they are); an
// infinite norm gives 0 and 0 * inf = NaN for the elements that were infinite.
CMB_PHD float cmb_optim_clip_coef(float sumsq, float grad_scale, float max_norm) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float c = max_norm / (grad_scale * sqrtf(sumsq) + 1e-6f);
  return c < 1.0f ? c : 1.0f;
}

// ---- AdamW --------------------------------------------------------------------------------------------------------------------------
// what one launch (one parameter group, one step count) needs, derived once on the host from the by-value hyper-parameters
struct cmb_adamw_consts {
  float decay;      // 1 - lr * weight_decay
  float beta1, omb1;
  float beta2, omb2;
  float step_size;  // lr / bias_correction1
  float sqrt_bc2;   // sqrt(bias_correction2)
  float eps;
};

CMB_PHD cmb_adamw_consts cmb_adamw_make(float lr, float beta1, float beta2, float eps, float weight_decay, float bc1,
                                        float bc2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  cmb_adamw_consts c;
  c.decay = 1.0f - lr * weight_decay;
  c.beta1 = beta1;
  c.omb1 = 1.0f - beta1;
  c.beta2 = beta2;
  c.omb2 = 1.0f - beta2;
  c.step_size = lr / bc1;
  c.sqrt_bc2 = sqrtf(bc2);
  c.eps = eps;
  return c;
}

// torch.optim.AdamW's update of one element, every operation a separately rounded fp32 one (no contraction: the host
// simulation and the kernel must agree), IEEE division and square root.  g is the effective gradient (scale and clip
// coefficient already applied).
CMB_PHD void cmb_adamw_update(float g, float& p, float& m, float& v, const cmb_adamw_consts& c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  p = p * c.decay;
  m = c.beta1 * m + c.omb1 * g;
  v = c.beta2 * v + c.omb2 * (g * g);
  const float denom = sqrtf(v) / c.sqrt_bc2 + c.eps;
  p = p - c.step_size * (m / denom);
}
