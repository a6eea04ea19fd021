// resample_core.h — per-axis arithmetic of the bilinear token-grid resample (elementwise.hip: resample_kernel and its
// adjoint resample_bwd_kernel), written as host+device functions so tests/csrc/resample_sim.cpp can run the very same code
// on the CPU (tests/test_resample_sim.py) before anything is launched on a GPU.
//
// Forward, one axis (torch upsample_bilinear2d, align_corners = False): output o reads inputs i0, i1 with weights 1 - l1, l1
//   src = max(0, scale * (o + 0.5) - 0.5),  i0 = min(floor(src), n_in - 1),  i1 = min(i0 + 1, n_in - 1),  l1 = src - i0
// with scale = n_in / n_out in float.  The adjoint gathers: input i sums over the outputs that name it.  src is monotone in
// o, so those outputs form one contiguous run; cmb_resample_window gives a conservative candidate range from the inverse map
// and cmb_resample_weight decides membership and weight by calling lerp_index itself, so that the two kernels cannot disagree.
//
// cmb_resample_accum (resample_accum.hip) sums up to CMB_RESAMPLE_ACCUM_MAX_SRC resized maps onto a base: its thread -> cell
// decomposition and the whole per-cell sum are cmb_resample_accum_decode / cmb_resample_accum_cell below, run on the CPU by
// tests/csrc/resample_accum_sim.cpp.
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

CMB_PHD void lerp_index(int o, float scale, int in_size, int& i0, int& i1, float& l1) {
  float src = scale * ((float)o + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  i0 = (int)src;
  if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
  l1 = src - (float)i0;
}

// weight of input i in output o along one axis; 0 when o does not name i.  At the clamped far edge i1 == i0 and both terms
// go to the same cell.
CMB_PHD float cmb_resample_weight(int o, float scale, int n_in, int i) {
  int i0, i1;
  float l1;
  lerp_index(o, scale, n_in, i0, i1, l1);
  return (i0 == i ? 1.f - l1 : 0.f) + (i1 == i ? l1 : 0.f);
}

// candidate outputs [lo, hi] of input i: o names i when floor(src) is i - 1 or i, i.e. src in [i - 1, i + 1), which the
// inverse map turns into o in [(i - 0.5) / scale - 0.5, (i + 1.5) / scale - 0.5); widened by one output on each side against
// the float rounding of either map.  src is clamped below at 0, so the outputs in front of the first sample point all read
// inputs 0 and 1 (the latter with weight 0): the windows of both start at 0.  i0 is clamped above at n_in - 1, so the last
// input owns every output up to n_out - 1.  Never empty; at most cmb_resample_window_bound wide.
CMB_PHD void cmb_resample_window(int i, int n_in, int n_out, int& lo, int& hi) {
  const float inv = (float)n_out / (float)n_in;
  lo = (int)floorf(((float)i - 0.5f) * inv - 0.5f) - 1;
  hi = (int)ceilf(((float)i + 1.5f) * inv - 0.5f) + 1;
  if (lo < 0 || i <= 1) lo = 0;
  if (hi > n_out - 1 || i == n_in - 1) hi = n_out - 1;
  if (lo > n_out - 1) lo = n_out - 1;
  if (hi < lo) hi = lo;
}

// the trip count the adjoint kernel's per-axis loops are sized for: the 2 / scale outputs of the interval above (2.5 / scale
// for input 1, whose window reaches down to output 0), its two end points and the two widening outputs.
CMB_PHD int cmb_resample_window_bound(int n_in, int n_out) { return (5 * ((n_out + n_in - 1) / n_in) + 1) / 2 + 4; }

// ---- cmb_resample_accum: pre = base + bias + sum_s lerp_s(src_s), one (output cell, 8 channels) at a time ----------------
#ifndef CMB_RESAMPLE_ACCUM_MAX_SRC
#define CMB_RESAMPLE_ACCUM_MAX_SRC 4
#endif

// work item i of B * Ho * Wo * nv (nv = C / 8 channel vectors, fastest) -> (batch, oy, ox, channel vector): consecutive
// lanes walk the channels of one cell, then the cells of a row — every access of a wave is one contiguous run per row
CMB_PHD void cmb_resample_accum_decode(int64_t i, int nv, int Ho, int Wo, int64_t& b, int& oy, int& ox, int& cv) {
  const int64_t cell = i / nv;
  cv = (int)(i - cell * nv);
  const int cells = Ho * Wo;
  b = cell / cells;
  const int r = (int)(cell - b * cells);
  oy = r / Wo;
  ox = r - oy * Wo;
}

// one source's bilinear sample of cell (oy, ox): the forward kernel's own expression (resample_kernel), on the four
// neighbours that lerp_index names.  load(row, v) reads the 8 channels of source row `row` = y * Wi + x as floats.
template <typename Load>
CMB_PHD void cmb_resample_lerp8(int oy, int ox, int Hi, int Wi, int Ho, int Wo, Load&& load, float (&o)[8]) {
  const float sy = (float)Hi / (float)Ho, sx = (float)Wi / (float)Wo;
  int y0, y1, x0, x1;
  float ly, lx;
  lerp_index(oy, sy, Hi, y0, y1, ly);
  lerp_index(ox, sx, Wi, x0, x1, lx);
  float v00[8], v01[8], v10[8], v11[8];
  load((int64_t)y0 * Wi + x0, v00);
  load((int64_t)y0 * Wi + x1, v01);
  load((int64_t)y1 * Wi + x0, v10);
  load((int64_t)y1 * Wi + x1, v11);
  const float hy = 1.f - ly, hx = 1.f - lx;
  for (int e = 0; e < 8; ++e) o[e] = hy * (hx * v00[e] + lx * v01[e]) + ly * (hx * v10[e] + lx * v11[e]);
}

// the cell's pre-activation: acc = base + bias on entry (zeros where absent), then the sources are added in list order, in
// fp32; the caller rounds once.  load(s, row, v) reads source s.
template <typename Load>
CMB_PHD void cmb_resample_accum_cell(int oy, int ox, int Ho, int Wo, int n_src, const int32_t* Hi, const int32_t* Wi,
                                     Load&& load, float (&acc)[8]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int s = 0; s < CMB_RESAMPLE_ACCUM_MAX_SRC; ++s) {
    if (s >= n_src) break;
    float o[8];
    cmb_resample_lerp8(oy, ox, Hi[s], Wi[s], Ho, Wo, [&](int64_t row, float (&v)[8]) { load(s, row, v); }, o);
    for (int e = 0; e < 8; ++e) acc[e] += o[e];
  }
}
