// resample_core.h — per-axis arithmetic of the bilinear token-grid resample (elementwise.hip: resample_kernel and its
// adjoint resample_bwd_kernel), written as host+device functions so tests/csrc/resample_sim.cpp can run the very same code
// on the CPU (tests/test_resample_sim.py) before anything is launched on a GPU.
//
// Forward, one axis (torch upsample_bilinear2d, align_corners = False): output o reads inputs i0, i1 with weights 1 - l1, l1
//   src = max(0, scale * (o + 0.5) - 0.5),  i0 = min(floor(src), n_in - 1),  i1 = min(i0 + 1, n_in - 1),  l1 = src - i0
// with scale = n_in / n_out in float.  The adjoint gathers: input i sums over the outputs that name it.  src is monotone in
// o, so those outputs form one contiguous run; cmb_resample_window gives a conservative candidate range from the inverse map
// and cmb_resample_weight decides membership and weight by calling lerp_index itself, so that the two kernels cannot disagree.
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
