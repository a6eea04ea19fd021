// rowmap.h — the 3-level row map (cmb_rowmap, include/cambrian_amd.h) as the kernels and the host-side planning read it.
// No HIP include: the kernels get it through common.h, gemm_plan.h and its CPU simulation include it directly.
#pragma once
#include <stdint.h>
#include "../../include/cambrian_amd.h"

#if defined(__HIPCC__)
#define CMB_HOST_DEVICE __host__ __device__
#else
#define CMB_HOST_DEVICE
#endif

struct RowMap {
  uint32_t n1, n2;
  int64_t s0, s1, s2;
};
static inline RowMap make_rowmap(const cmb_rowmap& m) {
  RowMap r;
  r.n1 = (uint32_t)m.n1; r.n2 = (uint32_t)(m.n2 ? m.n2 : 1);
  r.s0 = m.s0; r.s1 = m.s1; r.s2 = m.s2;
  return r;
}
CMB_HOST_DEVICE static inline int64_t row_off(const RowMap& m, uint32_t r) {
  if (m.n1 == 0) return (int64_t)r * m.s2;
  uint32_t a = r / m.n1, rem = r - a * m.n1;
  uint32_t b = rem / m.n2, c = rem - b * m.n2;
  return (int64_t)a * m.s0 + (int64_t)b * m.s1 + (int64_t)c * m.s2;
}
