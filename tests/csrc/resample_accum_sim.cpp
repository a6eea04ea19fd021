// Host-side run of cmb_resample_accum's per-cell code (cambrian_amd/csrc/resample_core.h, the very header
// resample_accum.hip includes): the kernel's loop over work items — cmb_resample_accum_decode, base + bias, then
// cmb_resample_accum_cell over the sources in list order, fp32 — against an independent double-precision bilinear sum
// (torch upsample_bilinear2d, align_corners = False, written out again here in double, indices included).
//   grids   (8 -> 12), (4 -> 12), (2 -> 8), (64 -> 96), (32 -> 96), (1 -> 4), (4, 6) -> (7, 3)
//   n_src   0, 1, 2 (the second source has half the first one's grid)
//   base / bias present and absent (n_src = 0 needs a base: that is the entry point's rule)
// Bound: 1e-5 of the largest reference value (the fp32 bound of the GPU tests): fp32 lerp weights and a sum of at most
// 2 + 2 * 4 fp32 terms of order 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../cambrian_amd/csrc/resample_core.h"

static int fails = 0;
static double worst = 0;
static int cases = 0;

static uint32_t lcg_state = 12345u;
static float rnd() {   // uniform in [-2, 2)
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return (float)((lcg_state >> 8) & 0xffff) / 16384.f - 2.f;
}

struct Src {
  int H, W;
  std::vector<float> x;   // [B, H*W, ld]
};

// double-precision reference, nothing shared with the header
static double ref_bilinear(const Src& s, int ld, int b, int c, int oy, int ox, int Ho, int Wo) {
  auto axis = [](int o, int n_in, int n_out, int& i0, int& i1, double& l) {
    double src = ((double)n_in / (double)n_out) * (o + 0.5) - 0.5;
    if (src < 0) src = 0;
    i0 = (int)std::floor(src);
    if (i0 > n_in - 1) i0 = n_in - 1;
    i1 = i0 + 1 < n_in ? i0 + 1 : n_in - 1;
    l = src - i0;
  };
  int y0, y1, x0, x1;
  double ly, lx;
  axis(oy, s.H, Ho, y0, y1, ly);
  axis(ox, s.W, Wo, x0, x1, lx);
  auto at = [&](int y, int x) { return (double)s.x[((size_t)b * s.H * s.W + (size_t)y * s.W + x) * ld + c]; };
  return (1 - ly) * ((1 - lx) * at(y0, x0) + lx * at(y0, x1)) + ly * ((1 - lx) * at(y1, x0) + lx * at(y1, x1));
}

static void run_case(int Hi, int Wi, int Ho, int Wo, int n_src, bool has_base, bool has_bias) {
  const int B = 2, C = 16, ld = C + 8;   // rows wider than C: a column slice of a wider buffer
  const int nv = C / 8;
  std::vector<Src> srcs(n_src);
  int32_t H[CMB_RESAMPLE_ACCUM_MAX_SRC] = {0}, W[CMB_RESAMPLE_ACCUM_MAX_SRC] = {0};
  for (int s = 0; s < n_src; ++s) {
    srcs[s].H = H[s] = s == 0 ? Hi : (Hi / 2 > 0 ? Hi / 2 : 1);
    srcs[s].W = W[s] = s == 0 ? Wi : (Wi / 2 > 0 ? Wi / 2 : 1);
    srcs[s].x.resize((size_t)B * H[s] * W[s] * ld);
    for (auto& v : srcs[s].x) v = rnd();
  }
  std::vector<float> base((size_t)B * Ho * Wo * ld), bias(C), out((size_t)B * Ho * Wo * ld, -777.f);
  for (auto& v : base) v = rnd();
  for (auto& v : bias) v = rnd();

  // the kernel's loop, one work item at a time
  const int64_t total = (int64_t)B * Ho * Wo * nv;
  for (int64_t i = 0; i < total; ++i) {
    int64_t b;
    int oy, ox, cv;
    cmb_resample_accum_decode(i, nv, Ho, Wo, b, oy, ox, cv);
    const int64_t cell = (int64_t)oy * Wo + ox;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (has_base)
      for (int e = 0; e < 8; ++e) acc[e] = base[((size_t)b * Ho * Wo + cell) * ld + cv * 8 + e];
    if (has_bias)
      for (int e = 0; e < 8; ++e) acc[e] += bias[cv * 8 + e];
    cmb_resample_accum_cell(oy, ox, Ho, Wo, n_src, H, W,
                            [&](int s, int64_t row, float (&v)[8]) {
                              for (int e = 0; e < 8; ++e) v[e] = srcs[s].x[((size_t)b * H[s] * W[s] + row) * ld + cv * 8 + e];
                            },
                            acc);
    for (int e = 0; e < 8; ++e) out[((size_t)b * Ho * Wo + cell) * ld + cv * 8 + e] = acc[e];
  }

  double max_ref = 0, max_err = 0;
  for (int b = 0; b < B; ++b)
    for (int oy = 0; oy < Ho; ++oy)
      for (int ox = 0; ox < Wo; ++ox) {
        const size_t row = ((size_t)b * Ho * Wo + (size_t)oy * Wo + ox) * ld;
        for (int c = 0; c < ld; ++c) {
          if (c >= C) {
            if (out[row + c] != -777.f) {
              if (++fails <= 20) std::printf("FAIL column %d outside the slice was written\n", c);
            }
            continue;
          }
          double r = (has_base ? (double)base[row + c] : 0.0) + (has_bias ? (double)bias[c] : 0.0);
          for (int s = 0; s < n_src; ++s) r += ref_bilinear(srcs[s], ld, b, c, oy, ox, Ho, Wo);
          max_ref = std::fmax(max_ref, std::fabs(r));
          max_err = std::fmax(max_err, std::fabs((double)out[row + c] - r));
        }
      }
  const double rel = max_err / std::fmax(max_ref, 1e-12);
  if (rel > worst) worst = rel;
  ++cases;
  if (!(rel < 1e-5)) {
    if (++fails <= 20)
      std::printf("FAIL (%d, %d) -> (%d, %d) n_src %d base %d bias %d: rel err %.3g\n", Hi, Wi, Ho, Wo, n_src, (int)has_base,
                  (int)has_bias, rel);
  }
}

int main() {
  const int grids[][4] = {{8, 8, 12, 12}, {4, 4, 12, 12}, {2, 2, 8, 8}, {64, 64, 96, 96}, {32, 32, 96, 96}, {1, 1, 4, 4}, {4, 6, 7, 3}};
  for (const auto& g : grids)
    for (int n_src = 0; n_src <= 2; ++n_src)
      for (int has_base = 0; has_base <= 1; ++has_base)
        for (int has_bias = 0; has_bias <= 1; ++has_bias) {
          if (n_src == 0 && !has_base) continue;
          run_case(g[0], g[1], g[2], g[3], n_src, has_base, has_bias);
        }
  std::printf("cases %d, worst rel err %.3g\n", cases, worst);
  if (fails) {
    std::printf("%d failures\n", fails);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
