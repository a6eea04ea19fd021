// Host-side check of the adjoint bilinear resample's per-axis arithmetic (cambrian_amd/csrc/resample_core.h, the very
// header elementwise.hip includes): for every (n_in, n_out) below and every input i
//   * the candidate window of i contains every output whose lerp_index names i (against a scan of ALL outputs),
//   * what the kernel does with the window (trim to the non-zero weights, sum in ascending order) collects exactly the
//     weights of that scan,
//   * the window is no wider than cmb_resample_window_bound, the trip count the kernel's loops are sized for,
// and every output's weights over all inputs sum to 1 within 2 ulp.
#include <cmath>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../cambrian_amd/csrc/resample_core.h"

static int fails = 0;
#define CHECK(c, ...)                                   \
  do {                                                  \
    if (!(c)) {                                         \
      if (++fails <= 20) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } \
    }                                                   \
  } while (0)

static int widest = 0, widest_in = 0, widest_out = 0;
static int widest_release = 0;

static void check_pair(int n_in, int n_out, bool release) {
  const float scale = (float)n_in / (float)n_out;
  const int bound = cmb_resample_window_bound(n_in, n_out);
  for (int i = 0; i < n_in; ++i) {
    int lo, hi;
    cmb_resample_window(i, n_in, n_out, lo, hi);
    CHECK(0 <= lo && lo <= hi && hi <= n_out - 1, "window [%d, %d] of input %d outside 0..%d (%d -> %d)", lo, hi, i, n_out - 1,
          n_in, n_out);
    const int width = hi - lo + 1;
    CHECK(width <= bound, "window of input %d is %d wide, bound %d (%d -> %d)", i, width, bound, n_in, n_out);
    if (width > widest) widest = width, widest_in = n_in, widest_out = n_out;
    if (release && width > widest_release) widest_release = width;
    // brute force: every output that names i
    int first = -1, last = -1, named = 0;
    for (int o = 0; o < n_out; ++o) {
      int i0, i1;
      float l1;
      lerp_index(o, scale, n_in, i0, i1, l1);
      if (i0 == i || i1 == i) {
        CHECK(lo <= o && o <= hi, "output %d names input %d outside its window [%d, %d] (%d -> %d)", o, i, lo, hi, n_in, n_out);
        CHECK(first < 0 || o == last + 1, "outputs naming input %d are not one run at %d (%d -> %d)", i, o, n_in, n_out);
        if (first < 0) first = o;
        last = o;
        ++named;
      } else {
        CHECK(cmb_resample_weight(o, scale, n_in, i) == 0.f, "output %d does not name input %d but weighs it (%d -> %d)", o, i,
              n_in, n_out);
      }
    }
    // the kernel's trimmed loop against the scan
    int tlo = lo, thi = hi;
    while (tlo <= thi && cmb_resample_weight(tlo, scale, n_in, i) == 0.f) ++tlo;
    while (thi >= tlo && cmb_resample_weight(thi, scale, n_in, i) == 0.f) --thi;
    double in_window = 0, all = 0;
    for (int o = tlo; o <= thi; ++o) in_window += cmb_resample_weight(o, scale, n_in, i);
    for (int o = 0; o < n_out; ++o) all += cmb_resample_weight(o, scale, n_in, i);
    CHECK(in_window == all, "input %d: trimmed window collects %.9g of %.9g (%d -> %d)", i, in_window, all, n_in, n_out);
    CHECK(tlo > thi || (named > 0 && tlo >= first && thi <= last), "input %d: trimmed window leaves the run (%d -> %d)", i, n_in, n_out);
  }
  for (int o = 0; o < n_out; ++o) {
    float sum = 0.f;
    for (int i = 0; i < n_in; ++i) sum += cmb_resample_weight(o, scale, n_in, i);
    CHECK(std::fabs(sum - 1.f) <= 2.f * 1.1920929e-7f, "output %d: weights sum to %.9g (%d -> %d)", o, sum, n_in, n_out);
  }
}

int main() {
  int pairs = 0;
  for (int n_in = 1; n_in <= 48; ++n_in)
    for (int n_out = 1; n_out <= 48; ++n_out) check_pair(n_in, n_out, false), ++pairs;
  const std::pair<int, int> release[] = {{256, 96}, {128, 96}, {64, 96}, {32, 96}, {27, 24}, {37, 27}};
  for (const auto& p : release) check_pair(p.first, p.second, true), ++pairs;
  std::printf("pairs %d, widest window %d (%d -> %d), widest at the release pairs %d\n", pairs, widest, widest_in, widest_out,
              widest_release);
  if (fails) {
    std::printf("%d failures\n", fails);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
