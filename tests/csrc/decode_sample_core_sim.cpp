// CPU run of cambrian_amd/csrc/decode_sample_core.h, the very header decode_sample.hip includes (tests/test_decode_sample_core_sim.py
// builds this with g++ under AddressSanitizer and UBSan): the Philox4x32-10 known answers, the uniform and the Gumbel noise at
// the ends of the word range and against fp64 over a sweep, the key map's order and its inverse, the fixed-point mass.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../cambrian_amd/csrc/decode_sample_core.h"

static int fails = 0;
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      ++fails;                                         \
      std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); \
      std::printf(__VA_ARGS__);                        \
      std::printf("\n");                               \
    }                                                  \
  } while (0)

static void philox_known_answers() {
  struct Kat { uint32_t c[4], k[2], want[4]; };
  const Kat kats[] = {
      {{0, 0, 0, 0}, {0, 0}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}},
      {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu},
       {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}},
      {{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u},
       {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}}};
  for (const Kat& t : kats) {
    const cmb_philox4 got = cmb_ds_philox(t.c[0], t.c[1], t.c[2], t.c[3], t.k[0], t.k[1]);
    for (int j = 0; j < 4; ++j) CHECK(got.w[j] == t.want[j], "word %d: %08x, want %08x", j, got.w[j], t.want[j]);
  }
  // the layout of a draw: counter (group, row, step, 0), key (seed low, seed high)
  const uint64_t seed = 0x299f31d0a4093822ull;
  const cmb_philox4 a = cmb_ds_words(seed, 0x243f6a88u, 0x85a308d3u, 0x13198a2eu);
  const cmb_philox4 b = cmb_ds_philox(0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0u, 0xa4093822u, 0x299f31d0u);
  CHECK(std::memcmp(&a, &b, sizeof a) == 0, "cmb_ds_words is not Philox over (group, row, step, 0)");
}

static void uniform_and_gumbel() {
  for (uint32_t word : {0u, 0xFFu, 0x100u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFF00u, 0xFFFFFFFFu}) {
    const double u = cmb_ds_u(word);
    CHECK(u > 0.0 && u < 1.0, "u(%08x) = %.17g", word, u);
    const float t = cmb_ds_neg_log_u(word), g = cmb_ds_gumbel(word);
    CHECK(t > 0.f && std::isfinite(t), "-log u(%08x) = %g", word, t);
    CHECK(std::isfinite(g) && std::fabs(g) <= 64.f, "g(%08x) = %g", word, g);
  }
  CHECK(cmb_ds_gumbel(0xFFFFFFFFu) <= CMB_DS_GUMBEL_MAX && cmb_ds_gumbel(0xFFFFFFFFu) > CMB_DS_GUMBEL_MAX - 0.01f, "the largest noise");
  CHECK(cmb_ds_u(0) == std::ldexp(1.0, -25) && cmb_ds_u(0xFFFFFFFFu) == 1.0 - std::ldexp(1.0, -25), "ends of u");
  // against fp64 over a sweep of words (both halves, the seam at n = 2^23 included): a few fp32 roundings
  double worst_t = 0, worst_g = 0;
  uint32_t word = 0;
  for (int i = 0; i < 200000; ++i, word += 21503u * 256u + 77u) {
    for (uint32_t w : {word, 0x7FFFFF00u + (uint32_t)(i & 511), 0x80000000u - (uint32_t)(i & 511)}) {
      const double u = cmb_ds_u(w), t = -std::log(u), g = -std::log(t);
      worst_t = std::fmax(worst_t, std::fabs((double)cmb_ds_neg_log_u(w) - t) / t);
      worst_g = std::fmax(worst_g, std::fabs((double)cmb_ds_gumbel(w) - g));
    }
  }
  // the cheap bound is one: never below the accurate noise, and (where it answers at all) less than twice its slack above
  word = 0;
  double over = 0;
  int asked = 0;
  for (int i = 0; i < 400000; ++i, word += 10739u * 256u + 3u) {
    for (uint32_t w : {word, 0x7FFFFF00u + (uint32_t)(i & 511), 0x80000000u - (uint32_t)(i & 511), 0xFFFFFFFFu - (uint32_t)i * 256u}) {
      const float hi = cmb_ds_gumbel_bound(w), g = cmb_ds_gumbel(w);
      CHECK(hi >= g, "bound(%08x) = %g below g = %g", w, hi, g);
      if (std::isinf(hi)) { ++asked; CHECK(cmb_ds_u(w) > 0.98, "no answer at u = %g", cmb_ds_u(w)); }
      else over = std::fmax(over, (double)hi - g);
    }
  }
  CHECK(over <= 2 * CMB_DS_GUMBEL_SLACK && asked > 0, "bound: %g above, %d unanswered", over, asked);
  CHECK(worst_t <= 4 * 5.97e-8, "-log u: relative error %g", worst_t);
  CHECK(worst_g <= 4e-6, "g: absolute error %g", worst_g);       // |g| <= 17.4: an ulp is at most 1.9e-6
}

static void key_map() {
  const float inf = std::numeric_limits<float>::infinity(), dmin = std::numeric_limits<float>::denorm_min();
  std::vector<float> v = {-inf, -3.4028234e38f, -64.f, -1.f, -1.17549435e-38f, -2 * dmin, -dmin};
  const size_t zeros = v.size();
  v.insert(v.end(), {-0.f, 0.f});
  v.insert(v.end(), {dmin, 2 * dmin, 1.17549435e-38f, 0.25f, 1.f, 1.0000001f, 64.f, 3.4028234e38f, inf});
  for (size_t i = 0; i + 1 < v.size(); ++i) {
    const uint32_t a = cmb_ds_key32(v[i]), b = cmb_ds_key32(v[i + 1]);
    if (i == zeros) CHECK(a == b, "-0 and +0 are one key");
    else CHECK(a < b, "key(%g) = %08x !< key(%g) = %08x", v[i], a, v[i + 1], b);
  }
  CHECK(cmb_ds_key32(-inf) == 0x007FFFFFu && cmb_ds_key32(inf) == 0xFF800000u, "keys of the infinities");
  CHECK(cmb_ds_key32(std::nanf("")) == 0xFFFFFFFFu && cmb_ds_key32(-std::nanf("")) == 0xFFFFFFFFu, "a NaN is the largest key");
  // a dense sweep over bit patterns: the order of the keys is the order of the floats, and the inverse gives the float back
  uint32_t bits = 0;
  for (int i = 0; i < 400000; ++i, bits += 10739u) {
    const float a = cmb_ds_float(bits), b = cmb_ds_float(bits + 1u + (uint32_t)(i % 977) * 4099u);
    if (a != a || b != b) continue;
    const uint32_t ka = cmb_ds_key32(a), kb = cmb_ds_key32(b);
    CHECK((a < b) == (ka < kb) && (a == b) == (ka == kb), "order of %g and %g", a, b);
    CHECK(cmb_ds_key32_value(ka) == a, "inverse of key(%g)", a);
  }
}

static void fixed_point_mass() {
  CHECK(cmb_ds_mass(3.5f, 3.5f) == (1ull << 40), "the maximum weighs 2^40");
  CHECK(cmb_ds_mass(-std::numeric_limits<float>::infinity(), 0.f) == 0, "-inf weighs nothing");
  CHECK(cmb_ds_mass(-64.f, 64.f) == 0, "a weight below 2^-40 counts as nothing");
  uint64_t sum = 0;
  for (int i = 0; i < (1 << 17); ++i) sum += cmb_ds_mass(1.f, 1.f);
  CHECK(sum == (1ull << 57), "2^17 ones: %llu", (unsigned long long)sum);
  // the nucleus target: the maximum is always kept, top_p = 1 drops nothing
  const uint64_t Z = 5 * (1ull << 40) + 12345;
  CHECK(cmb_ds_nucleus_target(1.f, Z) == 0, "top_p = 1");
  CHECK(cmb_ds_nucleus_target(1e-45f, Z) == Z - 1, "top_p next to 0");
  CHECK(cmb_ds_nucleus_target(0.5f, 1ull << 41) == (1ull << 40), "top_p = 1/2");
}

int main() {
  philox_known_answers();
  uniform_and_gumbel();
  key_map();
  fixed_point_mass();
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
