// Host-side run of the optimizer kernels' arithmetic: cambrian_amd/csrc/optim_core.h, the very header optim.hip includes,
// compiled with g++ (tests/test_optim_sim.py).  Checks
//   1. cmb_bf16_rne against an independent compare-based round-to-nearest-even on sign-magnitude integers, for all 65536
//      upper halves x 8 lower halves (below / at / above the tie, carries into the exponent and into infinity, NaN stays NaN),
//      and cmb_bf16_widen as its exact inverse;
//   2. the chunk sum of squares (the kernel's loop structure over the core functions) against a long double sum;
//   3. cmb_adamw_update over 10 steps against a double AdamW, next to a plain float restatement of the same formulas;
//   4. cmb_optim_clip_coef against the double expression, and its exact 1 below the threshold.
// Prints one line per part and "OK"; exit status 1 on any failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>

#include "../../cambrian_amd/csrc/optim_core.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double urand() {   // xorshift64*, uniform in [0, 1)
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (double)((rng_state * 0x2545f4914f6cdd1dull) >> 11) / 9007199254740992.0;
}
static float nrand() {   // roughly normal: sum of 4 uniforms, centred
  return (float)((urand() + urand() + urand() + urand() - 2.0) * 1.7320508);
}

static int failures = 0;
#define EXPECT(cond, ...)            \
  do {                               \
    if (!(cond)) {                   \
      if (failures < 20) {           \
        printf("FAIL: " __VA_ARGS__); \
        printf("\n");                \
      }                              \
      ++failures;                    \
    }                                \
  } while (0)

// ---- 1. bf16 ----------------------------------------------------------------------------------------------------------------
static bool is_nan_bits16(uint16_t h) { return (h & 0x7f80) == 0x7f80 && (h & 0x7f) != 0; }

static uint16_t ref_rne(uint32_t u) {   // finite or infinite input only
  const uint16_t up = (uint16_t)(u >> 16);
  const uint32_t lo = u & 0xffffu;
  if (lo < 0x8000u) return up;
  if (lo > 0x8000u) return (uint16_t)(up + 1);   // next magnitude: the mantissa carry moves into the exponent by itself
  return (up & 1) ? (uint16_t)(up + 1) : up;
}

static long check_bf16() {
  static const uint32_t lowers[8] = {0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff, 0x4000, 0xc000};
  long n = 0;
  for (uint32_t up = 0; up < 65536; ++up) {
    for (uint32_t lo : lowers) {
      const uint32_t u = (up << 16) | lo;
      const uint16_t got = cmb_bf16_rne(cmb_bits_f32(u));
      const bool in_nan = (u & 0x7fffffffu) > 0x7f800000u;
      if (in_nan) {
        EXPECT(is_nan_bits16(got), "bf16(NaN %08x) = %04x is not a NaN", u, got);
      } else {
        const uint16_t want = ref_rne(u);
        EXPECT(got == want, "bf16(%08x) = %04x, want %04x", u, got, want);
        EXPECT(!is_nan_bits16(got), "bf16(%08x) = %04x became a NaN", u, got);
      }
      ++n;
    }
    const float w = cmb_bf16_widen((uint16_t)up);
    EXPECT(cmb_f32_bits(w) == (up << 16), "widen(%04x)", up);
    if (!is_nan_bits16((uint16_t)up)) EXPECT(cmb_bf16_rne(w) == (uint16_t)up, "rne(widen(%04x))", up);
  }
  return n;
}

// ---- 2. chunk sums ----------------------------------------------------------------------------------------------------------
// grad_sqnorm_kernel's body for one chunk, thread by thread
static float chunk_partial(const float* g, int n_left) {
  static float red[CMB_OPTIM_THREADS];
  for (int tid = 0; tid < CMB_OPTIM_THREADS; ++tid) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int base = tid * 8; base < n_left; base += CMB_OPTIM_ROUND)
      for (int e = 0; e < 8; ++e) cmb_optim_sq_accum(acc[e], base + e < n_left ? g[base + e] : 0.f);
    red[tid] = cmb_optim_sum8(acc);
  }
  for (int o = CMB_OPTIM_THREADS / 2; o > 0; o >>= 1)
    for (int lane = 0; lane < CMB_OPTIM_THREADS; ++lane) cmb_optim_tree_lane(red, lane, o);
  return red[0];
}

static float sqnorm(const std::vector<float>& g) {
  const int64_t n = (int64_t)g.size(), chunks = cmb_optim_chunks_of(n);
  double s = 0.0;
  for (int64_t c = 0; c < chunks; ++c) {
    const int64_t off = c * CMB_OPTIM_CHUNK, rest = n - off;
    s = cmb_optim_final_add(s, chunk_partial(g.data() + off, rest < CMB_OPTIM_CHUNK ? (int)rest : CMB_OPTIM_CHUNK));
  }
  return (float)s;
}

static double check_sums(int& cases) {
  const int64_t sizes[7] = {1, 7, 8, 9, CMB_OPTIM_CHUNK - 1, CMB_OPTIM_CHUNK, CMB_OPTIM_CHUNK + 1};
  double worst = 0.0;
  cases = 0;
  for (int64_t n : sizes) {
    for (int kind = 0; kind < 2; ++kind) {
      std::vector<float> g((size_t)n);
      for (auto& x : g) x = kind == 0 ? nrand() * 3.0f : 0.3f;
      long double ref = 0.0L;
      for (float x : g) ref += (long double)x * (long double)x;
      const double rel = std::fabs((double)((long double)sqnorm(g) - ref) / (double)ref);
      EXPECT(rel <= 1e-5, "chunk sum n=%lld kind=%d: rel err %.3g", (long long)n, kind, rel);
      if (rel > worst) worst = rel;
      ++cases;
    }
  }
  EXPECT(cmb_optim_chunks_of(0) == 0 && cmb_optim_chunks_of(1) == 1 && cmb_optim_chunks_of(CMB_OPTIM_CHUNK) == 1 &&
             cmb_optim_chunks_of(CMB_OPTIM_CHUNK + 1) == 2,
         "cmb_optim_chunks_of");
  EXPECT((CMB_OPTIM_CHUNK & (CMB_OPTIM_CHUNK - 1)) == 0 && CMB_OPTIM_CHUNK <= 65536 && CMB_OPTIM_CHUNK % CMB_OPTIM_ROUND == 0,
         "CMB_OPTIM_CHUNK");
  return worst;
}

// ---- 3. the update ------------------------------------------------------------------------------------------------------------
static float ulp_of(float x) {
  const float a = std::fabs(x);
  return std::nextafterf(a, INFINITY) - a;
}

static void check_update(float wd, double& err_core, double& err_float, float& ulp) {
  const int N = 4096, STEPS = 10;
  const float lr = 1e-2f, b1 = 0.9f, b2 = 0.999f, eps = 1e-8f;
  std::vector<float> p(N), m(N, 0.f), v(N, 0.f), pf(N), mf(N, 0.f), vf(N, 0.f);
  std::vector<double> pd(N), md(N, 0.0), vd(N, 0.0);
  for (int i = 0; i < N; ++i) pd[i] = pf[i] = p[i] = nrand();
  const float scales[3] = {100.f, 1.f, 0.01f};
  for (int t = 1; t <= STEPS; ++t) {
    const double bc1d = 1.0 - std::pow((double)b1, t), bc2d = 1.0 - std::pow((double)b2, t);
    const float bc1 = (float)bc1d, bc2 = (float)bc2d;
    const cmb_adamw_consts k = cmb_adamw_make(lr, b1, b2, eps, wd, bc1, bc2);
    for (int i = 0; i < N; ++i) {
      const float g = nrand() * scales[t % 3];
      cmb_adamw_update(g, p[i], m[i], v[i], k);
      // plain float restatement of the same formulas
      pf[i] *= 1.0f - lr * wd;
      mf[i] = b1 * mf[i] + (1.0f - b1) * g;
      vf[i] = b2 * vf[i] + (1.0f - b2) * g * g;
      pf[i] -= (lr / bc1) * mf[i] / (std::sqrt(vf[i]) / std::sqrt(bc2) + eps);
      // double, from the same fp32 hyper-parameters
      const double gd = g;
      pd[i] *= 1.0 - (double)lr * (double)wd;
      md[i] = (double)b1 * md[i] + (1.0 - (double)b1) * gd;
      vd[i] = (double)b2 * vd[i] + (1.0 - (double)b2) * gd * gd;
      pd[i] -= ((double)lr / bc1d) * md[i] / (std::sqrt(vd[i]) / std::sqrt(bc2d) + (double)eps);
    }
  }
  err_core = err_float = 0.0;
  float pmax = 0.f;
  for (int i = 0; i < N; ++i) {
    err_core = std::fmax(err_core, std::fabs((double)p[i] - pd[i]));
    err_float = std::fmax(err_float, std::fabs((double)pf[i] - pd[i]));
    pmax = std::fmax(pmax, std::fabs((float)pd[i]));
  }
  ulp = ulp_of(pmax);
  EXPECT(err_core <= 2.0 * err_float + ulp, "update wd=%g: err_core %.3g > 2 * err_float %.3g + ulp %.3g", wd, err_core,
         err_float, ulp);
  EXPECT(err_core < 1e-4, "update wd=%g: err_core %.3g is not small", wd, err_core);
}

// ---- 4. the clip coefficient ------------------------------------------------------------------------------------------------------
static void check_clip() {
  const float sumsqs[5] = {1e-8f, 0.25f, 1.0f, 400.f, 1e12f};
  const float scales[2] = {1.0f, 0.125f};
  for (float ss : sumsqs)
    for (float gs : scales) {
      const float c = cmb_optim_clip_coef(ss, gs, 1.0f);
      const double want = std::fmin(1.0, 1.0 / ((double)gs * std::sqrt((double)ss) + 1e-6));
      EXPECT(std::fabs(c - want) <= 1e-6 * want, "clip coef(%g, %g) = %.9g, want %.9g", ss, gs, c, want);
      if (want == 1.0) EXPECT(c == 1.0f, "clip coef below the threshold is not exactly 1");
    }
  EXPECT(cmb_optim_clip_coef(1.0f, 1.0f, 1e30f) == 1.0f, "a huge threshold must give exactly 1");
  EXPECT(cmb_optim_clip_coef(NAN, 1.0f, 1.0f) == 1.0f, "NaN norm: the comparison fails, coefficient 1");
  EXPECT(cmb_optim_clip_coef(INFINITY, 1.0f, 1.0f) == 0.0f, "infinite norm: coefficient 0");
}

int main() {
  const long nb = check_bf16();
  printf("bf16 patterns %ld\n", nb);
  int cases = 0;
  const double worst = check_sums(cases);
  printf("sum cases %d, worst rel err %.3g\n", cases, worst);
  for (float wd : {0.0f, 0.1f}) {
    double ec, ef;
    float ulp;
    check_update(wd, ec, ef, ulp);
    printf("update wd %g: err_core %.3g err_float %.3g ulp %.3g\n", wd, ec, ef, ulp);
  }
  check_clip();
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("OK\n");
  return 0;
}
