// CPU check of the GEMM dispatch decisions (cambrian_amd/csrc/gemm_plan.h, the very header gemm.hip includes), compiled with
// g++ by tests/test_gemm_plan_sim.py.
//   gemm_plan_sim                 the assertions below on a 256-CU device, then "OK"
//   gemm_plan_sim replay <n_cu>   one problem per line of stdin (the `plan` lines of tests/golden/gemm_dispatch_parent.json:
//                                 "gemm k=v ...", "tn k=v ...", "pair k=v ... | k=v ...") -> "kernel tail_rows pair" per line,
//                                 as cmb_gemm_last_kernel / cmb_gemm_tail_rows(M, N) / cmb_gemm_pair_last would report them
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include "../../cambrian_amd/csrc/gemm_plan.h"

using namespace cmb_gemm_detail;

namespace {

float g_dummy[4];   // stands for every non-null pointer: the plan only asks whether an operand is there

struct Problem {
  cmb_gemm_desc d;
  GemmParams p;
  int es = 2, split_k = 1, hint = 0;
  GemmPolicy policy;
};

// keys: M N K es split_k hint act bias colscale residual pre_out ln out_f32 beta batch c_bs ldb ldc a_n1 a_n2 a_s0 a_s1 a_s2
// pol=M,N,K,act,kernel; everything not named is 0 / a plain row-major operand
Problem parse(const std::string& text) {
  std::map<std::string, std::string> kv;
  std::istringstream in(text);
  for (std::string tok; in >> tok;) {
    const size_t eq = tok.find('=');
    if (eq != std::string::npos) kv[tok.substr(0, eq)] = tok.substr(eq + 1);
  }
  auto num = [&](const char* k, long long dflt) { return kv.count(k) ? atoll(kv[k].c_str()) : dflt; };
  Problem pr;
  cmb_gemm_desc& d = pr.d;
  memset(&d, 0, sizeof d);
  d.M = num("M", 0); d.N = num("N", 0); d.K = num("K", 0);
  pr.es = (int)num("es", 2);
  d.dtype = pr.es == 4 ? (int)CMB_F32 : pr.es == 1 ? (int)CMB_FP8_E4M3 : (int)CMB_BF16;
  d.out_dtype = (pr.es == 4 || num("out_f32", 0)) ? CMB_F32 : CMB_BF16;
  d.A = d.B = g_dummy; d.C = g_dummy;
  d.a_map.n1 = num("a_n1", 0); d.a_map.n2 = num("a_n2", 0);
  d.a_map.s0 = num("a_s0", 0); d.a_map.s1 = num("a_s1", 0); d.a_map.s2 = num("a_s2", d.K);
  d.ldb = num("ldb", d.K);
  d.c_map.s2 = num("ldc", d.N);
  if (num("bias", 0) || num("ln", 0)) d.bias = g_dummy;
  if (num("colscale", 0)) d.colscale = g_dummy;
  if (num("residual", 0)) d.residual = g_dummy, d.r_map.s2 = d.N;
  if (num("pre_out", 0)) d.pre_out = g_dummy, d.p_map.s2 = d.N;
  if (num("ln", 0)) d.row_mean = d.row_rstd = d.col_sum = g_dummy;
  d.act = (int)num("act", 0);
  d.alpha = 1.0f; d.beta = (float)num("beta", 0);
  d.split_k = pr.split_k = (int)num("split_k", 1);
  d.tile_hint = pr.hint = (int)num("hint", 0);
  d.batch = (int)num("batch", 1);
  d.c_batch_stride = num("c_bs", 0);
  gemm_fill_params(&d, pr.p);
  if (pr.es == 1) pr.p.a_scale = pr.p.b_scale = g_dummy;
  if (kv.count("pol")) {
    long long v[5];
    if (sscanf(kv["pol"].c_str(), "%lld,%lld,%lld,%lld,%lld", v, v + 1, v + 2, v + 3, v + 4) == 5) pr.policy.set(v[0], v[1], v[2], (int)v[3], (int)v[4]);
  }
  return pr;
}

GemmPlan plan_of(const std::string& text, int n_cu = 256, const GemmEnv& env = GemmEnv()) {
  const Problem pr = parse(text);
  return gemm_plan(pr.p, pr.es, pr.split_k, pr.hint, env, pr.policy, n_cu);
}

PairPlan pair_of(const std::string& a, const std::string& b, int n_cu = 256) {
  const Problem p0 = parse(a), p1 = parse(b);
  if (!gemm_pair_desc_ok(&p0.d) || !gemm_pair_desc_ok(&p1.d)) return PairPlan{false, 0};
  return gemm_pair_plan(p0.p, p1.p, GemmEnv(), n_cu);
}

int g_failed = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++g_failed; } \
  } while (0)

int self_test() {
  // tests/test_gemm256_gpu.py::test_default_dispatch_reports_its_kernel
  const struct { const char* s; int want; } dflt[] = {
      {"M=32768 N=2048 K=512", 2590}, {"M=32768 N=1152 K=512", 2590}, {"M=32768 N=1160 K=512", 256}, {"M=32768 N=2048 K=64", 256},
      {"M=8192 N=2048 K=512", 2590},  {"M=1536 N=2048 K=512", 128},   {"M=64 N=64 K=64", 128}};
  for (const auto& c : dflt) CHECK(plan_of(c.s).kernel == c.want);

  // tests/test_gemm_policy.py::test_tail_split_rule
  const long tails[][3] = {{11680, 1536, 10752}, {11664, 4352, 11520}, {11680, 4608, 10752}, {9232, 4096, 8192}, {9216, 4096, 8192},
                           {65536, 6144, 0},     {147456, 2048, 0},    {11680, 8192, 0},     {9232, 1024, 0},    {9216, 1024, 0},
                           {11664, 1152, 0}};
  for (const auto& t : tails) CHECK(tail_split_rows_mn(t[0], t[1], GemmEnv(), 256) == t[2]);
  {
    const GemmPlan pl = plan_of("M=11680 N=1536 K=128");   // the plan carries the same cut, the head on the 4-wave kernel
    CHECK(pl.head_rows == 10752 && pl.kernel == 2590 && pl.splits == 1);
    CHECK(plan_of("M=11680 N=1536 K=128 hint=256").head_rows == 0);            // a tile_hint, split-K or the knob switch it off
    CHECK(plan_of("M=11680 N=1536 K=4096 split_k=2").head_rows == 0);
    GemmEnv off;
    off.tail_split = false;
    CHECK(plan_of("M=11680 N=1536 K=128", 256, off).head_rows == 0);
    // a row map whose outer period divides the cut (16384 rows) splits, one that does not is launched whole
    CHECK(plan_of("M=16896 N=4096 K=256 a_n1=4096 a_n2=4096 a_s0=1050368 a_s2=256").head_rows == 16384);
    CHECK(plan_of("M=16896 N=4096 K=256 a_n1=4224 a_n2=4224 a_s0=1083136 a_s2=256").head_rows == 0);
  }

  // a policy entry redirects the default choice; a tile_hint overrides the policy; split-K launches do not consult it
  CHECK(plan_of("M=8192 N=2048 K=512").kernel == 2590);
  CHECK(plan_of("M=8192 N=2048 K=512 pol=8192,2048,512,0,2560").kernel == 256);
  CHECK(plan_of("M=8192 N=2048 K=512 pol=8192,2048,512,0,128").kernel == 128);
  CHECK(plan_of("M=8192 N=2048 K=512 act=1 pol=8192,2048,512,0,2560").kernel == 2590);   // another activation: another problem
  CHECK(plan_of("M=8192 N=2048 K=512 hint=2590 pol=8192,2048,512,0,2560").kernel == 2590);
  CHECK(plan_of("M=8192 N=2048 K=512 hint=128 pol=8192,2048,512,0,2560").kernel == 128);
  CHECK(plan_of("M=8192 N=2048 K=512 split_k=2 pol=8192,2048,512,0,128").kernel == 2590);
  {
    const GemmPlan pl = plan_of("M=1000 N=512 K=256 hint=2561");
    CHECK(pl.kernel == 256 && pl.sched == 1);
    CHECK(plan_of("M=1000 N=512 K=256 hint=2560").sched == 0);
    GemmPolicy pol;
    CHECK(pol.set(1, 2, 3, 0, 777) != CMB_OK && pol.set(1, 2, 3, 0, 2590) == CMB_OK && pol.lookup(1, 2, 3, 0) == 2590);
    CHECK(pol.set(1, 2, 3, 0, 0) == CMB_OK && pol.n == 0 && pol.lookup(1, 2, 3, 0) == 0);
  }

  // split-K clamping: never more slices than K-steps, and slices too short for the 4-wave kernel's two-tile look-ahead
  {
    const GemmPlan a = plan_of("M=1024 N=1024 K=128 split_k=8 hint=2590");
    CHECK(a.splits == 2 && a.k_per_split == 64 && a.kernel != 2590);
    const GemmPlan b = plan_of("M=1024 N=1024 K=4096 split_k=8 hint=2590");
    CHECK(b.splits == 8 && b.k_per_split == 512 && b.kernel == 2590);
    const SplitK one = splitk_geometry(64, 64, 8), odd = splitk_geometry(9 * 64, 64, 4), tn = splitk_geometry(1000, 64, 4);
    CHECK(one.splits == 1 && one.k_per_split == 64);
    CHECK(odd.splits == 3 && odd.k_per_split == 192);
    CHECK(tn.splits == 4 && tn.k_per_split == 256);
    CHECK(splitk_geometry(0, 64, 4).splits == 1);
  }

  // the special kernels
  CHECK(plan_of("M=16 N=1024 K=1024").kernel == 32);
  CHECK(plan_of("M=16 N=1024 K=1024 bias=1").kernel == 128);
  CHECK(plan_of("M=16 N=1024 K=1024 hint=128").kernel == 128);
  CHECK(plan_of("M=300 N=1024 K=64 batch=16 c_bs=307200").kernel == 64);
  CHECK(plan_of("M=300 N=1024 K=128 batch=16 c_bs=307200").kernel == 128);
  CHECK(plan_of("M=300 N=1024 K=64 batch=16 c_bs=307200 residual=1").kernel == 128);
  {
    GemmEnv off;
    off.k64 = false;
    CHECK(plan_of("M=300 N=1024 K=64 batch=16 c_bs=307200", 256, off).kernel == 128);
  }
  CHECK(plan_of("M=32768 N=2048 K=512 es=4").kernel == 128 && plan_of("M=32768 N=2048 K=512 es=1").kernel == 128);

  // pair legality (DINOv2 beside SigLIP at 24 images) and what refuses it
  const char* d2 = "M=17520 N=1536 K=1536";
  const char* sl = "M=17496 N=1152 K=1152";
  {
    const PairPlan pp = pair_of(d2, sl);
    CHECK(pp.pair && pp.g0 >= 8 && pp.g0 <= 248);
    const Problem a = parse(d2), b = parse(sl);
    CHECK(gemm_pair_side_ok(a.p) && gemm_pair_side_ok(b.p) && gemm_p5_pair_gain(a.p, b.p, 256, pp.g0) >= 0.04);
    CHECK(pp.g0 == p5_pair_split(p5_items(a.p), 1536, p5_items(b.p), 1152, 256));
  }
  CHECK(pair_of("M=17520 N=1536 K=1536 act=1", "M=17496 N=1152 K=1152 act=1").pair);     // erf-GELU on both sides
  CHECK(!pair_of("M=17520 N=1536 K=1536 pre_out=1", sl).pair);                            // a pre-activation copy
  CHECK(!pair_of("M=17520 N=1536 K=1536 act=1", sl).pair);                                // mismatched activations
  CHECK(!pair_of("M=17520 N=1536 K=1536 act=4", "M=17496 N=1152 K=1152 act=4").pair);     // SiLU: no pair instantiation
  CHECK(!pair_of("M=65536 N=2048 K=256", "M=65536 N=2048 K=256").pair);                   // whole rounds already: no gain
  CHECK(!pair_of("M=300 N=264 K=320", "M=257 N=8 K=64").pair);                            // not on the persistent kernel at all
  CHECK(!pair_of("M=17520 N=1536 K=1536 out_f32=1", sl).pair);
  CHECK(!pair_of("M=17520 N=1536 K=1536 hint=2590", sl).pair && !pair_of(d2, "M=17496 N=1152 K=1152 split_k=2").pair);
  return g_failed;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "replay")) {
    const int n_cu = atoi(argv[2]);
    for (std::string line; std::getline(std::cin, line);) {
      const size_t sp = line.find(' ');
      const std::string kind = line.substr(0, sp), rest = sp == std::string::npos ? "" : line.substr(sp + 1);
      const size_t bar = rest.find('|');
      const Problem first = parse(rest.substr(0, bar));
      int kernel = kGemmTN, pair = 0;
      if (kind == "gemm") {
        kernel = gemm_plan(first.p, first.es, first.split_k, first.hint, GemmEnv(), first.policy, n_cu).kernel;
      } else if (kind == "pair") {
        pair = pair_of(rest.substr(0, bar), rest.substr(bar + 1), n_cu).pair;
        kernel = pair ? kGemmP5 : plan_of(rest.substr(bar + 1), n_cu).kernel;   // else the second of the two cmb_gemm calls
      }
      printf("%d %d %d\n", kernel, tail_split_rows_mn(first.p.M, first.p.N, GemmEnv(), n_cu), pair);
    }
    return 0;
  }
  if (self_test()) return 1;
  printf("OK\n");
  return 0;
}
