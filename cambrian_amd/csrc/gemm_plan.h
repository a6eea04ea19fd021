// gemm_plan.h — everything cmb_gemm / cmb_gemm_pair / cmb_gemm_tn DECIDE on the host before a launch, and nothing that
// launches: the environment knobs, the per-shape policy table, the cost models, the eligibility predicates of the special
// kernels, the tail split, split-K geometry and the pair arithmetic.  gemm_plan() and gemm_pair_plan() are the two entry
// points; gemm.hip switches on their answers.
// No HIP include: tests/csrc/gemm_plan_sim.cpp compiles this very file with g++ and checks the decisions on the CPU.
#pragma once
#include <stdlib.h>
#include "gemm_params.h"

namespace cmb_gemm_detail {

// cmb_gemm_last_kernel() ids
constexpr int kGemm128 = 128, kGemm256 = 256, kGemmP5 = 2590, kGemmK64 = 64, kGemmSmallM = 32, kGemmTN = 1281;

// ---- environment knobs (A/B runs and tests), read once per process ---------------------------------------------------------
struct GemmEnv {
  int tile = 0;            // CMB_GEMM_TILE=128|256|...: a tile_hint for every launch that gives none
  bool tail_split = true;  // CMB_GEMM_NO_TAIL_SPLIT=1 disables the tail split
  bool pair = true;        // CMB_GEMM_PAIR=0: cmb_gemm_pair always makes its two calls
  bool k64 = true;         // CMB_GEMM_K64=0: batched K = 64 problems stay on the 128 x 128 tile kernel
  static GemmEnv from_environment() {
    GemmEnv v;
    const char* e;
    if ((e = getenv("CMB_GEMM_TILE"))) v.tile = atoi(e);
    if ((e = getenv("CMB_GEMM_NO_TAIL_SPLIT"))) v.tail_split = atoi(e) == 0;
    if ((e = getenv("CMB_GEMM_PAIR"))) v.pair = atoi(e) != 0;
    if ((e = getenv("CMB_GEMM_K64"))) v.k64 = atoi(e) != 0;
    return v;
  }
};

// ---- per-shape dispatch policy (cmb_gemm_policy_set) -----------------------------------------------------------------------
// Which bf16 kernel a (M, N, K, act) problem takes when the caller gives no tile_hint.  Filled by the host's start-up
// calibration (cambrian_amd/ops.py::calibrate_gemm_dispatch times the candidates on THIS device — the 4-wave kernel's lead over
// the 8-wave one varies from box to box) and read by every launch: a handful of entries, linear scan.  Written only between
// steps (no launches in flight on other threads); the kernels it selects between are bit-identical in their results
// (tests/test_gemm256_gpu.py).
struct GemmPolicy {
  struct Entry { int64_t M, N, K; int act, kernel; };
  static constexpr int kMax = 64;
  Entry e[kMax];
  int n = 0;
  int find(int64_t M, int64_t N, int64_t K, int act) const {
    for (int i = 0; i < n; ++i)
      if (e[i].M == M && e[i].N == N && e[i].K == K && e[i].act == act) return i;
    return -1;
  }
  int lookup(int64_t M, int64_t N, int64_t K, int act) const {
    const int i = find(M, N, K, act);
    return i < 0 ? 0 : e[i].kernel;
  }
  int set(int64_t M, int64_t N, int64_t K, int act, int kernel) {   // kernel 0 removes the entry
    if (kernel != 0 && kernel != 128 && kernel != 2560 && kernel != 2590) return CMB_ERR_BAD_ARG;
    const int i = find(M, N, K, act);
    if (i >= 0) {
      if (kernel) e[i].kernel = kernel;
      else e[i] = e[--n];
      return CMB_OK;
    }
    if (!kernel) return CMB_OK;
    if (n == kMax) return CMB_ERR_WORKSPACE;
    e[n++] = Entry{M, N, K, act, kernel};
    return CMB_OK;
  }
};

// ---- split-K geometry (cmb_gemm: K a multiple of the K-step; cmb_gemm_tn: any K, 64-row steps) -----------------------------
// `want` slices over ceil(K / kstep) steps: never more slices than steps, equal whole steps per slice, and the slices
// recounted (7 steps on 4 slices = 2 per slice = 4 slices; 9 on 4 = 3 per slice = 3 slices).  One slice = the whole K.
struct SplitK { int splits, k_per_split; };
inline SplitK splitk_geometry(int K, int kstep, int want) {
  const int ksteps = (K + kstep - 1) / kstep;
  if (want <= 1 || ksteps <= 1) return SplitK{1, K};
  int splits = want < ksteps ? want : ksteps;
  const int per = (ksteps + splits - 1) / splits;
  splits = (ksteps + per - 1) / per;
  return splits > 1 ? SplitK{splits, per * kstep} : SplitK{1, K};
}

// ---- tile configuration of a bf16 problem ----------------------------------------------------------------------------------
// Cost unit = one "round" of the 256x256 kernel (256 workgroups, one per CU).  Measured on full grids the 256x256 / 8-phase
// kernel is ~1.33x the 128x128 one (tools/bench_kernels.py: 0.93-1.23 vs 0.70-0.90 PFLOP/s), and a round of 512 128x128
// workgroups (two per CU) covers half the output of a 256x256 round, so it costs 2 / 1.33 / 2 ~ 0.667 units; a last round of
// <= 256 such workgroups (one per CU, no co-resident partner) ~0.6 of that.  ov = cmb_gemm_desc.tile_hint, else CMB_GEMM_TILE,
// else the policy: 128 | 256 and the 256-tile kernel ids override (tests, A-B).
inline bool use_tile256(int M, int N, int splits, int ov) {
  if (ov == 256 || ov == 2560 || ov == 2561 || ov == 2590) return true;
  if (ov == 128) return false;
  const long t256 = (long)((M + 255) / 256) * ((N + 255) / 256) * splits;
  const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128) * splits;
  const double c256 = (double)((t256 + 255) / 256);
  const long rem = t128 % 512;
  const double c128 = 0.667 * ((double)(t128 / 512) + (rem == 0 ? 0.0 : (rem <= 256 ? 0.6 : 1.0)));
  return c256 <= c128;
}

// The 256 x 256 kernels address a tile's rows as a wave-uniform 64-bit base + a 32-bit per-lane byte offset: the span of
// 256 consecutive (row-mapped) rows of A and of B must fit (upper bound; negative strides never qualify).
inline bool tile_span_fits_u32(const RowMap& m, int64_t ldb) {
  if (m.s0 < 0 || m.s1 < 0 || m.s2 < 0 || ldb < 0) return false;
  double span = 256.0 * (double)m.s2;
  if (m.n1) span += (256.0 / (double)m.n2 + 1.0) * (double)m.s1 + (256.0 / (double)m.n1 + 1.0) * (double)m.s0;
  return 2.0 * span + 256.0 < 4.0e9 && 2.0 * 256.0 * (double)ldb + 256.0 < 4.0e9;
}

// gemm_p5.hip stages two 64-deep tiles ahead across item boundaries: every item (tile x K slice) must be at least two
// tiles long.
inline bool p5_ok(int K, const SplitK& sk) {
  const int last = K - (sk.splits - 1) * sk.k_per_split;
  return last >= 128 && sk.k_per_split >= 128;
}

// Where the register-buffered 4-wave kernel is the default 256 x 256 kernel: whole 128-column halves (round 4: in a last
// column tile with only its lower half in range the upper waves skip the epilogue; a half that is itself ragged leaves
// through the generic epilogue and drains the DMA pipeline — N = 1152 used to run 20-40 % behind the 8-wave kernel for that
// reason), no pre-activation copy (generic epilogue again) and at least 64 tiles.  Rounds 2-3 required more than one round of
// items per CU (the kernel's gain is the overlap ACROSS items, and a single round with an activation epilogue was 25 %
// faster on the 8-wave kernel); with round 4's epilogue (compile-time bias / LayerScale / residual variants, packed math) the
// start-up calibration found it ahead on all 20 hottest shapes of the step including the single-round ones (13824 x 1024 x
// 1024: 33.0 vs 36.4 us; profiles/r04_lab.md).
inline bool p5_default(const GemmParams& p, int splits) {
  const long tiles = (long)((p.M + 255) / 256) * ((p.N + 255) / 256) * splits;
  return p.N % 128 == 0 && !p.P && tiles >= 64;
}

// Which tile kernel a bf16 problem takes.  ov: 0 = the cost model (128x128 tile, or a 256x256 tile: the 4-wave
// register-buffered kernel gemm_nt_p5_kernel where p5_default() says, else the 8-wave kernel) | 128 | 256 (as the cost model's
// 256 branch) | 2560 / 2561 (8-wave kernel, schedule 0 / 1) | 2590 (gemm_nt_p5_kernel).
// Measured on the path's shapes (profiles/r02_gemm_lab.md): p5 is 3-11 % ahead of the 8-wave kernel when N is a
// multiple of 256 and up to 40 % behind when it is not (N = 384, 1152).
inline int choose_bf16_kernel(const GemmParams& p, const SplitK& sk, int ov, int* sched) {
  *sched = ov == 2561 ? 1 : 0;
  if (!use_tile256(p.M, p.N, sk.splits, ov) || !tile_span_fits_u32(p.a_map, p.ldb)) return kGemm128;
  if ((ov == 2590 || ((ov == 0 || ov == 256) && p5_default(p, sk.splits))) && p5_ok(p.K, sk)) return kGemmP5;
  return kGemm256;
}

// ---- the special kernels ---------------------------------------------------------------------------------------------------
// gemm_k64.hip: bf16 in and out, K == 64, N % 128 == 0, batch > 1, plain row maps, plain epilogue.
inline bool gemm_k64_eligible(const GemmParams& p, const GemmEnv& env) {
  return env.k64 && p.batch > 1 && p.K == 64 && (p.N % 128) == 0 && !p.out_f32 && !p.bias && !p.colscale && !p.R && !p.P && !p.slabs &&
         p.act == CMB_ACT_NONE && p.a_map.n1 == 0 && p.c_map.n1 == 0 && (p.c_map.s2 % 8) == 0 && (p.c_bs % 8) == 0 && !p.row_mean;
}

// gemm_smallm.hip: bf16 operands, M <= 32, one problem, whole K, N % 32 == 0, plain epilogue, no beta.
inline bool gemm_small_m_eligible(const GemmParams& p, int splits) {
  return p.M <= 32 && p.batch == 1 && splits == 1 && !p.slabs && (p.N % 32) == 0 && (p.K % 16) == 0 && !p.bias && !p.colscale && !p.R &&
         !p.P && p.act == CMB_ACT_NONE && !p.a_scale && !p.b_scale && !p.row_mean && p.beta == 0.0f && p.c_map.n1 == 0 &&
         (p.c_map.s2 % 4) == 0;
}

// ---- tail split (round 3) --------------------------------------------------------------------------------------------------
// A 256 x 256 grid of T tiles takes ceil(T / CUs) rounds; when T is a little more than a whole number of rounds the last
// round runs a handful of tiles on an otherwise idle chip (DINOv2's 11680 x 1536 GEMMs: 46 x 6 = 276 tiles = 2 rounds for
// 1.08 rounds of work; SigLIP's 11664 x 4352: 782 tiles = 4 rounds for 3.05).  Such a problem is launched as two row ranges:
// the first m1 row tiles (as many whole rounds as fit) on the 256-tile kernel the cost model picks for them, the remaining
// rows on the 128 x 128 kernel (two workgroups per CU, any epilogue), whose partial round is much shorter than a 256-tile
// round.  Cost model in 256-tile rounds: the 128-tile kernel runs ~1.6x longer per FLOP (profiles/r02_gemm_lab.md), 0.1 round
// for the extra launch; taken when it saves more than 7 %.  Row maps must be linear across the cut (identity, or the cut a
// multiple of the outer period).  Both return the rows of the first range or 0.
inline int tail_split_rows_mn(int64_t M, int64_t N, const GemmEnv& env, int64_t ncu) {
  if (!env.tail_split || N % 128 != 0 || ncu <= 0) return 0;
  const int64_t tm = (M + 255) / 256, tn = (N + 255) / 256, T = tm * tn;
  if (T <= ncu) return 0;
  const int64_t m1 = ((T / ncu) * ncu) / tn;   // row tiles that fill whole rounds
  if (m1 <= 0 || m1 >= tm) return 0;
  const int64_t tail = T - m1 * tn;
  const double now = (double)((T + ncu - 1) / ncu);
  const double hyb = (double)((m1 * tn + ncu - 1) / ncu) + 1.6 * (double)tail / (double)ncu + 0.1;
  return hyb < 0.93 * now ? (int)(m1 * 256) : 0;
}
inline bool map_linear_at(const RowMap& m, int64_t row) { return m.n1 == 0 || row % m.n1 == 0; }
inline int tail_split_rows(const GemmParams& p, int splits, int hint, const GemmEnv& env, int n_cu) {
  if (hint || env.tile || splits > 1 || p.slabs || p.a_scale || p.b_scale) return 0;
  const int m1 = tail_split_rows_mn(p.M, p.N, env, n_cu);
  if (!m1) return 0;
  if (!map_linear_at(p.a_map, m1) || !map_linear_at(p.c_map, m1) || (p.R && !map_linear_at(p.r_map, m1)) ||
      (p.P && !map_linear_at(p.p_map, m1)))
    return 0;
  return m1;
}

// ---- the plan of one cmb_gemm call -----------------------------------------------------------------------------------------
struct GemmPlan {
  int kernel;               // cmb_gemm_last_kernel() id
  int sched;                // 8-wave kernel: 0 = 8-phase ping-pong, 1 = in-wave pipeline
  int splits, k_per_split;  // effective split-K (1, K = one launch over the whole K, no slabs)
  int head_rows;            // tail split: rows [0, head_rows) on `kernel`, the rest on the 128 x 128 kernel (0 = launched whole)
};

// p: gemm_fill_params() of a descriptor that passed cmb_gemm's checks; elem_bytes: operand element size; split_k / hint: the
// descriptor's; n_cu: CUs of the device in whole XCDs.  Only bf16 has a choice: fp32 and fp8 run on the 128 x 128 kernel.
inline GemmPlan gemm_plan(const GemmParams& p, int elem_bytes, int split_k, int hint, const GemmEnv& env, const GemmPolicy& policy,
                          int n_cu) {
  const SplitK sk = splitk_geometry(p.K, 128 / elem_bytes, split_k);
  GemmPlan plan{kGemm128, 0, sk.splits, sk.k_per_split, 0};
  if (elem_bytes != 2) return plan;
  if (p.batch > 1) {
    if (gemm_k64_eligible(p, env)) plan.kernel = kGemmK64;
    return plan;
  }
  if (!hint && gemm_small_m_eligible(p, sk.splits)) {
    plan.kernel = kGemmSmallM;
    return plan;
  }
  if (const int m1 = tail_split_rows(p, sk.splits, hint, env, n_cu)) {
    GemmParams head = p;
    head.M = m1;
    // (256: the 256-tile branch of the cost model, no policy.  128 = tile_span_fits_u32 refused the 256-tile kernels — their
    // 32-bit per-lane offsets cannot span this row stride: no split, the whole problem on the 128-tile kernel)
    plan.kernel = choose_bf16_kernel(head, sk, 256, &plan.sched);
    if (plan.kernel != kGemm128) plan.head_rows = m1;
    return plan;
  }
  int ov = hint ? hint : env.tile;
  if (!ov && sk.splits == 1) ov = policy.lookup(p.M, p.N, p.K, p.act);
  plan.kernel = choose_bf16_kernel(p, sk, ov, &plan.sched);
  return plan;
}

// ---- pair launches of the persistent kernel (cmb_gemm_pair; gemm_p5.hip P5Args) --------------------------------------------
// Workgroups of problem 0 in a pair launch: the split g0 in [8, n_cu - 8] that minimises max over the two sides of
// rounds x (K tiles per item + epilogue), rounds = ceil(items / workgroups) (whole XCD multiples are not needed: a side's items
// are numbered from its own first workgroup).
inline double p5_side_time(int items, int k, int groups) { return (double)((items + groups - 1) / groups) * (k / 64.0 + 6.0); }
inline int p5_pair_split(int items0, int k0, int items1, int k1, int n_cu) {
  int best = n_cu / 2;
  double best_t = 1e30;
  for (int g = 8; g <= n_cu - 8; ++g) {
    const double t0 = p5_side_time(items0, k0, g), t1 = p5_side_time(items1, k1, n_cu - g);
    const double t = t0 > t1 ? t0 : t1;
    if (t < best_t - 1e-9) best_t = t, best = g;
  }
  return best;
}
inline int p5_items(const GemmParams& p) { return ((p.M + 255) / 256) * ((p.N + 255) / 256); }
// cost model of a pair launch split at g0 against the two single launches (whole rounds): > 0 = the pair wins
inline double gemm_p5_pair_gain(const GemmParams& a, const GemmParams& b, int n_cu, int g0) {
  const double single = p5_side_time(p5_items(a), a.K, n_cu) + p5_side_time(p5_items(b), b.K, n_cu);
  const double t0 = p5_side_time(p5_items(a), a.K, g0), t1 = p5_side_time(p5_items(b), b.K, n_cu - g0);
  return (single - (t0 > t1 ? t0 : t1)) / single;
}
// activation templates that have a pair instantiation (the residual linears of the ViT blocks are plain; every further
// instantiation is 35 s of compile time)
constexpr bool gemm_p5_pair_act_ok(int act) { return act == CMB_ACT_NONE || act == CMB_ACT_GELU_ERF; }

// One side of a pair: a single whole-K bf16 problem that is legal on the persistent kernel (whatever the single-launch cost
// model would pick: a tail split or the 128-tile kernel are answers to the same partly filled rounds the pair fills).
inline bool gemm_pair_side_ok(const GemmParams& p) {
  return p.batch == 1 && !p.out_f32 && !p.row_mean && !p.slabs && p5_default(p, 1) && p5_ok(p.K, SplitK{1, p.K}) &&
         tile_span_fits_u32(p.a_map, p.ldb);
}

// What cmb_gemm_pair asks of each descriptor before it builds parameters: a complete bf16 problem that leaves the kernel
// choice and the whole K to the library.
inline bool gemm_pair_desc_ok(const cmb_gemm_desc* d) {
  return d && d->A && d->B && d->C && d->M > 0 && d->N > 0 && d->K > 0 && d->dtype == CMB_BF16 && d->split_k <= 1 && !d->tile_hint;
}

struct PairPlan {
  bool pair;   // one launch for both problems
  int g0;      // ... with problem 0 on workgroups [0, g0) of n_cu
};
// Two independent problems whose descriptors passed gemm_pair_desc_ok(): one launch when both sides are legal, share an
// activation template that has a pair instantiation, and the round arithmetic says the pair saves at least 4 % (DINOv2's and
// SigLIP's 1.62- / 1.35-round linears side by side: 3.0 + 2.9 rounds on 138 + 118 workgroups instead of 2 + 2 on 256).
inline PairPlan gemm_pair_plan(const GemmParams& p0, const GemmParams& p1, const GemmEnv& env, int n_cu) {
  PairPlan plan{false, 0};
  if (!env.pair || env.tile || n_cu < 16 || p0.act != p1.act || !gemm_p5_pair_act_ok(p0.act) || !gemm_pair_side_ok(p0) ||
      !gemm_pair_side_ok(p1))
    return plan;
  plan.g0 = p5_pair_split(p5_items(p0), p0.K, p5_items(p1), p1.K, n_cu);
  plan.pair = gemm_p5_pair_gain(p0, p1, n_cu, plan.g0) >= 0.04;
  return plan;
}

}  // namespace cmb_gemm_detail
