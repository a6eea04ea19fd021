// gemm.hip — C[M,N] = epilogue(alpha * A[M,K] · B[N,K]^T) for gfx950 (MI355X).
//
// Design:
//   * operands stream HBM -> LDS with global_load_lds_dwordx4 (no VGPR round trip), two LDS stages,
//     one barrier per 128-byte K-step; the next K-step's DMA is issued before the current MFMAs.
//   * LDS tiles are XOR-swizzled (gemm_layout.h) so every ds_read_b128 fragment read is
//     bank-conflict free; the swizzle lives in the per-lane global source address.
//   * v_mfma_f32_32x32x16_bf16 (bf16) or v_mfma_f32_32x32x2_f32 (exact fp32 parity path),
//     fp32 accumulation in 64 accumulator registers per wave (2x2 tiles of 32x32).
//   * operands are swapped at the MFMA so a lane owns one output row and 4 consecutive columns per
//     register quad; the tile is staged through LDS once and leaves as 16/32-byte row-contiguous
//     stores with the whole epilogue (bias, activation, LayerScale, residual, fp32 accumulate) fused.
//   * block id -> tile mapping is XCD-aware (8 XCDs, private L2s).
//   * rows of A / C / residual / pre_out go through a 3-level row map so gathers such as the in-LLM
//     slice hidden[:, 91:691].view(B,24,25,H)[:, :, :24] are folded into the loads.
#include "gemm_common.h"

using namespace cmb_gemm_detail;

namespace {

template <int BM, int BN>
constexpr int gemm_smem_bytes() {
  return (2 * (BM + BN) * 128) > (BM * (BN + 4) * 4) ? (2 * (BM + BN) * 128) : (BM * (BN + 4) * 4);
}

template <typename T, int BM, int BN, int WM, int WN>
__global__ void __launch_bounds__(WM* WN * 64) gemm_nt_kernel(const GemmParams p_in) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  GemmParams p = p_in;
  if (p.batch > 1) {  // batched launch: problem blockIdx.z of p.batch (operand / result bases advance by the batch strides)
    const int64_t bz = blockIdx.z;
    p.A += bz * p.a_bs * (int64_t)sizeof(T);
    p.B += bz * p.b_bs * (int64_t)sizeof(T);
    p.C += bz * p.c_bs * (int64_t)(p.out_f32 ? 4 : sizeof(typename Mfma<T>::out_t));
    if (p.R) p.R += bz * p.c_bs * (int64_t)sizeof(T);   // a batched residual is laid out as C (same batch stride)
  }
  constexpr int NW = WM * WN;
  constexpr int NT = NW * 64;
  constexpr int BK = 128 / (int)sizeof(T);
  constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE = A_BYTES + B_BYTES;
  constexpr int WTM = BM / WM, WTN = BN / WN, TM = WTM / 32, TN = WTN / 32;
  constexpr int A_IT = BM / 8 / NW, B_IT = BN / 8 / NW;
  static_assert(BM % (8 * NW) == 0 && BN % (8 * NW) == 0, "tile rows must split over the waves");
  static_assert(WTM % 32 == 0 && WTN % 32 == 0, "wave tile must be a multiple of 32x32");
  typedef typename Mfma<T>::frag_t frag_t;
  typedef typename Mfma<T>::out_t out_t;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;

  const int nblk = p.tiles_m * p.tiles_n;
  const int id = gl_xcd_remap((int)blockIdx.x, nblk);
  int tile_m, tile_n;
  gl_group_tile(id, p.tiles_m, p.tiles_n, 8, &tile_m, &tile_n);  // 64 resident workgroups per XCD = 8 x 8 tiles
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int kz = blockIdx.y;
  const int kbeg = kz * p.k_per_split;
  const int kend = (kbeg + p.k_per_split < p.K) ? (kbeg + p.k_per_split) : p.K;
  const int nk = (kend > kbeg) ? (kend - kbeg) / BK : 0;

  // per-lane global source pointers of the LDS-DMA pieces this wave issues (row clamped at the edge:
  // out-of-range rows re-read the last valid row and are never stored)
  const char* a_src[A_IT];
  const char* b_src[B_IT];
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    const int grp = wave + i * NW;
    const int row = gl_dma_row(grp, lane), c = gl_dma_chunk(grp, lane);
    int gm = m0 + row;
    gm = gm < p.M ? gm : p.M - 1;
    a_src[i] = p.A + (row_off(p.a_map, (uint32_t)gm) + kbeg) * (int64_t)sizeof(T) + c * 16;
  }
#pragma unroll
  for (int i = 0; i < B_IT; ++i) {
    const int grp = wave + i * NW;
    const int row = gl_dma_row(grp, lane), c = gl_dma_chunk(grp, lane);
    int gn = n0 + row;
    gn = gn < p.N ? gn : p.N - 1;
    b_src[i] = p.B + ((int64_t)gn * p.ldb + kbeg) * (int64_t)sizeof(T) + c * 16;
  }

  // fragment read offsets (bytes inside a stage)
  int a_off[TM], a_swz[TM], b_off[TN], b_swz[TN];
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    const int row = wm * WTM + t * 32 + gl_frag_row(lane);
    a_off[t] = row * 128;
    a_swz[t] = gl_swz(row);
  }
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    const int row = wn * WTN + t * 32 + gl_frag_row(lane);
    b_off[t] = A_BYTES + row * 128;
    b_swz[t] = gl_swz(row);
  }

  f32x16_t acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  auto stage = [&](int s) {
    char* sa = smem + s * STAGE;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      glds16(a_src[i], sa + (wave + i * NW) * 1024);
      a_src[i] += 128;
    }
    char* sb = sa + A_BYTES;
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
      glds16(b_src[i], sb + (wave + i * NW) * 1024);
      b_src[i] += 128;
    }
  };

  if (nk > 0) {
    stage(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      if (kt + 1 < nk) stage(cur ^ 1);  // async: lands while this K-step's MFMAs run
      const char* base = smem + cur * STAGE;
#pragma unroll
      for (int ks = 0; ks < Mfma<T>::KSTEPS; ++ks) {
        frag_t a[TM], b[TN];
#pragma unroll
        for (int t = 0; t < TM; ++t) a[t] = Mfma<T>::load(base + a_off[t], a_swz[t], ks, lane);
#pragma unroll
        for (int t = 0; t < TN; ++t) b[t] = Mfma<T>::load(base + b_off[t], b_swz[t], ks, lane);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) Mfma<T>::run(b[j], a[i], acc[i][j]);  // swapped: rows=n, cols=m
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
  }

  // ---- epilogue: accumulators -> LDS (fp32, row stride BN+4) -> row-contiguous global stores ----
  constexpr int CS = BN + 4;
  float* cs = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = wm * WTM + i * 32 + gl_acc_m(lane);
        const int n = wn * WTN + j * 32 + gl_acc_n(4 * q, lane);
        f32x4_t v;
        v[0] = acc[i][j][4 * q + 0];
        v[1] = acc[i][j][4 * q + 1];
        v[2] = acc[i][j][4 * q + 2];
        v[3] = acc[i][j][4 * q + 3];
        *reinterpret_cast<f32x4_t*>(cs + m * CS + n) = v;
      }
  __syncthreads();

  constexpr int GPR = BN / 8;  // 8-column groups per tile row
  constexpr int GROUPS = BM * GPR;
  dispatch_act(p.slabs ? CMB_ACT_NONE : p.act, [&](auto act_c) __attribute__((always_inline)) {
    constexpr int ACT = decltype(act_c)::value;
    for (int grp = tid; grp < GROUPS; grp += NT) {
      const int row = grp / GPR, c8 = grp - row * GPR;
      const int gm = m0 + row, gn = n0 + c8 * 8;
      if (gm >= p.M || gn >= p.N) continue;
      float v[8];
      {
        const f32x4_t lo = *reinterpret_cast<const f32x4_t*>(cs + row * CS + c8 * 8);
        const f32x4_t hi = *reinterpret_cast<const f32x4_t*>(cs + row * CS + c8 * 8 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = lo[e]; v[4 + e] = hi[e]; }
      }
      gemm_epilogue8<out_t, ACT>(p, kz, gm, gn, v);
    }
  });
}

// out = alpha * sum_z slab[z] + beta * out   (fp32 slabs [Z][M][N]; out through the C row map)
template <typename TOut>
__global__ void __launch_bounds__(256) splitk_reduce_kernel(const float* slabs, int Z, int M, int N,
                                                            char* C, RowMap c_map, float alpha,
                                                            float beta) {
  const int64_t groups = (int64_t)M * (N / 8);
  for (int64_t gidx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; gidx < groups;
       gidx += (int64_t)gridDim.x * blockDim.x) {
    const int m = (int)(gidx / (N / 8)), n = (int)(gidx - (int64_t)m * (N / 8)) * 8;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int z = 0; z < Z; ++z) {
      float v[8];
      load8f(slabs + ((int64_t)z * M + m) * N + n, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += v[e];
    }
    TOut* cp = reinterpret_cast<TOut*>(C) + row_off(c_map, (uint32_t)m) + n;
    if (beta != 0.0f) {
      float old[8];
      Vec8<TOut>::load(cp, old);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = alpha * acc[e] + beta * old[e];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] *= alpha;
    }
    Vec8<TOut>::store(cp, acc);
  }
}

template <typename T, int BM, int BN, int WM, int WN>
int launch_gemm(GemmParams& p, int splits, hipStream_t s) {
  constexpr int smem = gemm_smem_bytes<BM, BN>();
  static CmbAttrOnce attr_once;
  auto kern = gemm_nt_kernel<T, BM, BN, WM, WN>;
  if (const uint32_t attr_bit = attr_once.need()) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                            hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess)
      return CMB_ERR_LAUNCH;
    attr_once.done(attr_bit);
  }
  p.tiles_m = (p.M + BM - 1) / BM;
  p.tiles_n = (p.N + BN - 1) / BN;
  dim3 grid((unsigned)(p.tiles_m * p.tiles_n), (unsigned)splits, (unsigned)(p.batch > 1 ? p.batch : 1));
  hipLaunchKernelGGL(kern, grid, dim3(WM * WN * 64), smem, s, p);
  CMB_CHECK_LAUNCH();
  return CMB_OK;
}


// out = alpha * sum of the slabs + beta * out behind a split-K launch (rows = p.slab_rows: cmb_gemm_tn's batched results are
// one contiguous [batch * M, N] matrix)
template <typename TOut>
int launch_splitk_reduce(const GemmParams& p, int splits, hipStream_t s) {
  const int64_t groups = (int64_t)p.slab_rows * (p.N / 8);
  int blocks = (int)((groups + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  if (p.out_f32)
    hipLaunchKernelGGL(splitk_reduce_kernel<float>, dim3(blocks), dim3(256), 0, s, p.slabs, splits, p.slab_rows, p.N, p.C, p.c_map,
                       p.alpha, p.beta);
  else
    hipLaunchKernelGGL(splitk_reduce_kernel<TOut>, dim3(blocks), dim3(256), 0, s, p.slabs, splits, p.slab_rows, p.N, p.C, p.c_map,
                       p.alpha, p.beta);
  CMB_CHECK_LAUNCH();
  return CMB_OK;
}

// split-K as planned (gemm_plan.h: splitk_geometry): K slice per launch and the fp32 slabs in the caller's workspace
int gemm_attach_slabs(const cmb_gemm_desc* d, GemmParams& p, int splits, int k_per_split) {
  if (splits <= 1) return CMB_OK;
  const int64_t need = (int64_t)splits * p.slab_rows * p.N * 4;
  if (!d->workspace || d->workspace_bytes < need) return CMB_ERR_WORKSPACE;
  p.k_per_split = k_per_split;
  p.slabs = (float*)d->workspace;
  return CMB_OK;
}

const GemmEnv& gemm_env() {
  static const GemmEnv env = GemmEnv::from_environment();
  return env;
}

GemmPolicy g_policy;                        // cmb_gemm_policy_set
thread_local int g_last_kernel = 0;         // cmb_gemm_last_kernel()
thread_local int g_last_pair = 0;           // cmb_gemm_pair_last(): did the thread's last cmb_gemm_pair take the one-launch path?

// descriptor -> parameter block of one cmb_gemm call and its checks (shared by cmb_gemm and cmb_gemm_pair); split-K is planned
// and attached by the caller
template <typename T>
int gemm_params_from_desc(const cmb_gemm_desc* d, GemmParams& p) {
  constexpr int BK = 128 / (int)sizeof(T);
  if (d->K % BK != 0 || d->N % 8 != 0) return CMB_ERR_SHAPE;
  gemm_fill_params(d, p);
  const bool split = d->split_k > 1;
  if (d->row_mean && (!d->row_rstd || !d->col_sum || !d->bias || d->alpha != 1.0f || split || p.batch > 1 || sizeof(T) != 2 ||
                      d->pre_out))
    return CMB_ERR_BAD_ARG;   // the folded-LayerNorm epilogue: bf16 operands, bias (b'), one launch over the whole K
  if (d->act == CMB_ACT_SWIGLU_PAIRS &&
      (split || d->colscale || d->residual || d->pre_out || d->out_dtype != d->dtype || d->N % 16 != 0 || p.batch > 1 ||
       sizeof(T) == 1))
    return CMB_ERR_BAD_ARG;   // the gated epilogue writes an N / 2 wide C of the operand dtype and nothing else
  if (p.batch > 1) {
    // batched problems: plain epilogue (alpha / activation / out dtype; a residual laid out as C: its batch stride is C's), no
    // split-K, 16-byte aligned strides
    if (split || d->bias || d->colscale || d->pre_out || sizeof(T) == 1) return CMB_ERR_BAD_ARG;
    if (d->residual && (d->out_dtype != d->dtype)) return CMB_ERR_BAD_ARG;
    if ((p.a_bs * (int64_t)sizeof(T)) % 16 || (p.b_bs * (int64_t)sizeof(T)) % 16 || (p.c_bs * 2) % 16) return CMB_ERR_ALIGNMENT;
  }
  if constexpr (sizeof(T) == 1) {
    if (split) return CMB_ERR_BAD_ARG;
    p.a_scale = d->a_scale; p.b_scale = d->b_scale;
  }
  // every row base and leading dimension must keep 16-byte chunks aligned
  const int64_t es = sizeof(T);
  if (!cmb_aligned16(d->A) || !cmb_aligned16(d->B) || (d->ldb * es) % 16 != 0 ||
      (d->a_map.s2 * es) % 16 != 0 || (d->a_map.n1 && ((d->a_map.s0 * es) % 16 || (d->a_map.s1 * es) % 16)))
    return CMB_ERR_ALIGNMENT;
  return CMB_OK;
}

// build the parameters, ask gemm_plan.h for the plan, launch what it names, reduce the slabs
template <typename T>
int gemm_dispatch(const cmb_gemm_desc* d, hipStream_t s) {
  GemmParams p;
  int rc = gemm_params_from_desc<T>(d, p);
  if (rc != CMB_OK) return rc;
  const GemmPlan plan = gemm_plan(p, (int)sizeof(T), d->split_k, d->tile_hint, gemm_env(), g_policy, gemm_device_cus());
  if ((rc = gemm_attach_slabs(d, p, plan.splits, plan.k_per_split)) != CMB_OK) return rc;
  g_last_kernel = plan.kernel;
  switch (plan.kernel) {
    case kGemmK64: rc = launch_gemm_k64_batched(p, s); break;
    case kGemmSmallM: rc = launch_gemm_small_m(p, s); break;
    case kGemmP5:
    case kGemm256: {
      GemmParams tail;
      if (const int m1 = plan.head_rows) {   // tail split: rows [m1, M) on the 128 x 128 kernel (no slabs: nothing reads p.M later)
        tail = p;
        tail.M = p.M - m1;
        tail.A += row_off(p.a_map, (uint32_t)m1) * 2;
        tail.C += row_off(p.c_map, (uint32_t)m1) * (p.out_f32 ? 4 : 2);
        if (p.R) tail.R += row_off(p.r_map, (uint32_t)m1) * 2;
        if (p.P) tail.P += row_off(p.p_map, (uint32_t)m1) * 2;
        if (p.row_mean) tail.row_mean += m1, tail.row_rstd += m1;
        p.M = m1;
      }
      rc = plan.kernel == kGemmP5 ? launch_gemm_p5_bf16(p, plan.splits, s) : launch_gemm256_bf16(p, plan.splits, plan.sched, s);
      if (rc == CMB_OK && plan.head_rows) rc = launch_gemm<T, 128, 128, 2, 2>(tail, 1, s);
      break;
    }
    default: rc = launch_gemm<T, 128, 128, 2, 2>(p, plan.splits, s); break;
  }
  if (rc == CMB_OK && p.slabs) rc = launch_splitk_reduce<typename Mfma<T>::out_t>(p, plan.splits, s);
  return rc;
}

// C[M,N] = alpha * At[K,M]^T Bt[K,N] (+ beta C): descriptor checks, split-K slabs and their reduction around gemm_tn.hip
int gemm_tn_dispatch(const cmb_gemm_desc* d, hipStream_t s) {
  if (d->dtype != CMB_BF16 || (d->out_dtype != CMB_F32 && d->out_dtype != CMB_BF16)) return CMB_ERR_BAD_ARG;
  if (d->bias || d->colscale || d->residual || d->pre_out || d->act != CMB_ACT_NONE || d->a_map.n1 != 0) return CMB_ERR_BAD_ARG;
  if (d->M % 8 != 0 || d->N % 8 != 0) return CMB_ERR_SHAPE;
  const int64_t lda = d->a_map.s2;
  if (!cmb_aligned16(d->A) || !cmb_aligned16(d->B) || (lda * 2) % 16 != 0 || (d->ldb * 2) % 16 != 0 || lda < d->M || d->ldb < d->N)
    return CMB_ERR_ALIGNMENT;
  if (d->row_mean) return CMB_ERR_BAD_ARG;
  GemmParams p;
  gemm_fill_params(d, p);   // (every epilogue field was refused above, so they are null here; the folded-LayerNorm companions
  p.row_rstd = p.col_sum = nullptr;   // of row_mean are ignored as they always were)
  const SplitK sk = splitk_geometry(p.K, 64, d->split_k);
  if (p.batch > 1) {
    if ((p.a_bs * 2) % 16 || (p.b_bs * 2) % 16 || (p.c_bs * 2) % 16) return CMB_ERR_ALIGNMENT;
    // split-K of a batch: the slabs are [split][batch * M][N], reduced as ONE matrix — the results must be contiguous
    if (d->split_k > 1 && (d->c_map.n1 != 0 || d->c_map.s2 != d->N || p.c_bs != (int64_t)p.M * p.N)) return CMB_ERR_BAD_ARG;
    if (sk.splits > 1) p.slab_rows = p.batch * p.M;
  }
  int rc = gemm_attach_slabs(d, p, sk.splits, sk.k_per_split);
  if (rc != CMB_OK) return rc;
  g_last_kernel = kGemmTN;
  rc = launch_gemm_tn_bf16(p, sk.splits, s);
  if (rc == CMB_OK && p.slabs) rc = launch_splitk_reduce<bf16_t>(p, sk.splits, s);
  return rc;
}

}  // namespace

namespace cmb_gemm_detail {
int gemm_device_cus() {
  static int n = 0;
  if (!n) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        n <= 0)
      n = 256;
    n -= n % 8;   // whole XCD rounds: item % 8 == block % 8 in every round of the persistent kernel
    if (n <= 0) n = 256;
  }
  return n;
}
}  // namespace cmb_gemm_detail

// Views of the plan's helpers for callers that label profiles: the cost model's tile and the tail split's first range for a
// bare shape.  They do not run gemm_plan(): a launch may still take another kernel than cmb_gemm_tile says (row strides beyond
// the 32-bit tile span, the M <= 32 and K = 64 kernels) or stay whole (row maps that are not linear at the cut).
extern "C" int cmb_gemm_tile(int dtype, int64_t M, int64_t N, int32_t split_k, int32_t tile_hint) {
  return dtype == CMB_BF16 && use_tile256((int)M, (int)N, split_k > 1 ? split_k : 1, tile_hint ? tile_hint : gemm_env().tile) ? 256 : 128;
}

extern "C" int64_t cmb_gemm_tail_rows(int64_t M, int64_t N) { return tail_split_rows_mn(M, N, gemm_env(), gemm_device_cus()); }

extern "C" int cmb_gemm_policy_set(int64_t M, int64_t N, int64_t K, int32_t act, int32_t kernel) {
  return g_policy.set(M, N, K, act, kernel);
}

extern "C" int cmb_gemm_policy_clear(void) {
  g_policy.n = 0;
  return CMB_OK;
}

extern "C" int cmb_gemm_last_kernel(void) { return g_last_kernel; }
extern "C" int cmb_gemm_pair_last(void) { return g_last_pair; }

extern "C" int cmb_gemm_tn(const cmb_gemm_desc* d, void* stream) {
  if (!d || !d->A || !d->B || !d->C) return CMB_ERR_BAD_ARG;
  if (d->M <= 0 || d->N <= 0 || d->K < 0) return CMB_ERR_BAD_ARG;
  return gemm_tn_dispatch(d, (hipStream_t)stream);
}

extern "C" int cmb_gemm(const cmb_gemm_desc* d, void* stream) {
  if (!d || !d->A || !d->B || !d->C) return CMB_ERR_BAD_ARG;
  if (d->M < 0 || d->N <= 0 || d->K <= 0) return CMB_ERR_BAD_ARG;
  if (d->M == 0) return CMB_OK;
  if (d->dtype == CMB_F32 && d->out_dtype != CMB_F32) return CMB_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (d->dtype == CMB_BF16) return gemm_dispatch<bf16_t>(d, s);
  if (d->dtype == CMB_F32) return gemm_dispatch<float>(d, s);
  if (d->dtype == CMB_FP8_E4M3) return gemm_dispatch<fp8e4m3_t>(d, s);
  return CMB_ERR_BAD_ARG;
}

// Two independent bf16 GEMMs.  One launch of the persistent 256 x 256 kernel with the workgroups split between the problems
// (gemm_p5.hip, P5Args) where gemm_pair_plan() says so; otherwise exactly the two cmb_gemm calls.  Results are bit-identical
// either way (same kernel, same item arithmetic).  CMB_GEMM_PAIR=0 forces the two calls (A/B runs).
extern "C" int cmb_gemm_pair(const cmb_gemm_desc* d0, const cmb_gemm_desc* d1, void* stream) {
  g_last_pair = 0;
  GemmParams p0, p1;
  if (gemm_env().pair && gemm_pair_desc_ok(d0) && gemm_pair_desc_ok(d1) && gemm_params_from_desc<bf16_t>(d0, p0) == CMB_OK &&
      gemm_params_from_desc<bf16_t>(d1, p1) == CMB_OK) {
    const PairPlan plan = gemm_pair_plan(p0, p1, gemm_env(), gemm_device_cus());
    if (plan.pair) {
      g_last_kernel = kGemmP5;
      const int rc = launch_gemm_p5_bf16(p0, 1, (hipStream_t)stream, &p1, plan.g0);
      if (rc == CMB_OK) g_last_pair = 1;
      return rc;
    }
  }
  const int rc = cmb_gemm(d0, stream);
  return rc != CMB_OK ? rc : cmb_gemm(d1, stream);
}
