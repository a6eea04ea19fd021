// decode_linear_wide.hip — cmb_decode_linear's contract for 1 <= M <= 64 rows: the linears of a decode step of generate() at
// 17-64 sequences (or beams), out[M, N'] = epilogue(prologue(x)[M, K] · W[N, K]^T), bf16 x and W, fp32 accumulation, the
// RMSNorm prologue and the SwiGLU / residual epilogues of decode_linear.hip.  At 64 rows a projection is still a stream of
// weights read once (64 FLOP per weight byte).  Roofline class: HBM (the weights; x is at most 1.8 MiB and stays in L2).
//
// Layout (decode_linear_wide_layout.h has the maps, the plan and the reasoning; tests/csrc/decode_linear_wide_layout_sim.cpp
// enumerates them).  x is B = ceil(M / 16) row blocks of the 16-column MFMA operand, B a template parameter.  A workgroup
// owns a slab of 16 P weight rows, P = 1 / 2 from the plan; its four waves take the 64-element k-steps round robin.  Weights
// go straight to VGPRs, 16 bytes per lane with non-temporal loads, a full 128-byte line per row and instruction, two groups
// of U steps in flight per wave; no LDS staging.  The two 8-row tiles of a pair trade their odd 8-lane groups by DPP, so that
// each MFMA multiplies 16 distinct weight rows at 32 k and no result is thrown away (the narrow kernel discards half).  The
// four waves' partial tiles are summed through LDS in wave order by the thread that owns the output element.  No split of K
// across workgroups, no atomics, no flags: the same inputs give the same bits, and a row's bits depend neither on M nor on
// the other rows nor on the slab.  They are not decode_linear.hip's bits (another order of the same sum).
#include "common.h"
#include "decode_linear_wide_layout.h"

namespace {

constexpr int DLW_THREADS = 64 * DLW_WAVES;
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

struct DlwParams {
  const bf16_t* x;
  int64_t x_ld;
  int32_t M;
  const bf16_t* norm_w;
  float eps;
  const bf16_t* W;
  int64_t w_ld, N, K;
  int32_t act;
  const bf16_t* res;
  int64_t r_ld;
  void* out;
  int64_t o_ld;
  int32_t out_f32;
};

// the 8 bf16 of a 16-byte fragment as fp32 (element 2 d in the low half of dword d)
__device__ __forceinline__ void dlw_unpack(const u32x4_t& r, float (&v)[8]) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    v[2 * d] = __builtin_bit_cast(float, r[d] << 16);
    v[2 * d + 1] = __builtin_bit_cast(float, r[d] & 0xffff0000u);
  }
}

// the two loaded tiles (a, b) of a pair -> the operands of half 0 and half 1 (dlw_op_src_tile / dlw_op_src_lane): lanes
// 8-15 of every row of 16 take half 0 from tile b's lane ^ 8, lanes 0-7 take half 1 from tile a's lane ^ 8.
// 0x128 = row_ror:8, the banks are the row's four groups of 4 lanes; a lane outside the bank mask keeps `old`
__device__ __forceinline__ void dlw_regroup(u32x4_t& a, u32x4_t& b) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const uint32_t h0 = __builtin_amdgcn_update_dpp(a[d], b[d], 0x128, 0xf, 0xc, false);
    const uint32_t h1 = __builtin_amdgcn_update_dpp(b[d], a[d], 0x128, 0xf, 0x3, false);
    a[d] = h0;
    b[d] = h1;
  }
}

// k-steps per group (two groups in flight).  A step holds 8 P + 8 B (+ 8 under the norm) registers of loads.  The budget is
// 256 registers everywhere, two workgroups per CU: with three and four row blocks a second wave per SIMD measured better than
// twice the steps in flight at one (Llama-3-8B layer at 64 rows 407 -> 353 us, profiles/decode_linear_wide.md)
template <int P, int NB, bool NORM>
constexpr int dlw_unroll() {
  return NB <= 2 ? (NORM ? (P == 2 ? 1 : 2) : (P == 2 ? 2 : 3)) : (NORM || P == 2 ? 1 : 2);
}

template <int P, int NB, bool NORM>
__global__ void __launch_bounds__(DLW_THREADS, 2) decode_linear_wide_kernel(const DlwParams p) {
  constexpr int T = 2 * P;
  constexpr int U = dlw_unroll<P, NB, NORM>();
  constexpr int RED = DLW_WAVES * P * DLW_MAX_M * DLW_PAIR_ROWS;
  __shared__ __attribute__((aligned(16))) float sm[RED + DLW_WAVES * DLW_MAX_M];   // partials (dlw_red_index), sums of squares [wave][m]

  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t K = p.K;
  const int64_t cols = p.act ? p.N / 2 : p.N;          // N'
  const int cols_wg = dlw_slab_cols(P, p.act);
  const int64_t col0 = (int64_t)blockIdx.x * cols_wg;

  // ---- operand pointers: row starts; a row past the end re-reads the last one (its sums are never stored) ----
  const bf16_t* wrow[T];
#pragma unroll
  for (int t = 0; t < T; ++t) wrow[t] = p.W + dlw_w_index(P, p.act, p.N, col0, t, lane) * p.w_ld;
  const int wk = dlw_w_k(lane);
  const bf16_t* xrow[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int m = DLW_BLOCK_M * b + dlw_x_row(lane);
    xrow[b] = p.x + (int64_t)(m < p.M ? m : p.M - 1) * p.x_ld;
  }

  struct Frag {
    u32x4_t w[U][T], x[U][2][NB], n[U][2];
    bool in[U][2];           // the x fragments lie inside K (else they are taken as zero: their loads re-read k = 0)
  };
  // group g of the wave: its steps g U .. g U + U - 1.  A fragment past K re-reads k = 0 and its x side is taken as zero in
  // multiply: every load is issued whatever K is, nothing branches around a load
  auto fetch = [&](Frag& f, int64_t g) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t k0 = ((g * U + u) * DLW_WAVES + wave) * DLW_KSTEP;
      const int64_t kw = k0 + wk < K ? k0 + wk : 0;
#pragma unroll
      for (int t = 0; t < T; ++t) f.w[u][t] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wrow[t] + kw));
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        int64_t kx = k0 + dlw_x_k(h, lane);
        f.in[u][h] = kx < K;
        kx = kx < K ? kx : 0;
#pragma unroll
        for (int b = 0; b < NB; ++b) f.x[u][h][b] = *reinterpret_cast<const u32x4_t*>(xrow[b] + kx);
        if (NORM) f.n[u][h] = *reinterpret_cast<const u32x4_t*>(p.norm_w + kx);
      }
    }
  };

  f32x4_t acc[P][NB];
  float ss[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    ss[b] = 0.f;
#pragma unroll
    for (int q = 0; q < P; ++q) acc[q][b] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }
  auto multiply = [&](const Frag& f) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      u32x4_t op[T];         // op[2 q + h]: the pair's 16 rows at the k of half h
#pragma unroll
      for (int q = 0; q < P; ++q) {
        op[2 * q] = f.w[u][2 * q];
        op[2 * q + 1] = f.w[u][2 * q + 1];
        dlw_regroup(op[2 * q], op[2 * q + 1]);
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float nv[8];
        if (NORM) dlw_unpack(f.n[u][h], nv);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          u32x4_t xr = f.x[u][h][b];
#pragma unroll
          for (int d = 0; d < 4; ++d) xr[d] = f.in[u][h] ? xr[d] : 0u;
          u32x4_t xlo = {0u, 0u, 0u, 0u};
          if (NORM) {
            // x[k] norm_w[k] is a product of two bf16: 16 significant bits, exact in fp32.  Its bf16 rounding and the
            // remainder (8 bits at most, a bf16 too) go through the matrix unit as two operands, so the normalised row is
            // never rounded
            float xv[8], hv[8];
            dlw_unpack(xr, xv);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              ss[b] = fmaf(xv[e], xv[e], ss[b]);
              xv[e] *= nv[e];
            }
            xr = __builtin_bit_cast(u32x4_t, cvt8_bf16(xv[0], xv[1], xv[2], xv[3], xv[4], xv[5], xv[6], xv[7]));
            dlw_unpack(xr, hv);
#pragma unroll
            for (int e = 0; e < 8; ++e) xv[e] -= hv[e];
            xlo = __builtin_bit_cast(u32x4_t, cvt8_bf16(xv[0], xv[1], xv[2], xv[3], xv[4], xv[5], xv[6], xv[7]));
          }
          const bf16x8_t xb = __builtin_bit_cast(bf16x8_t, xr), xl = __builtin_bit_cast(bf16x8_t, xlo);
#pragma unroll
          for (int q = 0; q < P; ++q) {
            const bf16x8_t wb = __builtin_bit_cast(bf16x8_t, op[2 * q + h]);
            acc[q][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb, xb, acc[q][b], 0, 0, 0);
            if (NORM) acc[q][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb, xl, acc[q][b], 0, 0, 0);
          }
        }
      }
    }
  };

  // ---- the wave's steps wave, wave + 4, ...: groups of U, one being multiplied while the next one lands ----
  const int64_t nsteps = (K + DLW_KSTEP - 1) / DLW_KSTEP;
  const int64_t cnt = nsteps > wave ? (nsteps - wave + DLW_WAVES - 1) / DLW_WAVES : 0;
  const int64_t groups = (cnt + U - 1) / U;
  if (groups > 0) {
    Frag fa, fb;
    fetch(fa, 0);
    for (int64_t g = 0; g < groups; g += 2) {
      // (the scheduler would otherwise sink the loads towards their uses and drain the queue once per iteration)
      fetch(fb, g + 1);       // the last one or two fetches may lie past the share: k = 0 again, multiplied as zero
      __builtin_amdgcn_sched_barrier(0);
      multiply(fa);
      __builtin_amdgcn_sched_barrier(0);
      fetch(fa, g + 2);
      __builtin_amdgcn_sched_barrier(0);
      multiply(fb);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- partial tiles and sums of squares to LDS ----
#pragma unroll
  for (int b = 0; b < NB; ++b) {
#pragma unroll
    for (int q = 0; q < P; ++q)
      *reinterpret_cast<f32x4_t*>(&sm[dlw_red_index(P, wave, q, DLW_BLOCK_M * b + dlw_acc_m(lane), dlw_acc_row(lane, 0))]) =
          acc[q][b];
    if (NORM) {
      float s = ss[b];
      s += __shfl_xor(s, 16, 64);       // the four lanes of an x row: k quarters of every half step
      s += __shfl_xor(s, 32, 64);
      if (lane < DLW_BLOCK_M) sm[RED + wave * DLW_MAX_M + DLW_BLOCK_M * b + lane] = s;
    }
  }
  __syncthreads();

  // ---- epilogue: one thread per output element, partials added in wave order ----
  auto total = [&](int tile, int r, int m) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < DLW_WAVES; ++w) s += sm[dlw_red_index(P, w, dlw_tile_pair(tile), m, dlw_tile_row(tile, r))];
    return s;
  };
  for (int idx = threadIdx.x; idx < cols_wg * p.M; idx += DLW_THREADS) {
    const int m = idx / cols_wg, c = idx - m * cols_wg;
    const int64_t col = col0 + c;
    if (col >= cols) continue;
    float rstd = 1.f;
    if (NORM) {
      float s2 = 0.f;
#pragma unroll
      for (int w = 0; w < DLW_WAVES; ++w) s2 += sm[RED + w * DLW_MAX_M + m];
      rstd = __builtin_amdgcn_rsqf(s2 / (float)K + p.eps);
    }
    const int tile = dlw_col_tile(c), r = c % DLW_TILE_ROWS;
    float v = total(tile, r, m) * rstd;
    if (p.act) {
      const float up = total(tile + P, r, m) * rstd;
      v = v * cmb_sigmoid(v) * up;
    }
    if (p.res) v += (float)p.res[(int64_t)m * p.r_ld + col];
    if (p.out_f32) reinterpret_cast<float*>(p.out)[(int64_t)m * p.o_ld + col] = v;
    else reinterpret_cast<bf16_t*>(p.out)[(int64_t)m * p.o_ld + col] = (bf16_t)v;
  }
}

int dlw_cu_count() {
  static std::atomic<int> cached{0};
  int n = cached.load(std::memory_order_relaxed);
  if (n > 0) return n;
  int dev = 0;
  n = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    return 256;          // no device (host-side queries): an MI355X's count; not cached
  }
  cached.store(n, std::memory_order_relaxed);
  return n;
}

bool dlw_shape_ok(int32_t M, int64_t N, int64_t K, int32_t act) {
  if (M < 1 || M > DLW_MAX_M || N < 1 || K < 8 || K % 8 != 0) return false;
  if (act != 0 && act != 1) return false;
  if (act == 1 && N % 2 != 0) return false;
  if (N > ((int64_t)1 << 31) || K > ((int64_t)1 << 31)) return false;     // grid.x and the step arithmetic
  return true;
}

}  // namespace

extern "C" int cmb_decode_linear_wide_supported(int32_t M, int64_t N, int64_t K, int32_t act) {
  return dlw_shape_ok(M, N, K, act) ? 1 : 0;
}

extern "C" int cmb_decode_linear_wide_plan(int32_t M, int64_t N, int64_t K, int32_t act, int32_t cus, int32_t* rows_out,
                                           int64_t* wgs_out) {
  if (!dlw_shape_ok(M, N, K, act) || cus < 0) return CMB_ERR_BAD_ARG;
  const int q = dlw_plan_pairs(M, N, K, act, cus > 0 ? cus : dlw_cu_count());
  if (rows_out) *rows_out = DLW_PAIR_ROWS * q;
  if (wgs_out) *wgs_out = dlw_plan_wgs(q, N, act);
  return CMB_OK;
}

extern "C" int cmb_decode_linear_wide(const void* x, int64_t x_ld, int32_t M, const void* norm_w, float norm_eps,
                                      const void* W, int64_t w_ld, int64_t N, int64_t K, int32_t act, const void* residual,
                                      int64_t r_ld, void* out, int64_t o_ld, int32_t out_f32, void* stream) {
  if (!x || !W || !out || !dlw_shape_ok(M, N, K, act)) return CMB_ERR_BAD_ARG;
  if (act == 1 && residual) return CMB_ERR_BAD_ARG;
  if (out_f32 != 0 && out_f32 != 1) return CMB_ERR_BAD_ARG;
  const int64_t cols = act ? N / 2 : N;
  if (x_ld < K || x_ld % 8 || w_ld < K || w_ld % 8 || o_ld < cols || o_ld % 8) return CMB_ERR_BAD_ARG;
  if (residual && (r_ld < cols || r_ld % 8)) return CMB_ERR_BAD_ARG;
  if (!cmb_aligned16(x) || !cmb_aligned16(W) || !cmb_aligned16(out) || !cmb_aligned16(norm_w) || !cmb_aligned16(residual))
    return CMB_ERR_BAD_ARG;
  if (!(norm_eps >= 0.f)) return CMB_ERR_BAD_ARG;

  DlwParams p;
  p.x = (const bf16_t*)x; p.x_ld = x_ld; p.M = M;
  p.norm_w = (const bf16_t*)norm_w; p.eps = norm_eps;
  p.W = (const bf16_t*)W; p.w_ld = w_ld; p.N = N; p.K = K;
  p.act = act;
  p.res = (const bf16_t*)residual; p.r_ld = r_ld;
  p.out = out; p.o_ld = o_ld; p.out_f32 = out_f32;

  const int q = dlw_plan_pairs(M, N, K, act, dlw_cu_count());
  const int nb = dlw_blocks(M);
  const dim3 grid((unsigned)dlw_plan_wgs(q, N, act));
  hipStream_t st = (hipStream_t)stream;
#define DLW_LAUNCH(P, NB, NORM) hipLaunchKernelGGL((decode_linear_wide_kernel<P, NB, NORM>), grid, dim3(DLW_THREADS), 0, st, p)
#define DLW_BLOCKS(P, NORM)                    \
  do {                                         \
    if (nb == 1) DLW_LAUNCH(P, 1, NORM);       \
    else if (nb == 2) DLW_LAUNCH(P, 2, NORM);  \
    else if (nb == 3) DLW_LAUNCH(P, 3, NORM);  \
    else DLW_LAUNCH(P, 4, NORM);               \
  } while (0)
#define DLW_PAIRS(NORM)                        \
  do {                                         \
    if (q == 1) DLW_BLOCKS(1, NORM);           \
    else DLW_BLOCKS(2, NORM);                  \
  } while (0)
  if (norm_w) DLW_PAIRS(true); else DLW_PAIRS(false);
#undef DLW_PAIRS
#undef DLW_BLOCKS
#undef DLW_LAUNCH
  CMB_CHECK_LAUNCH();
  return CMB_OK;
}
