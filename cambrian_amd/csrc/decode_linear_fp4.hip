// decode_linear_fp4.hip — decode_linear.hip's contract on MXFP4 weights (4.25 bits per weight): out[M, N'] = epilogue(rstd? ·
// Σ_k prologue(x)[m, k] · e2m1(Wq[n, k]) · 2^(Ws[n, k / 32] − 127)) for 1 <= M <= 16 rows of bf16, Wq the packed OCP e2m1
// nibbles and Ws the e8m0 block scales that cmb_quantize_mxfp4_rows writes, fp32 accumulation.  A decode step is a read of
// the frozen weights and nothing else, so a quarter of the bf16 bytes is the lever; prologue (RMSNorm as two exact bf16
// operands), epilogue (SwiGLU over packed [gate; up] rows, bf16 residual, bf16 / fp32 store) and the statuses mean what
// they mean in decode_linear.hip and decode_linear_fp8.hip.  Roofline class: HBM (the weights; x stays in L2).
//
// Layout (decode_linear_fp4_layout.h has the maps and the plan; tests/csrc/decode_linear_fp4_layout_sim.cpp enumerates
// them).  A workgroup owns a slab of 8 T weight rows; its four waves take the 256-element k-steps round robin.  Weights go
// straight to VGPRs, 16 bytes = 32 k = one MX block per lane with non-temporal loads, a full 128-byte line per row and
// instruction, plus the block's one scale byte; two groups of U steps in flight per wave; no LDS staging.  An e2m1 value
// times a power of two is exactly a bf16 (while it lies in bf16's range: scale codes 1 .. 252 with every nibble, see
// below) and a product of two bf16 is exact in fp32, so the nibbles are converted in registers — v_cvt_scalef32_pk_bf16_fp4
// takes a byte's two nibbles and the scale as an fp32 power of two and gives the pair, low nibble in the low half (a run
// over every byte, byte position and scale codes 1 .. 254 settled that: the instruction agrees with the format, keeps
// bf16 subnormals and overflows to infinity) — and v_mfma_f32_16x16x32_bf16 runs as in the bf16 kernel: eight MFMAs per
// load (4 parts x 2 halves), sixteen with the norm.  There is no per-row factor: the scale is inside the operand, and
// the fp32 sum is the only rounding.  The eight partial tiles are summed through LDS in a fixed order by the thread that
// owns the output element.  No split of K across workgroups, no atomics, no flags: the same inputs give the same bits,
// and a row's bits do not depend on M or on the slab.
// This is NOT the block-scaled v_mfma_scale_f32_*_f8f6f4 path: that one needs quantised activations, x stays bf16 here.
#include "common.h"
#include "decode_linear_fp4_layout.h"

namespace {

#ifndef DL4_NORM4_U
#define DL4_NORM4_U 1    /* lab builds: make DEFS=-DDL4_NORM4_U=2 BUILD=build_lab LIB=libcambrian_amd_lab_u2.so */
#endif
constexpr int DL4_THREADS = 64 * DL_WAVES;
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

struct Dl4Params {
  const bf16_t* x;
  int64_t x_ld;
  int32_t M;
  const bf16_t* norm_w;
  float eps;
  const uint8_t* W;
  int64_t w_ld;
  const uint8_t* S;
  int64_t s_ld;
  int64_t N, K;
  int32_t act;
  const bf16_t* res;
  int64_t r_ld;
  void* out;
  int64_t o_ld;
  int32_t out_f32;
};

// the 8 bf16 of a 16-byte fragment as fp32 (element 2 d in the low half of dword d)
__device__ __forceinline__ void dl4_unpack(const u32x4_t& r, float (&v)[8]) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    v[2 * d] = __builtin_bit_cast(float, r[d] << 16);
    v[2 * d + 1] = __builtin_bit_cast(float, r[d] & 0xffff0000u);
  }
}

// one dword = 8 e2m1 nibbles (nibble i = element i) and the block's scale 2^(code - 127) as fp32 -> 8 bf16, exactly.
// The scale codes are 1 .. 254 (never 0 or 255, which have no fp32 power of two / are NaN): a fragment past K re-reads
// real bytes and is multiplied by zero, and every e2m1 code is finite, so nothing but the scale could bring in a NaN.
__device__ __forceinline__ bf16x8_t dl4_convert(uint32_t w, float scale) {
  const bf16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0);
  const bf16x2_t b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1);
  const bf16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2);
  const bf16x2_t d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3);
  const u32x4_t r = {__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b), __builtin_bit_cast(uint32_t, c),
                     __builtin_bit_cast(uint32_t, d)};
  return __builtin_bit_cast(bf16x8_t, r);
}

// Two workgroups per CU, except the 32-row slab with the norm: its two groups in flight (2 x (16 weight + 4 scale + 32 x +
// 32 norm registers)) with 32 accumulators, the converted fragments and the norm's temporaries do not fit 256 registers (116
// bytes of scratch per lane when forced to), so that instantiation runs one workgroup per CU and overflows into AGPRs.
// Running such a call as 16-row slabs instead (two workgroups per CU, no overflow) measured slower on Llama-3-8B's
// gate / up (profiles/decode_fp4.md), so the plan's 32 rows stand with the norm too.
template <int T, bool NORM>
__global__ void __launch_bounds__(DL4_THREADS, (T == 4 && NORM) ? 1 : 2) decode_linear_fp4_kernel(const Dl4Params p) {
  // k-steps per group: a step is 4 T registers of weights, T of scales and 32 of x (64 with the norm), two groups in flight
  // (T = 4 with the norm has a CU's registers to itself; two steps per group there overflow 194 registers into AGPRs and
  // measured slower than one, profiles/decode_fp4.md)
  constexpr int U = NORM ? (T == 4 ? DL4_NORM4_U : 1) : (T == 4 ? 1 : 2);
  constexpr int RED = 2 * DL_WAVES * T * DL_TILE_ROWS * DL_MAX_M;
  __shared__ float sm[RED + DL_WAVES * DL_MAX_M];      // partial tiles [wave][half][tile][row][m], then sums of squares [wave][m]

  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t K = p.K;
  const int64_t cols = p.act ? p.N / 2 : p.N;          // N'
  const int cols_wg = p.act ? DL_TILE_ROWS * T / 2 : DL_TILE_ROWS * T;
  const int64_t col0 = (int64_t)blockIdx.x * cols_wg;

  // ---- operand pointers: row starts; a row past the end re-reads the last one (its sums are never stored) ----
  const uint8_t* wrow[T];
  const uint8_t* srow[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int64_t n = dl4_slab_row(T, p.act, col0, t, lane, p.N);
    wrow[t] = p.W + n * p.w_ld;
    srow[t] = p.S + n * p.s_ld;
  }
  const int wk = dl4_w_k(lane);
  const int xm = dl_x_row(lane) < p.M ? dl_x_row(lane) : p.M - 1;
  const bf16_t* xrow = p.x + (int64_t)xm * p.x_ld;

  struct Frag {
    u32x4_t w[U][T], x[U][2][DL4_PARTS], n[U][2][DL4_PARTS];
    uint32_t s[U][T];        // the block's e8m0 code
    bool in[U][2];           // the x fragments of the half lie inside K (else they are taken as zero: the loads re-read k = 0)
  };
  // group g of the wave: its steps g U .. g U + U - 1.  A fragment past K (the ragged last step, or a whole group past the
  // wave's share) re-reads k = 0 and its x side is taken as zero in multiply: every load is issued whatever K is and
  // nothing branches around a load.  K % 32 == 0: a lane's 32 weight elements with their scale, and the four parts of x
  // that meet them, lie inside K together or not at all
  auto fetch = [&](Frag& f, int64_t g) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t k0 = ((g * U + u) * DL_WAVES + wave) * DL4_KSTEP;
      const int64_t kw = k0 + wk < K ? k0 + wk : 0;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        f.w[u][t] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wrow[t] + (kw >> 1)));
        f.s[u][t] = srow[t][dl4_scale_index(kw)];
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        int64_t kx = k0 + dl4_x_k(0, h, lane);
        f.in[u][h] = kx < K;
        kx = kx < K ? kx : 0;
#pragma unroll
        for (int pt = 0; pt < DL4_PARTS; ++pt) {
          const int64_t kp = kx + (dl4_x_k(pt, h, lane) - dl4_x_k(0, h, lane));
          f.x[u][h][pt] = *reinterpret_cast<const u32x4_t*>(xrow + kp);
          if (NORM) f.n[u][h][pt] = *reinterpret_cast<const u32x4_t*>(p.norm_w + kp);
        }
      }
    }
  };

  f32x4_t acc[2][T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[0][t] = acc[1][t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  float ss = 0.f;
  auto multiply = [&](const Frag& f) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float sc[T];
#pragma unroll
      for (int t = 0; t < T; ++t) sc[t] = __builtin_bit_cast(float, f.s[u][t] << 23);     // 2^(code - 127), codes 1 .. 254
#pragma unroll
      for (int pt = 0; pt < DL4_PARTS; ++pt) {
        bf16x8_t wb[T];
#pragma unroll
        for (int t = 0; t < T; ++t) wb[t] = dl4_convert(f.w[u][t][pt], sc[t]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          u32x4_t xr = f.x[u][h][pt];
#pragma unroll
          for (int d = 0; d < 4; ++d) xr[d] = f.in[u][h] ? xr[d] : 0u;
          u32x4_t xlo = {0u, 0u, 0u, 0u};
          if (NORM) {
            // x[k] norm_w[k] as two bf16 operands (its rounding and the exact remainder), as in decode_linear.hip
            float xv[8], nv[8], hv[8];
            dl4_unpack(xr, xv);
            dl4_unpack(f.n[u][h][pt], nv);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              ss = fmaf(xv[e], xv[e], ss);
              xv[e] *= nv[e];
            }
            xr = __builtin_bit_cast(u32x4_t, cvt8_bf16(xv[0], xv[1], xv[2], xv[3], xv[4], xv[5], xv[6], xv[7]));
            dl4_unpack(xr, hv);
#pragma unroll
            for (int e = 0; e < 8; ++e) xv[e] -= hv[e];
            xlo = __builtin_bit_cast(u32x4_t, cvt8_bf16(xv[0], xv[1], xv[2], xv[3], xv[4], xv[5], xv[6], xv[7]));
          }
          const bf16x8_t xb = __builtin_bit_cast(bf16x8_t, xr), xl = __builtin_bit_cast(bf16x8_t, xlo);
#pragma unroll
          for (int t = 0; t < T; ++t) {
            acc[h][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[t], xb, acc[h][t], 0, 0, 0);
            if (NORM) acc[h][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[t], xl, acc[h][t], 0, 0, 0);
          }
        }
      }
    }
  };

  // ---- the wave's steps wave, wave + 4, ...: groups of U, one being multiplied while the next one lands ----
  const int64_t nsteps = (K + DL4_KSTEP - 1) / DL4_KSTEP;
  const int64_t cnt = nsteps > wave ? (nsteps - wave + DL_WAVES - 1) / DL_WAVES : 0;
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
  {
    const int half = dl_acc_half(lane), m = lane & 15;
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = half ? acc[1][t][r] : acc[0][t][r];
        sm[(((wave * 2 + half) * T + t) * DL_TILE_ROWS + dl_acc_row(lane, r)) * DL_MAX_M + m] = v;
      }
    }
    if (NORM) {
      ss += __shfl_xor(ss, 16, 64);     // the four lanes of an x row: k quarters of every step
      ss += __shfl_xor(ss, 32, 64);
      if (lane < DL_MAX_M) sm[RED + wave * DL_MAX_M + lane] = ss;
    }
  }
  __syncthreads();

  // ---- epilogue: one thread per output element, partials added in (wave, half) order ----
  auto total = [&](int t, int r, int m) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < 2 * DL_WAVES; ++w) s += sm[((w * T + t) * DL_TILE_ROWS + r) * DL_MAX_M + m];
    return s;
  };
  for (int idx = threadIdx.x; idx < cols_wg * p.M; idx += DL4_THREADS) {
    const int m = idx / cols_wg, c = idx - m * cols_wg;
    const int64_t col = col0 + c;
    if (col >= cols) continue;
    float rstd = 1.f;
    if (NORM) {
      float s2 = 0.f;
#pragma unroll
      for (int w = 0; w < DL_WAVES; ++w) s2 += sm[RED + w * DL_MAX_M + m];
      rstd = __builtin_amdgcn_rsqf(s2 / (float)K + p.eps);
    }
    const int t = c / DL_TILE_ROWS, r = c % DL_TILE_ROWS;
    float v = total(t, r, m) * rstd;
    if (p.act) {
      const float up = total(t + T / 2, r, m) * rstd;
      v = v * cmb_sigmoid(v) * up;
    }
    if (p.res) v += (float)p.res[(int64_t)m * p.r_ld + col];
    if (p.out_f32) reinterpret_cast<float*>(p.out)[(int64_t)m * p.o_ld + col] = v;
    else reinterpret_cast<bf16_t*>(p.out)[(int64_t)m * p.o_ld + col] = (bf16_t)v;
  }
}

int dl4_cu_count() {
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

// dl_shape_ok of decode_linear.hip with K a multiple of 32 (a lane's 16 bytes = one MX block) in place of 8
bool dl4_shape_ok(int32_t M, int64_t N, int64_t K, int32_t act) {
  if (M < 1 || M > DL_MAX_M || N < 1 || K < DL4_BLOCK || K % DL4_BLOCK != 0) return false;
  if (act != 0 && act != 1) return false;
  if (act == 1 && N % 2 != 0) return false;
  if (N > ((int64_t)1 << 31) || K > ((int64_t)1 << 31)) return false;     // grid.x and the step arithmetic
  return true;
}

}  // namespace

extern "C" int cmb_decode_linear_fp4_supported(int32_t M, int64_t N, int64_t K, int32_t act) {
  return dl4_shape_ok(M, N, K, act) ? 1 : 0;
}

extern "C" int cmb_decode_linear_fp4_plan(int32_t M, int64_t N, int64_t K, int32_t act, int32_t cus, int32_t* rows_out,
                                          int64_t* wgs_out) {
  if (!dl4_shape_ok(M, N, K, act) || cus < 0) return CMB_ERR_BAD_ARG;
  const int t = dl4_plan_tiles(M, N, K, act, cus > 0 ? cus : dl4_cu_count());
  if (rows_out) *rows_out = DL_TILE_ROWS * t;
  if (wgs_out) *wgs_out = dl_plan_wgs(t, N, act);
  return CMB_OK;
}

extern "C" int cmb_decode_linear_fp4(const void* x, int64_t x_ld, int32_t M, const void* norm_w, float norm_eps,
                                     const void* Wq, int64_t w_ld, const void* Ws, int64_t s_ld, int64_t N, int64_t K,
                                     int32_t act, const void* residual, int64_t r_ld, void* out, int64_t o_ld, int32_t out_f32,
                                     void* stream) {
  if (!x || !Wq || !Ws || !out || !dl4_shape_ok(M, N, K, act)) return CMB_ERR_BAD_ARG;
  if (act == 1 && residual) return CMB_ERR_BAD_ARG;
  if (out_f32 != 0 && out_f32 != 1) return CMB_ERR_BAD_ARG;
  const int64_t cols = act ? N / 2 : N;
  if (x_ld < K || x_ld % 8 || w_ld < K / 2 || w_ld % 16 || s_ld < K / DL4_BLOCK || o_ld < cols || o_ld % 8) return CMB_ERR_BAD_ARG;
  if (residual && (r_ld < cols || r_ld % 8)) return CMB_ERR_BAD_ARG;
  if (!cmb_aligned16(x) || !cmb_aligned16(Wq) || !cmb_aligned16(out) || !cmb_aligned16(norm_w) || !cmb_aligned16(residual))
    return CMB_ERR_BAD_ARG;
  if (!(norm_eps >= 0.f)) return CMB_ERR_BAD_ARG;

  Dl4Params p;
  p.x = (const bf16_t*)x; p.x_ld = x_ld; p.M = M;
  p.norm_w = (const bf16_t*)norm_w; p.eps = norm_eps;
  p.W = (const uint8_t*)Wq; p.w_ld = w_ld; p.S = (const uint8_t*)Ws; p.s_ld = s_ld; p.N = N; p.K = K;
  p.act = act;
  p.res = (const bf16_t*)residual; p.r_ld = r_ld;
  p.out = out; p.o_ld = o_ld; p.out_f32 = out_f32;

  const int t = dl4_plan_tiles(M, N, K, act, dl4_cu_count());
  const dim3 grid((unsigned)dl_plan_wgs(t, N, act));
  hipStream_t st = (hipStream_t)stream;
#define DL4_LAUNCH(T, NORM) hipLaunchKernelGGL((decode_linear_fp4_kernel<T, NORM>), grid, dim3(DL4_THREADS), 0, st, p)
#define DL4_TILES(NORM)                      \
  do {                                       \
    if (t == 1) DL4_LAUNCH(1, NORM);         \
    else if (t == 2) DL4_LAUNCH(2, NORM);    \
    else DL4_LAUNCH(4, NORM);                \
  } while (0)
  if (norm_w) DL4_TILES(true); else DL4_TILES(false);
#undef DL4_TILES
#undef DL4_LAUNCH
  CMB_CHECK_LAUNCH();
  return CMB_OK;
}
