// mxfp4.hip — OCP microscaling FP4 (MXFP4) quantisation of matrix rows: e2m1 values, two to a byte, with one shared e8m0
// power-of-two scale per block of 32 elements (4.25 bits per element).  Feeds cmb_decode_linear_fp4.  HBM-bound and run
// once per frozen weight: reads each element once (2 or 4 bytes), writes half a byte + 1/32 byte.
//
// Streaming: one thread owns one block of 32 — it loads the block, takes the block's amax, derives the scale and packs
// the 16 bytes — so no row is held in registers and K has no upper reach (any multiple of 32).  Per block:
//   amax = max |x|;  e = clamp(floor(log2 amax) - 2, -126, 127);  scale code = e + 127  (a zero block: code 127, zero nibbles)
//   nibble = e2m1(|x| * 2^-e) rounded to the grid {0, .5, 1, 1.5, 2, 3, 4, 6} to nearest, ties to the even code, saturating
//   at 6 (a block whose amax lies in (6, 8) * 2^e clamps: the OCP rule), sign in bit 3.
// floor(log2 amax) is the exponent field of the fp32 (a subnormal amax lands on the clamp), the scaling by 2^-e is an exact
// fp32 product, and the rounding is seven comparisons, so the result is a pure function of the input's bits; codes stay in
// 1 .. 252.  Inputs are finite.
#include "common.h"
#include "launch.h"

namespace {

constexpr int MX_THREADS = 256;
constexpr int MX_BLOCK = 32;

// |v| on the e2m1 grid: code 0 .. 7 = 0, .5, 1, 1.5, 2, 3, 4, 6; a tie goes to the even code
__device__ __forceinline__ uint32_t mx_e2m1(float v) {
  return (uint32_t)(v > 0.25f) + (uint32_t)(v >= 0.75f) + (uint32_t)(v > 1.25f) + (uint32_t)(v >= 1.75f) +
         (uint32_t)(v > 2.5f) + (uint32_t)(v >= 3.5f) + (uint32_t)(v > 5.0f);
}

template <typename T>
__global__ __launch_bounds__(MX_THREADS) void quantize_mxfp4_rows_kernel(const T* __restrict__ x, int64_t ldx, int64_t rows,
                                                                         int64_t nblk, uint8_t* __restrict__ q, int64_t ldq,
                                                                         uint8_t* __restrict__ scales, int64_t lds) {
  const int64_t i = (int64_t)blockIdx.x * MX_THREADS + threadIdx.x;
  if (i >= rows * nblk) return;
  const int64_t row = i / nblk, b = i - row * nblk;
  const T* xp = x + row * ldx + b * MX_BLOCK;
  float v[MX_BLOCK];
#pragma unroll
  for (int j = 0; j < MX_BLOCK / 8; ++j) {
    float t[8];
    Vec8<T>::load(xp + 8 * j, t);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[8 * j + e] = t[e];
  }
  uint32_t amax = 0;          // as bits: for finite values the order of the magnitudes
#pragma unroll
  for (int j = 0; j < MX_BLOCK; ++j) {
    const uint32_t a = __builtin_bit_cast(uint32_t, v[j]) & 0x7fffffffu;
    amax = a > amax ? a : amax;
  }
  int e = (int)(amax >> 23) - 127 - 2;
  e = e < -126 ? -126 : e;                                     // (the upper clamp, 127, is out of an fp32's reach)
  if (amax == 0) e = 0;
  const float inv = __builtin_bit_cast(float, (uint32_t)(127 - e) << 23);      // 2^-e
  uint32_t w[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    uint32_t pack = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float f = v[8 * d + j];
      const uint32_t sign = (__builtin_bit_cast(uint32_t, f) >> 31) << 3;
      const uint32_t code = mx_e2m1(fabsf(f) * inv);
      pack |= ((code ? sign : 0u) | code) << (4 * j);          // -0 is written as +0
    }
    w[d] = pack;
  }
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  *reinterpret_cast<u32x4*>(q + row * ldq + b * (MX_BLOCK / 2)) = u32x4{w[0], w[1], w[2], w[3]};
  scales[row * lds + b] = (uint8_t)(e + 127);
}

}  // namespace

extern "C" int cmb_quantize_mxfp4_rows(int dtype, const void* x, int64_t ldx, int64_t rows, int64_t K, void* q, int64_t ldq,
                                       void* scales, int64_t lds, void* stream) {
  if (rows == 0) return CMB_OK;
  if (!x || !q || !scales || rows < 0 || K <= 0) return CMB_ERR_BAD_ARG;
  if (dtype != CMB_BF16 && dtype != CMB_F32) return CMB_ERR_BAD_ARG;
  if (K % MX_BLOCK != 0 || ldx < K || ldq < K / 2 || ldq % 16 != 0 || lds < K / MX_BLOCK) return CMB_ERR_SHAPE;
  const int64_t nblk = K / MX_BLOCK;
  if (rows > ((int64_t)1 << 31) || nblk > ((int64_t)1 << 31) || rows * nblk > (((int64_t)1 << 31) - 1) * MX_THREADS) return CMB_ERR_SHAPE;
  const int64_t es = dtype == CMB_BF16 ? 2 : 4;
  if (!cmb_aligned16(x) || !cmb_aligned16(q) || (ldx * es) % 16 != 0) return CMB_ERR_ALIGNMENT;
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)((rows * nblk + MX_THREADS - 1) / MX_THREADS);
  DT_SWITCH(dtype, hipLaunchKernelGGL(quantize_mxfp4_rows_kernel<T>, dim3(grid), dim3(MX_THREADS), 0, s, (const T*)x, ldx, rows,
                                      nblk, (uint8_t*)q, ldq, (uint8_t*)scales, lds));
  CMB_CHECK_LAUNCH();
  return CMB_OK;
}
