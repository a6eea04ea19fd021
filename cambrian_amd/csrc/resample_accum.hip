// resample_accum.hip — cmb_resample_accum: out = act(base + bias + sum_s bilinear_s(src_s)).
//
// The tail of a linear whose input is a channel concatenation of bilinearly resized maps (the ConvNeXt aux projector): the
// resize acts on positions and the linear on channels, so a map with fewer positions than the output grid is projected at
// its own resolution and only the N-wide partial product is resized.  This kernel resizes up to four such partial products,
// adds them in list order onto the product of the maps that were resized first (`base`), adds the bias, and applies the
// activation — the epilogue the GEMMs could not run because their sum was not complete.
//
// One thread per (output cell, 8 channels), grid-stride, 16-byte accesses (fp32: two per vector).  HBM-bound: base is read
// once, pre_out and out are written once; the sources are 2.25x / 9x smaller than the output at the release grids and every
// source row is read by the (Ho / Hi)^2 neighbouring cells that share it, i.e. from L2.  The sum is fp32 in a fixed order
// and rounded once: no atomics, bit-reproducible.  The per-cell arithmetic is resample_core.h (host + device), run on the
// CPU by tests/csrc/resample_accum_sim.cpp.
#include "common.h"
#include "resample_core.h"

namespace {

struct AccumSrcs {
  const void* p[CMB_RESAMPLE_ACCUM_MAX_SRC];
  int64_t ld[CMB_RESAMPLE_ACCUM_MAX_SRC], bs[CMB_RESAMPLE_ACCUM_MAX_SRC];
  int32_t Hi[CMB_RESAMPLE_ACCUM_MAX_SRC], Wi[CMB_RESAMPLE_ACCUM_MAX_SRC];
  int32_t n;
};

// TO: element type of out / pre_out; TS: element type of base and the sources (fp32 partial products under a bf16 output
// stay unrounded until the one rounding here).  GELU: the bf16 GEMM epilogues' cmb_gelu_erf_bf16_x8 for a bf16 output, the
// fp32 kernels' act_apply for an fp32 one — equal pre-activations give the activations a fused GEMM would have given.
template <typename TO, typename TS, bool GELU>
__global__ void __launch_bounds__(256) resample_accum_kernel(const AccumSrcs srcs, const TS* __restrict__ base,
                                                             int64_t ld_base, int64_t bs_base,
                                                             const float* __restrict__ bias, int64_t B, int Ho, int Wo,
                                                             int C, TO* __restrict__ pre_out, int64_t ld_pre,
                                                             int64_t bs_pre, TO* __restrict__ out, int64_t ld_out,
                                                             int64_t bs_out) {
  const int nv = C >> 3;
  const int64_t total = B * Ho * Wo * (int64_t)nv;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t b;
    int oy, ox, cv;
    cmb_resample_accum_decode(i, nv, Ho, Wo, b, oy, ox, cv);
    const int64_t cell = (int64_t)oy * Wo + ox;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (base) Vec8<TS>::load(base + b * bs_base + cell * ld_base + cv * 8, acc);
    if (bias) {
      float bv[8];
      load8f(bias + cv * 8, bv);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += bv[e];
    }
    cmb_resample_accum_cell(oy, ox, Ho, Wo, srcs.n, srcs.Hi, srcs.Wi,
                            [&](int s, int64_t row, float (&v)[8]) {
                              Vec8<TS>::load(reinterpret_cast<const TS*>(srcs.p[s]) + b * srcs.bs[s] + row * srcs.ld[s] + cv * 8, v);
                            },
                            acc);
    if (pre_out) Vec8<TO>::store(pre_out + b * bs_pre + cell * ld_pre + cv * 8, acc);
    if (GELU) {
      if (sizeof(TO) == 2) {
        cmb_gelu_erf_bf16_x8(acc);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = act_apply(CMB_ACT_GELU_ERF, acc[e]);
      }
    }
    Vec8<TO>::store(out + b * bs_out + cell * ld_out + cv * 8, acc);
  }
}

template <typename TO, typename TS>
int launch(const cmb_resample_accum_desc* d, const AccumSrcs& srcs, hipStream_t s) {
  const int64_t total = d->B * d->Ho * d->Wo * (d->C / 8);
  int64_t blocks = (total + 255) / 256;
  if (blocks > 32768) blocks = 32768;
#define CMB_ACCUM_LAUNCH(G)                                                                                                \
  hipLaunchKernelGGL((resample_accum_kernel<TO, TS, G>), dim3((unsigned)blocks), dim3(256), 0, s, srcs, (const TS*)d->base, \
                     d->ld_base, d->batch_stride_base, d->bias, d->B, d->Ho, d->Wo, (int)d->C, (TO*)d->pre_out, d->ld_pre,  \
                     d->batch_stride_pre, (TO*)d->out, d->ld_out, d->batch_stride_out)
  if (d->act == CMB_ACT_GELU_ERF) CMB_ACCUM_LAUNCH(true);
  else CMB_ACCUM_LAUNCH(false);
#undef CMB_ACCUM_LAUNCH
  CMB_CHECK_LAUNCH();
  return CMB_OK;
}

}  // namespace

extern "C" int cmb_resample_accum(const cmb_resample_accum_desc* d, void* stream) {
  if (!d || !d->out || d->B < 0 || d->Ho <= 0 || d->Wo <= 0 || d->C <= 0 || (d->C & 7)) return CMB_ERR_BAD_ARG;
  if (d->n_src < 0 || d->n_src > CMB_RESAMPLE_ACCUM_MAX_SRC || (d->n_src == 0 && !d->base)) return CMB_ERR_BAD_ARG;
  if (d->act != CMB_ACT_NONE && d->act != CMB_ACT_GELU_ERF) return CMB_ERR_BAD_ARG;
  // (out, base / sources): bf16 | bf16, fp32 | fp32, and fp32 partial products under a bf16 output
  const bool pair_ok = (d->dtype == CMB_BF16 && (d->src_dtype == CMB_BF16 || d->src_dtype == CMB_F32)) ||
                       (d->dtype == CMB_F32 && d->src_dtype == CMB_F32);
  if (!pair_ok) return CMB_ERR_BAD_ARG;
  if ((d->ld_out & 7) || (d->batch_stride_out & 7) || d->ld_out < d->C) return CMB_ERR_BAD_ARG;
  if (d->pre_out && ((d->ld_pre & 7) || (d->batch_stride_pre & 7) || d->ld_pre < d->C)) return CMB_ERR_BAD_ARG;
  if (d->base && ((d->ld_base & 7) || (d->batch_stride_base & 7) || d->ld_base < d->C)) return CMB_ERR_BAD_ARG;
  AccumSrcs srcs = {};
  srcs.n = d->n_src;
  for (int s = 0; s < d->n_src; ++s) {
    if (!d->src[s] || d->Hi[s] <= 0 || d->Wi[s] <= 0 || (d->ld_src[s] & 7) || (d->batch_stride_src[s] & 7) ||
        d->ld_src[s] < d->C)
      return CMB_ERR_BAD_ARG;
    srcs.p[s] = d->src[s];
    srcs.ld[s] = d->ld_src[s];
    srcs.bs[s] = d->batch_stride_src[s];
    srcs.Hi[s] = d->Hi[s];
    srcs.Wi[s] = d->Wi[s];
  }
  if (!cmb_aligned16(d->out) || !cmb_aligned16(d->pre_out) || !cmb_aligned16(d->base) || !cmb_aligned16(d->bias))
    return CMB_ERR_ALIGNMENT;
  for (int s = 0; s < d->n_src; ++s)
    if (!cmb_aligned16(d->src[s])) return CMB_ERR_ALIGNMENT;
  if (d->B == 0) return CMB_OK;
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == CMB_BF16 && d->src_dtype == CMB_BF16) return launch<bf16_t, bf16_t>(d, srcs, st);
  if (d->dtype == CMB_BF16) return launch<bf16_t, float>(d, srcs, st);
  return launch<float, float>(d, srcs, st);
}
