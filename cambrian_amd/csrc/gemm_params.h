// gemm_params.h — the parameter block every GEMM kernel takes by value, and its filling from a cmb_gemm_desc.
// No HIP include (gemm_plan.h and its CPU simulation read the same struct the kernels do).
#pragma once
#include "rowmap.h"

namespace cmb_gemm_detail {

struct GemmParams {
  int M, N, K;
  const char* A; RowMap a_map;
  const char* B; int64_t ldb;
  char* C; RowMap c_map;
  const float* bias;
  const float* colscale;
  const char* R; RowMap r_map;
  char* P; RowMap p_map;
  int act;
  float alpha, beta;
  int out_f32;
  int tiles_m, tiles_n;
  int k_per_split;
  float* slabs;
  const float* a_scale;  // fp8 operands: per-row dequantisation factors (nullptr otherwise)
  const float* b_scale;
  int batch;                 // > 1: blockIdx.z walks independent problems of the same shape (128 x 128 kernel only)
  int64_t a_bs, b_bs, c_bs;  // element strides of A / B / C between consecutive problems of a batch
  int slab_rows;             // rows of one split-K slab (= M; batch * M for cmb_gemm_tn's batched split-K)
  const float* row_mean;     // LayerNorm folded into this linear (cmb_gemm_desc.row_mean): v = rstd[m] (acc - mean[m] colsum[n]) + bias[n]
  const float* row_rstd;
  const float* col_sum;
};

// descriptor -> parameter block, field for field: one whole-K launch, no slabs (gemm_attach_slabs adds split-K), no fp8
// scales (cmb_gemm's fp8 path adds them).  The entry points' own checks come before / after.
inline void gemm_fill_params(const cmb_gemm_desc* d, GemmParams& p) {
  p.M = (int)d->M; p.N = (int)d->N; p.K = (int)d->K;
  p.A = (const char*)d->A; p.a_map = make_rowmap(d->a_map);
  p.B = (const char*)d->B; p.ldb = d->ldb;
  p.C = (char*)d->C; p.c_map = make_rowmap(d->c_map);
  p.bias = d->bias; p.colscale = d->colscale;
  p.R = (const char*)d->residual; p.r_map = make_rowmap(d->r_map);
  p.P = (char*)d->pre_out; p.p_map = make_rowmap(d->p_map);
  p.act = d->act; p.alpha = d->alpha; p.beta = d->beta;
  p.out_f32 = (d->out_dtype == CMB_F32);
  p.tiles_m = p.tiles_n = 0;
  p.slabs = nullptr;
  p.k_per_split = p.K;
  p.a_scale = nullptr; p.b_scale = nullptr;
  p.batch = d->batch > 1 ? d->batch : 1;
  p.a_bs = d->a_batch_stride; p.b_bs = d->b_batch_stride; p.c_bs = d->c_batch_stride;
  p.slab_rows = p.M;
  p.row_mean = d->row_mean; p.row_rstd = d->row_rstd; p.col_sum = d->col_sum;
}

}  // namespace cmb_gemm_detail
