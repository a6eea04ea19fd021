/*
 * cambrian_amd.h — C-ABI of the MI355X (gfx950) kernel library behind Cambrian-1's
 * vision-tower + Spatial-Vision-Aggregator (SVA) hot path.
 *
 * The reference (cambrian-mllm/cambrian) is 100 % Python and has no FFI of its own
 * (SURVEY.md §8b); every entry point below therefore cites the *library call site* in the
 * reference that it replaces (file:line relative to the reference repo root).  The Python
 * host side (cambrian_amd/ops.py) binds these symbols with ctypes and wraps them in
 * torch.autograd.Function objects; INTEGRATION.md shows the binding a reference maintainer
 * would add.
 *
 * Conventions
 *   - plain C: pointers, sizes, scalars, POD structs.  No torch / C++ types.
 *   - every buffer is caller-owned device memory (HBM) valid on the given stream.
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream).
 *   - every function returns 0 (CMB_OK) or a negative cmb_status; nothing throws, nothing
 *     synchronises the host, nothing allocates.
 *   - dtype codes: CMB_BF16 = 0 (bf16 storage, fp32 accumulate), CMB_F32 = 1 (exact fp32
 *     path on v_mfma_f32_32x32x2_f32; used by the parity tests).
 *   - "rowmap": a logical row index r of a [rows, cols] matrix is mapped to an element
 *     offset  (r / n1) * s0 + ((r % n1) / n2) * s1 + (r % n2) * s2 ; n1 == 0 means the
 *     plain row-major case r * s2.  This is how the window re-arrangement
 *     (cambrian_arch.py:271-287) and the in-LLM slice hidden[:, 91:691] viewed as
 *     [B,24,25,H][:, :, :24] (cambrian_llama.py:181-207) are folded into the consumer's
 *     loads instead of being materialised.
 */
#ifndef CAMBRIAN_AMD_H
#define CAMBRIAN_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum cmb_status {
  CMB_OK = 0,
  CMB_ERR_BAD_ARG = -1,      /* null pointer, negative size, unsupported combination */
  CMB_ERR_ALIGNMENT = -2,    /* pointer / leading dimension not 16-byte aligned */
  CMB_ERR_SHAPE = -3,        /* K not a multiple of the K-step, N not a multiple of 8, ... */
  CMB_ERR_WORKSPACE = -4,    /* workspace too small */
  CMB_ERR_LAUNCH = -5        /* hipLaunchKernel / hipFuncSetAttribute failed */
} cmb_status;

enum { CMB_BF16 = 0, CMB_F32 = 1 };
/* 8-bit operands of cmb_gemm (OCP e4m3fn, gfx950's native fp8; BASELINE configs[4] "fp8 MFMA projection GEMMs"):
 * A / B are uint8 [rows, K] produced by cmb_quantize_fp8_rows, C / residual / pre_out are bf16 (or fp32 C). */
enum { CMB_FP8_E4M3 = 3 };
enum { CMB_ACT_NONE = 0, CMB_ACT_GELU_ERF = 1, CMB_ACT_GELU_TANH = 2, CMB_ACT_QUICK_GELU = 3,
       CMB_ACT_SILU = 4,
       /* cmb_gemm only: the gated activation of a packed (gate | up) projection whose weight rows are INTERLEAVED (row 2j =
        * gate_j, row 2j + 1 = up_j): C[m, j] = silu(v[m, 2j]) * v[m, 2j + 1] with v = alpha * acc + bias — C has N / 2
        * columns (HF Dinov2SwiGLUFFN reached from dino_encoder.py:159: weights_in + silu(x1) * x2 in one launch, the
        * [M, N] intermediate never written).  N % 16 == 0; no colscale / residual / pre_out / split-K / fp32 C. */
       CMB_ACT_SWIGLU_PAIRS = 5 };

typedef struct cmb_rowmap {
  int64_t n1, n2;      /* n1 == 0: identity (offset = r * s2) */
  int64_t s0, s1, s2;  /* element strides */
} cmb_rowmap;

/* library / build identification ("cambrian_amd <version> gfx950"). */
const char* cmb_version(void);
/* ABI revision: bumped whenever an entry point's signature or a descriptor's layout changes (round 2's key_valid
 * arguments = 2, round 3's fold_kv workspace = 3, the batch fields of cmb_gemm_desc = 4,
 * the kernel-selection knobs of round 4 = 5, cmb_layernorm_fwd_multi = 9, cmb_ln_multi_desc.dx_out = 10, the workspaces of
 * the deterministic column sums = 11, cmb_decode_attn and its plan / workspace queries = 12,
 * cmb_resample_bilinear_bwd = 13).  cmb_resample_accum and its descriptor, and later the optimizer entry points
 * (cmb_optim_chunks, cmb_grad_sqnorm, cmb_grad_sqnorm_workspace, cmb_adamw_step), and after them the decode-step linear
 * (cmb_decode_linear, cmb_decode_linear_supported, cmb_decode_linear_plan) and its 1-byte-weight form
 * (cmb_decode_linear_fp8, cmb_decode_linear_fp8_supported, cmb_decode_linear_fp8_plan), and then the one-call decode step
 * (cmb_decode_step, cmb_decode_step_ws, cmb_decode_next and the two descriptors), and then the sampled selection
 * (cmb_decode_sample), and then beam search (cmb_decode_beam, cmb_decode_beam_state_bytes, cmb_decode_beam_reorder), and then the MXFP4
 * decode-step linear (cmb_quantize_mxfp4_rows, cmb_decode_linear_fp4, cmb_decode_linear_fp4_supported,
 * cmb_decode_linear_fp4_plan, and the value 2 of cmb_decode_step_desc.fp8), and then the e4m3 K / V cache of the decode steps
 * (cmb_kv_quantize_e4m3, cmb_decode_attn_kv8, cmb_decode_step_kv8 and cmb_decode_kv8_factors), and then the multi-token
 * decode attention of prompt-lookup decoding (cmb_decode_attn_multi, cmb_decode_attn_multi_ws, cmb_decode_attn_multi_plan), and then the decode-step linear for up to
 * 64 rows (cmb_decode_linear_wide, cmb_decode_linear_wide_supported, cmb_decode_linear_wide_plan), and then the logits
 * processors of generate() (cmb_decode_process), and then chunk attention on the K / V cache (cmb_extend_attn,
 * cmb_extend_attn_ws, cmb_extend_attn_plan) were
 * ADDED under revision 13: no existing
 * signature or layout changed, which is the rule for a bump, so a binding written against 13 still calls everything it
 * knows correctly.  Bindings must compare it
 * with the revision they
 * were written against (CMB_ABI_VERSION; cambrian_amd/lib.py::load raises on a mismatch): every symbol of a stale
 * library still resolves, and a shifted argument list corrupts memory instead of failing. */
#define CMB_ABI_VERSION 13
int cmb_abi_version(void);

/* Run-time kernel-selection knobs: which of several kernels that compute the SAME function an entry point launches
 * (value 0 = the earlier kernel, kept for A/B runs; CMB_KNOB_DEFAULTS = what the library uses unless told otherwise).
 * Meant for same-process A/B measurements (tools/r04_lab.py, bench.py's `ab` block) and start-up calibration; none
 * changes an entry point's contract.  Not thread-safe against concurrent launches: set between steps.
 *   CMB_KNOB_LN_FWD     cmb_layernorm_fwd, affine rows without a position table: 0 = one row per wave at a time,
 *                       parameters re-read per row (rounds 1-3); 1 = parameters staged in LDS + next row prefetched,
 *                       rows / 16 workgroups up to 8192; > 1 = the same with that workgroup cap
 *   CMB_KNOB_DWCONV     cmb_dwconv7x7_nhwc (C % 64 == 0): 0 = LDS-tiled kernel (rounds 1-3); 1 = column-walking kernel with
 *                       register-resident taps, 64 rows per chunk for maps of >= 128 rows, else 32; > 1 = that many rows per chunk
 *   CMB_KNOB_VIT_ATTN   cmb_vit_attn_fwd (bf16): 0 = two barriers per key tile (round 3); 1 = two LDS tile buffers, one barrier
 *                       (both: register-staged K / V tiles, bit-identical); 2 = round 6: K / V tiles by LDS-DMA into swizzled
 *                       images, V by transposing reads, lazy rescale, XCD-grouped 1-D grid, 128 queries per workgroup; 3 = the
 *                       same with 256 queries per workgroup (2 / 3 agree with 0 / 1 to bf16 rounding, not bit for bit)
 *   CMB_KNOB_SVA_ABS    cmb_sva_abs_fwd / _bwd on bf16 operands: 0 = the MFMA kernels; 1 = the exact (plain fp32 arithmetic)
 *                       instantiation of the same algorithm that dtype CMB_F32 always runs (tests: one against the other)
 *   CMB_KNOB_LN_MULTI_CHUNK  cmb_layernorm_bwd_multi: layers per launch, 4 ... 7 (4, 5: two waves per SIMD; 6, 7: one).  13 layers of the
 *                       9216-token tower at 24 images: 4: 4684 us, 5: 4463, 6: 6431, 7: 6455 (profiles/r06_lab.md)
 *   CMB_KNOB_FLASH      cmb_flash_attn_fwd / _bwd, bit mask: 1 = forward, 2 = dQ on LDS-DMA operand tiles with transposing reads
 *                       (flash2.hip); 4 = the round-4 dK/dV kernel with the round-5 four-phase tile body; 16 = that kernel reading its
 *                       Q^T / dO^T fragments with transposing reads from swizzled row-major images (no transposed copies); 0 = the
 *                       round-4 kernels.  Default 23.  (Bit 8 selected a dK/dV kernel on LDS-DMA tiles that measured slower —
 *                       profiles/r05_lab.md — and was removed in round 6: values with it are rejected.)  dQ / dK / dV are
 *                       bit-identical across variants, the forward to fp32 rounding (tests/test_flash_bwd_gpu.py)
 *   CMB_KNOB_COLSUM_WGS cmb_colsum / cmb_colsum_scaled: 0 = 256 rows per workgroup whatever the input (rounds 1-5); n > 0 = rows per
 *                       workgroup chosen so that the launch has about n workgroups (16 ... 256 rows; same sums up to the order of
 *                       the fp32 atomics, which was never fixed; default 768: 13 824 x 1024 24 -> 14 us, scaled 42 -> 17 us)
 *   CMB_KNOB_LN_BWD_ROWS cmb_layernorm_bwd on inputs of < 65 536 rows per window position: rows per workgroup (4 ... 256; 16 = rounds
 *                       3-5, default 32: 13 824 x 1024 51 -> 39 us) — fewer workgroups = fewer end-of-block atomics on the parameter gradients, more = more rows in flight */
enum cmb_knob_id { CMB_KNOB_LN_FWD = 0, CMB_KNOB_DWCONV = 1, CMB_KNOB_VIT_ATTN = 2, CMB_KNOB_SVA_ABS = 3, CMB_KNOB_LN_MULTI_CHUNK = 4,
                   CMB_KNOB_FLASH = 5, CMB_KNOB_COLSUM_WGS = 6, CMB_KNOB_LN_BWD_ROWS = 7, CMB_KNOB_COUNT = 8 };
#define CMB_KNOB_DEFAULTS 1, 1, 2, 0, 5, 23, 768, 32
int cmb_knob_set(int32_t knob, int32_t value);   /* CMB_ERR_BAD_ARG for an unknown knob */
int cmb_knob_get(int32_t knob);                  /* -1 for an unknown knob */

/* ------------------------------------------------------------------------------------------
 * GEMM   C[M,N] = epilogue( alpha * A[M,K] · B[N,K]^T )            (nn.Linear layout)
 * replaces: every torch.nn.Linear / F.linear on the path —
 *   vision_sampler.py:170-175,187-189,232,240-245,254-255 (SVA projections),
 *   cambrian_arch.py:49,56,375,411 (mm_projector_aux_i / mm_projector),
 *   HF CLIPVisionModel / Dinov2Model / timm ViT + ConvNeXt linears reached from
 *   clip_encoder.py:104, siglip_encoder.py:97, dino_encoder.py:159, clip_convnext_encoder.py:133-136.
 * epilogue order:  v = alpha*acc + bias[n];  pre_out = v;  v = act(v);  v *= colscale[n];
 *                  v += residual[m,n];  v += beta*C_old[m,n] (fp32 C only);  C = v
 * requirements: K % (128 / sizeof(elem)) == 0; N % 8 == 0; 16-byte aligned rows.
 * dtype CMB_FP8_E4M3: v_mfma_f32_32x32x64_f8f6f4 (K = 64 per instruction, twice the bf16 MFMA rate), 128x128 tile,
 *   no split-K; see a_scale / b_scale.
 * two tile configurations: 128x128 / 4 waves, and for bf16 256x256 / 8 waves with the
 *   8-phase LDS-DMA schedule or the persistent 4-wave kernel; `tile_hint` = 0 lets the library pick (grid-fill cost model,
 *   per-shape policy, tail split: cambrian_amd/csrc/gemm_plan.h holds every rule).
 * split_k > 1: fp32 partial slabs go to `workspace` (split_k*M*N*4 bytes) and are reduced by a
 *   second kernel; only alpha/beta and out_dtype apply (used for weight gradients).
 * ---------------------------------------------------------------------------------------- */
typedef struct cmb_gemm_desc {
  int32_t dtype;       /* CMB_BF16 | CMB_F32 : element type of A, B, residual, pre_out */
  int32_t out_dtype;   /* CMB_BF16 | CMB_F32 : element type of C (bf16 requires dtype bf16) */
  int64_t M, N, K;
  const void* A;  cmb_rowmap a_map;
  const void* B;  int64_t ldb;
  void* C;        cmb_rowmap c_map;
  const float* bias;       /* [N] fp32 or NULL */
  const float* colscale;   /* [N] fp32 or NULL (LayerScale) */
  const void* residual; cmb_rowmap r_map;  /* NULL or [M,N] of `dtype` */
  void* pre_out;        cmb_rowmap p_map;  /* NULL or [M,N] of `dtype`: pre-activation copy */
  int32_t act;
  float alpha, beta;
  int32_t split_k;
  void* workspace; int64_t workspace_bytes;
  int32_t tile_hint;       /* 0 = choose by grid-fill cost model; 128 / 256 = force that block tile (bf16 only);
                              2560 / 2561 = 256 tile with schedule 0 (8-phase ping-pong, default) / 1 (in-wave pipeline);
                              2590 = 4-wave register-buffered 256x256 kernel (what 0 / 256 pick when N % 128 == 0, there is no
                              pre_out, the launch has at least 64 tiles and every K slice holds two 64-deep tiles; K slices
                              shorter than that run on the 8-wave kernel even under 2590).  0 also consults the per-shape policy
                              (cmb_gemm_policy_set), and only 0 allows the M <= 32 kernel and the tail split */
  const float* a_scale;    /* CMB_FP8_E4M3 only: [M] fp32 dequantisation factor of each A row (or NULL = 1) */
  const float* b_scale;    /* CMB_FP8_E4M3 only: [N] fp32 dequantisation factor of each B row (or NULL = 1);
                              the accumulator is multiplied by a_scale[m] * b_scale[n] before alpha / bias */
  int32_t batch;           /* > 1: `batch` independent problems of this shape in one launch (the sixteen per-head GEMMs of
                              the absorbed SVA projections, vision_sampler.py:187-189 restated per head): problem z uses
                              A + z * a_batch_stride, B + z * b_batch_stride, C + z * c_batch_stride (elements; 16-byte
                              multiples).  bf16 / fp32, 128x128 tile, no bias / colscale / pre_out / split-K; a residual (operand dtype)
                              is laid out as C: problem z adds residual + z * c_batch_stride through r_map */
  int64_t a_batch_stride, b_batch_stride, c_batch_stride;
  /* LayerNorm folded into the linear that follows it (round 6; the frozen towers' LN -> qkv / fc1 pairs: HF / timm blocks behind
   * clip_encoder.py:104, siglip_encoder.py:97, dino_encoder.py:159, clip_convnext_encoder.py:133-136):
   *   LN(x) W^T + b  =  rstd[m] * ( x W'^T - mean[m] * col_sum[n] ) + b'[n],   W' = W diag(gamma) (as stored in B),
   *   col_sum[n] = sum_k B[n,k] (of the stored, rounded values),  b' = b + W beta  (passed as `bias`)
   * so the GEMM reads the UN-normalised rows and cmb_row_stats replaces the LayerNorm kernel (no normalised copy is written).
   * With row_mean set the epilogue starts  v = row_rstd[m] * (acc - row_mean[m] * col_sum[n]) + bias[n]  (alpha must be 1,
   * bias / row_rstd / col_sum non-NULL; bf16 operands; no split-K, batch, fp8 scales); act, colscale, residual follow as usual. */
  const float* row_mean;   /* [M] fp32 or NULL */
  const float* row_rstd;   /* [M] fp32 */
  const float* col_sum;    /* [N] fp32 */
} cmb_gemm_desc;

int cmb_gemm(const cmb_gemm_desc* d, void* stream);
/* Two INDEPENDENT bf16 products in one call (round 6): the same results as cmb_gemm(d0) followed by cmb_gemm(d1), bit for bit.
 * When both would run on the persistent 256 x 256 kernel with their whole K, the same `act`, no batch / split_k / pre_out /
 * tile_hint / folded LayerNorm, and whole-round arithmetic says it pays, they leave as ONE launch whose workgroups are split
 * between the two problems — the frozen ViT towers' same-position linears (DINOv2 17520 x 1536 x {1536, 4096} beside SigLIP
 * 17496 x 1152 x {1152, 4352} at 24 images: 1.62 and 1.35 rounds of 256 workgroups each, 3.0 + 2.9 rounds on 138 + 118 side by
 * side; HF / timm blocks behind dino_encoder.py:156-165, siglip_encoder.py:95-99, towers independent: cambrian_arch.py:271-278).
 * Otherwise the two calls are made one after the other.  cmb_gemm_pair_last() = 1 if the calling thread's last cmb_gemm_pair
 * took the one-launch path.  CMB_GEMM_PAIR=0 in the environment forces two launches (A/B runs). */
int cmb_gemm_pair(const cmb_gemm_desc* d0, const cmb_gemm_desc* d1, void* stream);
int cmb_gemm_pair_last(void);
/* C[M,N] = alpha * At[K,M]^T * Bt[K,N] (+ beta * C): the weight-gradient product dW = g^T x of every trainable linear of
 * the path (autograd's addmm on a transposed view in the reference: the SVA projections vision_sampler.py:159-189, the
 * projectors cambrian_arch.py:49-56), with BOTH operands row-major over the contraction rows as the activations lie in
 * memory — no transposed copies.  Same descriptor as cmb_gemm, read as: A = At (row stride a_map.s2, a_map.n1 == 0),
 * B = Bt (row stride ldb), K = contraction rows (any count: rows beyond K contribute zero), M, N multiples of 8;
 * dtype CMB_BF16, out_dtype CMB_F32 | CMB_BF16; split_k / workspace and batch / *_batch_stride as cmb_gemm (both together
 * when the batch's results are contiguous: c_batch_stride == M * N, row stride N; workspace split_k * batch * M * N * 4 bytes);
 * bias, colscale, residual, pre_out, act must be unset.  cmb_gemm_last_kernel() reports 1281. */
int cmb_gemm_tn(const cmb_gemm_desc* d, void* stream);
/* Row-wise fp8 quantisation for cmb_gemm(CMB_FP8_E4M3): for every row r of x [rows, K] (dtype CMB_BF16 | CMB_F32, row
 * stride ldx elements):  amax = max|x[r,:]|;  s = 448 / amax (1 if amax == 0);
 * q[r,k] = e4m3fn_rne(clamp(x[r,k] * s, -448, 448));  inv_scale[r] = amax / 448 (1 if amax == 0).
 * One pass over x (a row lives in registers between the reduction and the cast).  K % 16 == 0, ldq % 16 == 0. */
int cmb_quantize_fp8_rows(int dtype, const void* x, int64_t ldx, int64_t rows, int64_t K, void* q, int64_t ldq,
                          float* inv_scale, void* stream);
/* block tile (128 or 256) cmb_gemm would run for this problem — lets the caller label profiles / rooflines per
 * kernel configuration.  dtype CMB_F32 always answers 128. */
int cmb_gemm_tile(int dtype, int64_t M, int64_t N, int32_t split_k, int32_t tile_hint);
/* which kernel the calling thread's most recent cmb_gemm launched (0 before the first): 128 = 128x128 tile kernel,
 * 256 = 8-wave 256x256 kernel (gemm256.hip), 2590 = 4-wave register-buffered 256x256 kernel (gemm_nt_p5_kernel,
 * gemm_p5.hip), 1281 = cmb_gemm_tn's 128x128 kernel (gemm_tn.hip), 64 = the batched K = 64 kernel (gemm_k64.hip), 32 = the
 * M <= 32 kernel (gemm_smallm.hip).  For labelling profiles and rooflines per kernel. */
int cmb_gemm_last_kernel(void);
/* Per-shape dispatch policy: bf16 launches of exactly (M, N, K, act) without a tile_hint and without split-K take
 * `kernel` (128 | 2560 = 8-wave 256x256 | 2590 = 4-wave 256x256; 0 removes the entry) instead of the built-in cost
 * model (a 256-tile entry still yields to the checks of the kernel it names: row strides beyond the 32-bit tile span run on
 * the 128 tile, K < 128 on the 8-wave kernel; problems that take the M <= 32 kernel or the tail split never reach the policy).  Meant for a
 * start-up calibration on the device at hand (the candidates give bit-identical results; which is
 * faster for a shape varies from box to box — VERDICT r2 #4).  At most 64 entries (CMB_ERR_WORKSPACE beyond); not
 * thread-safe against concurrent cmb_gemm calls: set it between steps. */
int cmb_gemm_policy_set(int64_t M, int64_t N, int64_t K, int32_t act, int32_t kernel);
/* Tail split of bf16 launches without tile_hint / split-K (gemm_plan.h "tail split"): when an M x N problem's 256 x 256 tile
 * count is a little more than a whole number of rounds of the device's CUs, rows [0, m1) run on the 256-tile kernel and
 * rows [m1, M) on the 128 x 128 kernel, two launches inside one cmb_gemm call.  Returns m1 (0 = launched whole).
 * CMB_GEMM_NO_TAIL_SPLIT=1 in the environment disables it (A/B runs). */
int64_t cmb_gemm_tail_rows(int64_t M, int64_t N);
int cmb_gemm_policy_clear(void);

/* out[C, R_pad] = in[R, C]^T, zero-filling columns R..R_pad-1 (R_pad >= R). Used to put the
 * reduction dimension innermost for weight-gradient GEMMs (autograd of the linears above). */
int cmb_transpose(int dtype, const void* in, int64_t R, int64_t C, int64_t ld_in,
                  void* out, int64_t R_pad, void* stream);

/* out[c] (fp32) += sum_r in[r, c]   — bias gradients (caller zero-fills).  Deterministic: every workgroup writes its partial
 * row into `workspace` (fp32, at least cmb_colsum_workspace(R, C) floats, else CMB_ERR_WORKSPACE) and the rows are added
 * to out in a fixed order — the same bits on every run (float atomics added them in completion order). */
int64_t cmb_colsum_workspace(int64_t R, int64_t C);
int cmb_colsum(int dtype, const void* in, int64_t R, int64_t C, int64_t ld_in,
               float* out, float* workspace, int64_t workspace_floats, void* stream);
/* out[c] += sum_r row_scale[r * ld_scale + c / group] * in[r, c]  (fp32 accumulation; out must be zero-filled by the caller;
 * group % 8 == 0, C % group == 0).  The bias gradients of the absorbed SVA projections: d b_k[c] = sum_q d(cb)[q, h(c)] q[q, c],
 * d b_v[c] = sum_q m3[q, h(c)] d out[q, c] with group = 64 = one head (vision_sampler.py:187-189's k_proj / v_proj biases,
 * restated per head: DESIGN.md section 4.5) — one pass over the rows instead of a broadcast product + reduction.  Workspace
 * and fixed summation order as cmb_colsum. */
int cmb_colsum_scaled(int dtype, const void* in, int64_t R, int64_t C, int64_t ld_in, const float* row_scale,
                      int64_t ld_scale, int32_t group, float* out, float* workspace, int64_t workspace_floats, void* stream);

/* y = (T)x elementwise casts between fp32 and bf16 (n elements). to_dtype/from_dtype are CMB_*. */
int cmb_cast(int from_dtype, const void* in, int to_dtype, void* out, int64_t n, void* stream);

/* Weight preparation: bf16 copy [rows, cols] (dst, row stride cols) and transposed bf16 copy [cols, rows_pad] (dst_t, zero
 * columns rows .. rows_pad - 1) of a 2-D weight (fp32 master or bf16; row stride ld_src) — what the linears of
 * vision_sampler.py:170-175,254-259 and cambrian_arch.py:49-56 need per step in bf16 compute: W for y = x W^T, W^T for
 * dx = g W.  cmb_weight_prep takes a table of jobs in DEVICE memory (tile0 = prefix sum of cmb_weight_prep_tiles over the
 * jobs before it) and covers every job in ONE launch; cmb_weight_prep_one takes one job by value (host memory).  Either
 * output pointer may be NULL.  cols, rows_pad, ld_src multiples of 8; 16-byte aligned pointers. */
typedef struct cmb_prep_job {
  const void* src;
  void* dst;
  void* dst_t;
  int64_t ld_src;
  int32_t src_dtype; /* CMB_F32 | CMB_BF16 */
  int32_t rows, cols, rows_pad;
  int32_t tile0;
  int32_t reserved;
} cmb_prep_job;
int64_t cmb_weight_prep_tiles(int64_t rows_pad, int64_t cols);
int cmb_weight_prep_one(const cmb_prep_job* job, void* stream);
int cmb_weight_prep(const cmb_prep_job* jobs_device, int32_t n_jobs, int64_t total_tiles, void* stream);

/* Row statistics of a LayerNorm without its output: mean[r], rstd[r] = 1 / sqrt(var + eps) of x [rows, D] (row stride ldx),
 * the two-pass fp32 arithmetic of cmb_layernorm_fwd — the operands of cmb_gemm_desc.row_mean / row_rstd.  D % 8 == 0, D <= 4096. */
int cmb_row_stats(int dtype, const void* x, int64_t rows, int64_t D, int64_t ldx, float eps, float* mean, float* rstd, void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm   y[r,:] = (x[r,:] (+ add[pos(r),:]) - mean) * rstd (* gamma + beta)
 * replaces: nn.LayerNorm at vision_sampler.py:170,173-174,261 and cambrian_arch.py:56, the
 *   pos_embed add at vision_sampler.py:304-309, and the HF/timm LayerNorms of the towers.
 * add: optional [grid_r*grid_r, D] fp32 table (SVA pos_embed_i); the row -> table-row map is
 *   the window-local position of token r on a square side×side token grid:
 *   pos = ((r % (side*side)) / side % grid_r) * grid_r + (r % side) % grid_r.
 * gamma/beta may be NULL (pure normalisation: the SVA path folds the K- and V-LayerNorm affines
 *   into the projection weights so that one normalised tensor serves both).
 * mean/rstd: optional fp32 [rows] outputs for the backward.
 * ---------------------------------------------------------------------------------------- */
int cmb_layernorm_fwd(int dtype, const void* x, int64_t rows, int64_t D, int64_t ldx,
                      const float* add, int32_t side, int32_t grid_r,
                      const float* gamma, const float* beta, float eps,
                      void* y, int64_t ldy, float* mean, float* rstd, void* stream);

/* dx (+)= LN backward.  dy: [rows,D]; xhat is recomputed from x (+add), mean, rstd.
 * dx_accumulate != 0: dx += result (gradient accumulation across the 13 SVA layers that share
 * the aux features, SURVEY.md §7 "hard parts").  dgamma/dbeta/dadd are fp32 and are
 * *accumulated into*, caller zero-fills; any may be NULL (dgamma / dbeta need gamma, dadd needs add).  Every workgroup
 * writes its partial rows into `workspace` (fp32): cmb_layernorm_bwd_workspace(rows, D, grid_r) floats (grid_r = 1 without
 * add) per wanted output, else CMB_ERR_WORKSPACE; they are added in a fixed order — the same bits on every run. */
int64_t cmb_layernorm_bwd_workspace(int64_t rows, int64_t D, int32_t grid_r);
int cmb_layernorm_bwd(int dtype, const void* dy, int64_t lddy, const void* x, int64_t ldx,
                      int64_t rows, int64_t D,
                      const float* add, int32_t side, int32_t grid_r,
                      const float* gamma, const float* mean, const float* rstd,
                      void* dx, int64_t lddx, int32_t dx_accumulate,
                      float* dgamma, float* dbeta, float* dadd, float* workspace, int64_t workspace_floats,
                      void* stream);

/* Backward of SEVERAL non-affine LayerNorms of one input in one pass (the 13 SVA layers each normalise the same aux feature
 * tensor with their own position table: vision_sampler.py:304-309 reached 13 times per step, cambrian_llama.py:168-207):
 *   dx[r,:] (+)= sum_l  rstd_l[r] * ( dy_l[r,:] - mean(dy_l[r,:]) - xh_l[r,:] * mean(dy_l[r,:] * xh_l[r,:]) ),
 *   xh_l[r,:] = (x[r,:] + add_l[pos(r),:] - mean_l[r]) * rstd_l[r],      dadd_l[pos,:] += the layer's term summed over rows
 * with mean_l / rstd_l as cmb_layernorm_fwd returned them (add = add_l, no gamma / beta) and pos(r) the window position
 * of row r on a side x side grid in grid_r x grid_r windows (as cmb_layernorm_fwd).  x is read once, every dy_l once
 * (dense rows: leading dimension D), dx (fp32, leading dimension lddx) is written once (`accumulate` != 0: added to).
 * add[l] may be NULL (no table for that layer; then dadd[l] is ignored); dadd[l] may be NULL (gradient not wanted);
 * caller zero-fills dadd.  layers <= CMB_LN_MULTI_MAX (run as launches of up to 7 layers: x is read once per launch),
 * D <= 1024. */
#define CMB_LN_MULTI_MAX 16
typedef struct cmb_ln_multi_desc {
  int32_t dtype;          /* CMB_BF16 | CMB_F32: element type of x and dy_l */
  int32_t layers;
  const void* x;  int64_t ldx;
  int64_t rows, D;
  int32_t side, grid_r;
  const void* dy[CMB_LN_MULTI_MAX];
  const float* add[CMB_LN_MULTI_MAX];
  const float* mean[CMB_LN_MULTI_MAX];
  const float* rstd[CMB_LN_MULTI_MAX];
  float* dadd[CMB_LN_MULTI_MAX];
  float* dx;      int64_t lddx;
  int32_t accumulate;
  int32_t reserved;
  void* dx_out;           /* optional (round 6): the call's LAST launch writes the finished sum here in x's dtype (dense rows,
                           * leading dimension D) instead of updating dx — the cast of the fp32 accumulator at the end of the
                           * deferred backward; dx then holds the sum without the last launch's layers */
  float* workspace;       /* fp32 partial rows of the dadd sums (added in a fixed order: the same bits on every run), */
  int64_t workspace_floats;   /* at least cmb_layernorm_bwd_multi_workspace(d) floats, else CMB_ERR_WORKSPACE */
} cmb_ln_multi_desc;
int64_t cmb_layernorm_bwd_multi_workspace(const cmb_ln_multi_desc* d);
int cmb_layernorm_bwd_multi(const cmb_ln_multi_desc* d, void* stream);

/* Forward of SEVERAL non-affine LayerNorms of one input in one pass (round 6): y_l[r,:] = normalise(x[r,:] + add_l[pos(r),:]),
 * l < layers — the 13 SVA layers' normalisations of the windowed tower's tokens (vision_sampler.py:304-309 reached 13 times per
 * step on the SAME aux features; only the position table differs).  x is read once instead of `layers` times: 2 + 2 layers
 * instead of 4 layers bytes per element.  Every y_l / mean_l / rstd_l equals, bit for bit, what cmb_layernorm_fwd(add = add_l,
 * gamma = beta = NULL) returns.  add[l] may be NULL; y_l dense rows (leading dimension D); mean[l] / rstd[l] fp32 [rows],
 * required.  layers <= CMB_LN_MULTI_MAX, D <= 1024 (D % 8 == 0). */
typedef struct cmb_ln_fwd_multi_desc {
  int32_t dtype;          /* CMB_BF16 | CMB_F32: element type of x and y_l */
  int32_t layers;
  const void* x;  int64_t ldx;
  int64_t rows, D;
  int32_t side, grid_r;
  float eps;  int32_t reserved;
  const float* add[CMB_LN_MULTI_MAX];
  void* y[CMB_LN_MULTI_MAX];
  float* mean[CMB_LN_MULTI_MAX];
  float* rstd[CMB_LN_MULTI_MAX];
} cmb_ln_fwd_multi_desc;
int cmb_layernorm_fwd_multi(const cmb_ln_fwd_multi_desc* d, void* stream);

/* RMSNorm: y = (x * rsqrt(mean(x^2)+eps)) * w, fp32 math, weight multiplied BEFORE the down-cast
 * (the reference's patched LlamaRMSNorm: train_fsdp.py:1429-1438; phi3/modeling_phi3.py:83-97). */
int cmb_rmsnorm_fwd(int dtype, const void* x, int64_t rows, int64_t D, const float* w, float eps,
                    void* y, float* rstd, void* stream);
int cmb_rmsnorm_bwd(int dtype, const void* dy, const void* x, int64_t rows, int64_t D,
                    const float* w, const float* rstd, void* dx, float* dw, void* stream);

/* Fused residual add + RMSNorm of the decoder layer ("h = h + attn(...); x = post_attention_layernorm(h)"):
 * sum = x + res (stored in the compute dtype), y = rmsnorm(sum) * w, one pass; rstd fp32 [rows] for the backward. */
int cmb_add_rmsnorm_fwd(int dtype, const void* x, const void* res, int64_t rows, int64_t D, const float* w, float eps,
                        void* sum, void* y, float* rstd, void* stream);
/* dx = rmsnorm_backward(dy; x, w, rstd) + dadd (dadd may be NULL), single pass, frozen weight (no dw): the gradient of
 * the residual stream and of the normalised branch leave as one tensor. */
int cmb_rmsnorm_bwd_add(int dtype, const void* dy, const void* x, const void* dadd, int64_t rows, int64_t D,
                        const float* w, const float* rstd, void* dx, void* stream);

/* RoPE (rotate-half form): x[t,h,:] = x*cos + rotate_half(x)*sin with
 * cos/sin = cos/sin(position_ids[t] * base^(-2i/Dh)) evaluated in fp32
 * (phi3/modeling_phi3.py:114-141,257-281 and the HF Llama equivalent).
 * cmb_rope_table builds the [ntok, Dh/2] fp32 tables once per forward; cmb_rope_apply rotates
 * x [ntok, H, Dh] (token stride row_stride elements) in place; inverse != 0 applies the transposed
 * rotation (the backward). */
int cmb_rope_table(const int64_t* position_ids, int64_t ntok, int64_t Dh, float base,
                   float* cos_t, float* sin_t, void* stream);
int cmb_rope_apply(int dtype, void* x, const float* cos_t, const float* sin_t, int64_t ntok,
                   int64_t H, int64_t Dh, int64_t row_stride, int32_t inverse, void* stream);

/* ------------------------------------------------------------------------------------------
 * SVA windowed cross-attention core  (vision_sampler.py:193-230, F.scaled_dot_product_attention
 * at :215-220, with the window partition of cambrian_arch.py:271-287 done by index arithmetic).
 *   q   : [Bq, heads*hd]            Bq = B * qside*qside queries, one query row each
 *   kv_i: [B * (qside*r_i)^2, 2*heads*hd]  tower-token-major (NOT window-rearranged);
 *         K = columns [0, heads*hd), V = columns [heads*hd, 2*heads*hd)
 *   mask_i: uint8 [Bq, r_i*r_i] (1 = may attend), may be NULL (= all ones)
 *   out : [Bq, heads*hd];  lse: fp32 [Bq, heads] (log-sum-exp of the scaled scores)
 * query (b, qy, qx) attends, for every tower i, to tokens ((qy*r_i+ry)*qside*r_i + qx*r_i+rx).
 * Softmax in fp32 over the concatenation of all towers' keys, scale = 1/sqrt(hd).
 * ---------------------------------------------------------------------------------------- */
#define CMB_SVA_MAX_TOWERS 8
typedef struct cmb_sva_desc {
  int32_t dtype;
  int32_t B, qside, heads, hd, ntowers;
  int32_t window_major;  /* 0: kv_i tower-token-major (below); 1: kv_i is [Bq, r_i*r_i, 2*heads*hd] */
  int32_t r[CMB_SVA_MAX_TOWERS];
  const void* q;   int64_t ldq;
  const void* kv[CMB_SVA_MAX_TOWERS]; int64_t ldkv[CMB_SVA_MAX_TOWERS];
  const uint8_t* mask[CMB_SVA_MAX_TOWERS];
  void* out;       int64_t ldo;
  float* lse;
  /* backward only */
  const void* dout; int64_t lddo;
  void* dq;         int64_t lddq;
  void* dkv[CMB_SVA_MAX_TOWERS];   /* same layout as kv; every element written exactly once */
} cmb_sva_desc;

int cmb_sva_attn_fwd(const cmb_sva_desc* d, void* stream);
int cmb_sva_attn_bwd(const cmb_sva_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * SVA cross-attention core with ONE windowed tower's K / V projections absorbed into the query side
 * (same reference lines as above: vision_sampler.py:187-230; heads = 16, hd = 64, feature width 1024; bf16 on the MFMA, or
 * fp32 through an exact instantiation of the same algorithm — `dtype`).
 * Every token of an s x s-window tower is seen by exactly one query, so instead of projecting K and V per token
 * (kv_i above) the caller supplies, for that tower,
 *   xhat : [B * (qside*ra)^2, 1024]  the LayerNorm-normalised tokens (affines folded into W_k, W_v, b_k, b_v)
 *   U    : [Bq, 16, 1024]            U[q,h,:] = W_k,h^T q_h           (cmb_gemm, batch = 16, K = 64)
 *   bk, bv : fp32 [1024]             the folded K / V biases: the kernel forms cb[q,h] = b_k,h . q_h itself
 * and receives, besides the joint-softmax probabilities P (fp32 [Bq, 16, 20]: columns [0, 4) the direct towers' keys,
 * [4, 20) the absorbed tower's window tokens, zero where absent or masked; saved for the backward),
 *   out  : [Bq, 1024]   sum over the DIRECT towers' keys of p * V, plus m3[q,h] b_v,h   (kv / mask / r as in cmb_sva_desc; r_i == 1)
 *   xbar : [Bq, 16, 1024]  Xb[q,h,:] = sum_t p[q,h,t] xhat_t     -> the layer's attention output is out + W_v,h Xb
 *   m3   : fp32 [Bq, 16]   sum_t p[q,h,t] over the absorbed tower's tokens (kept by the caller: d b_v = sum_q m3 d out)
 * with score[q,h,t] = (xhat_t . U[q,h,:] + cb[q,h]) / sqrt(hd) for the absorbed tokens and q_h . K_h / sqrt(hd) for the
 * direct ones.  The backward takes d(out), d(xbar) and writes dq (the direct towers' part and d(cb) b_k), dkv of the direct
 * towers, dU, d(cb) (fp32 [Bq, 16]: d b_k = sum_q d(cb) q) and d(xhat) (every element exactly once).  Neither K|V nor
 * dK|dV of the absorbed tower exist.
 * ---------------------------------------------------------------------------------------- */
typedef struct cmb_sva_abs_desc {
  int32_t B, qside, heads, hd;
  int32_t ntowers;       /* directly projected towers (may be 0), each with r_i == 1 */
  int32_t window_major;  /* layout of xhat: 0 tower-token-major, 1 [Bq, ra*ra, 1024] */
  int32_t r[CMB_SVA_MAX_TOWERS];
  const void* q;   int64_t ldq;
  const void* kv[CMB_SVA_MAX_TOWERS]; int64_t ldkv[CMB_SVA_MAX_TOWERS];
  const uint8_t* mask[CMB_SVA_MAX_TOWERS];
  int32_t ra;            /* window side of the absorbed tower, ra*ra <= 16 */
  int32_t dtype;         /* CMB_BF16 (= 0: the MFMA kernels) | CMB_F32 (the exact instantiation of the same algorithm: plain fp32
                            arithmetic, test speed): element type of q, kv, xhat, U, out, xbar and of every gradient */
  const void* xhat; int64_t ldx;
  const uint8_t* mask_a; /* uint8 [Bq, ra*ra] or NULL */
  const void* U;
  const float* bk;
  void* out;       int64_t ldo;
  void* xbar;
  float* m3;
  float* P;
  /* backward only */
  const void* dout; int64_t lddo;
  const void* dxbar;
  const float* bv;       /* (forward AND backward: see bk, bv above) */
  void* dq;         int64_t lddq;
  void* dkv[CMB_SVA_MAX_TOWERS];
  void* dU;
  float* dcb;
  void* dxhat;      int64_t lddx;
} cmb_sva_abs_desc;

int cmb_sva_abs_fwd(const cmb_sva_abs_desc* d, void* stream);
int cmb_sva_abs_bwd(const cmb_sva_abs_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Embedding merge (static layout): cambrian_arch.py:413-420 (newline column) + :457-490.
 *   out[b,t,:] = feat[b, i*side+j, :]   if t = p_b + i*(side+1) + j, j < side
 *              = newline[:]             if t = p_b + i*(side+1) + side
 *              = table[ids'[b,t], :]    otherwise (ids' = ids with image_token -> 0)
 * p_b = first index with ids[b,t] == image_token (rows without one are pure text).
 * Copies only: bit-exact.  `pos` (int32 [B]) receives p_b (or -1).
 * ---------------------------------------------------------------------------------------- */
int cmb_embed_splice_fwd(int dtype, const int64_t* ids, int64_t B, int64_t S, int64_t H,
                         int64_t image_token, const void* table, int64_t vocab,
                         const void* feat, int32_t side, const void* newline,
                         void* out, int32_t* pos, void* stream);
/* dfeat[b,i*side+j,:] = dout[b, p_b+i*(side+1)+j, :];  dnewline (fp32 [H], accumulated) +=
 * sum_{b,i} dout[b, p_b+i*(side+1)+side, :], summed in a fixed order through `workspace` (fp32, B * side * H floats when
 * dnewline is not NULL, else CMB_ERR_WORKSPACE). */
int cmb_embed_splice_bwd(int dtype, const void* dout, const int32_t* pos, int64_t B, int64_t S,
                         int64_t H, int32_t side, void* dfeat, float* dnewline, float* workspace,
                         int64_t workspace_floats, void* stream);

/* K|V weight folding of one tower of one SVA layer (vision_sampler.py:173-174,188-189: k_proj_i / v_proj_i = LayerNorm ->
 * Linear; the two LayerNorms share their statistics, so their affines are folded into one projection):
 *   w_out[n,:] = W[n,:] * gamma,  b_out[n] = W[n,:] . beta;  rows 0..H-1 from (wk, gk, bk), rows H..2H-1 from (wv, gv, bv).
 * All fp32 (master parameters); wk / wv [H, K] row-major, K % 4 == 0.  bwd: given d(w_out) [2H, K] and d(b_out) [2H]
 * writes dW = dw * gamma + db (x) beta, dgamma = colsum(dw o W), dbeta = W^T db for both halves.  Deterministic (two
 * passes through a caller-owned workspace of cmb_sva_fold_kv_bwd_workspace(H, K) bytes; CMB_ERR_WORKSPACE if smaller). */
int cmb_sva_fold_kv_fwd(const float* wk, const float* gk, const float* bk, const float* wv, const float* gv, const float* bv,
                        int64_t H, int64_t K, float* w_out, float* b_out, void* stream);
int cmb_sva_fold_kv_bwd(const float* dw_out, const float* db_out, const float* wk, const float* gk, const float* bk,
                        const float* wv, const float* gv, const float* bv, int64_t H, int64_t K, float* dwk, float* dgk,
                        float* dbk, float* dwv, float* dgv, float* dbv, void* workspace, int64_t workspace_bytes,
                        void* stream);
int64_t cmb_sva_fold_kv_bwd_workspace(int64_t H, int64_t K);

/* mean over tokens: out[b,:] = mean_t x[b,t,:]  (cambrian_arch.py:377); bwd broadcasts. */
int cmb_token_mean_fwd(int dtype, const void* x, int64_t B, int64_t T, int64_t D, void* out,
                       void* stream);
/* acc[b,t,:] (fp32) += g[b,:] / T  — backward of the mean, into the fp32 aux-feature accumulator. */
int cmb_token_mean_bwd(int dtype, const void* g, int64_t B, int64_t T, int64_t D, float* acc,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * Vision-tower kernels (frozen towers: forward only; SURVEY.md §8a T1–T4)
 * ---------------------------------------------------------------------------------------- */
/* Non-causal multi-head self-attention over packed QKV rows (HF CLIPAttention / Dinov2 /
 * timm Attention reached from clip_encoder.py:104, dino_encoder.py:159, siglip_encoder.py:97).
 * qkv: [B*N, 3*heads*hd] with q|k|v column blocks; out: [B*N, heads*hd]. hd in {64, 96}
 * (SigLIP's 72 is zero-padded to 96 by the weight packer). scale is applied to the scores.
 * bf16 with hd in {64,96} runs the MFMA flash kernel; fp32 (and force_simple != 0) runs the
 * one-wave-per-query VALU kernel used as the exact-fp32 parity path. */
int cmb_vit_attn_fwd(int dtype, const void* qkv, int64_t B, int64_t N, int32_t heads, int32_t hd,
                     float scale, void* out, int32_t force_simple, void* stream);

/* Patch gather for a stride==kernel conv (ViT patch-embed 14x14/14, ConvNeXt stem 4x4/4):
 * img NCHW [B,C,H,W] (fp32 or bf16) -> cols [B*(H/p)*(W/p), Kpad], column order (c, dy, dx),
 * zero padded to Kpad. */
int cmb_patchify_nchw(int in_dtype, const void* img, int64_t B, int64_t C, int64_t H, int64_t W,
                      int32_t p, int out_dtype, void* cols, int64_t Kpad, void* stream);
/* 2x2/2 patch gather on an NHWC map (ConvNeXt downsample): x [B,H,W,C] -> [B*(H/2)*(W/2), 4C],
 * column order (dy, dx, c). */
int cmb_patchify2x2_nhwc(int dtype, const void* x, int64_t B, int64_t H, int64_t W, int64_t C,
                         void* cols, void* stream);
/* Depthwise 7x7, pad 3, NHWC (timm ConvNeXtBlock.conv_dw): w [49, C] fp32 (tap-major), bias [C]. */
int cmb_dwconv7x7_nhwc(int dtype, const void* x, int64_t B, int64_t H, int64_t W, int64_t C,
                       const float* w, const float* bias, void* y, void* stream);
/* Weight gradient of that depthwise 7x7 (towers that train): every one of `slots` workgroup rows
 * writes the partial sum over the 8x8 tiles it walked to partial[slot][49][C] (fp32); the caller column-sums the slots
 * (cmb_colsum on [slots, 49*C]).  dX of the same layer is cmb_dwconv7x7_nhwc on dY with the taps reversed and a zero
 * bias; d(bias) is a column sum of dY.  C % 64 == 0. */
int cmb_dwconv7x7_wgrad(int dtype, const void* x, const void* dy, int64_t B, int64_t H, int64_t W, int64_t C,
                        float* partial, int32_t slots, void* stream);
/* Bilinear resample (align_corners=False, fp32 lerp) of a token grid, channels-last:
 * in [B, Hi*Wi, C] (row stride ld_in) -> out [B, Ho*Wo, ...] written at column offset into rows
 * of stride ld_out (so the 4 ConvNeXt stage maps land in one [B,9216,5760] buffer).
 * replaces F.interpolate at clip_encoder.py:83-88, siglip_encoder.py:80-85, dino_encoder.py:141-146,
 * clip_convnext_encoder.py:112-118 and the permutes around them. */
int cmb_resample_bilinear(int dtype, const void* in, int64_t B, int32_t Hi, int32_t Wi, int64_t C,
                          int64_t ld_in, int64_t batch_stride_in, void* out, int32_t Ho, int32_t Wo,
                          int64_t ld_out, int64_t batch_stride_out, void* stream);
/* Exact adjoint of cmb_resample_bilinear (towers that train, the S5 query-group resize): dout [B, Ho*Wo, ...] read at the
 * pointer given with row stride ld_dout (a column slice of the concatenated gradient is read in place) -> din [B, Hi*Wi, C],
 * written in full: a cell no output refers to gets an exact 0, nothing is accumulated into and no memset is needed.  Gather
 * form, one thread per (input cell, 8 channels), fp32 sum in a fixed order (oy, then ox, ascending), rounded once: no
 * atomics, bit-reproducible, and the weights are the forward's own (csrc/resample_core.h).  Replaces ATen's
 * upsample_bilinear2d_backward and the fp32 NCHW copies around it. */
int cmb_resample_bilinear_bwd(int dtype, const void* dout, int64_t B, int32_t Ho, int32_t Wo, int64_t C,
                              int64_t ld_dout, int64_t batch_stride_dout, void* din, int32_t Hi, int32_t Wi,
                              int64_t ld_din, int64_t batch_stride_din, void* stream);
/* Sum of bilinearly resized maps onto a base, bias and activation in one pass (resample_accum.hip):
 *     pre[b, o, c] = base[b, o, c] (0 if base == NULL) + bias[c] (0 if NULL) + sum_s lerp_s(src_s)[b, o, c],  s in list order
 *     out[b, o, c] = act(pre),  act = CMB_ACT_NONE | CMB_ACT_GELU_ERF (the GEMM epilogues' own GELU)
 * over the Ho x Wo output grid, channels-last.  Source s is [B, Hi[s]*Wi[s], C] with row stride ld_src[s] and batch stride
 * batch_stride_src[s] (elements) and is resized with the arithmetic of cmb_resample_bilinear (align_corners=False, fp32
 * lerp).  base, pre_out (optional) and out are [B, Ho*Wo, C] with their own row / batch strides, so column slices of wider
 * buffers work in place.  `dtype` is the element type of out and pre_out, `src_dtype` that of base and the sources: equal,
 * or CMB_F32 under a CMB_BF16 `dtype` (partial products kept unrounded).  fp32 sum in the stated order, rounded once; no
 * atomics, bit-reproducible.  n_src <= CMB_RESAMPLE_ACCUM_MAX_SRC (n_src == 0 needs a base); C and every stride % 8 == 0
 * (CMB_ERR_BAD_ARG), every pointer 16-byte aligned (CMB_ERR_ALIGNMENT); all checks run before any launch.
 * Use: a linear over channel-concatenated resized maps, with the maps that have fewer positions than the output projected
 * at their own resolution (src_s = X_s W_s^T); d(src_s) = cmb_resample_bilinear_bwd of d(pre). */
#define CMB_RESAMPLE_ACCUM_MAX_SRC 4
typedef struct cmb_resample_accum_desc {
  int32_t dtype, src_dtype;
  int32_t act, n_src;
  int64_t B;
  int32_t Ho, Wo;
  int64_t C;
  const void* base;
  int64_t ld_base, batch_stride_base;
  const float* bias;
  const void* src[CMB_RESAMPLE_ACCUM_MAX_SRC];
  int32_t Hi[CMB_RESAMPLE_ACCUM_MAX_SRC], Wi[CMB_RESAMPLE_ACCUM_MAX_SRC];
  int64_t ld_src[CMB_RESAMPLE_ACCUM_MAX_SRC], batch_stride_src[CMB_RESAMPLE_ACCUM_MAX_SRC];
  void* pre_out;
  int64_t ld_pre, batch_stride_pre;
  void* out;
  int64_t ld_out, batch_stride_out;
} cmb_resample_accum_desc;
int cmb_resample_accum(const cmb_resample_accum_desc* d, void* stream);
/* ------------------------------------------------------------------------------------------
 * Optimizer: global gradient norm and a one-pass AdamW step (csrc/optim.hip, arithmetic in csrc/optim_core.h).
 * Replaces transformers.Trainer's clip_grad_norm_ + optimizer.step() that the reference inherits (train_fsdp.py:122
 * derives TrainingArguments from transformers', no script under scripts/cambrian passes --max_grad_norm, so every recipe clips
 * at the default 1.0) and the up-cast / torch AdamW / cast-back passes of train/master.py.
 *
 * Both entry points take a table of jobs in DEVICE memory, one job per tensor.  Every pointer is element-aligned only
 * (gradients are views into flat buckets): a job whose pointers are all 16-byte aligned is moved with 16-byte accesses,
 * any other job element by element; any n >= 0 is legal.  A tensor is cut into chunks of a fixed element count (a
 * compile-time constant of the library); cmb_optim_chunks(n) is the chunk count of n elements (0 for n <= 0), chunk0 the
 * sum of the chunk counts of the jobs before this one, total_chunks the sum over all jobs.  The table is not validated on
 * the host (it is device memory); the scalar arguments are, before anything is launched (CMB_ERR_BAD_ARG: NULL table with
 * n_jobs > 0, a negative count, total_chunks > 0 with n_jobs == 0, NULL outputs, bias corrections <= 0, NaN lr).
 *
 * cmb_grad_sqnorm: *sumsq_out = sum over all jobs of sum g^2 (bf16 widened exactly; param / low / moments are not read).
 * Deterministic and independent of the launch geometry and of the alignment path: each chunk's sum is formed in a fixed
 * fp32 tree order into partial[chunk] (at least cmb_grad_sqnorm_workspace(total_chunks) floats, else CMB_ERR_WORKSPACE),
 * a second launch adds the partials in index order in fp64 and rounds once.  total_chunks == 0 gives 0.  No atomics.
 *
 * cmb_adamw_step: one pass, for every element, all in fp32 with IEEE division and square root,
 *     g  = grad * (grad_scale * coef)
 *     p *= 1 - lr * weight_decay
 *     m  = beta1 m + (1 - beta1) g
 *     v  = beta2 v + (1 - beta2) g^2
 *     p -= (lr / bias_correction1) * (m / (sqrt(v) / sqrt(bias_correction2) + eps))
 *     low = bf16(p), round to nearest even, where low != NULL
 * with coef = 1 when sumsq == NULL or max_norm <= 0, else min(1, max_norm / (grad_scale * sqrt(*sumsq) + 1e-6)), the
 * expression of torch.nn.utils.clip_grad_norm_; *sumsq is read on the device, the host never waits for it.  A NaN *sumsq
 * gives coef = 1, an infinite one coef = 0.  grad_scale: 1 / world for gradients that are sums over ranks, else 1.  One
 * launch serves one parameter group at one step count (bias_correction = 1 - beta^step, formed by the caller). */
typedef struct cmb_optim_job {
  const void* grad;      /* CMB_F32 | CMB_BF16, n elements */
  float* param;          /* fp32: the master, or the parameter itself */
  void* low;             /* bf16 compute copy of param to refresh, or NULL */
  float* exp_avg;        /* fp32 */
  float* exp_avg_sq;     /* fp32 */
  int64_t n;
  int64_t chunk0;
  int32_t grad_dtype;
  int32_t reserved;
} cmb_optim_job;
int64_t cmb_optim_chunks(int64_t n);
int64_t cmb_grad_sqnorm_workspace(int64_t total_chunks);
int cmb_grad_sqnorm(const cmb_optim_job* jobs_device, int64_t n_jobs, int64_t total_chunks, float* partial,
                    int64_t partial_floats, float* sumsq_out, void* stream);
int cmb_adamw_step(const cmb_optim_job* jobs_device, int64_t n_jobs, int64_t total_chunks, float lr, float beta1,
                   float beta2, float eps, float weight_decay, float bias_correction1, float bias_correction2,
                   float grad_scale, const float* sumsq, float max_norm, void* stream);

/* Elementwise y = act(a) * b (SwiGLU: act = SiLU) / y = act(a); a,b,y [rows, D] with strides. */
int cmb_act_mul(int dtype, int32_t act, const void* a, int64_t lda, const void* b, int64_t ldb,
                int64_t rows, int64_t D, void* y, int64_t ldy, void* stream);
/* dx = dy * act'(pre)  (GELU backward for the SVA / projector MLPs). */
int cmb_act_bwd(int dtype, int32_t act, const void* dy, const void* pre, int64_t n, void* dx,
                void* stream);
/* dst[dst_map(r), 0:D] = src[src_map(r), 0:D] for r in [0,rows); src == NULL zero-fills.  Row gather /
 * scatter of the in-LLM SVA hook: hidden[:, p:p+600].view(B,24,25,H)[:, :, :24] <-> [B*576, H]
 * (cambrian_llama.py:181-207) and its backward. */
int cmb_copy_rows(int dtype, const void* src, const cmb_rowmap* src_map, void* dst,
                  const cmb_rowmap* dst_map, int64_t rows, int64_t D, void* stream);

/* dst[r*ld : r*ld+D] = src[0:D] for r in [0,nrows) — CLS-token rows of the ViT sequence buffers
 * (the position-embedding add itself rides in the patch-embed GEMM epilogue as a row-mapped residual). */
int cmb_bcast_rows(int dtype, void* dst, int64_t ld, int64_t nrows, int64_t D, const void* src,
                   void* stream);

/* ------------------------------------------------------------------------------------------
 * LLM-side HBM-bound kernels (llm_ops.hip)
 * ---------------------------------------------------------------------------------------- */
/* Shifted cross-entropy of cambrian_llama.py:411-422 without materialising logits.float():
 * logits [rows, V] (bf16 or fp32, row stride ld), labels int64 [rows] ALREADY shifted by the caller
 * (labels_shift[b, t] = labels[b, t+1], last position = ignore_index).  fwd: lse[row] = log sum_v exp(x_v) in fp32,
 * loss[row] = lse - x[label] (0 for ignored rows); the caller reduces mean over the non-ignored rows.
 * bwd: dlogits[row, v] = (exp(x_v - lse[row]) - [v == label]) * scale[0], zeros for ignored rows; dlogits may alias
 * logits (in-place).  Rows that are not 16-byte aligned (odd vocabularies) take a scalar path. */
int cmb_cross_entropy_fwd(int dtype, const void* logits, int64_t rows, int64_t V, int64_t ld,
                          const int64_t* labels, int64_t ignore_index, float* lse, float* loss, void* stream);
int cmb_cross_entropy_bwd(int dtype, const void* logits, int64_t rows, int64_t V, int64_t ld,
                          const int64_t* labels, int64_t ignore_index, const float* lse, const float* scale,
                          void* dlogits, int64_t ldd, void* stream);
/* Fused QKV hand-off of a decoder layer: packed [B*S, (nh + 2*nkv)*Dh] (q heads | k heads | v heads per token)
 * -> q [B,S,nh,Dh], k [B,S,nkv,Dh], v [B,S,nkv,Dh] (token-major) with RoPE (tables of cmb_rope_table) on q and k; merge != 0 is the
 * backward: (dq, dk, dv) -> d(packed) with the transposed rotation.  Replaces the q/k/v views, two rotary passes and
 * the transposes in front of the attention (HF LlamaAttention reached from cambrian_llama.py:157-166). Dh % 16 == 0. */
int cmb_qkv_rope(int dtype, int32_t merge, void* packed, const float* cos_t, const float* sin_t, int64_t B, int64_t S,
                 int32_t nh, int32_t nkv, int32_t Dh, void* q, void* k, void* v, void* stream);
/* Backward of causal self-attention with grouped KV heads (the decoder's F.scaled_dot_product_attention(is_causal=True,
 * enable_gqa=True); HF LlamaAttention reached from cambrian_llama.py:157-166).  bf16, head_dim 128, S % 128 == 0.
 * q / o / dout / dq are [B,S,H,128] and k / v / dk / dv [B,S,HKV,128] through (batch, token, head) element strides;
 * lse fp32 [B,H,S] = log sum_j exp(scale * q.k_j) from the forward; dvec fp32 [2,B,H,S] is scratch (ABI 6: [0] receives rowsum(dO*O), [1] lse * log2 e for the
 * LDS-DMA dK/dV kernel).
 * Two MFMA kernels (dQ; dK+dV), no atomics, bit-reproducible. */
/* Forward of the same attention: out [B,S,H,128] (strides of q), lse fp32 [B,H,S].
 * causal == 0 is the bidirectional form used when the vision towers train (HF CLIPAttention /
 * Dinov2SelfAttention / timm Attention reached from clip_encoder.py:104, dino_encoder.py:159, siglip_encoder.py:97):
 * every query sees keys [0, kv_len); rows [kv_len, S) are padding (S = kv_len rounded up to 128, zero-filled by the
 * caller, head_dim zero-padded to 128) whose outputs / gradients are don't-care / zero.
 * key_valid (causal only; may be NULL): the collator's key-padding mask (train_fsdp.py:1057-1085, 1089-1165 — padded rows /
 * columns of the 24 x 25 visual span, padded sequence tail), [B, S] bytes, non-zero = attendable.  Query q sees key k iff
 * k <= q and (key_valid[b][k] or k == q): HF's causal AND padding mask (cambrian_llama.py:142-166) with the diagonal
 * kept open so a padded query row is never empty.  Tiles made of padding only are skipped. */
int cmb_flash_attn_fwd(const void* q, const void* k, const void* v, int64_t B, int64_t S, int32_t H, int32_t HKV,
                       int32_t hd, int64_t q_sb, int64_t q_ss, int64_t q_sh, int64_t kv_sb, int64_t kv_ss, int64_t kv_sh,
                       float scale, int32_t causal, int64_t kv_len, const uint8_t* key_valid, void* out, float* lse,
                       void* stream);
int cmb_flash_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                       int64_t B, int64_t S, int32_t H, int32_t HKV, int32_t hd,
                       int64_t q_sb, int64_t q_ss, int64_t q_sh, int64_t kv_sb, int64_t kv_ss, int64_t kv_sh,
                       float scale, int32_t causal, int64_t kv_len, const uint8_t* key_valid, float* dvec, void* dq, void* dk,
                       void* dv, void* stream);
/* One decode step of a decoder layer's attention against the K/V cache (generate(); HF LlamaAttention / Phi3Attention with
 * use_cache reached from cambrian_llama.py:157-166), everything between the QKV projection and o_proj in one call:
 * RoPE (rotate-half, tables of cmb_rope_table, cos_t / sin_t [B, hd/2]) on the new token's q [B, nh*hd] and k [B, nkv*hd],
 * roped k and raw v [B, nkv*hd] stored into slot t of kcache / vcache [B, nkv, Lmax, hd] (element strides c_sb, c_sh, c_st, last
 * dimension contiguous), then out [B, nh*hd] (contiguous, compute dtype) = softmax(scale * q.K^T).V per query head over cache
 * keys 0..t, query head h reading KV head h / (nh / nkv).  q / k / v have row strides in elements and may point into one
 * packed projection row.  key_valid: bytes [B, >= t+1] with row stride kv_ld, non-zero = attendable; slot t is always
 * attendable (the "diagonal open" rule of cmb_flash_attn_fwd), so no row is empty.  Masked slots are not attended to
 * whatever they hold; slots past t are not read.  The attended k of slot t is the value stored (rounded to the cache dtype).
 * dtype CMB_BF16 | CMB_F32 (fp32 scores, running max / sum and accumulators in both); hd 64 | 96 | 128; nh % nkv == 0 and
 * nh / nkv <= 8; B, nkv <= 65535; all pointers and strides 16-byte aligned (CMB_ERR_ALIGNMENT).
 * The key range is cut into `splits` contiguous chunks, one workgroup per (batch row, KV head, chunk) holding all nh / nkv
 * query heads, so a cache row is read once per step; splits > 1 writes un-normalised fp32 partials to `ws` and a second small
 * launch merges them in chunk order (no atomics: bit-reproducible).  splits == 0 is the library's choice, a pure function of
 * (B, nkv, t, CU count); 1 .. max_splits forces one (fewer are used when t + 1 is short: cmb_decode_attn_plan reports the
 * effective count and the chunk length, splits * chunk >= t + 1 > (splits - 1) * chunk).  cmb_decode_attn_ws: floats of
 * `ws` the call needs (0 when it runs unsplit; ws may then be NULL), or a negative status.  Both queries are host functions. */
int cmb_decode_attn(int dtype, const void* q, int64_t q_ld, const void* k, int64_t k_ld, const void* v, int64_t v_ld,
                    const float* cos_t, const float* sin_t, void* kcache, void* vcache, int64_t c_sb, int64_t c_sh,
                    int64_t c_st, int64_t B, int32_t nh, int32_t nkv, int32_t hd, int64_t t, const uint8_t* key_valid,
                    int64_t kv_ld, float scale, int32_t splits, float* ws, int64_t ws_floats, void* out, void* stream);
int64_t cmb_decode_attn_ws(int64_t B, int32_t nh, int32_t nkv, int32_t hd, int64_t t, int32_t splits);
int cmb_decode_attn_plan(int64_t B, int32_t nkv, int64_t t, int32_t splits, int32_t* splits_out, int64_t* chunk_out,
                         int32_t* max_splits_out);
/* The linears of a decode step (generate(); the projections of HF LlamaDecoderLayer / Phi3DecoderLayer and the lm_head at
 * one token per sequence): out[M, N'] = epilogue(prologue(x)[M, K] . W[N, K]^T), bf16 x and W, fp32 accumulation, 1 <= M <= 16.
 * A stream of weights read once: non-temporal 16-byte loads straight to registers, a slab of weight rows per workgroup, K
 * split over the workgroup's four waves and summed through LDS; no split of K across workgroups, no atomics, no workspace,
 * the same bits on every run, and row m's bits do not depend on M.
 *   norm_w != NULL   RMSNorm prologue, bf16 weights [K]: the result is RMSNorm(x; norm_w, norm_eps) . W^T.  x[m, k] * norm_w[k]
 *                    is rounded to bf16 as it is read (the matrix unit's operand), the row's sum of squares is gathered on the
 *                    same pass and rsqrt(mean + eps) scales the fp32 accumulator: the normalised row itself is never rounded,
 *                    which differs from cmb_rmsnorm_fwd followed by a GEMM within bf16 rounding.
 *   act              0 = none (N' = N); 1 = SwiGLU over packed [gate; up] rows, the convention of cmb_act_mul on a packed
 *                    buffer: N = 2 I, out[m, j] = silu(acc[m, j]) * acc[m, I + j], N' = I.
 *   residual         NULL or bf16 [M, N'] with row stride r_ld, added in fp32 before the one rounding; not with act = 1.
 *   out_f32          0 = bf16 store, 1 = fp32 store (the logits).
 * Everything is checked on the host before any launch and refused with CMB_ERR_BAD_ARG: x, W, out non-NULL; M in 1 .. 16;
 * K % 8 == 0, K >= 8; N >= 1, even for act = 1; N, K <= 2^31; act in {0, 1}; out_f32 in {0, 1}; norm_eps >= 0; x_ld, w_ld >= K and
 * o_ld, r_ld >= N', all multiples of 8 elements; every pointer given 16-byte aligned.  Rows of x past M - 1, columns past K of
 * x and W and everything around out's [M, N'] are neither read nor written.
 * cmb_decode_linear_supported: 1 / 0 for the shape conditions above, no launch.  cmb_decode_linear_plan: the weight rows a
 * workgroup owns (8, 16 or 32; with act = 1 half of them gate rows and half the matching up rows) and the number of
 * workgroups, a pure function of (M, N, K, act, CU count): the largest slab that leaves two workgroups per CU (one and a half for M > 4), 8 rows (16
 * with act = 1) when none does.  cus = 0 asks for the current device's count (256 when there is none). */
int cmb_decode_linear(const void* x, int64_t x_ld, int32_t M, const void* norm_w, float norm_eps, const void* W,
                      int64_t w_ld, int64_t N, int64_t K, int32_t act, const void* residual, int64_t r_ld, void* out,
                      int64_t o_ld, int32_t out_f32, void* stream);
int cmb_decode_linear_supported(int32_t M, int64_t N, int64_t K, int32_t act);
int cmb_decode_linear_plan(int32_t M, int64_t N, int64_t K, int32_t act, int32_t cus, int32_t* rows_out, int64_t* wgs_out);
/* cmb_decode_linear for 1 <= M <= 64 rows (decode steps of 17-64 sequences or beams): the same function, arguments, checks
 * and statuses, with "M in 1 .. 64" in place of "M in 1 .. 16".  x is taken as ceil(M / 16) row blocks of the 16-column
 * operand of the matrix unit; weights stream as in cmb_decode_linear (non-temporal 16-byte loads straight to registers, a
 * full 128-byte line per row and instruction, every weight byte read from HBM once per launch); a workgroup owns a slab of
 * 16 or 32 weight rows and reads all of x through the caches; K is split over the workgroup's four waves and summed through
 * LDS in wave order.  No split of K across workgroups, no atomics, no flags, no workspace.  The same inputs give the same
 * bits on every run, and the bits of an output row depend neither on M nor on the other rows nor on the slab.  The order of
 * a row's sum is NOT cmb_decode_linear's: the two agree within fp32 summation error, not to the bit.  Under the norm
 * prologue x[m, k] * norm_w[k] goes through the matrix unit as its bf16 rounding plus the (exact, bf16) remainder, so the
 * normalised row is never rounded.
 * cmb_decode_linear_wide_supported: 1 / 0 for the shape conditions, no launch.  cmb_decode_linear_wide_plan: the weight rows
 * a workgroup owns (16 or 32; with act = 1 half of them gate rows and half the matching up rows) and the number of
 * workgroups, a pure function of (N, act, CU count): 32 rows where that leaves one workgroup per CU, else 16.  cus = 0 asks
 * for the current device's count (256 when there is none). */
int cmb_decode_linear_wide(const void* x, int64_t x_ld, int32_t M, const void* norm_w, float norm_eps, const void* W,
                           int64_t w_ld, int64_t N, int64_t K, int32_t act, const void* residual, int64_t r_ld, void* out,
                           int64_t o_ld, int32_t out_f32, void* stream);
int cmb_decode_linear_wide_supported(int32_t M, int64_t N, int64_t K, int32_t act);
int cmb_decode_linear_wide_plan(int32_t M, int64_t N, int64_t K, int32_t act, int32_t cus, int32_t* rows_out,
                                int64_t* wgs_out);
/* cmb_decode_linear on weight-only e4m3 weights, half the weight stream of a decode step:
 *   out = epilogue(rstd? * w_inv_scale[n] * sum_k prologue(x)[m, k] * e4m3(Wq[n, k]))
 * Wq: OCP e4m3fn bytes [N, K] with row stride w_ld BYTES, w_inv_scale: fp32 [N] — what cmb_quantize_fp8_rows writes (a
 * row's largest magnitude maps to 448, inv_scale = amax / 448, 1.0 for a zero row).  Every byte of Wq[N, K] must be FINITE
 * (not 0x7F / 0xFF, the NaN codes, which the quantiser never writes): fragments past a ragged K re-read bytes at k = 0 and
 * multiply them by zero, so a NaN anywhere in a row could reach its sum.  x stays bf16: every e4m3 value is
 * exactly a bf16, so the bytes are converted in registers and the products are those of cmb_decode_linear on the
 * dequantised-without-scale weights; the row factor multiplies the finished fp32 sum once (together with rstd under the
 * norm prologue; with act = 1 gate and up each take their own row's before silu(g) * u).  norm_w, act, residual, out_f32,
 * the determinism and the statuses are cmb_decode_linear's; the shape rule differs in K % 16 == 0, K >= 16, w_ld >= K and
 * w_ld % 16 == 0 (a lane loads 16 bytes = 16 k), Wq 16-byte aligned, w_inv_scale non-NULL and 4-byte aligned.
 * cmb_decode_linear_fp8_plan: as cmb_decode_linear_plan, with the largest slab that leaves ONE workgroup per CU at every
 * M (a slab carries half the bytes per row, the x fragments per k-step stay). */
int cmb_decode_linear_fp8(const void* x, int64_t x_ld, int32_t M, const void* norm_w, float norm_eps, const void* Wq,
                          int64_t w_ld, const void* w_inv_scale, int64_t N, int64_t K, int32_t act, const void* residual,
                          int64_t r_ld, void* out, int64_t o_ld, int32_t out_f32, void* stream);
int cmb_decode_linear_fp8_supported(int32_t M, int64_t N, int64_t K, int32_t act);
int cmb_decode_linear_fp8_plan(int32_t M, int64_t N, int64_t K, int32_t act, int32_t cus, int32_t* rows_out, int64_t* wgs_out);
/* MXFP4 quantisation of matrix rows (OCP microscaling: e2m1 values with one shared e8m0 scale per 32 elements, 4.25 bits per
 * element) for cmb_decode_linear_fp4.  x [rows, K] (dtype CMB_BF16 | CMB_F32, row stride ldx elements), FINITE values only.
 *   q      uint8 [rows, K / 2], row stride ldq bytes: byte j of a row holds element 2 j in its low nibble and element 2 j + 1
 *          in its high nibble; a nibble is an e2m1 code, bit 3 the sign, magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6
 *   scales uint8 [rows, K / 32], row stride lds bytes: code c means 2^(c - 127)
 * Per block of 32: amax = max |x|; e = clamp(floor(log2 amax) - 2, -126, 127); code = e + 127 (a zero block: code 127 and
 * zero nibbles); every x * 2^-e is rounded to the e2m1 grid, to nearest, ties to the even code, saturating at +-6 — a block
 * whose amax lies in (6, 8) * 2^e clamps (the OCP rule).  -0 and values that round to zero are written as +0.  Codes 0 and
 * 255 are never written.  A streaming kernel, one block of 32 per thread: any K % 32 == 0, no upper limit.  Deterministic.
 * CMB_ERR_SHAPE: K % 32 != 0, ldx < K, ldq < K / 2, ldq % 16 != 0, lds < K / 32; CMB_ERR_ALIGNMENT: x or q not 16-byte
 * aligned, or x rows that are not.  rows == 0 is CMB_OK. */
int cmb_quantize_mxfp4_rows(int dtype, const void* x, int64_t ldx, int64_t rows, int64_t K, void* q, int64_t ldq, void* scales,
                            int64_t lds, void* stream);
/* cmb_decode_linear on MXFP4 weights, a quarter of the bf16 weight stream (4.25 bits per weight):
 *   out = epilogue(rstd? * sum_k prologue(x)[m, k] * e2m1(Wq[n, k]) * 2^(Ws[n, k / 32] - 127))
 * Wq / Ws: the nibbles [N, K / 2] (row stride w_ld BYTES) and e8m0 block scales [N, K / 32] (row stride s_ld bytes) in
 * cmb_quantize_mxfp4_rows' format.  Scale codes 1 .. 254 are accepted; 0 and 255 (NaN in e8m0) must not appear anywhere in
 * Ws[N, K / 32]: fragments past a ragged K re-read the block at k = 0 and multiply it by zero.  x stays bf16: an e2m1 value
 * times a power of two is exactly a bf16 wherever it lies in bf16's range (codes 1 .. 252 with every nibble; 6 * 2^126 and
 * above is infinity, as in a bf16 copy of the dequantised weight), so the nibbles are converted in registers and the
 * products are those of cmb_decode_linear on the dequantised weights; the fp32 sum is the only rounding.  There is no
 * per-row factor.  norm_w, act, residual, out_f32, the determinism and the statuses are cmb_decode_linear's; the shape rule
 * differs in K % 32 == 0, K >= 32, w_ld >= K / 2 and w_ld % 16 == 0 (a lane loads 16 bytes = 32 k = one block), s_ld >= K / 32,
 * Wq 16-byte aligned, Ws non-NULL (bytes: no alignment rule).
 * cmb_decode_linear_fp4_plan: cmb_decode_linear_fp8_plan's rule (the largest slab that leaves one workgroup per CU). */
int cmb_decode_linear_fp4(const void* x, int64_t x_ld, int32_t M, const void* norm_w, float norm_eps, const void* Wq,
                          int64_t w_ld, const void* Ws, int64_t s_ld, int64_t N, int64_t K, int32_t act, const void* residual,
                          int64_t r_ld, void* out, int64_t o_ld, int32_t out_f32, void* stream);
int cmb_decode_linear_fp4_supported(int32_t M, int64_t N, int64_t K, int32_t act);
int cmb_decode_linear_fp4_plan(int32_t M, int64_t N, int64_t K, int32_t act, int32_t cus, int32_t* rows_out, int64_t* wgs_out);
/* One token's pass through the whole decoder in ONE call (generate(); the decode-step loop over HF LlamaDecoderLayer /
 * Phi3DecoderLayer and the lm_head): per layer norm + QKV linear, cmb_decode_attn (with its combine launch when the plan
 * splits), o_proj + skip, norm + gate / up + SwiGLU, down_proj + skip; then final norm + lm_head into fp32 logits.  It calls
 * cmb_decode_linear / cmb_decode_linear_fp8 / cmb_decode_attn with the arguments the five-launch path passes, 5 layers + 1
 * launches (+ 1 per layer when the attention splits) on `stream`, ordered by the stream alone: no new GEMM or attention kernel,
 * no grid-wide barrier, no device-side flag, so logits and caches carry the bits of the separate calls.
 * cmb_decode_layer, one per layer, in HOST memory: the four weights [N, K] with their row strides (bf16: elements; fp8: bytes
 * of e4m3fn with w_*_scale the fp32 row factors of cmb_quantize_fp8_rows, else NULL), both RMSNorm weights (bf16 [H]) and the
 * layer's K / V caches [B, nkv, Lmax, hd].  w_qkv is [(nh + 2 nkv) hd, H] (q | k | v heads), w_o [H, nh hd], w_gate_up
 * [2 I, H] ([gate; up], cmb_decode_linear's act = 1), w_down [H, I].
 * cmb_decode_step_desc: geometry, eps (every norm), the attention scale, the caches' element strides (shared by all layers),
 * the final norm and the lm_head [V, H]; fp8 == 1: every weight of every layer and the head is e4m3 with row factors;
 * fp8 == 2: every weight is MXFP4 (cmb_quantize_mxfp4_rows' nibbles, row strides in bytes) and w_*_scale / head_scale point to
 * its e8m0 scale BYTES with row stride K / 32 (the fields keep their const float* type for existing callers; no alignment
 * rule applies to them in this mode) and cmb_decode_linear_fp4 runs the linears; 0: bf16.  Any other value is
 * CMB_ERR_BAD_ARG.
 * Per call: x bf16 [B, H] (row stride x_ld, outside ws), cos_t / sin_t fp32 [B, hd/2], cache slot t, key_valid bytes
 * [B, >= t+1] (row stride kv_ld), ws fp32 [>= cmb_decode_step_ws(...) at this t] (csrc/decode_step_layout.h), logits fp32
 * [B, V] with row stride logits_ld (a multiple of 8).  bf16 only.
 * Every rule is checked before any launch: CMB_ERR_BAD_ARG for a NULL pointer, layers < 1, B outside 1 .. 16, a geometry or
 * stride the launchers refuse, x inside ws; CMB_ERR_ALIGNMENT for a pointer that is not 16-byte aligned (row factors: 4) or a
 * cache stride that is no multiple of 8 elements; CMB_ERR_WORKSPACE for ws_floats below the need.
 * cmb_decode_step_ws: floats of ws for steps up to slot t_max (non-decreasing in t_max), or a negative status. */
typedef struct cmb_decode_layer {
  const void* w_qkv; int64_t ld_qkv; const float* w_qkv_scale;
  const void* w_o; int64_t ld_o; const float* w_o_scale;
  const void* w_gate_up; int64_t ld_gate_up; const float* w_gate_up_scale;
  const void* w_down; int64_t ld_down; const float* w_down_scale;
  const void* norm1; const void* norm2;
  void* kcache; void* vcache;
} cmb_decode_layer;
typedef struct cmb_decode_step_desc {
  int32_t B, layers, H, I, nh, nkv, hd, fp8;
  int64_t V;
  float eps, scale;
  int64_t c_sb, c_sh, c_st;
  const void* final_norm;
  const void* head; int64_t ld_head; const float* head_scale;
} cmb_decode_step_desc;
int cmb_decode_step(const cmb_decode_step_desc* d, const cmb_decode_layer* layers, const void* x, int64_t x_ld,
                    const float* cos_t, const float* sin_t, int64_t t, const uint8_t* key_valid, int64_t kv_ld, float* ws,
                    int64_t ws_floats, float* logits, int64_t logits_ld, void* stream);
int64_t cmb_decode_step_ws(int32_t B, int32_t H, int32_t I, int32_t nh, int32_t nkv, int32_t hd, int64_t t_max);
/* The K / V cache of the decode steps in one byte per element (opt-in; it changes numerics).
 * Format.  kcache / vcache: uint8 [B, nkv, Lmax, hd], OCP e4m3fn bytes, with BYTE strides c_sb / c_sh / c_st (last dimension
 * contiguous; multiples of 16, c_st >= hd) and one fp32 factor per (row, KV head, slot): k_inv / v_inv [B, nkv, Lmax] with
 * element strides i_sb / i_sh and slot stride 1 — 1 + 4 / hd bytes per element.  A cache row of hd values is quantised by
 * cmb_quantize_fp8_rows' rule, expression for expression: amax = max |x|; byte = e4m3(clamp(x * (448 / amax), +-448)), round to
 * nearest even; factor = amax / 448; a zero row takes scale and factor 1.  The NaN codes 0x7F / 0xFF are never written.  The
 * value of an entry is e4m3(byte) * factor.
 *
 * cmb_kv_quantize_e4m3: the prefill's K (or V) into slots 0 .. L-1 of such a cache, one launch per tensor.  src: bf16
 * [B, nkv, L, hd] with ELEMENT strides s_sb / s_sh / s_st (last dimension contiguous).  Bytes and factors are those
 * cmb_quantize_fp8_rows gives for the same rows, bit for bit, and those cmb_decode_attn_kv8 writes for the same bf16 values.
 * Slots >= L, and bytes between a row's hd bytes and the next row when c_st > hd, are neither read nor written.  A streaming
 * kernel (a row across a group of lanes, several rows per wave), deterministic.
 * CMB_ERR_BAD_ARG: a NULL pointer, hd outside 16 .. 128 or hd % 16 != 0, a negative count or stride, s_st or c_st < hd;
 * CMB_ERR_ALIGNMENT: src or cache not 16-byte aligned, inv not 4-byte aligned, a source stride that is no multiple of 8
 * elements, a cache stride that is no multiple of 16 bytes.  B, nkv or L == 0 is CMB_OK.
 *
 * cmb_decode_attn_kv8: cmb_decode_attn's step on that cache.  q / k / v (bf16, row strides in elements), cos_t / sin_t,
 * key_valid / kv_ld, slot t, scale, splits / ws / ws_floats (cmb_decode_attn_plan and cmb_decode_attn_ws serve it unchanged),
 * out (bf16 [B, nh*hd]) and the geometry rule (hd 64 | 96 | 128, nh % nkv == 0, nh / nkv <= 8; B, nkv <= 65535) are that
 * function's; activations are bf16 only.  Slots 0 .. t-1 are read as e4m3(byte) * factor.  The new token's k is roped and
 * rounded to bf16 (the value a bf16 cache would hold), that row and the raw v row are quantised by the rule above and stored
 * — bytes and both factors — into slot t, and the step attends to the dequantised slot, which is what later steps read.  A
 * slot that is not attendable (masked, or past t) may hold any bytes and factors, NaN included; slots past t are not read.
 * Deterministic: the same bits on every run, in out and in the caches.
 * CMB_ERR_BAD_ARG: a NULL pointer (ws may be NULL when the call runs unsplit), a geometry outside the rule, t < 0, kv_ld < t + 1,
 * c_st < hd, a negative stride, ws_floats below the need; CMB_ERR_ALIGNMENT: q, k, v, the caches or out not 16-byte
 * aligned, a factor array not 4-byte aligned, a q / k / v row stride that is no multiple of 8 elements, a cache stride that is
 * no multiple of 16 bytes.  Everything is checked before any launch; B == 0 is CMB_OK.
 *
 * cmb_decode_step_kv8: cmb_decode_step on such caches.  layers[l].kcache / vcache are the byte caches, d->c_sb / c_sh / c_st
 * their BYTE strides (multiples of 16, c_st >= hd), factors[l] (HOST memory, one per layer) the layer's factor arrays with
 * strides i_sb / i_sh.  Launch 1 of every layer is cmb_decode_attn_kv8; everything else, all three values of d->fp8 included,
 * is cmb_decode_step's, by the same code; cmb_decode_step_ws gives the workspace.  Statuses as cmb_decode_step, plus
 * CMB_ERR_BAD_ARG for factors == NULL, a NULL factor array or a negative factor stride and CMB_ERR_ALIGNMENT for a factor array
 * that is not 4-byte aligned or a cache stride that is no multiple of 16 bytes. */
typedef struct cmb_decode_kv8_factors {
  float* k_inv; float* v_inv;          /* slot t of both is written by the step */
} cmb_decode_kv8_factors;
int cmb_kv_quantize_e4m3(const void* src, int64_t s_sb, int64_t s_sh, int64_t s_st, int64_t B, int32_t nkv, int64_t L, int32_t hd,
                         void* cache, int64_t c_sb, int64_t c_sh, int64_t c_st, float* inv, int64_t i_sb, int64_t i_sh,
                         void* stream);
int cmb_decode_attn_kv8(const void* q, int64_t q_ld, const void* k, int64_t k_ld, const void* v, int64_t v_ld,
                        const float* cos_t, const float* sin_t, void* kcache, void* vcache, int64_t c_sb, int64_t c_sh,
                        int64_t c_st, float* k_inv, float* v_inv, int64_t i_sb, int64_t i_sh, int64_t B, int32_t nh, int32_t nkv,
                        int32_t hd, int64_t t, const uint8_t* key_valid, int64_t kv_ld, float scale, int32_t splits, float* ws,
                        int64_t ws_floats, void* out, void* stream);
int cmb_decode_step_kv8(const cmb_decode_step_desc* d, const cmb_decode_layer* layers, const cmb_decode_kv8_factors* factors,
                        int64_t i_sb, int64_t i_sh, const void* x, int64_t x_ld, const float* cos_t, const float* sin_t, int64_t t,
                        const uint8_t* key_valid, int64_t kv_ld, float* ws, int64_t ws_floats, float* logits, int64_t logits_ld,
                        void* stream);
/* cmb_decode_attn for Q consecutive new tokens per cache row (the verify step of prompt-lookup speculative decoding in
 * generate()): bf16 only, no dtype argument.  q [B*Q, nh*hd], k / v [B*Q, nkv*hd] (un-roped rows of the packed projection, row
 * strides in elements), cos_t / sin_t fp32 [B*Q, hd/2], out [B*Q, nh*hd] contiguous; row b*Q + j is token j of sequence b.
 * Roped k (fp32 rotate-half RoPE, then rounded to bf16) and raw v (bit for bit) of row (b, j) are stored into slot t0 + j of
 * cache row b.  Query (b, j) attends slots s <= t0 + j: cached slots s < t0 under key_valid[b][s], the step's own slots
 * t0 .. t0 + j always (cmb_decode_attn's "slot t is open" rule, extended); bytes of key_valid at slots >= t0 are not read,
 * slots past t0 + Q - 1 are neither read nor written, and a masked or unwritten slot may hold anything, NaN included.  No
 * workgroup reads from the cache a slot the launch writes: the new keys and values come from the arguments, the attended new
 * k being the value as stored.
 * hd 64 | 96 | 128; nh % nkv == 0, G = nh / nkv <= 8; 1 <= Q <= 16 and Q * G <= 64; B, nkv <= 65535; pointers and strides
 * 16-byte aligned.  fp32 scores, running max / sum and accumulators; both products run on the bf16 MFMA (q after RoPE and the
 * softmax weights are rounded to bf16), so Q = 1 agrees with cmb_decode_attn within bf16 rounding, not in bits.  One workgroup
 * per (batch row, KV head, chunk of keys) holds all Q * G query rows: the cache is read once per launch.  splits / ws /
 * ws_floats as cmb_decode_attn, planned over slots 0 .. t0 + Q - 1 (splits == 0: a pure function of (B, nkv, t0 + Q, CU
 * count); splits * chunk >= t0 + Q > (splits - 1) * chunk; the last chunk holds the step's own slots); partials are merged in
 * chunk order by a second small launch: no atomics, the same bits on every run.
 * Statuses and check order of cmb_decode_attn, everything before any launch: CMB_ERR_BAD_ARG for a NULL pointer (ws may be
 * NULL when the call runs unsplit), a geometry or Q outside the rule, B or nkv out of range, t0 < 0, kv_ld < t0 + Q, ws_floats
 * below the need; CMB_ERR_ALIGNMENT; B == 0 is CMB_OK.  cmb_decode_attn_multi_ws: floats of `ws` (0 when unsplit) or a negative
 * status; both queries are host functions. */
int cmb_decode_attn_multi(const void* q, int64_t q_ld, const void* k, int64_t k_ld, const void* v, int64_t v_ld,
                          const float* cos_t, const float* sin_t, void* kcache, void* vcache, int64_t c_sb, int64_t c_sh,
                          int64_t c_st, int64_t B, int32_t nh, int32_t nkv, int32_t hd, int32_t Q, int64_t t0,
                          const uint8_t* key_valid, int64_t kv_ld, float scale, int32_t splits, float* ws, int64_t ws_floats,
                          void* out, void* stream);
int64_t cmb_decode_attn_multi_ws(int64_t B, int32_t nh, int32_t nkv, int32_t hd, int32_t Q, int64_t t0, int32_t splits);
int cmb_decode_attn_multi_plan(int64_t B, int32_t nkv, int64_t t0, int32_t Q, int32_t splits, int32_t* splits_out,
                               int64_t* chunk_out, int32_t* max_splits_out);
/* Attention of a CHUNK of Q >= 1 consecutive new tokens per cache row against the bf16 K / V cache: the suffix of a prompt
 * whose head is already cached (generate(prefix=...)), the next turn of a chat.  Arguments, layouts and stores are
 * cmb_decode_attn_multi's: q [B*Q, nh*hd], k / v [B*Q, nkv*hd] (un-roped, row strides in elements), cos_t / sin_t fp32
 * [B*Q, hd/2], out [B*Q, nh*hd] contiguous, row b*Q + j is token j of sequence b; roped k (fp32 rotate-half RoPE, rounded to
 * bf16 once) and raw v (bit for bit) of row (b, j) go into slot t0 + j of cache row b, and nothing outside slots
 * t0 .. t0 + Q - 1 of the caches is written.
 * The mask is the one difference: query (b, j) sees slot s iff s <= t0 + j and (key_valid[b][s] != 0 or s == t0 + j), the same
 * rule for cached slots and the chunk's own — cmb_flash_attn_fwd's "causal AND key padding, diagonal open", so a batch whose
 * suffixes are left-padded inside the chunk is legal and a padded query row still gives a finite row (it sees itself).
 * key_valid is read for slots 0 .. t0 + Q - 1 (kv_ld >= t0 + Q); a slot no query may see (a masked cached slot, any slot past
 * t0 + Q - 1) may hold anything, NaN included.  The attention launch reads the new slots from the cache: an earlier launch of
 * the same call on the same stream wrote them.
 * hd 64 | 96 | 128; nh % nkv == 0, G = nh / nkv <= 8; 1 <= Q <= 4096; t0 <= 2^31 - 1 - 4096 (so that t0 + Q < 2^31 whatever Q is); B, nkv <= 65535; bf16 only; pointers and
 * strides 16-byte aligned.  Launches: the stores; attention over a grid of (batch row, KV head, row block of min(16, 64 / G)
 * tokens, chunk of keys) with cmb_decode_attn_multi's workgroup (fp32 scores, running max / sum and accumulators, both
 * products on the bf16 MFMA), every row under its own causal limit; when split, a merge of the fp32 partials in chunk order
 * (no atomics, the same bits on every run).  The cache of a KV head is read once per row block.
 * splits / ws / ws_floats as cmb_decode_attn_multi.  cmb_extend_attn_plan: the split of slots 0 .. t0 + Q - 1, splits * chunk
 * >= t0 + Q > (splits - 1) * chunk; splits == 0 asks for the library's choice, a pure function of (B, nkv, t0, Q, CU count)
 * that counts the ceil(Q / 16) row blocks as batch rows, so long chunks split little or not at all.  cmb_extend_attn_ws: floats
 * of `ws` (0 when unsplit; B * Q * nh * splits * (hd + 2) otherwise) or a negative status; both queries are host functions.
 * Statuses and check order of cmb_decode_attn_multi, everything before any launch: CMB_ERR_BAD_ARG for a NULL pointer (ws may
 * be NULL when the call runs unsplit), a geometry or Q outside the rule, B or nkv out of range, t0 < 0, kv_ld < t0 + Q; then
 * B == 0 is CMB_OK; then CMB_ERR_BAD_ARG for splits outside 0 .. the maximum, t0 > 2^31 - 1 - 4096 or ws_floats below the need; then
 * CMB_ERR_ALIGNMENT. */
int cmb_extend_attn(const void* q, int64_t q_ld, const void* k, int64_t k_ld, const void* v, int64_t v_ld, const float* cos_t,
                    const float* sin_t, void* kcache, void* vcache, int64_t c_sb, int64_t c_sh, int64_t c_st, int64_t B,
                    int32_t nh, int32_t nkv, int32_t hd, int32_t Q, int64_t t0, const uint8_t* key_valid, int64_t kv_ld,
                    float scale, int32_t splits, float* ws, int64_t ws_floats, void* out, void* stream);
int64_t cmb_extend_attn_ws(int64_t B, int32_t nh, int32_t nkv, int32_t hd, int32_t Q, int64_t t0, int32_t splits);
int cmb_extend_attn_plan(int64_t B, int32_t nkv, int64_t t0, int32_t Q, int32_t splits, int32_t* splits_out, int64_t* chunk_out,
                         int32_t* max_splits_out);
/* Greedy token selection and the next step's inputs in one launch (+ the cmb_rope_table launch), one workgroup per row b:
 *   nxt = argmax(logits[b, 0..V))       fp32 logits, row stride logits_ld; ties: the lowest index; a NaN is greater than
 *                                       every number and the first NaN wins (torch.argmax's rules); -0 == +0
 *   eos >= 0:  nxt = done[b] ? eos : nxt;  done[b] |= (nxt == eos)            (eos = -1: none, done may be NULL)
 *   out_ids[b * out_ld + step] = nxt;  pos[b] = n_tok[b] + step;  key_valid[b * kv_ld + t] = 1;
 *   x[b, 0..H) = embed[nxt, 0..H)       bf16 rows copied in 16-byte pieces (H % 8 == 0, strides multiples of 8)
 * then cos_t / sin_t [B, hd/2] = cmb_rope_table(pos, B, hd, rope_base).  No atomics, the same bits on every run.
 * CMB_ERR_BAD_ARG: a NULL pointer, B outside 1 .. 16, V < 1 or > 2^31 - 1, V > embed_rows, eos outside -1 .. embed_rows - 1,
 * step, t < 0, step >= out_ld, t >= kv_ld, H, hd or a stride out of rule; CMB_ERR_ALIGNMENT: embed or x not 16-byte aligned. */
int cmb_decode_next(const float* logits, int64_t logits_ld, int32_t B, int64_t V, int64_t eos, uint8_t* done,
                    int64_t* out_ids, int64_t out_ld, int64_t step, const int64_t* n_tok, int64_t* pos, uint8_t* key_valid,
                    int64_t kv_ld, int64_t t, const void* embed, int64_t embed_ld, int64_t embed_rows, int64_t H, void* x,
                    int64_t x_ld, int32_t hd, float rope_base, float* cos_t, float* sin_t, void* stream);
/* Sampled token selection: cmb_decode_next with the argmax replaced by temperature -> top-k -> top-p -> a random draw, one
 * workgroup per row b, one launch (+ the cmb_rope_table launch).  With z_i = logits[b, i] * inv_temperature (one fp32 multiply):
 *   - the row's maximum (cmb_decode_next's order) is not finite — a NaN, +inf, every logit -inf, or z_max overflows:
 *     nxt = cmb_decode_next's argmax, thr[b] = NaN, n_keep[b] = 0, nothing below applies;
 *   - top_k > 0: keep i iff z_i >= the min(top_k, V)-th largest z (ties at that value are all kept);  0 = off
 *   - top_p < 1: over what top-k kept, w_i = exp(z_i - z_max) counted in units of 2^-40, Z = sum w; a value v is kept iff the
 *     mass of the kept elements with z <= v exceeds (1 - top_p) * Z; the maximum is always kept; equal values are kept or
 *     dropped together (HF's TopPLogitsWarper splits such ties by its sort order);  1 = off
 *   - both filters are one threshold, keep iff z_i >= thr (-inf with both off);
 *   - nxt = the kept i with the largest s_i = z_i + g_i (fp32), the lowest index among equals, where g = -log(-log u),
 *     u = ((word >> 8) + 0.5) * 2^-24 and word = output (i & 3) of Philox4x32-10 with counter (i >> 2, b, step, 0) and key
 *     (*seed & 0xFFFFFFFF, *seed >> 32).  `seed` is read on the device.  A row's id depends on (*seed, b, step) and the row
 *     alone, not on B;
 * then the eos rule, out_ids, pos, key_valid, x, cos_t / sin_t exactly as cmb_decode_next.  thr [B] and n_keep [B] (the
 * threshold and how many elements passed it) are optional outputs, NULL = not written.  Integer LDS atomics only: the same bits
 * on every run.  Argument rules and statuses of cmb_decode_next, checked in its order, and: CMB_ERR_BAD_ARG for seed NULL,
 * inv_temperature not finite or <= 0, top_p outside (0, 1], top_k < 0; CMB_ERR_ALIGNMENT for seed not 8-byte, thr or n_keep
 * not 4-byte aligned. */
int cmb_decode_sample(const float* logits, int64_t logits_ld, int32_t B, int64_t V, float inv_temperature, int64_t top_k,
                      float top_p, const uint64_t* seed, int64_t eos, uint8_t* done, int64_t* out_ids, int64_t out_ld,
                      int64_t step, const int64_t* n_tok, int64_t* pos, uint8_t* key_valid, int64_t kv_ld, int64_t t,
                      const void* embed, int64_t embed_ld, int64_t embed_rows, int64_t H, void* x, int64_t x_ld, int32_t hd,
                      float rope_base, float* cos_t, float* sin_t, float* thr, int32_t* n_keep, void* stream);
/* The logits processors of generate() that read the ids produced so far, applied to a step's fp32 logits IN PLACE before
 * cmb_decode_next / cmb_decode_sample select from them: one launch, one workgroup per row b, any B >= 1.  HF's
 * RepetitionPenalty, NoRepeatNGram, NoBadWords, MinNewTokensLength and SuppressTokens processors chained in that order over the
 * GENERATED ids (generate() with inputs_embeds never shows them the prompt); restated in torch in
 * cambrian_amd/model/language_model/processors.py (apply_torch), the predicates are those of csrc/decode_process_core.h.
 * With h = hist[b * hist_ld + 0 .. n_hist) (int64), n = n_hist, and "column of id" = id when 0 <= id < V, else none:
 *   penalty != 1: for every DISTINCT id of h that has a column, once: l = logits[b, id]; logits[b, id] = l < 0 ? l * penalty
 *                 : l / penalty  (fp32, IEEE-rounded; the lane at the id's first occurrence applies it);
 *   then -inf at the column of each of:
 *   - ngram = g > 0 and n + 1 >= g: every h[i + g - 1] with 0 <= i <= n - g and h[i .. i + g - 1) == h[n - g + 1 .. n)
 *     (g = 1: every id of h);
 *   - bans[0 .. n_bans): suppressed tokens and bad words of one id;
 *   - word w = word_ids[word_off[w] .. word_off[w + 1]) of m ids, 0 <= w < n_words: its last id, when m == 1, or m <= n and
 *     h[n - m + 1 .. n) == w[0 .. m - 1)  (HF's length rule is m <= n, not m - 1 <= n); offsets that do not describe a piece
 *     of word_ids[0 .. n_word_ids) ban nothing;
 *   - n < min_new: every id of eos[0 .. n_eos).
 *   done != NULL, n_eos > 0, n >= 1 and h[n - 1] in eos: done[b] = 1 (else done[b] is left alone) — the selection that follows
 *   then emits ITS eos argument, eos[0], for that row, which is how a row ends on any id of an eos set.
 * An id without a column (the eos of an embedding table padded past V, a placeholder) is never used as an index and still
 * takes part in n-gram and word matching.  Elements the rule does not name keep their bits; columns V .. logits_ld are not
 * touched.  A barrier separates the penalty from the bans, so a banned id ends at -inf; plain stores, no atomics: the same bits
 * on every run.  hist, eos, bans, word_ids and word_off (int64, n_words + 1 offsets) are DEVICE arrays; a list of no entries
 * may be NULL, hist too when n_hist == 0.  Checked before any launch: CMB_ERR_BAD_ARG for logits NULL, a negative count, a
 * missing list, n_word_ids < n_words, B < 1, V < 1 or > 2^31 - 1, logits_ld < V, hist_ld < n_hist, penalty not finite or <= 0,
 * ngram < 0, min_new < 0; then CMB_ERR_ALIGNMENT for logits not 4-byte or an int64 array not 8-byte aligned (any row stride
 * and any row alignment of the logits are taken). */
int cmb_decode_process(float* logits, int64_t logits_ld, int32_t B, int64_t V, const int64_t* hist, int64_t hist_ld,
                       int64_t n_hist, float penalty, int64_t ngram, int64_t min_new, const int64_t* eos, int32_t n_eos,
                       const int64_t* bans, int32_t n_bans, const int64_t* word_ids, int64_t n_word_ids, const int64_t* word_off,
                       int32_t n_words, uint8_t* done, void* stream);
/* Beam search between two decode steps: cmb_decode_next's place in the loop when rows = prompts * num_beams rows of a decode step
 * are the beams of `prompts` prompts (row r = prompt * num_beams + slot).  HF GenerationMixin._beam_search with do_sample = False,
 * length_penalty = 1, early_stopping = False, equal scores ordered by the lowest index; restated in torch in
 * cambrian_amd/model/language_model/beam.py, the per-prompt step is cmb_beam_step of csrc/decode_beam_core.h.  Per prompt, with
 * K = 2 num_beams and step s (0-based; the last step is s + 1 == max_new):
 *   score[beam, tok] = run_score[beam] + log_softmax(logits[beam])[tok]   fp32; the log-sum-exp from fixed-point masses
 *   the K largest under (score descending, beam * V + tok ascending); a candidate hits when tok == eos (eos = -1: none) or on
 *   the last step; the running beams are the top num_beams of score - 1e9 * hit; candidates ranked < num_beams that hit become
 *   hypotheses of score / (s + 1) (1e9 lower once the early-stop flag is satisfied), merged behind the kept ones, the top
 *   num_beams kept; unsat &= any(run_score[0] / (s + 1) > (fin_ok ? min(fin_score) : -1e9)).
 * A row contributes its min(K, V) largest LOGITS (equal logits by the lowest index): the prompt's top K scores are among them
 * unless two different logits at a row's cut round to the same score.  A NaN or +inf logit is outside the contract (CMB_OK,
 * every index in range).
 * state: ONE block of cmb_decode_beam_state_bytes(prompts, num_beams, max_new) bytes, 16-byte aligned, allocated and
 * zero-initialised by the caller once per generate() call and passed to every step; step 0 reads none of it.  Sections in this
 * order, each starting at a multiple of 16 bytes (csrc/decode_beam_core.h: cmb_beam_make_layout), R = rows, M = max_new:
 *   float run_score[R]; float fin_score[R]; int32 fin_len[R]; int32 parent[R]; int32 tok[R]; float cand_lp[R][K];
 *   int32 cand_tok[R][K]; uint8 fin_ok[R]; uint8 unsat[prompts]; uint8 all_hit[prompts]; int64 run_ids[2][R][M];
 *   int64 fin_ids[R][M]
 * run_score / run_ids: the running beams, best first; after step s the sequences are in half (s + 1) & 1, s + 1 tokens each.
 * fin_*: the kept hypotheses, best first; fin_len counts the generated tokens, the eos included.  parent / tok: the slot each
 * running beam continued in this step and the token it appended.
 * Then, per row: pos = n_tok + step, key_valid[r * kv_ld + t] = 1, x[r] = embed[tok] (cmb_decode_next's tail), and with d / layers
 * (cmb_decode_step's descriptors, both or neither NULL; d->B == rows) cmb_decode_beam_reorder on columns L0 .. t - 1; `unfinished`
 * (one DEVICE byte) = any(unsat) && !all(all_hit): whether the search goes on; cos_t / sin_t = cmb_rope_table(pos).
 * Three launches + the RoPE-table launch, integer LDS atomics only: the same bits on every run, a prompt's result independent of
 * the other prompts.  Checked before any launch, in this order: CMB_ERR_BAD_ARG for state / unfinished NULL or only one of
 * d / layers, then cmb_decode_next's rules in its order with rows for B and max_new for out_ld, then num_beams outside 2 .. 16,
 * rows % num_beams, V < 2, V * num_beams >= 2^31; CMB_ERR_WORKSPACE for state_bytes below the need; CMB_ERR_BAD_ARG for a cache
 * description out of rule (below); CMB_ERR_ALIGNMENT as cmb_decode_next, state not 16-byte aligned, then the caches'.
 * cmb_decode_beam_reorder: in every layer's K and V cache [rows, nkv, Lmax, hd] (d: B = rows, nkv, hd, c_sb / c_sh / c_st; layers:
 * kcache / vcache; nothing else is read) and for every generated column L0 <= c < t, row prompt * num_beams + i takes the values
 * of row prompt * num_beams + parent[that row], in place; parent: int32 [rows] in DEVICE memory, a value outside
 * 0 .. num_beams - 1 leaves its row as it is.  No other byte is written.  CMB_ERR_BAD_ARG: a NULL pointer, B outside 1 .. 16 or no
 * multiple of num_beams, layers < 1, nkv < 1, hd < 8 or hd % 8, a negative stride, c_st < hd, L0 outside 0 .. t;
 * CMB_ERR_ALIGNMENT: a cache stride that is no multiple of 8 elements, a cache pointer not 16-byte aligned. */
int64_t cmb_decode_beam_state_bytes(int32_t prompts, int32_t num_beams, int64_t max_new);
int cmb_decode_beam(const float* logits, int64_t logits_ld, int32_t rows, int32_t num_beams, int64_t V, int64_t eos, void* state,
                    int64_t state_bytes, int64_t step, int64_t max_new, const int64_t* n_tok, int64_t* pos, uint8_t* key_valid,
                    int64_t kv_ld, int64_t t, const void* embed, int64_t embed_ld, int64_t embed_rows, int64_t H, void* x,
                    int64_t x_ld, int32_t hd, float rope_base, float* cos_t, float* sin_t, const cmb_decode_step_desc* d,
                    const cmb_decode_layer* layers, int64_t L0, uint8_t* unfinished, void* stream);
int cmb_decode_beam_reorder(const cmb_decode_step_desc* d, const cmb_decode_layer* layers, const int32_t* parent,
                            int32_t num_beams, int64_t L0, int64_t t, void* stream);
/* Backward of h = silu(g) * u (Llama MLP gate; forward is cmb_act_mul with CMB_ACT_SILU):
 * dg = dh * u * silu'(g), du = dh * silu(g); all [rows, D] with row strides. */
int cmb_swiglu_bwd(int dtype, const void* dh, int64_t lddh, const void* g, int64_t ldg, const void* u, int64_t ldu,
                   int64_t rows, int64_t D, void* dg, int64_t lddg, void* du, int64_t lddu, void* stream);

/* ------------------------------------------------------------------------------------------
 * Image pre-processing on the step boundary
 * replaces, per sample and per tower:  train_fsdp.py:985-1008 / mm_utils.py:153-165,183-201
 *     image_aux = expand2square(image, tuple(int(x*255) for x in processor.image_mean)).resize((R, R))
 *     image_aux = processor.preprocess(image_aux, return_tensors='pt')['pixel_values'][0]
 * i.e. letter-box to a square with the tower's mean colour, Pillow's two-pass fixed-point bicubic
 * resample (libImaging/Resample.c, 22-bit coefficients, uint8 intermediate), then the processor's pointwise
 * rescale + normalise, emitted planar [3,R,R].  Integer work: results are bit-identical to Pillow's; the
 * pointwise stage is a caller-built table lut[c][level] (fp32), so it reproduces whichever processor flavour
 * (HF rescale/normalize or torchvision ToTensor/Normalize) the tower uses exactly.
 * One launch pair handles a whole batch x all towers through a job table.
 * ---------------------------------------------------------------------------------------- */
enum { CMB_F16 = 2 };          /* extra output element type of cmb_image_preprocess only */

typedef struct cmb_image_job {
  int64_t src_off;     /* byte offset of this sample's uint8 [h, w, 3] pixels in `src` */
  int64_t tmp_off;     /* byte offset (multiple of 4) of this job's scratch planes [3, side, pitch] in `tmp`,
                          pitch = (out_side + 3) & ~3; unused when ksize == 0 */
  int64_t dst_off;     /* element offset of this job's [3, out_side, out_side] output in `dst` */
  int32_t w, h;        /* source size */
  int32_t side;        /* max(w, h): the letter-boxed square (mm_utils.py:153-165) */
  int32_t off_x, off_y;/* where the source sits inside the square: ((side-w)/2, 0) or (0, (side-h)/2) */
  int32_t out_side;    /* R */
  int32_t ksize;       /* taps per output; 0 = side == out_side, Image.resize returns a copy */
  int32_t coef_off;    /* int32 offset of this job's tap-major coefficients [ksize, out_side] in `coefs` */
  int32_t bounds_off;  /* int32 offset of this job's [out_side, 2] (first, count) in `bounds` */
  int32_t lut_off;     /* element offset of this tower's fp32 [3, 256] table in `lut` */
  uint32_t background; /* r | g << 8 | b << 16 */
  int32_t reserved;
} cmb_image_job;

/* HOST function (no device work): taps of Pillow's bicubic resample of `in_size` -> `out_size` samples over the
 * full box.  Returns ksize = 2*ceil(2*max(in/out,1)) + 1, or a negative status.  With non-null outputs fills
 * bounds [out_size, 2] = (first, count) and coefs [ksize, out_size] (tap-major, 22-bit fixed point, zero beyond
 * count).  Follows precompute_coeffs + normalize_coeffs_8bpc; double precision, no contraction. */
int cmb_resize_coeffs(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* coefs);
/* Runs the horizontal pass (src -> tmp) and the vertical + table pass (tmp -> dst) for n_jobs jobs.
 * jobs_dev / jobs_host are the same table in device and host memory (the host copy sizes the grids).
 * out_dtype: CMB_BF16 | CMB_F32 | CMB_F16 (table value rounded to nearest even). */
int cmb_image_preprocess(const cmb_image_job* jobs_dev, const cmb_image_job* jobs_host, int32_t n_jobs,
                         const uint8_t* src, const int32_t* bounds, const int32_t* coefs, const float* lut,
                         int32_t out_dtype, uint8_t* tmp, void* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CAMBRIAN_AMD_H */
