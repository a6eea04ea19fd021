// decode_step_layout.h — the workspace of cmb_decode_step (decode_step.hip) and which buffer every launch of a decoder layer
// reads and writes, free of HIP types so that tests/csrc/decode_step_layout_sim.cpp runs the very same functions on the host.
//
// One token's pass through the decoder is a chain of launches on one stream; what the Python five-launch path keeps in fresh
// tensors lives here in one fp32 workspace, cut into (offsets and sizes in FLOATS, every offset a multiple of 4 = 16 bytes;
// a bf16 row of n elements takes dsl_row(n) / 2 floats):
//   qkv      bf16 [B, dsl_row((nh + 2 nkv) hd)]   the packed projection row: q heads | k heads | v heads
//   attn     bf16 [B, nh hd]                      cmb_decode_attn's output (contiguous rows, its contract)
//   res[2]   bf16 [B, dsl_row(H)] each            the residual stream
//   inner    bf16 [B, dsl_row(I)]                 silu(gate) * up
//   partial  fp32 [attn_floats]                   cmb_decode_attn's split partials (cmb_decode_attn_ws at the largest t)
// Row strides are multiples of 8 elements, the rule of cmb_decode_linear's x / out / residual.  `partial` comes last, so
// no other offset depends on t.
//
// Launches of layer l (DSL_LAUNCHES per layer) and their buffers — x operand, residual operand, output:
//   0  norm + QKV linear          x = in(l)    res = -        out = qkv
//   1  attention on the cache     x = qkv      res = -        out = attn
//   2  o_proj + skip              x = attn     res = in(l)    out = res[0]
//   3  norm + gate / up + SwiGLU  x = res[0]   res = -        out = inner
//   4  down_proj + skip           x = inner    res = res[0]   out = res[1]
// in(0) is the caller's x (outside the workspace), in(l > 0) = res[1], the previous layer's output; the final norm + lm_head
// launch reads res[1] and writes the caller's logits.  Launch 4 of layer l > 0 overwrites in(l), which launch 2 was the
// last to read: no launch's output is its own x or residual (dsl_launch_bufs + the sim's check over every layer).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSL_HD __host__ __device__ static inline
#else
#define DSL_HD static inline
#endif

#define DSL_MAX_B 16
#define DSL_LAUNCHES 5

enum dsl_buf { DSL_NONE = -1, DSL_EXT_X = 0, DSL_QKV = 1, DSL_ATTN = 2, DSL_RES0 = 3, DSL_RES1 = 4, DSL_INNER = 5,
               DSL_PARTIAL = 6, DSL_BUFS = 7 };

typedef struct dsl_layout {
  int64_t ld_qkv, ld_attn, ld_res, ld_inner;       /* row strides in bf16 elements */
  int64_t off[DSL_BUFS], size[DSL_BUFS];           /* floats; off[DSL_EXT_X] = size[DSL_EXT_X] = 0 (not in the workspace) */
  int64_t total;                                   /* floats */
} dsl_layout;

DSL_HD int64_t dsl_row(int64_t n) { return (n + 7) / 8 * 8; }                 /* bf16 elements, a multiple of 8 */
DSL_HD int64_t dsl_bf16_floats(int64_t rows, int64_t ld) { return (rows * ld / 2 + 3) / 4 * 4; }   /* ld is even */

DSL_HD dsl_layout dsl_make(int64_t B, int64_t H, int64_t I, int64_t nh, int64_t nkv, int64_t hd, int64_t attn_floats) {
  dsl_layout L;
  L.ld_qkv = dsl_row((nh + 2 * nkv) * hd);
  L.ld_attn = dsl_row(nh * hd);
  L.ld_res = dsl_row(H);
  L.ld_inner = dsl_row(I);
  for (int i = 0; i < DSL_BUFS; ++i) L.off[i] = L.size[i] = 0;
  L.size[DSL_QKV] = dsl_bf16_floats(B, L.ld_qkv);
  L.size[DSL_ATTN] = dsl_bf16_floats(B, L.ld_attn);
  L.size[DSL_RES0] = L.size[DSL_RES1] = dsl_bf16_floats(B, L.ld_res);
  L.size[DSL_INNER] = dsl_bf16_floats(B, L.ld_inner);
  L.size[DSL_PARTIAL] = (attn_floats + 3) / 4 * 4;
  int64_t at = 0;
  for (int i = DSL_QKV; i < DSL_BUFS; ++i) {
    L.off[i] = at;
    at += L.size[i];
  }
  L.total = at;
  return L;
}

/* where layer l's input lives */
DSL_HD int dsl_layer_in(int layer) { return layer == 0 ? DSL_EXT_X : DSL_RES1; }

/* launch j of layer l: its x operand, its residual operand (DSL_NONE: none) and its output */
DSL_HD void dsl_launch_bufs(int layer, int j, int* x, int* res, int* out) {
  const int in = dsl_layer_in(layer);
  switch (j) {
    case 0: *x = in;        *res = DSL_NONE; *out = DSL_QKV;   break;
    case 1: *x = DSL_QKV;   *res = DSL_NONE; *out = DSL_ATTN;  break;
    case 2: *x = DSL_ATTN;  *res = in;       *out = DSL_RES0;  break;
    case 3: *x = DSL_RES0;  *res = DSL_NONE; *out = DSL_INNER; break;
    default: *x = DSL_INNER; *res = DSL_RES0; *out = DSL_RES1; break;
  }
}
/* the final norm + lm_head launch reads the last layer's output */
DSL_HD int dsl_head_in(void) { return DSL_RES1; }
