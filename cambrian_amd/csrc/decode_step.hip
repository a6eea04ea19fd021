// decode_step.hip — one token's pass through the whole decoder issued from ONE host call (cmb_decode_step): the launches of
// the five-launch decode layer (cambrian_llama.py decode_layer_fused: norm + QKV linear, cmb_decode_attn, o_proj + skip,
// norm + gate / up + SwiGLU, down_proj + skip) for every layer, then final norm + lm_head into fp32 logits.  There is no
// kernel in this file: it calls cmb_decode_linear / _fp8 / _fp4 / cmb_decode_attn with the arguments the Python
// path passes, on one stream, so logits and caches carry the same bits; what it removes is the host work between launches
// (per launch: the binding's predicates, two or three ctypes queries and a tensor allocation, for 32 layers).
// Ordering comes from the stream alone.  Buffers: decode_step_layout.h.
// cmb_decode_step_kv8 is the same body with cmb_decode_attn_kv8 (e4m3 K / V caches, decode_attn_kv8.hip) as launch 1.
#include "common.h"
#include "decode_step_layout.h"

namespace {

inline bool aligned4(const void* p) { return (((uintptr_t)p) & 3u) == 0; }

// the attention launch's workspace need at slot t (cmb_decode_attn_ws: 0 when it runs unsplit), < 0: a status
inline int64_t ds_attn_floats(int64_t B, int32_t nh, int32_t nkv, int32_t hd, int64_t t) {
  return cmb_decode_attn_ws(B, nh, nkv, hd, t, 0);
}

inline bool ds_geometry_ok(int32_t B, int32_t H, int32_t I, int32_t nh, int32_t nkv, int32_t hd, int fp8) {
  if (B < 1 || B > DSL_MAX_B || H < 1 || I < 1 || nh < 1 || nkv < 1 || hd < 1) return false;
  const int64_t nq = (int64_t)nh * hd, nqkv = ((int64_t)nh + 2 * (int64_t)nkv) * hd;
  if (fp8 == 2)
    return cmb_decode_linear_fp4_supported(B, nqkv, H, 0) && cmb_decode_linear_fp4_supported(B, H, nq, 0) &&
           cmb_decode_linear_fp4_supported(B, 2 * (int64_t)I, H, 1) && cmb_decode_linear_fp4_supported(B, H, I, 0);
  if (fp8)
    return cmb_decode_linear_fp8_supported(B, nqkv, H, 0) && cmb_decode_linear_fp8_supported(B, H, nq, 0) &&
           cmb_decode_linear_fp8_supported(B, 2 * (int64_t)I, H, 1) && cmb_decode_linear_fp8_supported(B, H, I, 0);
  return cmb_decode_linear_supported(B, nqkv, H, 0) && cmb_decode_linear_supported(B, H, nq, 0) &&
         cmb_decode_linear_supported(B, 2 * (int64_t)I, H, 1) && cmb_decode_linear_supported(B, H, I, 0);
}

struct DsLinear {
  const void* w;
  int64_t ld;
  const void* scale;       // e4m3: fp32 row factors; MXFP4: e8m0 bytes, rows K / 32 apart
};

inline int ds_linear(int fp8, const void* x, int64_t x_ld, int32_t M, const void* norm_w, float eps, const DsLinear& w,
                     int64_t N, int64_t K, int32_t act, const void* res, int64_t r_ld, void* out, int64_t o_ld,
                     int32_t out_f32, void* stream) {
  if (fp8 == 2)
    return cmb_decode_linear_fp4(x, x_ld, M, norm_w, eps, w.w, w.ld, w.scale, K / 32, N, K, act, res, r_ld, out, o_ld, out_f32,
                                 stream);
  if (fp8)
    return cmb_decode_linear_fp8(x, x_ld, M, norm_w, eps, w.w, w.ld, w.scale, N, K, act, res, r_ld, out, o_ld, out_f32, stream);
  return cmb_decode_linear(x, x_ld, M, norm_w, eps, w.w, w.ld, N, K, act, res, r_ld, out, o_ld, out_f32, stream);
}

// a weight's pointer rules: [N, K] with row stride ld (elements, bytes of e4m3, or bytes of two e2m1 each); 0 = fine, else
// the status
inline int ds_weight_status(int fp8, const DsLinear& w, int64_t K) {
  if (!w.w || (fp8 && !w.scale)) return CMB_ERR_BAD_ARG;
  if (w.ld < (fp8 == 2 ? K / 2 : K) || w.ld % (fp8 ? 16 : 8)) return CMB_ERR_BAD_ARG;
  if (!cmb_aligned16(w.w) || (fp8 == 1 && !aligned4(w.scale))) return CMB_ERR_ALIGNMENT;
  return CMB_OK;
}

}  // namespace

extern "C" int64_t cmb_decode_step_ws(int32_t B, int32_t H, int32_t I, int32_t nh, int32_t nkv, int32_t hd, int64_t t_max) {
  if (B < 1 || B > DSL_MAX_B || H < 1 || I < 1 || t_max < 0) return CMB_ERR_BAD_ARG;
  const int64_t attn = ds_attn_floats(B, nh, nkv, hd, t_max);
  if (attn < 0) return attn;
  return dsl_make(B, H, I, nh, nkv, hd, attn).total;
}

namespace {

// cmb_decode_step (kv8 == nullptr: bf16 caches, element strides) and cmb_decode_step_kv8 (kv8[l]: layer l's factor arrays;
// the caches are e4m3 bytes and d->c_s* byte strides): one body, launch 1 of a layer is the only difference
int ds_step(const cmb_decode_step_desc* d, const cmb_decode_layer* layers, const cmb_decode_kv8_factors* kv8, int64_t i_sb,
            int64_t i_sh, const void* x, int64_t x_ld, const float* cos_t, const float* sin_t, int64_t t,
            const uint8_t* key_valid, int64_t kv_ld, float* ws, int64_t ws_floats, float* logits, int64_t logits_ld,
            void* stream) {
  // ---- every rule before any launch ----
  if (!d || !layers || !x || !cos_t || !sin_t || !key_valid || !ws || !logits) return CMB_ERR_BAD_ARG;
  if (d->layers < 1 || d->B < 1 || d->B > DSL_MAX_B) return CMB_ERR_BAD_ARG;
  if (d->fp8 < 0 || d->fp8 > 2) return CMB_ERR_BAD_ARG;
  const int fp8 = d->fp8;          // 0: bf16, 1: e4m3 with row factors, 2: MXFP4 with e8m0 block scales
  const int32_t B = d->B, H = d->H, I = d->I, nh = d->nh, nkv = d->nkv, hd = d->hd;
  if (!ds_geometry_ok(B, H, I, nh, nkv, hd, fp8)) return CMB_ERR_BAD_ARG;
  if (d->V < 1 || !(fp8 == 2 ? cmb_decode_linear_fp4_supported(B, d->V, H, 0)
                             : fp8 ? cmb_decode_linear_fp8_supported(B, d->V, H, 0) : cmb_decode_linear_supported(B, d->V, H, 0)))
    return CMB_ERR_BAD_ARG;
  if (!(d->eps >= 0.f) || t < 0 || kv_ld < t + 1 || nkv > 65535) return CMB_ERR_BAD_ARG;
  if (x_ld < H || x_ld % 8 || logits_ld < d->V || logits_ld % 8) return CMB_ERR_BAD_ARG;
  if (d->c_sb < 0 || d->c_sh < 0 || d->c_st < hd) return CMB_ERR_BAD_ARG;
  if (kv8 && (i_sb < 0 || i_sh < 0)) return CMB_ERR_BAD_ARG;
  const int64_t attn = ds_attn_floats(B, nh, nkv, hd, t);
  if (attn < 0) return CMB_ERR_BAD_ARG;
  const int64_t nq = (int64_t)nh * hd, nk = (int64_t)nkv * hd, nqkv = nq + 2 * nk;
  const DsLinear head = {d->head, d->ld_head, d->head_scale};
  if (!d->final_norm) return CMB_ERR_BAD_ARG;
  int rc = ds_weight_status(fp8, head, H), align = CMB_OK;
  if (rc == CMB_ERR_BAD_ARG) return rc;
  if (rc != CMB_OK) align = rc;
  for (int32_t l = 0; l < d->layers; ++l) {
    const cmb_decode_layer& L = layers[l];
    if (!L.norm1 || !L.norm2 || !L.kcache || !L.vcache) return CMB_ERR_BAD_ARG;
    const DsLinear w[4] = {{L.w_qkv, L.ld_qkv, L.w_qkv_scale}, {L.w_o, L.ld_o, L.w_o_scale},
                           {L.w_gate_up, L.ld_gate_up, L.w_gate_up_scale}, {L.w_down, L.ld_down, L.w_down_scale}};
    const int64_t K[4] = {H, nq, H, I};
    for (int i = 0; i < 4; ++i) {
      rc = ds_weight_status(fp8, w[i], K[i]);
      if (rc == CMB_ERR_BAD_ARG) return rc;
      if (rc != CMB_OK) align = rc;
    }
    if (!cmb_aligned16(L.norm1) || !cmb_aligned16(L.norm2) || !cmb_aligned16(L.kcache) || !cmb_aligned16(L.vcache))
      align = CMB_ERR_ALIGNMENT;
    if (kv8) {
      if (!kv8[l].k_inv || !kv8[l].v_inv) return CMB_ERR_BAD_ARG;
      if (!aligned4(kv8[l].k_inv) || !aligned4(kv8[l].v_inv)) align = CMB_ERR_ALIGNMENT;
    }
  }
  const int cs_mult = kv8 ? 16 : 8;      // 16 bytes either way
  if (align != CMB_OK || !cmb_aligned16(x) || !cmb_aligned16(ws) || !cmb_aligned16(logits) || !cmb_aligned16(d->final_norm) ||
      d->c_sb % cs_mult || d->c_sh % cs_mult || d->c_st % cs_mult)
    return CMB_ERR_ALIGNMENT;
  const dsl_layout lay = dsl_make(B, H, I, nh, nkv, hd, attn);
  if (ws_floats < lay.total) return CMB_ERR_WORKSPACE;
  {  // the caller's x is read by layer 0 while the workspace is being written
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + ((uintptr_t)(B - 1) * x_ld + H) * 2;
    const uintptr_t w0 = (uintptr_t)ws, w1 = w0 + (uintptr_t)lay.total * 4;
    if (x0 < w1 && w0 < x1) return CMB_ERR_BAD_ARG;
  }

  // ---- launches ----
  void* buf[DSL_BUFS];
  int64_t ld[DSL_BUFS];
  for (int i = 0; i < DSL_BUFS; ++i) {
    buf[i] = ws + lay.off[i];
    ld[i] = 0;
  }
  buf[DSL_EXT_X] = const_cast<void*>(x);
  ld[DSL_EXT_X] = x_ld;
  ld[DSL_QKV] = lay.ld_qkv;
  ld[DSL_ATTN] = lay.ld_attn;
  ld[DSL_RES0] = ld[DSL_RES1] = lay.ld_res;
  ld[DSL_INNER] = lay.ld_inner;
  float* partial = attn > 0 ? (float*)buf[DSL_PARTIAL] : nullptr;

  for (int32_t l = 0; l < d->layers; ++l) {
    const cmb_decode_layer& L = layers[l];
    const DsLinear w_qkv = {L.w_qkv, L.ld_qkv, L.w_qkv_scale}, w_o = {L.w_o, L.ld_o, L.w_o_scale};
    const DsLinear w_gu = {L.w_gate_up, L.ld_gate_up, L.w_gate_up_scale}, w_down = {L.w_down, L.ld_down, L.w_down_scale};
    int xi, ri, oi;
    dsl_launch_bufs(l, 0, &xi, &ri, &oi);
    rc = ds_linear(fp8, buf[xi], ld[xi], B, L.norm1, d->eps, w_qkv, nqkv, H, 0, nullptr, 0, buf[oi], ld[oi], 0, stream);
    if (rc != CMB_OK) return rc;
    dsl_launch_bufs(l, 1, &xi, &ri, &oi);
    const bf16_t* row = (const bf16_t*)buf[xi];
    if (kv8)
      rc = cmb_decode_attn_kv8(row, ld[xi], row + nq, ld[xi], row + nq + nk, ld[xi], cos_t, sin_t, L.kcache, L.vcache, d->c_sb,
                               d->c_sh, d->c_st, kv8[l].k_inv, kv8[l].v_inv, i_sb, i_sh, B, nh, nkv, hd, t, key_valid, kv_ld,
                               d->scale, 0, partial, attn, buf[oi], stream);
    else
      rc = cmb_decode_attn(CMB_BF16, row, ld[xi], row + nq, ld[xi], row + nq + nk, ld[xi], cos_t, sin_t, L.kcache, L.vcache,
                           d->c_sb, d->c_sh, d->c_st, B, nh, nkv, hd, t, key_valid, kv_ld, d->scale, 0, partial, attn, buf[oi],
                           stream);
    if (rc != CMB_OK) return rc;
    dsl_launch_bufs(l, 2, &xi, &ri, &oi);
    rc = ds_linear(fp8, buf[xi], ld[xi], B, nullptr, 0.f, w_o, H, nq, 0, buf[ri], ld[ri], buf[oi], ld[oi], 0, stream);
    if (rc != CMB_OK) return rc;
    dsl_launch_bufs(l, 3, &xi, &ri, &oi);
    rc = ds_linear(fp8, buf[xi], ld[xi], B, L.norm2, d->eps, w_gu, 2 * (int64_t)I, H, 1, nullptr, 0, buf[oi], ld[oi], 0,
                   stream);
    if (rc != CMB_OK) return rc;
    dsl_launch_bufs(l, 4, &xi, &ri, &oi);
    rc = ds_linear(fp8, buf[xi], ld[xi], B, nullptr, 0.f, w_down, H, I, 0, buf[ri], ld[ri], buf[oi], ld[oi], 0, stream);
    if (rc != CMB_OK) return rc;
  }
  const int hi = dsl_head_in();
  return ds_linear(fp8, buf[hi], ld[hi], B, d->final_norm, d->eps, head, d->V, H, 0, nullptr, 0, logits, logits_ld, 1, stream);
}

}  // namespace

extern "C" int cmb_decode_step(const cmb_decode_step_desc* d, const cmb_decode_layer* layers, const void* x, int64_t x_ld,
                               const float* cos_t, const float* sin_t, int64_t t, const uint8_t* key_valid, int64_t kv_ld,
                               float* ws, int64_t ws_floats, float* logits, int64_t logits_ld, void* stream) {
  return ds_step(d, layers, nullptr, 0, 0, x, x_ld, cos_t, sin_t, t, key_valid, kv_ld, ws, ws_floats, logits, logits_ld, stream);
}

extern "C" int cmb_decode_step_kv8(const cmb_decode_step_desc* d, const cmb_decode_layer* layers,
                                   const cmb_decode_kv8_factors* factors, int64_t i_sb, int64_t i_sh, const void* x, int64_t x_ld,
                                   const float* cos_t, const float* sin_t, int64_t t, const uint8_t* key_valid, int64_t kv_ld,
                                   float* ws, int64_t ws_floats, float* logits, int64_t logits_ld, void* stream) {
  if (!factors) return CMB_ERR_BAD_ARG;
  return ds_step(d, layers, factors, i_sb, i_sh, x, x_ld, cos_t, sin_t, t, key_valid, kv_ld, ws, ws_floats, logits, logits_ld,
                 stream);
}
