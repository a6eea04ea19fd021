// flash_common.h — parameter block, mask helpers and the host-side argument checks / instantiation choice shared by flash_bwd.hip
// (the round-4 forward and dQ kernels; the dK/dV kernel with its round-5 PIPE / TR variants) and flash2.hip (the round-5
// forward and dQ on LDS-DMA tiles).
#pragma once
#include <type_traits>
#include "common.h"
#include "flash_map.h"

namespace cmb_flash {

constexpr int HD = 128;       // head dim
constexpr int KS = HD / 16;   // MFMA k-steps over the head dim
constexpr int DT = HD / 32;   // 32-wide d tiles
constexpr int LDR = HD + 8;   // row-major LDS tile row stride (elements): conflict-free ds_read_b128
constexpr int LDT = 68;       // transposed LDS tile row stride (elements): conflict-free ds_read_b64
constexpr float LOG2E = 1.4426950408889634f;

struct FlashParams {
  const bf16_t *q, *k, *v, *o, *dout;
  bf16_t *dq, *dk, *dv;
  const float* lse;  // [B, H, S]
  float* dvec;       // [2, B, H, S]: [0] D = rowsum(dO * O); [1] unused since round 6 (was lse * log2 e for the removed flash_dkdv2_kernel)
  int64_t q_sb, q_ss, q_sh;     // strides of q / o / do / dq (elements)
  int64_t kv_sb, kv_ss, kv_sh;  // strides of k / v / dk / dv
  int B, S, H, HKV;
  int kv_len;   // non-causal kernels: keys >= kv_len are padding (masked); S is kv_len rounded up to 128
  float scale;
  // causal kernels: optional key-padding mask, [B, S] bytes, non-zero = the key may be attended to.  A query may see key k
  // iff k <= q and (key_valid[b][k] or k == q): the collator's attention_mask (train_fsdp.py:1057-1085) AND the causal
  // triangle, with the diagonal kept open so that a padded query row is never empty (its loss is ignored).
  const uint8_t* key_valid;
};

// validity bits of the 64 keys of tile t (lane i contributes key 64 t + i); all ones without a mask
__device__ __forceinline__ uint8_t kv_byte(const FlashParams& p, int b, int t, int lane) {
  return p.key_valid ? p.key_valid[(int64_t)b * p.S + t * 64 + lane] : (uint8_t)1;
}

// Which of this lane's 16 keys of one 32-key half tile are open to its query: bit (r & 3) + 8 (r >> 2) <-> accumulator
// element r (key = half tile base + 4 g + that bit index).  `vw` is the tile's 64-bit key-validity ballot; `dq` = the
// lane's query index minus the half tile's first key: the query's own key stays open even when it is padding (the
// diagonal of the collator mask, train_fsdp.py:1057-1085) — folded into the word here so that the per-element test is
// one constant-bit test.
__device__ __forceinline__ uint32_t flash_open_bits(uint64_t vw, int kt, int g, int dq) {
  const uint32_t w = (uint32_t)(vw >> (kt * 32)) >> (4 * g);
  const uint32_t pos = (uint32_t)(dq - 4 * g);  // bit of the query's own key in w (if < 32 and in this lane's groups)
  return w | ((pos < 32u && !(pos & 4u)) ? (1u << pos) : 0u);
}

// ---- host side of cmb_flash_attn_fwd / _bwd -------------------------------------------------------------------------
// The argument checks of both entry points, in their order, and the fields of the parameter block they share (the caller
// tests its further pointers first — every null pointer is CMB_ERR_BAD_ARG, ahead of the other checks — and sets the
// backward's tensors afterwards; they are null here).  CMB_OK with p.B == 0 is an empty batch: nothing to launch.
inline int flash_fill_params(FlashParams& p, const void* q, const void* k, const void* v, int64_t B, int64_t S, int32_t H,
                             int32_t HKV, int32_t hd, int64_t q_sb, int64_t q_ss, int64_t q_sh, int64_t kv_sb, int64_t kv_ss,
                             int64_t kv_sh, float scale, int32_t causal, int64_t kv_len, const uint8_t* key_valid) {
  p = FlashParams{};
  if (!q || !k || !v) return CMB_ERR_BAD_ARG;
  if (hd != HD || S <= 0 || (S % 128) != 0 || H <= 0 || HKV <= 0 || (H % HKV) != 0 || B < 0) return CMB_ERR_SHAPE;
  if (!causal && (kv_len <= 0 || kv_len > S)) return CMB_ERR_SHAPE;
  if (B == 0) return CMB_OK;
  if ((q_ss % 8) || (q_sh % 8) || (q_sb % 8) || (kv_ss % 8) || (kv_sh % 8) || (kv_sb % 8)) return CMB_ERR_ALIGNMENT;
  p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v;
  p.q_sb = q_sb; p.q_ss = q_ss; p.q_sh = q_sh; p.kv_sb = kv_sb; p.kv_ss = kv_ss; p.kv_sh = kv_sh;
  p.B = (int)B; p.S = (int)S; p.H = H; p.HKV = HKV; p.scale = scale; p.kv_len = causal ? (int)S : (int)kv_len;
  p.key_valid = causal ? key_valid : nullptr;
  return CMB_OK;
}

// f(CAUSAL, MASKED) as two std::integral_constant<bool, ...> for the three instantiations the kernels have: causal with a
// key-padding mask, causal, bidirectional (a mask is honoured only when causal)
template <typename F>
inline void flash_dispatch(bool causal, bool masked, F&& f) {
  if (causal && masked) f(std::true_type{}, std::true_type{});
  else if (causal) f(std::true_type{}, std::false_type{});
  else f(std::false_type{}, std::false_type{});
}
// f for each of the three (the hipFuncSetAttribute loops)
template <typename F>
inline void flash_dispatch_all(F&& f) {
  for (int i = 0; i < 3; ++i) flash_dispatch(i < 2, i == 0, f);
}

// flash2.hip: forward on LDS-DMA operand tiles (flash_layout.h), selected by knob CMB_KNOB_FLASH bit 0
int launch_flash_fwd2(const FlashParams& p, bf16_t* out, float* lse, bool causal, hipStream_t stream);
// flash2.hip: dQ on the same tiles (knob bit 1); it also writes dvec (D = rowsum(dO o O)) for the dK/dV kernel
int launch_flash_dq2(const FlashParams& p, bool causal, hipStream_t stream);

}  // namespace cmb_flash
