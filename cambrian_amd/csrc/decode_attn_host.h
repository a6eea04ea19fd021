// decode_attn_host.h — the host side that cmb_decode_attn, cmb_decode_attn_kv8, cmb_decode_attn_multi and cmb_extend_attn share:
// the argument checks that run before a launch, the workspace need, the base-2 scale and the launch of decode_combine_kernel.  Host code
// only; included after decode_attn_common.h.  Each launcher keeps the ORDER of its checks (a call that breaks two rules gets the
// status it always got, and the three look at B == 0 at different points), so the pieces here are predicates, not a sequence.
#pragma once
#include <initializer_list>

// The geometry rule and the split plan live in decode_attn.hip (the CU count behind the plan is cached in that translation
// unit); these two are how the other files reach them.  Not extern "C": exports.map keeps them inside the library.
// dtype bf16 / fp32, head_dim 64 / 96 / 128, nh a multiple of nkv with at most DEC_MAX_GROUP query heads per KV head
bool dec_geometry_ok(int dtype, int32_t nh, int32_t nkv, int32_t hd);
// cmb_decode_attn_plan for a step that owns slots t0 .. t0 + n - 1: the plan over slots 0 .. t0 + n - 1, every output optional.
// CMB_ERR_BAD_ARG: B < 1, nkv < 1, t0 < 0, n < 1 or `forced` outside 0 .. DEC_MAX_SPLITS
int dec_plan_slots(int64_t B, int32_t nkv, int64_t t0, int64_t n, int32_t forced, int32_t* splits_out, int64_t* chunk_out,
                   int32_t* max_splits_out);

namespace {

constexpr float DEC_LOG2E = 1.4426950408889634f;   // scores live in the base-2 exponent domain: the kernels take scale * log2(e)

// fp32 elements of the split partials, (acc[hd], m, l) per query row (counted over batch, tokens and heads) and chunk
inline int64_t dec_ws_need(int64_t rows, int32_t s, int32_t hd) { return s == 1 ? 0 : rows * s * (int64_t)(hd + 2); }

inline bool dec_all_set(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (!p) return false;
  return true;
}

// the batch and KV heads fit the grid, and the key mask's rows cover the step's slots t0 .. t0 + n - 1
inline bool dec_range_ok(int64_t B, int32_t nkv, int64_t t0, int64_t n, int64_t kv_ld) {
  return B >= 0 && B <= 65535 && nkv <= 65535 && t0 >= 0 && kv_ld >= t0 + n;
}

// 16-byte pointers, and row strides of `es`-byte elements that keep every row so
inline bool dec_aligned16(std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> strides, int64_t es) {
  for (const void* p : ptrs)
    if (!cmb_aligned16(p)) return false;
  for (int64_t ld : strides)
    if ((ld * es) % 16) return false;
  return true;
}

// the second launch of a split run of the single-token kernels; rows = B * nh
template <typename T>
inline void dec_launch_combine(int64_t rows, const float* ws, int G, int32_t hd, int32_t s, void* out, hipStream_t st) {
  hipLaunchKernelGGL(decode_combine_kernel<T>, dim3((unsigned)rows), dim3(128), 0, st, ws, G, (int)hd, (int)s, (T*)out);
}

}  // namespace
