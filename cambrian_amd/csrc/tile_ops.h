// tile_ops.h — the small device helpers of the LDS-DMA / transposing-read operand path, shared by flash2.hip, flash_bwd.hip,
// vit_attn.hip, sva_absorbed.hip and gemm_tn.hip.  (gemm_p5*.hip and gemm256.hip keep private copies of the pointer helper and
// the fence: the PMC summaries under profiles/ are keyed by a hash of those sources.)
#pragma once
#include "common.h"

// nothing is scheduled across this point: fixes the order of the LDS reads, MFMAs and vector arithmetic around it
#define CMB_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)

typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef short s16x8_t __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4_t* lds_tr_ptr;

// ds_read_b64_tr_b16 at LDS address p: four 16-bit elements of ONE column out of a row-major [4][16] block
__device__ __forceinline__ s16x4_t lds_read_tr16(const char* p) { return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)p); }

// two fp32 -> one packed bf16 pair (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t cvt2_bf16(float a, float b) {
  typedef __bf16 bf16x2_v __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2_t){a, b}, bf16x2_v));
}

// a 64-bit pointer the compiler may keep in scalar registers (the caller knows it is the same in every lane)
__device__ __forceinline__ const char* wave_uniform_ptr(const char* q) {
  const uint64_t v = (uint64_t)q;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (const char*)(((uint64_t)hi << 32) | lo);
}

// one LDS-DMA piece: 64 lanes x 16 bytes from base + voff (per lane) to LDS byte address lds (wave-uniform), lane-linear
__device__ __forceinline__ void lds_dma_piece(const char* base, uint32_t voff, uint32_t lds) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
               :
               : "v"(voff), "s"(base), "s"(lds)
               : "memory", "m0");
}
