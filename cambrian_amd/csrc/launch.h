// launch.h — what the HBM-bound "streaming" units (norm, elementwise, llm_ops, dwconv) share: the two loop headers of their
// kernels and the host-side dtype / NCH / bool dispatch of their entry points.  Everything a kernel sees here is a TEXT macro:
// a shared function or a lambda, even force-inlined, changes scheduling and register allocation of these tuned kernels,
// a macro leaves the compiled kernel as it was (profiles/streaming_refactor_asm.md; DESIGN.md, "Sharing kernel text").
#pragma once
#include "common.h"

// ---- device side: loop headers ---------------------------------------------------------------------------------------
// for each of this lane's vec8 chunks of the row; expects `NCH`, `lane` and `nvec` in scope, declares chunk `c` and vec8 index `vi`
#define FOR_ROW_CHUNKS(c, vi) _Pragma("unroll") for (int c = 0; c < NCH; ++c) if (const int vi = lane + c * 64; vi < nvec)
// for each of the 8 elements of a vec8, unrolled; expects nothing in scope, declares `e`
#define FOR8(e) _Pragma("unroll") for (int e = 0; e < 8; ++e)

// ---- host side: run-time value -> compile-time name ------------------------------------------------------------------
// Each runs the statement(s) given after its first arguments once, in the branch that matches; they nest, so an entry point
// writes ONE argument list per launch.  They are statements of an entry point that returns a cmb status: the failing branch
// returns from it.
// dtype code -> `T` (bf16_t / float); any other code returns CMB_ERR_BAD_ARG
#define DT_SWITCH(dtype, ...)                                    \
  if ((dtype) == CMB_BF16) { typedef bf16_t T; __VA_ARGS__; }    \
  else if ((dtype) == CMB_F32) { typedef float T; __VA_ARGS__; } \
  else return CMB_ERR_BAD_ARG;
// bool -> `constexpr bool NAME`
#define BOOL_SWITCH(flag, NAME, ...)                      \
  if (flag) { constexpr bool NAME = true; __VA_ARGS__; }  \
  else { constexpr bool NAME = false; __VA_ARGS__; }
// one case of a switch over an int -> `constexpr int NAME`
#define INT_CASE(NAME, n, ...) case n: { constexpr int NAME = n; __VA_ARGS__; break; }
// vec8 chunks per lane (nch_for) -> `NCH` in {2, 4, 8, 16}; any other value returns CMB_ERR_SHAPE
#define DISPATCH_NCH(nch, ...)      \
  switch (nch) {                    \
    INT_CASE(NCH, 2, __VA_ARGS__)   \
    INT_CASE(NCH, 4, __VA_ARGS__)   \
    INT_CASE(NCH, 8, __VA_ARGS__)   \
    INT_CASE(NCH, 16, __VA_ARGS__)  \
    default: return CMB_ERR_SHAPE;  \
  }
// the same without NCH = 16, for the kernels whose register budget ends at D = 4096
#define DISPATCH_NCH8(nch, ...)     \
  switch (nch) {                    \
    INT_CASE(NCH, 2, __VA_ARGS__)   \
    INT_CASE(NCH, 4, __VA_ARGS__)   \
    INT_CASE(NCH, 8, __VA_ARGS__)   \
    default: return CMB_ERR_SHAPE;  \
  }

// workgroups of a grid-stride launch: `items` at `per_block` each, clamped to [1, cap]
static inline unsigned grid_for(int64_t items, int64_t per_block, int64_t cap) {
  int64_t b = (items + per_block - 1) / per_block;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (unsigned)b;
}
