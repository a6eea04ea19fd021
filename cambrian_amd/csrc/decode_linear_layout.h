// decode_linear_layout.h — who reads which k in decode_linear.hip, and the row-slab plan, free of HIP types so that
// tests/csrc/decode_linear_layout_sim.cpp runs the very same functions on the host.
//
// A workgroup owns a slab of 8 * T weight rows (T tiles of 8 rows); its four waves take the 64-element k-steps round robin
// (step s -> wave s & 3).  One load instruction of a wave fetches one tile's 8 rows x 64 k: lane l reads the 8 elements at
// dl_w_k(l) of row dl_w_row(l), so every row is read in one contiguous run of 128 bytes (a full line) per instruction.
// v_mfma_f32_16x16x32_bf16 sums over 32 k only, so the tile is the 16-row operand "8 rows at k 0..31 over the same 8 rows at
// k 32..63", and two MFMAs follow the load: half h multiplies it with x at k 32 h .. 32 h + 31 (lane l supplies row
// dl_x_row(l), elements dl_x_k(h, l) ..+7).  Operand rows 8 h' .. 8 h' + 7 met the right k only in the MFMA h == h'; the
// others are never looked at.  The accumulator of MFMA h holds operand rows 4 (l >> 4) .. +3 in lane l, so lanes 0-31 keep
// their half-0 accumulator and lanes 32-63 their half-1 one (dl_acc_half), both as weight rows dl_acc_row(l, reg), and the
// two halves of a row are two of the eight partials (4 waves x 2 halves) the workgroup sums through LDS.
// No k is permuted inside an MFMA: element e of a lane's fragment is k + e on both operands.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DL_HD __host__ __device__ __forceinline__
#else
#define DL_HD static inline
#endif

#define DL_WAVES 4
#define DL_KSTEP 64      /* k per wave step: two MFMAs of 32 */
#define DL_TILE_ROWS 8
#define DL_MAX_TILES 4   /* slab = 8, 16 or 32 rows */
#define DL_MAX_M 16

DL_HD int dl_step_wave(int64_t step) { return (int)(step & (DL_WAVES - 1)); }
// weight operand: row inside the tile and first k inside the step of lane l's 8 elements
DL_HD int dl_w_row(int lane) { return lane & 7; }
DL_HD int dl_w_k(int lane) { return 32 * ((lane >> 3) & 1) + 8 * (lane >> 4); }
// x operand of MFMA `half`: row of x and first k inside the step of lane l's 8 elements
DL_HD int dl_x_row(int lane) { return lane & 15; }
DL_HD int dl_x_k(int half, int lane) { return 32 * half + 8 * (lane >> 4); }
// accumulators: which MFMA's result lane l keeps, and the weight row (inside the tile) of its register `reg` (0..3)
DL_HD int dl_acc_half(int lane) { return lane >> 5; }
DL_HD int dl_acc_row(int lane, int reg) { return 4 * ((lane >> 4) & 1) + reg; }

// Row-slab plan: tiles per workgroup, a pure function of (M, N, K, CU count) — the largest slab that still leaves
// dl_plan_want workgroups, 8 rows when none does.  Two workgroups per CU for M <= 4; above that one and a half: every
// workgroup reads all of x through the caches, M rows of it, so at M = 16 and 8-row slabs x is twice the weights' traffic
// and fewer, larger slabs are the better trade (N = 4096 keeps two per CU at every M: 16-row slabs would leave one).
// act = 1 (SwiGLU over packed [gate; up] rows): a workgroup owns the same 4 * T gate and up rows, so T is even.  K does
// not enter today.  The order in which a row's k are summed does not depend on the slab, so neither do the result's bits.
DL_HD int64_t dl_plan_wgs(int tiles, int64_t N, int act) {
  const int64_t per = act ? DL_TILE_ROWS * tiles / 2 : DL_TILE_ROWS * tiles;
  const int64_t cols = act ? N / 2 : N;
  return (cols + per - 1) / per;
}
DL_HD int64_t dl_plan_want(int M, int cus) { return M > 4 ? 3 * (int64_t)cus / 2 : 2 * (int64_t)cus; }
DL_HD int dl_plan_tiles(int M, int64_t N, int64_t K, int act, int cus) {
  (void)K;
  const int least = act ? 2 : 1;
  for (int t = DL_MAX_TILES; t > least; t >>= 1)
    if (dl_plan_wgs(t, N, act) >= dl_plan_want(M, cus)) return t;
  return least;
}
