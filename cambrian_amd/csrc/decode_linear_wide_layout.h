// decode_linear_wide_layout.h — who reads which k in decode_linear_wide.hip, the regrouping of the weight tiles, the LDS
// reduction's addresses and the row-slab plan, free of HIP types so that tests/csrc/decode_linear_wide_layout_sim.cpp runs
// the very same functions on the host.
//
// x [M <= 64, K] is taken as B = ceil(M / 16) row blocks of the 16-column operand of v_mfma_f32_16x16x32_bf16: lane l
// supplies row 16 b + dlw_x_row(l), elements dlw_x_k(h, l) ..+7 of the k-step's half h.  A workgroup owns a slab of
// 16 P weight rows (P pairs of 8-row tiles, P = 1 or 2); its four waves take the 64-element k-steps round robin.
//
// Loads.  As in decode_linear.hip one load instruction of a wave fetches one tile's 8 rows x 64 k: lane l reads the 8
// elements at dlw_w_k(l) of row dlw_w_row(l), a contiguous run of 128 bytes (a full line) per row and instruction.
// Regrouping.  The narrow kernel multiplies that tile as "8 rows at k 0..31 over the same rows at k 32..63" and throws half
// of every MFMA away, which at four row blocks costs 128 accumulator registers and, under the norm prologue, as many matrix
// cycles as the weight stream leaves.  Here the two tiles of a pair trade their odd 8-lane groups (lane l <-> l ^ 8, a DPP
// row rotation by 8 inside each row of 16 lanes, no LDS): operand h of the pair then holds the pair's 16 rows at
// k 32 h .. 32 h + 31, row dlw_op_row(l) and elements dlw_op_k(h, l) ..+7 in lane l — dlw_op_src says which loaded tile and
// lane that fragment came from.  Every MFMA result is used, the accumulators are 4 P B registers (32 at P = 2, B = 4), and
// a k-step costs 2 P B MFMAs (twice that under the norm): 32 x 16 cycles for 4 KiB of weights at the largest instantiation,
// 8 B per cycle and SIMD, about 2.4x what a CU's share of the HBM stream asks for.
// No k is permuted inside an MFMA: element e of a lane's fragment is k + e on both operands.
//
// Order of a row's sum (the bits of out[m, n]): inside wave w the steps w, w + 4, ... in turn, half 0 then half 1 of each
// (under the norm: the rounded operand, then its remainder), all into one accumulator; then the four waves' partials are
// added in wave order by the thread that owns the element.  Nothing in that order looks at M, at the row block or at the
// slab: a row's bits are a function of (K, its x row, its weight row(s)) alone.  It is NOT decode_linear.hip's order (which
// keeps the two halves apart until the end), so the two kernels agree to rounding, not to the bit.
//
// x traffic.  Every workgroup reads all M rows of x through the caches, each element once (the four waves own disjoint k).
// Staging x in LDS therefore saves nothing: no element is read twice inside a workgroup.  What is left is how many
// workgroups there are.  A split of K across workgroups would need a workspace and a sixth launch per layer (no atomics, no
// flags) and is not taken.  So the slab is the knob: 32 rows wherever that still leaves one workgroup per CU, 16 rows
// otherwise.  At M = 64: down_proj of Llama-3-8B (N 4096, K 14336) 256 workgroups of 16 rows read 470 MB of x from L2
// against 117 MB of weights from HBM; gate / up (N 28672, K 4096) 896 workgroups of 32 rows read 470 MB against 235 MB.
// x itself (at most 1.8 MB here) stays resident in every XCD's L2, whose bandwidth is several times HBM's; a 64-row slab
// would halve that traffic again but leave N = 4096 with 64 workgroups on 256 CUs.
// What was measured (profiles/decode_linear_wide.md) says the reckoning above is too kind: the kernel's time grows with the
// row blocks while the weight bytes stay put (2.2-2.6 TB/s of weights at 64 rows, 3.3-3.8 at 32, against 4.0-4.9 for the
// narrow kernel at 16), so it is bound by x through the CU's vector-memory path — (M / slab rows) x the weight bytes — and,
// under the norm, by splitting x * norm_w again in every workgroup, not by HBM.  Both fall only with slabs of at least M
// rows for every N, which means the split of K across workgroups with a reduction pass; that is the next step, not this.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DLW_HD __host__ __device__ __forceinline__
#else
#define DLW_HD static inline
#endif

#define DLW_WAVES 4
#define DLW_KSTEP 64       /* k per wave step: two halves of 32 */
#define DLW_TILE_ROWS 8    /* weight rows per load instruction */
#define DLW_PAIR_ROWS 16   /* weight rows per MFMA operand: a pair of tiles */
#define DLW_MAX_PAIRS 2    /* slab = 16 or 32 rows */
#define DLW_BLOCK_M 16     /* x rows per row block */
#define DLW_MAX_BLOCKS 4
#define DLW_MAX_M 64

DLW_HD int dlw_blocks(int M) { return (M + DLW_BLOCK_M - 1) / DLW_BLOCK_M; }
DLW_HD int dlw_step_wave(int64_t step) { return (int)(step & (DLW_WAVES - 1)); }
// weight load of one tile: row inside the tile and first k inside the step of lane l's 8 elements
DLW_HD int dlw_w_row(int lane) { return lane & 7; }
DLW_HD int dlw_w_k(int lane) { return 32 * ((lane >> 3) & 1) + 8 * (lane >> 4); }
// weight operand of half h after the regrouping: row inside the pair and first k inside the step of lane l's 8 elements
DLW_HD int dlw_op_row(int lane) { return lane & 15; }
DLW_HD int dlw_op_k(int half, int lane) { return 32 * half + 8 * (lane >> 4); }
// ... and where it came from: the tile of the pair (0 / 1) and the lane that loaded it (the lane itself or lane ^ 8)
DLW_HD int dlw_op_src_tile(int lane) { return (lane >> 3) & 1; }
DLW_HD int dlw_op_src_lane(int half, int lane) { return ((lane >> 3) & 1) == half ? lane : lane ^ 8; }
// x operand of half h, row block b: row of x and first k inside the step of lane l's 8 elements
DLW_HD int dlw_x_row(int lane) { return lane & 15; }
DLW_HD int dlw_x_k(int half, int lane) { return 32 * half + 8 * (lane >> 4); }
// accumulator of (pair, block): x row (inside the block) of lane l and the weight row (inside the pair) of its register reg
DLW_HD int dlw_acc_m(int lane) { return lane & 15; }
DLW_HD int dlw_acc_row(int lane, int reg) { return 4 * (lane >> 4) + reg; }
// LDS partials, floats: [wave][pair][m 0..63][row 0..15] — a lane's four registers are one 16-byte store, and the 64 lanes
// of a store write 64 distinct slots of one contiguous KiB
DLW_HD int dlw_red_index(int pairs, int wave, int pair, int m, int row) {
  return ((wave * pairs + pair) * DLW_MAX_M + m) * DLW_PAIR_ROWS + row;
}
// output column c of the slab (0 .. dlw_slab_cols - 1) -> pair and row of its sum; with act = 1 the gate sum, the up sum
// being the same row of tile + pairs (tiles 0 .. pairs - 1 are gate rows, pairs .. 2 pairs - 1 the matching up rows)
DLW_HD int dlw_slab_cols(int pairs, int act) { return act ? DLW_TILE_ROWS * pairs : DLW_PAIR_ROWS * pairs; }
DLW_HD int dlw_col_tile(int c) { return c / DLW_TILE_ROWS; }
DLW_HD int dlw_tile_pair(int tile) { return tile >> 1; }
DLW_HD int dlw_tile_row(int tile, int r) { return DLW_TILE_ROWS * (tile & 1) + r; }
// weight row of W that lane l loads for tile t of the slab starting at output column col0; rows past the end re-read the last
DLW_HD int64_t dlw_w_index(int pairs, int act, int64_t N, int64_t col0, int tile, int lane) {
  if (act) {
    const int64_t cols = N / 2;
    int64_t j = col0 + DLW_TILE_ROWS * (tile % pairs) + dlw_w_row(lane);
    j = j < cols ? j : cols - 1;
    return (tile >= pairs ? cols : 0) + j;
  }
  const int64_t n = col0 + DLW_TILE_ROWS * tile + dlw_w_row(lane);
  return n < N ? n : N - 1;
}

// Row-slab plan: pairs per workgroup, a pure function of (N, act, CU count) — 32 rows where that leaves a workgroup per CU,
// else 16 (see "x traffic" above).  M and K do not enter; the order of a row's sum does not depend on the slab either.
DLW_HD int64_t dlw_plan_wgs(int pairs, int64_t N, int act) {
  const int64_t per = dlw_slab_cols(pairs, act);
  const int64_t cols = act ? N / 2 : N;
  return (cols + per - 1) / per;
}
DLW_HD int dlw_plan_pairs(int M, int64_t N, int64_t K, int act, int cus) {
  (void)M;
  (void)K;
  return dlw_plan_wgs(DLW_MAX_PAIRS, N, act) >= (int64_t)cus ? DLW_MAX_PAIRS : 1;
}
