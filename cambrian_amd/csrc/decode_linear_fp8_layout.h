// decode_linear_fp8_layout.h — who reads which k in decode_linear_fp8.hip, and its row-slab plan, free of HIP types so that
// tests/csrc/decode_linear_fp8_layout_sim.cpp runs the very same functions on the host.  What decode_linear_layout.h says
// about slabs, waves and accumulators holds here too (DL_WAVES, DL_TILE_ROWS, DL_MAX_TILES, DL_MAX_M, dl_step_wave,
// dl_w_row, dl_x_row, dl_acc_half, dl_acc_row, dl_plan_wgs are used as they are); what changes is k.
//
// A weight element is one byte (e4m3fn), so the 16 bytes a lane loads are 16 k-elements and a k-step is 128 elements: lane
// l reads the 16 elements at dl8_w_k(l) of row dl_w_row(l), and the eight lanes of a row cover k 0..127 of the step — one
// contiguous run of 128 bytes (a full line) per row and load instruction, as in the bf16 kernel.  The 16 bytes convert to
// two bf16 fragments of 8 (part p = bytes 8 p .. 8 p + 7, i.e. dwords 2 p and 2 p + 1), and v_mfma_f32_16x16x32_bf16 sums
// over 32 k, so four MFMAs follow a load: (part p, half h) multiplies operand rows "8 rows at the k of lanes with bit 3
// clear over the same 8 rows at the k of lanes with bit 3 set" with x at the k of half h: lane l supplies row dl_x_row(l),
// elements dl8_x_k(p, h, l) .. +7.  Operand rows 8 h' .. 8 h' + 7 met the right k only in the MFMAs with h == h'; both parts
// of a half add into the same accumulator, so the accumulators, dl_acc_half and dl_acc_row are those of the bf16 kernel.
// No k is permuted inside a lane's 16 elements: byte b of the load is k + b, element e of part p is k + 8 p + e on both
// operands (byte 0 of a dword converts to the low half of the packed pair, as a bf16 fragment is laid out in memory).
#pragma once
#include "decode_linear_layout.h"

#define DL8_KSTEP 128    /* k per wave step: 2 parts x 2 halves, four MFMAs of 32 */
#define DL8_PARTS 2
#define DL8_K_MULT 16    /* K and the weight row stride are multiples of this: a lane's 16 bytes never straddle K */

// weight operand: first k inside the step of lane l's 16 elements (row: dl_w_row)
DL_HD int dl8_w_k(int lane) { return 64 * ((lane >> 3) & 1) + 16 * (lane >> 4); }
// x operand of MFMA (part, half): first k inside the step of lane l's 8 elements (row: dl_x_row)
DL_HD int dl8_x_k(int part, int half, int lane) { return 64 * half + 16 * (lane >> 4) + 8 * part; }

// Row-slab plan, a pure function of (M, N, K, act, CU count): the largest slab that still leaves one workgroup per CU,
// 8 rows (16 with SwiGLU) when none does.  The bf16 plan asks for two (M <= 4) or one and a half per CU; here a slab
// carries half the bytes per row while every k-step still needs its four x fragments (eight with the norm), so the load
// instructions that fetch x are twice as many per weight byte — at 8-row slabs four of five — and only rows per workgroup
// amortise them.  That is reasoning, not measurement: no A/B of the slab rule against the bf16 kernel's is recorded
// (profiles/decode_fp8.md has one rule only).  With the kernel's groups (U steps of T tiles, two groups in flight) a
// lane holds 128 / 192 / 256 bytes of weights in flight at T = 1 / 2 / 4, and 64 / 128 / 128 with the norm prologue, whose
// x and norm operands leave registers for fewer steps — half of what the bf16 kernel keeps in flight there, the likelier
// reason its gate / up stream stays at about half the HBM rate.  M and K do not enter.  N = 4096 gives 256 workgroups
// of 16 rows.  The order in which a row's k are summed does not depend on the slab, so neither do the result's bits.
DL_HD int64_t dl8_plan_want(int cus) { return (int64_t)cus; }
DL_HD int dl8_plan_tiles(int M, int64_t N, int64_t K, int act, int cus) {
  (void)M;
  (void)K;
  const int least = act ? 2 : 1;
  for (int t = DL_MAX_TILES; t > least; t >>= 1)
    if (dl_plan_wgs(t, N, act) >= dl8_plan_want(cus)) return t;
  return least;
}
