// decode_linear_fp4_layout.h — who reads which k in decode_linear_fp4.hip, and its row-slab plan, free of HIP types so that
// tests/csrc/decode_linear_fp4_layout_sim.cpp runs the very same functions on the host.  What decode_linear_layout.h says
// about slabs, waves and accumulators holds here too (DL_WAVES, DL_TILE_ROWS, DL_MAX_TILES, DL_MAX_M, dl_step_wave,
// dl_w_row, dl_x_row, dl_acc_half, dl_acc_row, dl_plan_wgs are used as they are); what changes is k.
//
// A weight element is a nibble (OCP e2m1; byte j of a row holds element 2 j in its low nibble and 2 j + 1 in its high
// one), so the 16 bytes a lane loads are 32 k-elements — exactly one MX block, one e8m0 scale byte — and a k-step is 256
// elements: lane l reads the 32 elements at dl4_w_k(l) of row dl_w_row(l), and the eight lanes of a row cover k 0..255 of
// the step, one contiguous run of 128 bytes (a full line) per row and load instruction, as in the bf16 and e4m3 kernels.
// The lane's scale byte is the row's byte dl4_scale_index(k) = k / 32 of its load.  The 16 bytes convert to four bf16
// fragments of 8 (part p = bytes 4 p .. 4 p + 3 = dword p, elements 8 p .. 8 p + 7 of the block), all four with the one
// scale, and v_mfma_f32_16x16x32_bf16 sums over 32 k, so eight MFMAs follow a load: (part p, half h) multiplies operand
// rows "8 rows at the k of lanes with bit 3 clear over the same 8 rows at the k of lanes with bit 3 set" with x at the k
// of half h: lane l supplies row dl_x_row(l), elements dl4_x_k(p, h, l) .. +7.  Operand rows 8 h' .. 8 h' + 7 met the
// right k only in the MFMAs with h == h'; the four parts of a half add into the same accumulator, so the accumulators,
// dl_acc_half and dl_acc_row are those of the bf16 kernel.  No k is permuted inside a lane's 32 elements: nibble i of the
// load is k + i, element e of part p is k + 8 p + e on both operands (the low nibble of a byte converts to the low half
// of the packed pair, as a bf16 fragment is laid out in memory).
//
// x traffic.  A k-step fetches 8 x fragments of 16 bytes per lane (16 with the norm) for T weight loads: per weight byte
// four times the bf16 kernel's and twice the e4m3 kernel's.  x comes straight from L2 / the vector cache as in both
// existing kernels and is NOT staged in LDS: a workgroup reads each x element exactly once (its four waves take disjoint
// k-steps, and inside a wave lane l's fragments are its own), so LDS staging would add a write and a read per element
// without removing any fetch; what it could save is the 4x replication of a fragment across the four lane groups that
// share dl_x_row — there is none, every lane's (row, k) pair is distinct (rows past M re-read row M - 1; at M = 16 none
// do).  K = 4096 at M = 16 is 128 KB and would not fit at all.  That is reasoning, not measurement: no A/B of an LDS
// variant was built or recorded.
#pragma once
#include "decode_linear_layout.h"

#define DL4_KSTEP 256    /* k per wave step: 4 parts x 2 halves, eight MFMAs of 32 */
#define DL4_PARTS 4
#define DL4_BLOCK 32     /* elements per e8m0 scale: K, and twice the weight row stride in bytes, are multiples of this */

// weight operand: first k inside the step of lane l's 32 elements (row: dl_w_row); its bytes start at k / 2
DL_HD int dl4_w_k(int lane) { return 128 * ((lane >> 3) & 1) + 32 * (lane >> 4); }
// x operand of MFMA (part, half): first k inside the step of lane l's 8 elements (row: dl_x_row)
DL_HD int dl4_x_k(int part, int half, int lane) { return 128 * half + 32 * (lane >> 4) + 8 * part; }
// index in a row of scale bytes of the block that starts at k (k % 32 == 0)
DL_HD int64_t dl4_scale_index(int64_t k) { return k / DL4_BLOCK; }

// weight row that lane l reads for tile t (0 .. tiles - 1) of the workgroup whose first output column is col0.  Plain: the
// slab's rows in order.  SwiGLU over packed [gate; up] rows (N' = N / 2 columns): tiles 0 .. tiles / 2 - 1 are gate rows of
// the workgroup's columns and tile t + tiles / 2 holds the up rows of tile t's columns, so the epilogue's column
// 8 t + r takes partial tiles t and t + tiles / 2.  A row past the end re-reads the last one (its sums are never stored).
DL_HD int64_t dl4_slab_row(int tiles, int act, int64_t col0, int t, int lane, int64_t N) {
  if (act) {
    const int64_t cols = N / 2;
    const int th = tiles / 2 > 0 ? tiles / 2 : 1;
    int64_t j = col0 + DL_TILE_ROWS * (t % th) + dl_w_row(lane);
    j = j < cols ? j : cols - 1;
    return (t >= th ? cols : 0) + j;
  }
  const int64_t n = col0 + DL_TILE_ROWS * t + dl_w_row(lane);
  return n < N ? n : N - 1;
}

// Row-slab plan, a pure function of (M, N, K, act, CU count): the largest slab that still leaves one workgroup per CU,
// 8 rows (16 with SwiGLU) when none does — the e4m3 kernel's rule, for its reason taken one step further: a slab row
// carries a quarter of the bf16 bytes while every k-step still needs its eight x fragments (sixteen with the norm), so at
// 8-row slabs eight of nine load instructions (not counting the scale bytes) fetch x, and only rows per workgroup amortise
// them.  A rule that asks for fewer workgroups than CUs would amortise more and leave CUs idle; it was not tried.  That is
// reasoning, not measurement: no A/B of the slab rule is recorded (profiles/decode_fp4.md has one rule only).  M and K do
// not enter.  N = 4096 gives 256 workgroups of 16 rows.  The order in which a row's k are summed does not depend on the
// slab, so neither do the result's bits.
DL_HD int64_t dl4_plan_want(int cus) { return (int64_t)cus; }
DL_HD int dl4_plan_tiles(int M, int64_t N, int64_t K, int act, int cus) {
  (void)M;
  (void)K;
  const int least = act ? 2 : 1;
  for (int t = DL_MAX_TILES; t > least; t >>= 1)
    if (dl_plan_wgs(t, N, act) >= dl4_plan_want(cus)) return t;
  return least;
}
