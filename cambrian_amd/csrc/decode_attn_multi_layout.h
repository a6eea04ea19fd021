// decode_attn_multi_layout.h — the lane maps of decode_attn_multi.hip, free of HIP types so that
// tests/csrc/decode_attn_multi_layout_sim.cpp runs the very same functions on the host under the documented operand layouts of
// v_mfma_f32_16x16x32_bf16 / v_mfma_f32_16x16x16_bf16 and of ds_read_b64_tr_b16 (model in tests/csrc/gemm_tn_layout_sim.cpp).
//
// A workgroup holds the R = Q * G query rows of one (sequence, KV head): row r = j * G + g is token j, query head g of the
// group, padded to RT = ceil(R / 16) tiles of 16.  A wave takes 16 keys at a time (a "key tile").
//   scores   S^T[key][row] = K . Q^T   one v_mfma_f32_16x16x32_bf16 per (row tile, 32 columns of d):
//            A = K: lane l holds key l & 15, d = 32 ks + 8 (l >> 4) + e   (16 bytes straight from the cache row)
//            B = Q: lane l holds row 16 rt + (l & 15), the same d
//            D: lane l holds keys 4 (l >> 4) + i (i = 0..3) of row 16 rt + (l & 15)
//   P . V    O^T[d][row] = V^T . P^T   one v_mfma_f32_16x16x16_bf16 per (row tile, 16 columns of d):
//            B = P: lane l holds row 16 rt + (l & 15), keys 4 (l >> 4) + e — the score registers, converted in place
//            A = V^T: lane l holds d = 16 dt + (l & 15), keys 4 (l >> 4) + e — a transposing read of the V tile in LDS
//            D: lane l holds d = 16 dt + 4 (l >> 4) + i of row 16 rt + (l & 15)
// The V tile of a wave is 16 rows (keys) of hd bf16 in LDS, written in the K operand's map (lane l: key l & 15, 16-byte piece
// (l >> 4) + 4 ks).  Its rows are SKEWED, not XOR-swizzled: a row is hd * 2 + 32 bytes long (160 / 224 / 288: an odd number of
// 32-byte units for all three head sizes, where an XOR on hd 96's six units would leave the row).  A transposing read's 32-lane
// half takes 8 rows x 32 bytes; with the skew they lie on 8 different 32-byte positions of the 256-byte bank row.
#pragma once
#include "gemm_layout.h"   // CMB_HD

#define DAM_KEYS 16                 // keys per wave and iteration
#define DAM_MAX_ROWS 64             // Q * G
#define DAM_MAX_Q 16

CMB_HD int dam_row_tiles(int R) { return (R + 15) / 16; }
CMB_HD int dam_v_row_bytes(int hd) { return hd * 2 + 32; }
CMB_HD int dam_v_tile_bytes(int hd) { return DAM_KEYS * dam_v_row_bytes(hd); }

// scores: A (K) and B (Q) operand of k-step ks, element e of lane l
CMB_HD int dam_k_key(int lane) { return lane & 15; }
CMB_HD int dam_q_row(int rt, int lane) { return 16 * rt + (lane & 15); }
CMB_HD int dam_qk_d(int ks, int lane, int e) { return 32 * ks + 8 * (lane >> 4) + e; }
// scores: register i of lane l
CMB_HD int dam_s_key(int lane, int i) { return 4 * (lane >> 4) + i; }
CMB_HD int dam_s_row(int rt, int lane) { return 16 * rt + (lane & 15); }
// P . V: B (P) operand element e = score register e; A (V^T) operand element e of lane l, tile dt
CMB_HD int dam_p_key(int lane, int e) { return 4 * (lane >> 4) + e; }
CMB_HD int dam_vt_d(int dt, int lane) { return 16 * dt + (lane & 15); }
CMB_HD int dam_vt_key(int lane, int e) { return 4 * (lane >> 4) + e; }
// P . V: register i of lane l
CMB_HD int dam_o_d(int dt, int lane, int i) { return 16 * dt + 4 * (lane >> 4) + i; }

// V tile in LDS: where lane l puts its 16-byte piece of k-step ks (key l & 15, columns dam_qk_d(ks, l, 0..7)) ...
CMB_HD int dam_v_write_off(int hd, int ks, int lane) { return (lane & 15) * dam_v_row_bytes(hd) + (32 * ks + 8 * (lane >> 4)) * 2; }
// ... and the address lane l SUPPLIES to the transposing read of d tile dt: inside its group of 16 lanes, lane 4 q + p names
// row (key) 4 (l >> 4) + q, columns 16 dt + 4 p .. + 3; lane i of the group RECEIVES column 16 dt + i of those four rows
CMB_HD int dam_v_tr_off(int hd, int dt, int lane) {
  const int i = lane & 15;
  return (4 * (lane >> 4) + (i >> 2)) * dam_v_row_bytes(hd) + (16 * dt + 4 * (i & 3)) * 2;
}

// query row r of the workgroup -> token and head of the group; which of a step's own keys (new slot jn) row r may see (the
// kernel keeps token(r) per lane, divided once, and applies this rule as jn < Q && jn <= token(r))
CMB_HD int dam_row_token(int r, int G) { return r / G; }
CMB_HD int dam_row_head(int r, int G) { return r % G; }
CMB_HD bool dam_new_key_open(int r, int G, int Q, int jn) { return jn < Q && jn <= r / G; }
