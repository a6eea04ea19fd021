// Host-side enumeration of decode_attn_multi.hip's lane maps (cambrian_amd/csrc/decode_attn_multi_layout.h, the very header the
// kernel includes), compiled with g++ by tests/test_decode_attn_multi_layout_sim.py.
// Operand layouts modelled (cdna_hip_programming.md, MFMA operand maps):
//   v_mfma_f32_16x16x32_bf16: lane l holds A[row l & 15][k = 8 (l >> 4) + e], B[k = 8 (l >> 4) + e][col l & 15], e = 0..7;
//   v_mfma_f32_16x16x16_bf16: lane l holds A[row l & 15][k = 4 (l >> 4) + e], B[k = 4 (l >> 4) + e][col l & 15], e = 0..3;
//   both: D[row 4 (l >> 4) + i][col l & 15], i = 0..3.
// ds_read_b64_tr_b16 as in gemm_tn_layout_sim.cpp: inside a group of 16 lanes, lane i' supplies the address of 4 consecutive bf16
// = row i' >> 2, columns 4 (i' & 3) .. + 3 of a [4][16] block; lane i receives column i, element j = row j, taken from the piece
// that lane 4 j + (i >> 2) supplied, element i & 3.  Serviced in two halves of 32 lanes; bank of byte address a = (a / 4) % 64.
// For hd 64 / 96 / 128 and R = Q * G of 1, 7, 32, 33, 64 (G over 1..8 where it divides), chunk lengths that end inside a key tile:
//   1. every (query row, key, d) product of the scores is formed exactly once, and both operands of it carry the same d;
//   2. the score register a lane converts into the P operand names the key the V^T operand's element carries, the d of the V^T
//      operand is the d of the accumulator row, and every (query row, key, d) product of P . V is formed exactly once;
//   3. padded query rows carry q = 0 and keys past the chunk weight 0 (closed), as do a step's own keys past the row's token;
//   4. the V tile is written exactly once per element, transposing reads are 8-byte aligned, stay inside the tile, deliver the
//      element the map promises, and are conflict-free in both halves of the wave.
#include <cstdio>
#include <set>
#include <vector>
#include "../../cambrian_amd/csrc/decode_attn_multi_layout.h"

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

static int check(int hd, int R, int G, int nkeys /* live keys of the tile, 1..16 */, bool own) {
  const int KS = hd / 32, DT = hd / 16, RT = dam_row_tiles(R);
  const int Q = R / G;
  // ---- V tile image: value = key * 1024 + d, -1 = never written
  std::vector<int> lds(dam_v_tile_bytes(hd) / 2, -1);
  for (int ks = 0; ks < KS; ++ks)
    for (int lane = 0; lane < 64; ++lane) {
      const int off = dam_v_write_off(hd, ks, lane);
      if (off % 16 || off < 0 || off + 16 > dam_v_tile_bytes(hd)) FAIL("V write outside the tile or unaligned");
      for (int e = 0; e < 8; ++e) {
        if (lds[off / 2 + e] != -1) FAIL("V element written twice");
        const bool live = dam_k_key(lane) < nkeys;          // the kernel zeroes rows of closed keys: value 0 would do; keep the tag
        (void)live;
        lds[off / 2 + e] = dam_k_key(lane) * 1024 + dam_qk_d(ks, lane, e);
      }
    }
  std::set<int> vseen;
  for (int v : lds) if (v >= 0) vseen.insert(v);
  if ((int)vseen.size() != DAM_KEYS * hd) FAIL("V tile incomplete: %d of %d", (int)vseen.size(), DAM_KEYS * hd);

  // ---- scores
  std::vector<int> qk(RT * 16 * DAM_KEYS * hd, 0);  // (row, key, d) -> count
  auto at = [&](int r, int k, int d) { return (r * DAM_KEYS + k) * hd + d; };
  for (int rt = 0; rt < RT; ++rt)
    for (int ks = 0; ks < KS; ++ks)
      // the MFMA pairs A element (row i = key, k) with B element (k, col j = query): lanes la, lb with equal l >> 4 and e
      for (int la = 0; la < 64; ++la)
        for (int lb = 0; lb < 64; ++lb) {
          if ((la >> 4) != (lb >> 4)) continue;
          for (int e = 0; e < 8; ++e) {
            const int da = dam_qk_d(ks, la, e), db = dam_qk_d(ks, lb, e);
            if (da != db) FAIL("score operands carry different d");
            if (da < 0 || da >= hd) FAIL("d outside the head");
            qk[at(dam_q_row(rt, lb), dam_k_key(la), da)]++;
          }
        }
  for (int r = 0; r < RT * 16; ++r)
    for (int k = 0; k < DAM_KEYS; ++k)
      for (int d = 0; d < hd; ++d)
        if (qk[at(r, k, d)] != 1) FAIL("score product (%d, %d, %d) formed %d times", r, k, d, qk[at(r, k, d)]);
  // the D register (lane, i) of the product is (key 4 (l >> 4) + i, row l & 15): what dam_s_key / dam_s_row say
  for (int rt = 0; rt < RT; ++rt)
    for (int lane = 0; lane < 64; ++lane)
      for (int i = 0; i < 4; ++i) {
        if (dam_s_key(lane, i) != 4 * (lane >> 4) + i || dam_s_row(rt, lane) != 16 * rt + (lane & 15)) FAIL("score register map");
        // weights: a padded row's q operand is zero, a key past the chunk is closed, an own key past the row's token is closed
        const int r = dam_s_row(rt, lane), k = dam_s_key(lane, i);
        const bool row_live = r < R;
        bool open = k < nkeys;
        if (own) open = row_live ? dam_new_key_open(r, G, Q, k) : false;
        if (own && row_live && open != (k < Q && k <= dam_row_token(r, G))) FAIL("causal rule");
        if (!own && k >= nkeys && open) FAIL("key past the chunk open");
        if (row_live && (dam_row_token(r, G) >= Q || dam_row_head(r, G) >= G || dam_row_token(r, G) * G + dam_row_head(r, G) != r))
          FAIL("row -> (token, head)");
      }

  // ---- P . V
  std::vector<int> pv(RT * 16 * DAM_KEYS * hd, 0);  // (row, key, d) -> count
  for (int dt = 0; dt < DT; ++dt) {
    int addr[64];
    for (int lane = 0; lane < 64; ++lane) {
      addr[lane] = dam_v_tr_off(hd, dt, lane);
      if (addr[lane] % 8) FAIL("transposing read not 8-byte aligned");
      if (addr[lane] < 0 || addr[lane] + 8 > dam_v_tile_bytes(hd)) FAIL("transposing read outside the tile");
    }
    int got_key[64][4], got_d[64][4];
    for (int lane = 0; lane < 64; ++lane) {
      const int g = lane >> 4, i = lane & 15;
      for (int j = 0; j < 4; ++j) {
        const int supplier = g * 16 + 4 * j + (i >> 2);
        const int v = lds[addr[supplier] / 2 + (i & 3)];
        if (v < 0) FAIL("transposing read of an unwritten element");
        got_key[lane][j] = v / 1024;
        got_d[lane][j] = v % 1024;
        if (got_key[lane][j] != dam_vt_key(lane, j) || got_d[lane][j] != dam_vt_d(dt, lane))
          FAIL("hd %d dt %d lane %d element %d: got (key %d, d %d), map says (key %d, d %d)", hd, dt, lane, j, got_key[lane][j],
               got_d[lane][j], dam_vt_key(lane, j), dam_vt_d(dt, lane));
      }
    }
    for (int h = 0; h < 2; ++h) {
      std::set<int> banks;
      for (int lane = 32 * h; lane < 32 * h + 32; ++lane)
        for (int w = 0; w < 2; ++w)
          if (!banks.insert((addr[lane] / 4 + w) % 64).second) FAIL("bank conflict hd %d dt %d half %d", hd, dt, h);
    }
    for (int rt = 0; rt < RT; ++rt)
      for (int la = 0; la < 64; ++la)          // A = V^T: row l & 15 = d, k = key
        for (int lb = 0; lb < 64; ++lb) {      // B = P: k = key, col l & 15 = query row
          if ((la >> 4) != (lb >> 4)) continue;
          for (int e = 0; e < 4; ++e) {
            if (got_key[la][e] != dam_p_key(lb, e)) FAIL("P and V^T operands carry different keys");
            if (dam_p_key(lb, e) != dam_s_key(lb, e)) FAIL("P operand element is not the score register");
            pv[at(dam_q_row(rt, lb), got_key[la][e], got_d[la][e])]++;
          }
        }
    for (int lane = 0; lane < 64; ++lane)
      for (int i = 0; i < 4; ++i)
        if (dam_o_d(dt, lane, i) != 16 * dt + 4 * (lane >> 4) + i || dam_o_d(dt, lane, i) >= hd) FAIL("accumulator map");
  }
  for (int r = 0; r < RT * 16; ++r)
    for (int k = 0; k < DAM_KEYS; ++k)
      for (int d = 0; d < hd; ++d)
        if (pv[at(r, k, d)] != 1) FAIL("P . V product (%d, %d, %d) formed %d times", r, k, d, pv[at(r, k, d)]);
  return 0;
}

int main() {
  const int hds[3] = {64, 96, 128}, Rs[5] = {1, 7, 32, 33, 64};
  int cases = 0;
  for (int hd : hds) {
    if (dam_v_row_bytes(hd) % 32 || (dam_v_row_bytes(hd) / 32) % 2 == 0) { printf("row skew is not an odd number of 32-byte units\n"); return 1; }
    for (int R : Rs)
      for (int G = 1; G <= 8; ++G) {
        if (R % G || R / G > DAM_MAX_Q) continue;
        for (int nkeys : {1, 5, 15, 16}) {
          if (check(hd, R, G, nkeys, false)) return 1;
          ++cases;
        }
        if (check(hd, R, G, R / G, true)) return 1;
        ++cases;
      }
  }
  if (cases == 0) { printf("no case ran\n"); return 1; }
  printf("OK %d cases\n", cases);
  return 0;
}
