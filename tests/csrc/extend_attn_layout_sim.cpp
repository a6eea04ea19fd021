// Host-side enumeration of extend_attn.hip's row-block map and mask rule (cambrian_amd/csrc/extend_attn_layout.h, the very
// header the kernel includes), compiled with g++ by tests/test_extend_attn_layout_sim.py.  Inside a row block the lane maps are
// decode_attn_multi_layout.h's, which tests/csrc/decode_attn_multi_layout_sim.cpp enumerates; here the walk of the kernel is
// repeated — row block, key chunk, wave, key tile, lane, row tile, score register — for G of 1, 2, 4, 7, 8, Q of 1, 15, 16, 17,
// 33, several t0 and chunk lengths, with a key mask that has holes in the cached part and in the chunk:
//   1. a row block holds at most 64 rows of tokens inside the chunk, the blocks tile the chunk's Q * G rows exactly once, and
//      row -> (token, head, global row) is consistent;
//   2. every (query row, slot <= the row's limit) pair is owned by exactly one (row block, chunk, wave, tile, lane, register),
//      and no register owns a slot outside its chunk or past the block's last token;
//   3. the limit the kernel's arithmetic uses (slot of the tile's key 0 minus t0, minus the token) is t0 + token(row), and
//      exa_key_open over it is the rule "s <= t0 + j and (key_valid[s] or s == t0 + j)" of a brute-force double loop;
//   4. the V row of a slot is zeroed iff the slot is cached and masked (exa_v_keep on the slot's own key_valid bit): every
//      slot some row may see keeps its row;
//   5. a chunk the kernel skips (it starts past the block's last token) holds no visible pair, and the merge's count of chunks
//      a row reads, (t0 + j) / chunk + 1, covers every chunk that holds one.
#include <cstdio>
#include <map>
#include <utility>
#include <vector>
#include "../../cambrian_amd/csrc/extend_attn_layout.h"

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

static int check(int G, int Q, long long t0, int splits) {
  const long long len = t0 + Q;
  if (splits > len) splits = (int)len;
  const long long chunk = (len + splits - 1) / splits;
  splits = (int)((len + chunk - 1) / chunk);
  std::vector<bool> valid(len);
  for (long long s = 0; s < len; ++s) valid[s] = !(s < 2 || s % 5 == 3 || (s >= t0 && s < t0 + Q / 3));

  const int TB = exa_block_tokens(G), NB = exa_blocks(Q, G);
  if (TB < 1 || TB > DAM_MAX_Q || TB * G > DAM_MAX_ROWS) FAIL("G %d: %d tokens per block", G, TB);
  std::vector<int> row_seen(Q * G, 0);
  std::map<std::pair<int, long long>, int> owned;         // (global row, slot) -> count
  for (int rb = 0; rb < NB; ++rb) {
    const int R = exa_block_rows(rb, Q, G), RT = dam_row_tiles(R);
    if (R < 1 || R > DAM_MAX_ROWS || RT > dam_row_tiles(exa_block_rows(0, Q, G))) FAIL("block %d holds %d rows", rb, R);
    for (int r = 0; r < R; ++r) {
      const int j = exa_row_token(rb, r, G), g = exa_row_head(r, G), rg = exa_row_global(rb, r, G);
      if (j < 0 || j >= Q || g < 0 || g >= G || rg != j * G + g) FAIL("row (%d, %d) -> token %d head %d global %d", rb, r, j, g, rg);
      row_seen[rg]++;
    }
    const long long kend = exa_block_key_end(t0, rb, Q, G);
    if (kend != t0 + exa_row_token(rb, R - 1, G) + 1 || kend > len) FAIL("block %d: key end %lld", rb, kend);
    for (int c = 0; c < splits; ++c) {
      const long long c0 = c * chunk;
      if (c0 >= kend) {                                       // skipped: nothing of it may be visible to a row of the block
        for (int r = 0; r < R; ++r)
          if (t0 + exa_row_token(rb, r, G) >= c0) FAIL("a skipped chunk holds a visible slot");
        continue;
      }
      const long long c1 = c0 + chunk < kend ? c0 + chunk : kend;
      for (int wave = 0; wave < 4; ++wave)
        for (int it = 0; exa_tile_base(c0, wave, it) < c1; ++it) {
          const long long base = exa_tile_base(c0, wave, it);
          const int rel0 = (int)(base - t0);
          for (int lane = 0; lane < 64; ++lane) {
            const long long vslot = base + dam_k_key(lane);   // the slot whose K / V rows the lane fetches
            const bool in = vslot < c1;
            for (int rt = 0; rt < RT; ++rt) {
              const int r = dam_s_row(rt, lane);
              if (r >= R) continue;
              const int j = exa_row_token(rb, r, G);
              for (int i = 0; i < 4; ++i) {
                const int kk = dam_s_key(lane, i);
                const long long slot = base + kk;
                if (slot >= c1) continue;                     // the `in` bit of the key is clear
                if (slot < c0 || slot >= kend) FAIL("a register owns slot %lld outside [%lld, %lld)", slot, c0, kend);
                const long long rel = kk + rel0 - j;
                if (rel != slot - (t0 + j)) FAIL("limit of row (%d, %d) is not t0 + token", rb, r);
                const bool want = slot <= t0 + j && (valid[slot] || slot == t0 + j);
                if (exa_key_open(rel, valid[slot]) != want) FAIL("mask rule at row token %d slot %lld", j, slot);
                if (want && !exa_v_keep(slot, t0, valid[slot])) FAIL("V row of a visible slot %lld zeroed", slot);
                owned[{exa_row_global(rb, r, G), slot}]++;
                if (want && c >= (t0 + j) / chunk + 1) FAIL("the merge does not read chunk %d for token %d", c, j);
              }
            }
            // zeroed iff no row of any block may see the slot: a masked slot of the cached part (a masked slot of the chunk is
            // seen by its own token)
            if (in && exa_v_keep(vslot, t0, valid[vslot]) != !(vslot < t0 && !valid[vslot])) FAIL("V row of slot %lld", vslot);
          }
        }
    }
  }
  for (int rg = 0; rg < Q * G; ++rg) {
    if (row_seen[rg] != 1) FAIL("global row %d in %d row blocks", rg, row_seen[rg]);
    const int j = rg / G;
    for (long long s = 0; s <= t0 + j; ++s) {
      const auto f = owned.find({rg, s});
      if (f == owned.end() || f->second != 1)
        FAIL("G %d Q %d t0 %lld splits %d: pair (row %d, slot %lld) owned %d times", G, Q, t0, splits, rg, s,
             f == owned.end() ? 0 : f->second);
    }
  }
  for (const auto& kv : owned)
    if (kv.second != 1) FAIL("pair (row %d, slot %lld) owned %d times", kv.first.first, kv.first.second, kv.second);
  return 0;
}

int main() {
  int cases = 0;
  for (int G : {1, 2, 4, 7, 8})
    for (int Q : {1, 15, 16, 17, 33})
      for (long long t0 : {0LL, 1LL, 37LL, 130LL})
        for (int splits : {1, 2, 3, 7}) {
          if (check(G, Q, t0, splits)) return 1;
          ++cases;
        }
  for (int G = 1; G <= 8; ++G)
    if (exa_block_tokens(G) * G > 64 || (exa_block_tokens(G) + 1) * G <= 64 && exa_block_tokens(G) < DAM_MAX_Q) {
      printf("G %d: block of %d tokens is not the largest of at most 64 rows and 16 tokens\n", G, exa_block_tokens(G));
      return 1;
    }
  printf("OK %d cases\n", cases);
  return 0;
}
