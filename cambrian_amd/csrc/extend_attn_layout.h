// extend_attn_layout.h — the row-block map and the mask rule of extend_attn.hip, free of HIP types so that
// tests/csrc/extend_attn_layout_sim.cpp runs the very same functions on the host.  Inside a row block the lane maps are
// decode_attn_multi_layout.h's (dam_*: 16 x 16 score tiles, one query row per lane, the skewed V tile), unchanged.
//
// A chunk of Q new tokens per cache row is cut into row blocks of TB = min(16, 64 / G) consecutive tokens (G query heads per KV
// head): a workgroup holds the TB * G <= 64 query rows of one (sequence, KV head, row block), row r = (token - first token) * G
// + head, padded to tiles of 16.  The block's keys are cache slots 0 .. t0 + (its last token), cut into the plan's key chunks;
// inside a chunk, wave w of the four takes key tiles w, w + 4, ... of 16 slots.  Row r carries its own causal limit
// t0 + token(r): it sees slot s iff s <= limit and (key_valid[s] or s == limit).
#pragma once
#include "decode_attn_multi_layout.h"

#define EXA_MAX_Q 4096

CMB_HD int exa_block_tokens(int G) { return 64 / G < DAM_MAX_Q ? 64 / G : DAM_MAX_Q; }
CMB_HD int exa_blocks(int Q, int G) { return (Q + exa_block_tokens(G) - 1) / exa_block_tokens(G); }
// first token of row block rb, and how many tokens / query rows it holds (the last block may be short)
CMB_HD int exa_block_first(int rb, int G) { return rb * exa_block_tokens(G); }
CMB_HD int exa_block_count(int rb, int Q, int G) {
  const int left = Q - exa_block_first(rb, G);
  return left < exa_block_tokens(G) ? left : exa_block_tokens(G);
}
CMB_HD int exa_block_rows(int rb, int Q, int G) { return exa_block_count(rb, Q, G) * G; }
// row r of row block rb -> token of the chunk, head of the group, row among the Q * G rows of the (sequence, KV head)
CMB_HD int exa_row_token(int rb, int r, int G) { return exa_block_first(rb, G) + r / G; }
CMB_HD int exa_row_head(int r, int G) { return r % G; }
CMB_HD int exa_row_global(int rb, int r, int G) { return exa_block_first(rb, G) * G + r; }
// one past the last slot any row of the block may see
CMB_HD long long exa_block_key_end(long long t0, int rb, int Q, int G) {
  return t0 + exa_block_first(rb, G) + exa_block_count(rb, Q, G);
}
// slot of key kk (0 .. 15) of wave w's it-th tile in the chunk that starts at slot c0
CMB_HD long long exa_tile_base(long long c0, int wave, int it) { return c0 + (long long)(wave + 4 * it) * DAM_KEYS; }
// the mask: key slot `rel` places after the row's limit (rel = slot - limit, <= 0 is causal) with its key_valid byte
CMB_HD bool exa_key_open(long long rel, bool valid) { return rel <= 0 && (valid || rel == 0); }
// whether the V row of a slot is staged as it is or as zeros: a slot some row may see (valid, or one of the chunk's own slots,
// which hold finite values written by the call itself); a masked cached slot may hold anything
CMB_HD bool exa_v_keep(long long slot, long long t0, bool valid) { return valid || slot >= t0; }
