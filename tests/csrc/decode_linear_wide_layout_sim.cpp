// Host enumeration of decode_linear_wide.hip's maps (cambrian_amd/csrc/decode_linear_wide_layout.h, the header the kernel
// includes) under the documented operand layout of v_mfma_f32_16x16x32_bf16: lane l supplies A[l & 15][8 (l >> 4) + e] and
// B[8 (l >> 4) + e][l & 15], e = 0..7, and receives D[4 (l >> 4) + reg][l & 15], reg = 0..3.
// It replays whole launches — every workgroup, every wave's steps (two groups past its share included), the loads of the
// 8-row tiles, the exchange of lanes l <-> l ^ 8 between the tiles of a pair exactly as the kernel's two DPP moves do it, the
// MFMAs of every (pair, row block, half), the LDS partials and the epilogue's index arithmetic — and checks that
//   * the regrouped operands are what dlw_op_row / dlw_op_k / dlw_op_src_* say,
//   * the weight element and the x element of every product carry the SAME k, and no k >= K is ever multiplied,
//   * every (x row m < M, weight row n < N, k < K) product occurs exactly once in the sums an output element is made of,
//   * every out[m, col] is stored exactly once, rows >= M and columns >= N' never, and only LDS slots that were written are read,
//   * the order in which a row's k enter its sum is the same for every M,
//   * the 64 lanes of an LDS store write 64 distinct 16-byte slots of one contiguous KiB (one run of 1 KiB),
//   * the plan is a pure function of (N, act, CUs), covers N' exactly and keeps a workgroup per CU where it takes 32 rows.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>
#include "../../cambrian_amd/csrc/decode_linear_wide_layout.h"

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

struct Frag { int64_t n, k; };        // what a lane's 8 elements are: weight row (or x row) and first k; k = -1: zeroed x

// order of the k chunks in the sum of (x row m, first column of the launch), to be compared across M
typedef std::vector<int64_t> Order;

static void run(int M, int64_t N, int64_t K, int P, int act, std::map<int, Order>& orders) {
  const int NB = dlw_blocks(M), T = 2 * P;
  const int64_t cols = act ? N / 2 : N;
  const int cols_wg = dlw_slab_cols(P, act);
  const int64_t wgs = dlw_plan_wgs(P, N, act);
  const int64_t nsteps = (K + DLW_KSTEP - 1) / DLW_KSTEP;
  std::vector<int> stored(M * cols, 0);
  for (int64_t wg = 0; wg < wgs; ++wg) {
    const int64_t col0 = wg * cols_wg;
    // seen[m][pair][row][k]: products in the partials of (m, pair, row), summed over the waves as the epilogue does
    std::vector<int> seen((size_t)DLW_MAX_M * P * DLW_PAIR_ROWS * K, 0);
    std::vector<int64_t> wrow_of(P * DLW_PAIR_ROWS, -1);                     // weight row behind (pair, row)
    std::vector<int> written(DLW_WAVES * P * DLW_MAX_M * DLW_PAIR_ROWS, 0);
    Order order[DLW_WAVES];
    for (int wave = 0; wave < DLW_WAVES; ++wave) {
      const int64_t cnt = nsteps > wave ? (nsteps - wave + DLW_WAVES - 1) / DLW_WAVES : 0;
      for (int64_t j = 0; j < (cnt ? cnt + 3 : 0); ++j) {                  // steps past the share: the last groups' padding
        const int64_t step = j * DLW_WAVES + wave, k0 = step * DLW_KSTEP;
        CHECK(dlw_step_wave(step) == wave, "step %lld is not wave %d's", (long long)step, wave);
        Frag tile[4][64], op[2][2][64], xf[2][DLW_MAX_BLOCKS][64];
        for (int t = 0; t < T; ++t)
          for (int l = 0; l < 64; ++l) {
            const int64_t kw = k0 + dlw_w_k(l);
            tile[t][l] = {dlw_w_index(P, act, N, col0, t, l), kw < K ? kw : 0};
            CHECK(tile[t][l].n >= 0 && tile[t][l].n < N, "weight row %lld outside W", (long long)tile[t][l].n);
            CHECK(tile[t][l].k + 8 <= K, "weight load past K");
          }
        for (int q = 0; q < P; ++q)
          for (int l = 0; l < 64; ++l) {
            // the kernel's DPP pair: row_ror:8 reads lane l ^ 8; bank mask 0xc writes lanes with bit 3 set, 0x3 the others
            const bool hi = (l >> 3) & 1;
            op[q][0][l] = hi ? tile[2 * q + 1][l ^ 8] : tile[2 * q][l];
            op[q][1][l] = hi ? tile[2 * q + 1][l] : tile[2 * q][l ^ 8];
            for (int h = 0; h < 2; ++h) {
              const Frag& want = tile[2 * q + dlw_op_src_tile(l)][dlw_op_src_lane(h, l)];
              CHECK(op[q][h][l].n == want.n && op[q][h][l].k == want.k, "dlw_op_src: lane %d half %d", l, h);
              const int64_t kk = k0 + dlw_op_k(h, l);
              CHECK(op[q][h][l].k == (kk < K ? kk : 0), "dlw_op_k: lane %d half %d", l, h);
              CHECK(op[q][h][l].n == dlw_w_index(P, act, N, col0, 2 * q + (dlw_op_row(l) >> 3), dlw_op_row(l) & 7), "dlw_op_row: lane %d", l);
            }
          }
        for (int h = 0; h < 2; ++h)
          for (int b = 0; b < NB; ++b)
            for (int l = 0; l < 64; ++l) {
              const int m = DLW_BLOCK_M * b + dlw_x_row(l);
              const int64_t kx = k0 + dlw_x_k(h, l);
              xf[h][b][l] = {m < M ? m : M - 1, kx < K ? kx : -1};
            }
        for (int h = 0; h < 2; ++h)
          for (int b = 0; b < NB; ++b)
            for (int q = 0; q < P; ++q)
              for (int l = 0; l < 64; ++l)
                for (int reg = 0; reg < 4; ++reg) {
                  const int drow = 4 * (l >> 4) + reg, dcol = l & 15;        // D[drow][dcol] of acc[q][b]
                  CHECK(dlw_acc_row(l, reg) == drow && dlw_acc_m(l) == dcol, "accumulator map");
                  const int m = DLW_BLOCK_M * b + dcol;
                  bool any = false;
                  for (int kk = 0; kk < 32; ++kk) {                          // D[drow][dcol] += A[drow][kk] * B[kk][dcol]
                    const int la = drow + 16 * (kk >> 3), lb = dcol + 16 * (kk >> 3), e = kk & 7;
                    const Frag &w = op[q][h][la], &x = xf[h][b][lb];
                    CHECK(x.n == (m < M ? m : M - 1), "x row");
                    if (x.k < 0) continue;                                   // zeroed x: no contribution
                    CHECK(w.k + e == x.k + e && x.k + e < K, "K %lld step %lld half %d: weight k %lld meets x k %lld", (long long)K,
                          (long long)step, h, (long long)(w.k + e), (long long)(x.k + e));
                    int64_t& wr = wrow_of[q * DLW_PAIR_ROWS + drow];
                    CHECK(wr < 0 || wr == w.n, "(pair %d, row %d) mixes weight rows", q, drow);
                    wr = w.n;
                    ++seen[(((size_t)m * P + q) * DLW_PAIR_ROWS + drow) * K + x.k + e];
                    any = true;
                  }
                  if (any && q == 0 && drow == 0 && wg == 0 && m == 0) order[wave].push_back(k0 + 32 * h);
                }
      }
      // the wave's partial tiles: one 16-byte store per lane and (pair, block)
      for (int b = 0; b < NB; ++b)
        for (int q = 0; q < P; ++q) {
          std::vector<int> slot;
          for (int l = 0; l < 64; ++l) {
            const int i = dlw_red_index(P, wave, q, DLW_BLOCK_M * b + dlw_acc_m(l), dlw_acc_row(l, 0));
            CHECK(i % 4 == 0 && i >= 0 && i + 4 <= DLW_WAVES * P * DLW_MAX_M * DLW_PAIR_ROWS, "LDS store outside the tile");
            for (int r = 0; r < 4; ++r) {
              CHECK(i + r == dlw_red_index(P, wave, q, DLW_BLOCK_M * b + dlw_acc_m(l), dlw_acc_row(l, r)), "registers not consecutive");
              ++written[i + r];
            }
            slot.push_back(i / 4);
          }
          int lo = slot[0], hi = slot[0];
          for (int s : slot) { lo = s < lo ? s : lo; hi = s > hi ? s : hi; }
          CHECK(hi - lo == 63, "a store's 64 slots are not one contiguous KiB");       // 64 distinct values in a range of 64
          std::vector<int> once(64, 0);
          for (int s : slot) CHECK(++once[s - lo] == 1, "two lanes store to one slot");
        }
    }
    for (int w : written) CHECK(w <= 1, "an LDS slot written twice");
    // epilogue: the kernel's index arithmetic
    for (int idx = 0; idx < cols_wg * M; ++idx) {
      const int m = idx / cols_wg, c = idx - m * cols_wg;
      const int64_t col = col0 + c;
      if (col >= cols) continue;
      CHECK(m < M, "row %d >= M stored", m);
      const int tile = dlw_col_tile(c), r = c % DLW_TILE_ROWS;
      for (int part = 0; part < (act ? 2 : 1); ++part) {
        const int tl = tile + part * P, q = dlw_tile_pair(tl), row = dlw_tile_row(tl, r);
        CHECK(q < P && row < DLW_PAIR_ROWS, "epilogue reads outside the slab");
        for (int w = 0; w < DLW_WAVES; ++w)
          CHECK(written[dlw_red_index(P, w, q, m, row)] == 1 || nsteps <= w, "epilogue reads an unwritten partial (wave %d)", w);
        const int64_t want = act ? part * cols + col : col;
        CHECK(wrow_of[q * DLW_PAIR_ROWS + row] == want, "out column %lld part %d sums weight row %lld", (long long)col, part,
              (long long)wrow_of[q * DLW_PAIR_ROWS + row]);
        for (int64_t k = 0; k < K; ++k) {
          const int s = seen[(((size_t)m * P + q) * DLW_PAIR_ROWS + row) * K + k];
          CHECK(s == 1, "M %d N %lld K %lld: (m %d, n %lld, k %lld) multiplied %d times", M, (long long)N, (long long)K, m, (long long)want, (long long)k, s);
        }
      }
      ++stored[m * cols + col];
    }
    if (wg == 0) {
      Order all;
      for (int w = 0; w < DLW_WAVES; ++w) all.insert(all.end(), order[w].begin(), order[w].end());
      CHECK((int64_t)all.size() == (K + 31) / 32, "row 0: %zu chunks for K %lld", all.size(), (long long)K);
      auto it = orders.find(0);
      if (it == orders.end()) orders[0] = all;
      else CHECK(it->second == all, "K %lld: the order of row 0's sum depends on M (%d) or on the slab (%d pairs)", (long long)K, M, P);
    }
  }
  for (int v : stored) CHECK(v == 1, "an output element stored %d times", v);
}

int main() {
  // lanes of one load instruction: every tile row in one run of 128 contiguous bytes (64 k), each 16-byte chunk once
  {
    int hit[DLW_TILE_ROWS][8] = {};
    for (int l = 0; l < 64; ++l) {
      CHECK(dlw_w_k(l) % 8 == 0 && dlw_w_k(l) < DLW_KSTEP, "dlw_w_k");
      ++hit[dlw_w_row(l)][dlw_w_k(l) / 8];
    }
    for (int r = 0; r < DLW_TILE_ROWS; ++r)
      for (int c = 0; c < 8; ++c) CHECK(hit[r][c] == 1, "row %d chunk %d fetched %d times", r, c, hit[r][c]);
  }
  for (int64_t K : {8, 64, 72, 264}) {
    std::map<int, Order> orders;                         // shared by every M, slab, N and epilogue of this K
    for (int M : {1, 16, 17, 32, 33, 48, 49, 64})
      for (int P = 1; P <= DLW_MAX_PAIRS; ++P)
        for (int act = 0; act < 2; ++act)
          for (int64_t N : {1, 2, 30, 34, 70}) {
            if (act && (N & 1)) continue;
            run(M, N, K, P, act, orders);
          }
  }
  {
    std::map<int, Order> orders;
    run(64, 40, 4096, 2, 0, orders);
    run(17, 18, 4096, 1, 1, orders);
  }

  // plan
  for (int cus : {64, 104, 256, 304})
    for (int act = 0; act < 2; ++act)
      for (int64_t N = act ? 2 : 1; N <= 200000; N += (N < 600 ? 1 + act : 1 + act + 2 * (N / 97))) {
        if (act && (N & 1)) continue;
        const int q = dlw_plan_pairs(64, N, 4096, act, cus);
        CHECK(q == 1 || q == 2, "pairs %d", q);
        for (int M : {1, 17, 33, 64})
          for (int64_t K : {8, 4096, 14336}) CHECK(dlw_plan_pairs(M, N, K, act, cus) == q, "the plan depends on M or K");
        const int64_t wgs = dlw_plan_wgs(q, N, act), per = dlw_slab_cols(q, act), cols = act ? N / 2 : N;
        CHECK((wgs - 1) * per < cols && cols <= wgs * per, "N %lld: %lld workgroups of %lld columns", (long long)N, (long long)wgs, (long long)per);
        if (q == 2) CHECK(wgs >= cus, "32-row slabs leave CUs without a workgroup");
        else CHECK(dlw_plan_wgs(2, N, act) < cus, "a larger slab would still fill the chip");
      }
  CHECK(dlw_plan_pairs(64, 4096, 14336, 0, 256) == 1 && dlw_plan_wgs(1, 4096, 0) == 256, "down_proj: one workgroup per CU");
  CHECK(dlw_plan_pairs(64, 28672, 4096, 1, 256) == 2 && dlw_plan_wgs(2, 28672, 1) == 896, "gate / up");
  std::printf("OK\n");
  return 0;
}
