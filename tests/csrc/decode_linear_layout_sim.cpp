// Host enumeration of decode_linear.hip's lane -> k maps (cambrian_amd/csrc/decode_linear_layout.h, the header the kernel
// includes) under the documented operand layout of v_mfma_f32_16x16x32_bf16: lane l supplies A[l & 15][8 (l >> 4) + e] and
// B[8 (l >> 4) + e][l & 15], e = 0..7, and receives D[4 (l >> 4) + reg][l & 15], reg = 0..3.
// For K from one 16-byte chunk to several steps past a workgroup's round of 4 waves x 64 k it replays what the kernel does
// — every wave's steps, the two MFMAs of a step, the clamp of fragments past K — and checks that
//   * in the accumulator rows a lane keeps, the weight element and the x element of every product carry the SAME k,
//   * every (weight row of the tile, k < K) is multiplied exactly once over the whole workgroup and no k >= K ever,
//   * the eight (wave, half) partials the epilogue adds are exactly the ones that were written, each once.
// Then the plan: exact cover of N' and two workgroups per CU at N = 4096.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../cambrian_amd/csrc/decode_linear_layout.h"

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

static void run_k(int64_t K) {
  const int64_t nsteps = (K + DL_KSTEP - 1) / DL_KSTEP;
  std::vector<int> seen(DL_TILE_ROWS * K, 0);           // products per (tile row, k)
  int written[DL_WAVES][2][DL_TILE_ROWS] = {};          // LDS partial slots (wave, half, row) written for x row 0
  for (int wave = 0; wave < DL_WAVES; ++wave) {
    const int64_t cnt = nsteps > wave ? (nsteps - wave + DL_WAVES - 1) / DL_WAVES : 0;
    // the kernel also runs up to two groups past cnt: steps there lie past K like the ones checked below (j = cnt, cnt + 1)
    for (int64_t j = 0; j < cnt + 2; ++j) {
      const int64_t step = j * DL_WAVES + wave;
      CHECK(dl_step_wave(step) == wave, "step %lld is not wave %d's", (long long)step, wave);
      const int64_t k0 = step * DL_KSTEP;
      // operand registers as the kernel fills them: k of element 0, or -1 for "x side zeroed"
      int64_t a_k[64], b_k[2][64];
      for (int l = 0; l < 64; ++l) {
        const int64_t kw = k0 + dl_w_k(l);
        a_k[l] = kw < K ? kw : 0;                        // clamped re-read of k = 0: a real weight, multiplied by zero
        for (int h = 0; h < 2; ++h) {
          const int64_t kx = k0 + dl_x_k(h, l);
          b_k[h][l] = kx < K ? kx : -1;
        }
      }
      for (int h = 0; h < 2; ++h) {
        for (int l = 0; l < 64; ++l) {                   // lane l's accumulator registers of MFMA h
          if (dl_acc_half(l) != h) continue;             // it keeps the other MFMA's
          for (int reg = 0; reg < 4; ++reg) {
            const int drow = 4 * (l >> 4) + reg, dcol = l & 15;      // D[drow][dcol]
            CHECK((drow >> 3) == h, "lane %d reg %d: row %d kept from MFMA %d", l, reg, drow, h);
            CHECK(dl_acc_row(l, reg) == (drow & 7), "lane %d reg %d: dl_acc_row", l, reg);
            for (int kk = 0; kk < 32; ++kk) {            // D[drow][dcol] += A[drow][kk] * B[kk][dcol]
              const int la = drow + 16 * (kk >> 3), lb = dcol + 16 * (kk >> 3), e = kk & 7;
              CHECK(dl_w_row(la) == (drow & 7) && dl_x_row(lb) == dcol, "operand rows");
              if (b_k[h][lb] < 0) continue;              // zero x: no contribution, whatever the clamped weight is
              const int64_t kx = b_k[h][lb] + e, kw = a_k[la] + e;
              CHECK(kx == kw, "K %lld step %lld half %d row %d kk %d: weight k %lld meets x k %lld", (long long)K,
                    (long long)step, h, drow, kk, (long long)kw, (long long)kx);
              CHECK(kx < K, "k %lld >= K %lld multiplied", (long long)kx, (long long)K);
              if (dcol == 0) ++seen[(drow & 7) * K + kx];
            }
            if (dcol == 0) written[wave][h][dl_acc_row(l, reg)] = 1;
          }
        }
      }
    }
  }
  for (int r = 0; r < DL_TILE_ROWS; ++r)
    for (int64_t k = 0; k < K; ++k) CHECK(seen[r * K + k] == 1, "K %lld: (row %d, k %lld) multiplied %d times", (long long)K, r, (long long)k, seen[r * K + k]);
  const int64_t nst = (K + DL_KSTEP - 1) / DL_KSTEP;
  for (int w = 0; w < DL_WAVES; ++w)
    for (int h = 0; h < 2; ++h)
      for (int r = 0; r < DL_TILE_ROWS; ++r)
        CHECK(written[w][h][r] == 1 || nst <= w, "partial (wave %d, half %d, row %d) never written", w, h, r);
}

int main() {
  // lanes of one load instruction: every tile row in one run of 128 contiguous bytes (64 k), each 16-byte chunk once
  {
    int hit[DL_TILE_ROWS][8] = {};
    for (int l = 0; l < 64; ++l) {
      CHECK(dl_w_k(l) % 8 == 0 && dl_w_k(l) < DL_KSTEP, "dl_w_k");
      ++hit[dl_w_row(l)][dl_w_k(l) / 8];
    }
    for (int r = 0; r < DL_TILE_ROWS; ++r)
      for (int c = 0; c < 8; ++c) CHECK(hit[r][c] == 1, "row %d chunk %d fetched %d times", r, c, hit[r][c]);
  }
  const int64_t round = DL_WAVES * DL_KSTEP;             // one step of every wave
  for (int64_t K = 8; K <= 5 * round + 64; K += 8) run_k(K);
  for (int64_t K : {4096, 4104, 8192 - 8, 14336}) run_k(K);

  // plan
  for (int cus : {64, 104, 256, 304})
    for (int act = 0; act < 2; ++act)
      for (int64_t N = act ? 2 : 1; N <= 200000; N += (N < 600 ? 1 + act : 1 + act + 2 * (N / 97))) {
        if (act && (N & 1)) continue;
        int prev = 0;
        for (int M : {1, 4, 5, 16}) {
          const int t = dl_plan_tiles(M, N, 4096, act, cus);
          CHECK(t == 1 || t == 2 || t == 4, "tiles %d", t);
          CHECK(!act || t >= 2, "SwiGLU needs gate and up tiles");
          CHECK(t == dl_plan_tiles(M, N, 14336, act, cus), "plan depends on K");
          CHECK(t >= prev, "more rows of x, smaller slab");
          prev = t;
          const int64_t wgs = dl_plan_wgs(t, N, act), per = act ? 4 * t : 8 * t, cols = act ? N / 2 : N;
          CHECK((wgs - 1) * per < cols && cols <= wgs * per, "N %lld: %lld workgroups of %lld columns", (long long)N, (long long)wgs, (long long)per);
          if (2 * t <= DL_MAX_TILES) CHECK(dl_plan_wgs(2 * t, N, act) < dl_plan_want(M, cus), "a larger slab would still fill the chip");
        }
        CHECK(dl_plan_tiles(1, N, 64, act, cus) == dl_plan_tiles(4, N, 64, act, cus) && dl_plan_tiles(5, N, 64, act, cus) == dl_plan_tiles(16, N, 64, act, cus), "M classes");
      }
  CHECK(dl_plan_wgs(dl_plan_tiles(1, 4096, 4096, 0, 256), 4096, 0) >= 512, "N = 4096: fewer than two workgroups per CU");
  CHECK(dl_plan_wgs(dl_plan_tiles(16, 4096, 14336, 0, 256), 4096, 0) >= 512, "N = 4096: fewer than two workgroups per CU");
  std::printf("OK\n");
  return 0;
}
