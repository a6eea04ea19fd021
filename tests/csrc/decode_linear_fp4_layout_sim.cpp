// Host enumeration of decode_linear_fp4.hip's lane -> k maps (cambrian_amd/csrc/decode_linear_fp4_layout.h, the header the
// kernel includes) under the documented operand layout of v_mfma_f32_16x16x32_bf16: lane l supplies A[l & 15][8 (l >> 4) + e]
// and B[8 (l >> 4) + e][l & 15], e = 0..7, and receives D[4 (l >> 4) + reg][l & 15], reg = 0..3.  A lane's weight load is 16
// bytes = 32 nibbles = 32 k = one MX block; part p of it (dword p, nibble i = k + i) is the A fragment of the MFMAs
// (p, half 0) and (p, half 1), converted with the block's one scale byte.  For K = 32, 224, 256, 288, 800 (one block, a
// ragged step, one step, a step + a block, three steps + ragged), every multiple of 32 up to several rounds of the four
// waves, and the real sizes, it replays what the kernel does — every wave's steps, the eight MFMAs of a step, the clamp of
// fragments past K — and checks that
//   * in the accumulator rows a lane keeps, the weight element and the x element of every product carry the SAME k,
//   * every (weight row of the tile, k < K) is multiplied exactly once over the whole workgroup and no k >= K ever,
//   * the scale byte a lane loads is the row's byte k / 32 of its load, the block of every element it converts,
//   * a lane's 32 weight elements and its x fragments never straddle K (K % 32 == 0),
//   * the eight (wave, half) partials the epilogue adds are exactly the ones that were written,
//   * every load instruction reads each tile row as one whole, aligned 128-byte line.
// Then the plan: pure, monotone in N, exact cover of N', one workgroup per CU at least whenever a smaller slab was chosen,
// and a SwiGLU slab owns matching gate and up rows.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../cambrian_amd/csrc/decode_linear_fp4_layout.h"

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

static void run_k(int64_t K) {
  const int64_t nsteps = (K + DL4_KSTEP - 1) / DL4_KSTEP;
  std::vector<int> seen(DL_TILE_ROWS * K, 0);           // products per (tile row, k)
  int written[DL_WAVES][2][DL_TILE_ROWS] = {};          // LDS partial slots (wave, half, row) written for x row 0
  for (int wave = 0; wave < DL_WAVES; ++wave) {
    const int64_t cnt = nsteps > wave ? (nsteps - wave + DL_WAVES - 1) / DL_WAVES : 0;
    // the kernel also runs up to two groups of up to 2 steps past cnt: steps there lie past K like the ones checked here
    for (int64_t j = 0; j < cnt + 6; ++j) {
      const int64_t step = j * DL_WAVES + wave;
      CHECK(dl_step_wave(step) == wave, "step %lld is not wave %d's", (long long)step, wave);
      const int64_t k0 = step * DL4_KSTEP;
      // operand registers as the kernel fills them: k of nibble / element 0, or -1 for "x side zeroed"
      int64_t a_k[64], a_s[64], b_k[DL4_PARTS][2][64];
      for (int l = 0; l < 64; ++l) {
        const int64_t kw = k0 + dl4_w_k(l);
        a_k[l] = kw < K ? kw : 0;                        // clamped re-read of k = 0: real weights, multiplied by zero
        CHECK(a_k[l] % DL4_BLOCK == 0 && a_k[l] + DL4_BLOCK <= K, "K %lld: lane %d's block at %lld straddles K", (long long)K, l,
              (long long)a_k[l]);
        CHECK((a_k[l] >> 1) % 16 == 0 && (a_k[l] >> 1) + 16 <= K / 2, "lane %d's 16 bytes leave the row", l);
        a_s[l] = dl4_scale_index(a_k[l]);
        CHECK(a_s[l] >= 0 && a_s[l] < K / DL4_BLOCK, "lane %d's scale byte %lld leaves the row", l, (long long)a_s[l]);
        for (int h = 0; h < 2; ++h) {
          const int64_t kx = k0 + dl4_x_k(0, h, l);      // the kernel tests part 0's k and offsets the other parts from it
          for (int p = 0; p < DL4_PARTS; ++p) {
            const int64_t kp = (kx < K ? kx : 0) + (dl4_x_k(p, h, l) - dl4_x_k(0, h, l));
            CHECK(kp >= 0 && kp + 8 <= K, "K %lld: lane %d's x fragment at %lld straddles K", (long long)K, l, (long long)kp);
            b_k[p][h][l] = kx < K ? kp : -1;
            CHECK(kx >= K || kp == k0 + dl4_x_k(p, h, l), "x fragment offset");
          }
        }
      }
      for (int p = 0; p < DL4_PARTS; ++p)
        for (int h = 0; h < 2; ++h) {
          for (int l = 0; l < 64; ++l) {                 // lane l's accumulator registers of the MFMAs of half h
            if (dl_acc_half(l) != h) continue;           // it keeps the other half's
            for (int reg = 0; reg < 4; ++reg) {
              const int drow = 4 * (l >> 4) + reg, dcol = l & 15;      // D[drow][dcol]
              CHECK((drow >> 3) == h, "lane %d reg %d: row %d kept from half %d", l, reg, drow, h);
              CHECK(dl_acc_row(l, reg) == (drow & 7), "lane %d reg %d: dl_acc_row", l, reg);
              for (int kk = 0; kk < 32; ++kk) {          // D[drow][dcol] += A[drow][kk] * B[kk][dcol]
                const int la = drow + 16 * (kk >> 3), lb = dcol + 16 * (kk >> 3), e = kk & 7;
                CHECK(dl_w_row(la) == (drow & 7) && dl_x_row(lb) == dcol, "operand rows");
                if (b_k[p][h][lb] < 0) continue;         // zero x: no contribution, whatever the clamped weight is
                const int64_t kx = b_k[p][h][lb] + e, kw = a_k[la] + 8 * p + e;     // nibble 8 p + e of the lane's load
                CHECK(kx == kw, "K %lld step %lld part %d half %d row %d kk %d: weight k %lld meets x k %lld", (long long)K,
                      (long long)step, p, h, drow, kk, (long long)kw, (long long)kx);
                CHECK(kx < K, "k %lld >= K %lld multiplied", (long long)kx, (long long)K);
                CHECK(a_s[la] == kw / DL4_BLOCK, "k %lld converted with the scale of block %lld", (long long)kw, (long long)a_s[la]);
                if (dcol == 0) ++seen[(drow & 7) * K + kx];
              }
              if (dcol == 0 && j < cnt) written[wave][h][dl_acc_row(l, reg)] = 1;
            }
          }
        }
    }
  }
  for (int r = 0; r < DL_TILE_ROWS; ++r)
    for (int64_t k = 0; k < K; ++k) CHECK(seen[r * K + k] == 1, "K %lld: (row %d, k %lld) multiplied %d times", (long long)K, r, (long long)k, seen[r * K + k]);
  for (int w = 0; w < DL_WAVES; ++w)
    for (int h = 0; h < 2; ++h)
      for (int r = 0; r < DL_TILE_ROWS; ++r)
        CHECK(written[w][h][r] == 1 || nsteps <= w, "partial (wave %d, half %d, row %d) never written", w, h, r);
}

// the rows a SwiGLU workgroup owns, as the kernel forms them: tile t < T / 2 is gate rows, tile t + T / 2 the up rows of the
// same output columns
static void run_swiglu_rows(int T, int64_t N, int64_t wg) {
  const int64_t cols = N / 2, col0 = wg * (DL_TILE_ROWS * T / 2);
  const int th = T / 2;
  for (int t = 0; t < th; ++t)
    for (int l = 0; l < 64; ++l) {
      const int64_t gate = dl4_slab_row(T, 1, col0, t, l, N), up = dl4_slab_row(T, 1, col0, t + th, l, N);
      CHECK(up - gate == cols && gate < cols && up < N, "T %d N %lld wg %lld: gate row %lld with up row %lld", T, (long long)N,
            (long long)wg, (long long)gate, (long long)up);
      // the epilogue's output column col0 + 8 t + r takes row r of partial tiles t and t + T / 2
      const int64_t col = col0 + DL_TILE_ROWS * t + dl_w_row(l);
      CHECK(col >= cols || gate == col, "column %lld is fed gate row %lld", (long long)col, (long long)gate);
    }
}

int main() {
  // lanes of one load instruction: every tile row as one aligned run of 128 contiguous bytes, each 16-byte chunk once
  {
    int hit[DL_TILE_ROWS][8] = {};
    for (int l = 0; l < 64; ++l) {
      CHECK(dl4_w_k(l) % DL4_BLOCK == 0 && dl4_w_k(l) >= 0 && dl4_w_k(l) + DL4_BLOCK <= DL4_KSTEP, "dl4_w_k");
      ++hit[dl_w_row(l)][dl4_w_k(l) / 2 / 16];
    }
    for (int r = 0; r < DL_TILE_ROWS; ++r)
      for (int c = 0; c < 8; ++c) CHECK(hit[r][c] == 1, "row %d chunk %d fetched %d times", r, c, hit[r][c]);
    CHECK(DL4_KSTEP == 256 && DL4_KSTEP / 2 == 128, "a step is one whole 128-byte line of a row");
    CHECK(DL4_BLOCK == 32 && DL4_PARTS * 8 == DL4_BLOCK, "a lane's 16 bytes are one block, four fragments of 8");
  }
  for (int64_t K : {32, 224, 256, 288, 800}) run_k(K);
  const int64_t round = DL_WAVES * DL4_KSTEP;            // one step of every wave
  for (int64_t K = 32; K <= 3 * round + 256; K += 32) run_k(K);
  for (int64_t K : {4096, 4128, 8192 - 32, 14336, 20480}) run_k(K);

  // plan
  for (int cus : {64, 104, 256, 304})
    for (int act = 0; act < 2; ++act) {
      int last[17] = {};
      for (int64_t N = act ? 2 : 1; N <= 200000; N += (N < 600 ? 1 + act : 1 + act + 2 * (N / 97))) {
        if (act && (N & 1)) continue;
        int prev = 0;
        for (int M : {1, 4, 5, 16}) {
          const int t = dl4_plan_tiles(M, N, 4096, act, cus);
          CHECK(t == 1 || t == 2 || t == 4, "tiles %d", t);
          CHECK(!act || t >= 2, "SwiGLU needs gate and up tiles");
          CHECK(t == dl4_plan_tiles(M, N, 20480, act, cus) && t == dl4_plan_tiles(M, N, 4096, act, cus), "plan is not pure / depends on K");
          CHECK(t >= prev, "more rows of x, smaller slab");
          prev = t;
          CHECK(t >= last[M], "N %lld: the slab shrank as N grew (%d after %d)", (long long)N, t, last[M]);      // monotone in N
          last[M] = t;
          const int64_t wgs = dl_plan_wgs(t, N, act), per = act ? 4 * t : 8 * t, cols = act ? N / 2 : N;
          CHECK((wgs - 1) * per < cols && cols <= wgs * per, "N %lld: %lld workgroups of %lld columns", (long long)N, (long long)wgs, (long long)per);
          if (2 * t <= DL_MAX_TILES) CHECK(dl_plan_wgs(2 * t, N, act) < dl4_plan_want(cus), "a larger slab would still fill the chip");
          if (t > (act ? 2 : 1)) CHECK(wgs >= cus, "a slab above the least one leaves CUs empty");
          if (act) {
            run_swiglu_rows(t, N, 0);
            run_swiglu_rows(t, N, wgs - 1);              // the ragged last workgroup
          }
        }
      }
    }
  for (int M : {1, 4, 5, 16})
    CHECK(dl_plan_wgs(dl4_plan_tiles(M, 4096, 14336, 0, 256), 4096, 0) >= 256, "N = 4096: fewer workgroups than CUs");
  std::printf("OK\n");
  return 0;
}
