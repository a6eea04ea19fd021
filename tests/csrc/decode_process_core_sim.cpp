// CPU run of cambrian_amd/csrc/decode_process_core.h — the very header decode_process.hip includes — for
// tests/test_decode_process_core_sim.py (g++ -fsanitize=address,undefined).  Without arguments: the argument rules of
// cmb_decode_process and the predicates on hand-made cases.  With a table file: every case goes through one row's pass in the
// kernel's order (penalty at first occurrences, then the bans, then the done flag) and the logits' bits are printed.
//
// table file:  <cases>  then per case
//   V n g penalty_bits min_new n_eos n_bans n_words n_word_ids
//   eos ids | ban ids | word offsets (n_words + 1) | word ids | history (n ids) | logits bits (V, hex)      one line each
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cambrian_amd/csrc/decode_process_core.h"

static int fails = 0;
#define EXPECT(c)                                              \
  do {                                                         \
    if (!(c)) {                                                \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);       \
      ++fails;                                                 \
    }                                                          \
  } while (0)

static float from_bits(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
static uint32_t to_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

static void ban(std::vector<float>& row, int64_t id) {
  const int32_t c = cmb_dp_index(id, (int64_t)row.size());
  if (c >= 0) row[c] = from_bits(0xFF800000u);
}

// one row, the kernel's order; exact-size vectors so that AddressSanitizer sees any read or write outside them
static int one_row(std::vector<float>& row, const std::vector<int64_t>& h, int64_t g, float penalty, int64_t min_new,
                   const std::vector<int64_t>& eos, const std::vector<int64_t>& bans, const std::vector<int64_t>& off,
                   const std::vector<int64_t>& ids) {
  const int64_t n = (int64_t)h.size(), V = (int64_t)row.size();
  if (penalty != 1.0f)
    for (int64_t j = 0; j < n; ++j) {
      const int32_t c = cmb_dp_index(h[j], V);
      if (c >= 0 && cmb_dp_first_occurrence(h.data(), j)) row[c] = cmb_dp_penalise(row[c], penalty);
    }
  if (cmb_dp_ngram_active(n, g))
    for (int64_t i = 0; i <= n - g; ++i)
      if (cmb_dp_ngram_hits(h.data(), n, g, i)) ban(row, h[i + g - 1]);
  for (int64_t id : bans) ban(row, id);
  for (int64_t w = 0; w + 1 < (int64_t)off.size(); ++w) {
    int64_t first = 0;
    const int64_t m = cmb_dp_word_at(off.data(), w, (int64_t)ids.size(), &first);
    if (m > 0 && cmb_dp_word_hits(h.data(), n, ids.data() + first, m)) ban(row, ids[first + m - 1]);
  }
  if (n < min_new)
    for (int64_t id : eos) ban(row, id);
  return n >= 1 && cmb_dp_in_set(h[n - 1], eos.data(), (int64_t)eos.size()) ? 1 : 0;
}

static void self_checks() {
  alignas(16) static char buf[64];
  const float* lg = (const float*)buf;
  const int64_t* q = (const int64_t*)buf;
  const uint8_t* d = (const uint8_t*)buf;
  auto call = [&](const float* logits, int64_t ld, int32_t B, int64_t V, const int64_t* hist, int64_t hld, int64_t n, float p,
                  int64_t g, int64_t mn, const int64_t* eos, int32_t ne, const int64_t* bans, int32_t nb, const int64_t* ids,
                  int64_t ni, const int64_t* off, int32_t nw) {
    return cmb_dp_check_args(logits, ld, B, V, hist, hld, n, p, g, mn, eos, ne, bans, nb, ids, ni, off, nw, d);
  };
  EXPECT(call(lg, 1011, 3, 1000, q, 40, 37, 1.3f, 3, 0, q, 2, q, 2, q, 5, q, 2) == CMB_OK);
  EXPECT(call(lg, 1000, 1, 1000, nullptr, 0, 0, 1.0f, 0, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0) == CMB_OK);
  EXPECT(call(nullptr, 1011, 3, 1000, q, 40, 37, 1.3f, 3, 0, q, 2, q, 2, q, 5, q, 2) == CMB_ERR_BAD_ARG);
  EXPECT(call(lg, 1011, 3, 1000, nullptr, 40, 37, 1.3f, 3, 0, q, 2, q, 2, q, 5, q, 2) == CMB_ERR_BAD_ARG);
  EXPECT(call(lg, 1011, 3, 1000, q, 40, 37, 1.3f, 3, 0, nullptr, 2, q, 2, q, 5, q, 2) == CMB_ERR_BAD_ARG);
  EXPECT(call(lg, 1011, 3, 1000, q, 40, 37, 1.3f, 3, 0, q, 2, nullptr, 2, q, 5, q, 2) == CMB_ERR_BAD_ARG);
  EXPECT(call(lg, 1011, 3, 1000, q, 40, 37, 1.3f, 3, 0, q, 2, q, 2, nullptr, 5, q, 2) == CMB_ERR_BAD_ARG);
  EXPECT(call(lg, 1011, 3, 1000, q, 40, 37, 1.3f, 3, 0, q, 2, q, 2, q, 5, nullptr, 2) == CMB_ERR_BAD_ARG);
  EXPECT(call(lg, 1011, 3, 1000, q, 40, 37, 1.3f, 3, 0, q, 2, q, 2, q, 1, q, 2) == CMB_ERR_BAD_ARG);
  EXPECT(call(lg, 1011, 0, 1000, q, 40, 37, 1.3f, 3, 0, q, 2, q, 2, q, 5, q, 2) == CMB_ERR_BAD_ARG);
  EXPECT(call(lg, 999, 3, 1000, q, 40, 37, 1.3f, 3, 0, q, 2, q, 2, q, 5, q, 2) == CMB_ERR_BAD_ARG);
  EXPECT(call(lg, 1ll << 31, 3, 1ll << 31, q, 40, 37, 1.3f, 3, 0, q, 2, q, 2, q, 5, q, 2) == CMB_ERR_BAD_ARG);
  EXPECT(call(lg, 0x7FFFFFFFll, 3, 0x7FFFFFFFll, q, 40, 37, 1.3f, 3, 0, q, 2, q, 2, q, 5, q, 2) == CMB_OK);
  EXPECT(call(lg, 1011, 3, 1000, q, 36, 37, 1.3f, 3, 0, q, 2, q, 2, q, 5, q, 2) == CMB_ERR_BAD_ARG);
  EXPECT(call(lg, 1011, 3, 1000, q, 40, -1, 1.3f, 3, 0, q, 2, q, 2, q, 5, q, 2) == CMB_ERR_BAD_ARG);
  EXPECT(call(lg, 1011, 3, 1000, q, 40, 37, 0.0f, 3, 0, q, 2, q, 2, q, 5, q, 2) == CMB_ERR_BAD_ARG);
  EXPECT(call(lg, 1011, 3, 1000, q, 40, 37, -1.3f, 3, 0, q, 2, q, 2, q, 5, q, 2) == CMB_ERR_BAD_ARG);
  EXPECT(call(lg, 1011, 3, 1000, q, 40, 37, from_bits(0x7F800000u), 3, 0, q, 2, q, 2, q, 5, q, 2) == CMB_ERR_BAD_ARG);
  EXPECT(call(lg, 1011, 3, 1000, q, 40, 37, from_bits(0x7FC00000u), 3, 0, q, 2, q, 2, q, 5, q, 2) == CMB_ERR_BAD_ARG);
  EXPECT(call(lg, 1011, 3, 1000, q, 40, 37, 1.3f, -1, 0, q, 2, q, 2, q, 5, q, 2) == CMB_ERR_BAD_ARG);
  EXPECT(call(lg, 1011, 3, 1000, q, 40, 37, 1.3f, 3, -1, q, 2, q, 2, q, 5, q, 2) == CMB_ERR_BAD_ARG);
  EXPECT(call((const float*)(buf + 2), 1011, 3, 1000, q, 40, 37, 1.3f, -1, 0, q, 2, q, 2, q, 5, q, 2) == CMB_ERR_BAD_ARG);
  EXPECT(call((const float*)(buf + 2), 1011, 3, 1000, q, 40, 37, 1.3f, 3, 0, q, 2, q, 2, q, 5, q, 2) == CMB_ERR_ALIGNMENT);
  EXPECT(call((const float*)(buf + 4), 1011, 3, 1000, q, 40, 37, 1.3f, 3, 0, q, 2, q, 2, q, 5, q, 2) == CMB_OK);
  EXPECT(call(lg, 1011, 3, 1000, (const int64_t*)(buf + 4), 40, 37, 1.3f, 3, 0, q, 2, q, 2, q, 5, q, 2) == CMB_ERR_ALIGNMENT);

  EXPECT(cmb_dp_index(0, 5) == 0 && cmb_dp_index(4, 5) == 4 && cmb_dp_index(5, 5) == -1 && cmb_dp_index(-1, 5) == -1);
  EXPECT(cmb_dp_index(1ll << 40, 0x7FFFFFFFll) == -1 && cmb_dp_index(0x7FFFFFFEll, 0x7FFFFFFFll) == 0x7FFFFFFE);
  EXPECT(to_bits(cmb_dp_penalise(-0.0f, 1.3f)) == 0x80000000u && to_bits(cmb_dp_penalise(from_bits(0xFF800000u), 0.8f)) == 0xFF800000u);
  EXPECT(cmb_dp_penalise(2.0f, 0.5f) == 4.0f && cmb_dp_penalise(-2.0f, 0.5f) == -1.0f);
  const int64_t h[6] = {7, 8, 7, 8, 7, 9};
  EXPECT(!cmb_dp_ngram_active(5, 0) && !cmb_dp_ngram_active(1, 3) && cmb_dp_ngram_active(2, 3) && cmb_dp_ngram_active(0, 1));
  EXPECT(!cmb_dp_ngram_hits(h, 5, 3, 0) && cmb_dp_ngram_hits(h, 5, 3, 1) && !cmb_dp_ngram_hits(h, 5, 3, 2));   // tail 8 7
  EXPECT(cmb_dp_ngram_hits(h, 6, 1, 3));
  const int64_t w[3] = {8, 7, 5};
  EXPECT(cmb_dp_word_hits(h, 5, w, 3) && !cmb_dp_word_hits(h, 6, w, 3) && !cmb_dp_word_hits(h, 2, w, 3));
  EXPECT(cmb_dp_word_hits(h, 0, w, 1) && !cmb_dp_word_hits(h, 3, w, 0));
  const int64_t two[2] = {7, 8};
  EXPECT(!cmb_dp_word_hits(h, 1, two, 2) && cmb_dp_word_hits(h, 3, two, 2));     // m <= n: a history of m - 1 ids bans nothing
  EXPECT(cmb_dp_first_occurrence(h, 0) && cmb_dp_first_occurrence(h, 1) && !cmb_dp_first_occurrence(h, 2) && cmb_dp_first_occurrence(h, 5));
  const int64_t off[4] = {0, 2, 2, 9};
  int64_t first = -1;
  EXPECT(cmb_dp_word_at(off, 0, 3, &first) == 2 && first == 0);
  EXPECT(cmb_dp_word_at(off, 1, 3, &first) == 0 && cmb_dp_word_at(off, 2, 3, &first) == 0);      // empty, and past the ids
  EXPECT(cmb_dp_in_set(9, h, 6) && !cmb_dp_in_set(1, h, 6) && !cmb_dp_in_set(7, h, 0));
}

static std::vector<int64_t> read_ids(FILE* f, int64_t n) {
  std::vector<int64_t> v((size_t)n);
  for (auto& x : v) {
    long long t;
    if (std::fscanf(f, "%lld", &t) != 1) std::exit(2);
    x = t;
  }
  return v;
}

int main(int argc, char** argv) {
  self_checks();
  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    long long cases;
    if (std::fscanf(f, "%lld", &cases) != 1) return 2;
    for (long long c = 0; c < cases; ++c) {
      long long V, n, g, min_new, ne, nb, nw, ni;
      unsigned pbits;
      if (std::fscanf(f, "%lld %lld %lld %x %lld %lld %lld %lld %lld", &V, &n, &g, &pbits, &min_new, &ne, &nb, &nw, &ni) != 9) return 2;
      const std::vector<int64_t> eos = read_ids(f, ne), bans = read_ids(f, nb), off = read_ids(f, nw ? nw + 1 : 0),
                                 ids = read_ids(f, ni), h = read_ids(f, n);
      std::vector<float> row((size_t)V);
      for (auto& x : row) {
        unsigned u;
        if (std::fscanf(f, "%x", &u) != 1) return 2;
        x = from_bits(u);
      }
      const int done = one_row(row, h, g, from_bits(pbits), min_new, eos, bans, off, ids);
      std::printf("C %lld %d", c, done);
      for (float x : row) std::printf(" %x", to_bits(x));
      std::printf("\n");
    }
    std::fclose(f);
  }
  std::printf(fails ? "FAILED\n" : "OK\n");
  return fails ? 1 : 0;
}
