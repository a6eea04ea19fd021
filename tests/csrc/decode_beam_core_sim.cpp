// decode_beam_core_sim.cpp — whole beam searches on the host through cambrian_amd/csrc/decode_beam_core.h, the very header
// decode_beam.hip includes: the ordering key, cmb_beam_step (running beams, hypotheses, the merge, the flag) and the state
// block's layout.  Built by tests/test_decode_beam_core_sim.py with g++ under AddressSanitizer and UBSan and run directly.
//
// Input (argv[1], text): the number of cases, then per case a line "nb V steps max_new eos" and `steps` lines of nb * V fp32 bit
// patterns (hex): the log-probabilities of slot i's row at that step.  The sequences are moved the way the kernel moves
// them: the running ones between two halves, the kept ones column by column, every read before the first write.
// Output: per step one line "S <case> <step> | parent | tok | run_score bits | fin_score bits | fin_len | fin_ok | unsat all_hit"
// and the lines "R <slot> <ids>" / "F <slot> <ids>" of the running and the kept sequences; "OK" at the end.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cambrian_amd/csrc/decode_beam_core.h"

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      return 1;                                                   \
    }                                                             \
  } while (0)

static int check_layout() {
  for (int prompts = 1; prompts <= 8; ++prompts)
    for (int nb = 2; nb * prompts <= 16; ++nb)
      for (int64_t M : {1, 2, 7, 512}) {
        const cmb_beam_layout L = cmb_beam_make_layout(prompts, nb, M);
        const int64_t R = prompts * nb, K = 2 * nb;
        const int64_t bytes[CMB_BEAM_SECTIONS] = {4 * R, 4 * R, 4 * R, 4 * R, 4 * R, 4 * R * K, 4 * R * K, R, prompts, prompts,
                                                  16 * R * M, 8 * R * M};
        CHECK(L.off[0] == 0);
        for (int i = 0; i < CMB_BEAM_SECTIONS; ++i) {
          CHECK(L.off[i] % 16 == 0);
          const int64_t end = i + 1 < CMB_BEAM_SECTIONS ? L.off[i + 1] : L.total;
          CHECK(L.off[i] + bytes[i] <= end && end - L.off[i] - bytes[i] < 16);
        }
      }
  return 0;
}

static int check_key() {
  // larger score first; equal scores (and -0 / +0) by the lower index; -inf below every number; distinct indices, distinct keys
  CHECK(cmb_beam_key(1.f, 7) > cmb_beam_key(0.5f, 0));
  CHECK(cmb_beam_key(-1.f, 7) > cmb_beam_key(-1.5f, 0));
  CHECK(cmb_beam_key(2.f, 3) > cmb_beam_key(2.f, 4));
  CHECK(cmb_beam_key(0.f, 3) > cmb_beam_key(-0.f, 4) && cmb_beam_key(-0.f, 3) > cmb_beam_key(0.f, 4));
  CHECK(cmb_beam_key(-INFINITY, 0) < cmb_beam_key(-3.0e38f, 0x7FFFFFFFu));
  CHECK(cmb_beam_key(-1.0e9f, 5) != cmb_beam_key(-1.0e9f, 6));
  CHECK(cmb_beam_hyp_score(-6.f, 3) == -2.f);
  return 0;
}

int main(int argc, char** argv) {
  if (check_layout() || check_key()) return 1;
  if (argc < 2) {
    std::printf("OK\n");
    return 0;
  }
  FILE* in = std::fopen(argv[1], "r");
  CHECK(in);
  int cases = 0;
  CHECK(std::fscanf(in, "%d", &cases) == 1);
  for (int cs = 0; cs < cases; ++cs) {
    int nb, V, steps;
    long long max_new, eos;
    CHECK(std::fscanf(in, "%d %d %d %lld %lld", &nb, &V, &steps, &max_new, &eos) == 5);
    CHECK(nb >= 2 && nb <= CMB_BEAM_MAX && V >= 2 && steps >= 1 && steps <= max_new);
    const int K = 2 * nb;
    const int64_t M = max_new;
    cmb_beam_prompt P;
    cmb_beam_init(&P, nb);
    std::vector<int64_t> run[2] = {std::vector<int64_t>(nb * M, 0), std::vector<int64_t>(nb * M, 0)};
    std::vector<int64_t> fin(nb * M, 0);
    for (int step = 0; step < steps; ++step) {
      std::vector<cmb_beam_cand> all(nb * V);
      std::vector<uint64_t> keys(nb * V);
      for (int i = 0; i < nb * V; ++i) {
        unsigned bits;
        CHECK(std::fscanf(in, "%x", &bits) == 1);
        all[i].beam = i / V;
        all[i].tok = i % V;
        all[i].score = P.run_score[i / V] + cmb_ds_float(bits);
        keys[i] = cmb_beam_key(all[i].score, (uint32_t)i);
      }
      std::vector<int> order(nb * V);
      for (int i = 0; i < nb * V; ++i) order[i] = i;
      std::sort(order.begin(), order.end(), [&](int a, int b) { return keys[a] > keys[b]; });
      cmb_beam_cand top[CMB_BEAM_MAXK];
      for (int c = 0; c < K; ++c) top[c] = all[order[c]];
      cmb_beam_step(&P, top, nb, step, eos, step + 1 == max_new);

      const std::vector<int64_t>& old_run = run[step & 1];
      std::vector<int64_t>& new_run = run[(step + 1) & 1];
      for (int i = 0; i < nb; ++i) {
        CHECK(P.parent[i] >= 0 && P.parent[i] < nb && P.tok[i] >= 0 && P.tok[i] < V);
        CHECK(top[P.run_src[i]].beam == P.parent[i] && top[P.run_src[i]].tok == P.tok[i]);
        for (int c = 0; c <= step; ++c) new_run[i * M + c] = c < step ? old_run[P.parent[i] * M + c] : P.tok[i];
      }
      bool moved = false;
      for (int i = 0; i < nb; ++i) moved |= P.fin_src[i] != i;
      CHECK(moved == (P.fin_moved != 0));
      if (P.fin_moved)
        for (int c = 0; c <= step; ++c) {
          int64_t val[CMB_BEAM_MAX];
          for (int i = 0; i < nb; ++i) {
            const int src = P.fin_src[i];
            CHECK(src >= 0 && src < nb + K);
            val[i] = src < nb ? fin[src * M + c] : (c < step ? old_run[top[src - nb].beam * M + c] : top[src - nb].tok);
          }
          for (int i = 0; i < nb; ++i) fin[i * M + c] = val[i];
        }

      std::printf("S %d %d |", cs, step);
      for (int i = 0; i < nb; ++i) std::printf(" %d", P.parent[i]);
      std::printf(" |");
      for (int i = 0; i < nb; ++i) std::printf(" %d", P.tok[i]);
      std::printf(" |");
      for (int i = 0; i < nb; ++i) std::printf(" %08x", cmb_ds_bits(P.run_score[i]));
      std::printf(" |");
      for (int i = 0; i < nb; ++i) std::printf(" %08x", cmb_ds_bits(P.fin_score[i]));
      std::printf(" |");
      for (int i = 0; i < nb; ++i) std::printf(" %d", P.fin_len[i]);
      std::printf(" |");
      for (int i = 0; i < nb; ++i) std::printf(" %d", P.fin_ok[i]);
      std::printf(" | %d %d\n", P.unsat, P.all_hit);
      for (int i = 0; i < nb; ++i) {
        std::printf("R %d", i);
        for (int c = 0; c <= step; ++c) std::printf(" %lld", (long long)new_run[i * M + c]);
        std::printf("\nF %d", i);
        for (int c = 0; c < P.fin_len[i]; ++c) std::printf(" %lld", (long long)fin[i * M + c]);
        std::printf("\n");
      }
    }
  }
  std::fclose(in);
  std::printf("OK\n");
  return 0;
}
