// Host enumeration of cmb_decode_step's workspace (cambrian_amd/csrc/decode_step_layout.h, the very header decode_step.hip
// includes): every buffer 16-byte aligned with row strides that are multiples of 8 elements and wide enough for its rows,
// the buffers disjoint and the total their exact end, and no launch of any layer handed its own x or residual as output —
// with real byte ranges written and read in a heap block of exactly `total` floats (AddressSanitizer sees a byte past it).
//   sim                          the full check over B = 1..16 and the three model geometries; prints OK
//   sim --total B H I nh nkv hd attn [...]   prints dsl_make(...).total per group of seven (the host test's cross-check)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cambrian_amd/csrc/decode_step_layout.h"

struct Geo { const char* name; int64_t H, I, nh, nkv, hd; };
static const Geo GEOS[] = {{"llama3-8b", 4096, 14336, 32, 8, 128},
                           {"yi-34b", 7168, 20480, 56, 8, 128},
                           {"phi3-mini", 3072, 8192, 32, 32, 96},
                           {"test", 256, 512, 4, 2, 64}};

static int fail(const char* what, const Geo& g, int64_t B, int64_t attn) {
  std::printf("FAIL %s: %s B=%lld attn=%lld\n", what, g.name, (long long)B, (long long)attn);
  return 1;
}

static int check(const Geo& g, int64_t B, int64_t attn, int layers) {
  const dsl_layout L = dsl_make(B, g.H, g.I, g.nh, g.nkv, g.hd, attn);
  // strides: multiples of 8 elements, as wide as the rows they hold
  const int64_t lds[4] = {L.ld_qkv, L.ld_attn, L.ld_res, L.ld_inner};
  const int64_t widths[4] = {(g.nh + 2 * g.nkv) * g.hd, g.nh * g.hd, g.H, g.I};
  for (int i = 0; i < 4; ++i)
    if (lds[i] % 8 || lds[i] < widths[i]) return fail("row stride", g, B, attn);
  if (L.ld_attn != g.nh * g.hd) return fail("attention rows are contiguous", g, B, attn);
  // bytes each buffer must hold
  int64_t need[DSL_BUFS] = {0};
  need[DSL_QKV] = B * L.ld_qkv * 2;
  need[DSL_ATTN] = B * L.ld_attn * 2;
  need[DSL_RES0] = need[DSL_RES1] = B * L.ld_res * 2;
  need[DSL_INNER] = B * L.ld_inner * 2;
  need[DSL_PARTIAL] = attn * 4;
  int64_t end = 0;
  for (int i = DSL_QKV; i < DSL_BUFS; ++i) {
    if (L.off[i] % 4 || L.off[i] < 0) return fail("16-byte alignment", g, B, attn);
    if (L.size[i] * 4 < need[i]) return fail("buffer too small", g, B, attn);
    if (L.off[i] != end) return fail("gap or overlap", g, B, attn);       // packed in order: disjoint by construction ...
    end = L.off[i] + L.size[i];
    for (int j = DSL_QKV; j < i; ++j)                                     // ... and checked pairwise all the same
      if (L.off[i] < L.off[j] + L.size[j] && L.off[j] < L.off[i] + L.size[i]) return fail("overlap", g, B, attn);
  }
  if (L.total != end) return fail("total", g, B, attn);
  if (L.off[DSL_EXT_X] != 0 || L.size[DSL_EXT_X] != 0) return fail("external x has no room in the workspace", g, B, attn);

  // a block of exactly `total` floats: stamp every buffer with its id, read the stamps back
  std::vector<float> block((size_t)L.total);
  unsigned char* base = reinterpret_cast<unsigned char*>(block.data());
  for (int i = DSL_QKV; i < DSL_BUFS; ++i) std::memset(base + L.off[i] * 4, i, (size_t)need[i]);
  for (int i = DSL_QKV; i < DSL_BUFS; ++i)
    for (int64_t k = 0; k < need[i]; k += (need[i] > 4096 ? need[i] / 64 : 1))
      if (base[L.off[i] * 4 + k] != i) return fail("stamp overwritten", g, B, attn);
  if (need[DSL_PARTIAL] && base[L.off[DSL_PARTIAL] * 4 + need[DSL_PARTIAL] - 1] != DSL_PARTIAL)
    return fail("last byte", g, B, attn);

  // the launches: no output is that launch's x or residual; every operand holds what the launch before left there
  int holds[DSL_BUFS];          // which (layer, launch) wrote the buffer last: layer * 8 + launch, -1 = the caller
  for (int i = 0; i < DSL_BUFS; ++i) holds[i] = -2;
  holds[DSL_EXT_X] = -1;
  int stream_at = -1;           // the residual stream's latest version
  for (int l = 0; l < layers; ++l) {
    if (dsl_layer_in(l) != (l == 0 ? DSL_EXT_X : DSL_RES1)) return fail("layer input", g, B, attn);
    if (holds[dsl_layer_in(l)] != stream_at) return fail("layer input is stale", g, B, attn);
    for (int j = 0; j < DSL_LAUNCHES; ++j) {
      int x, r, o;
      dsl_launch_bufs(l, j, &x, &r, &o);
      if (o == x || o == r || o == DSL_EXT_X || o == DSL_NONE || o == DSL_PARTIAL) return fail("output aliases an operand", g, B, attn);
      if (x == DSL_NONE || x == DSL_PARTIAL || r == DSL_PARTIAL) return fail("operand", g, B, attn);
      const int want_x = j == 0 ? stream_at : l * 8 + j - 1;            // the launch before feeds this one
      if (holds[x] != want_x) return fail("x is not the previous launch's output", g, B, attn);
      if (j == 2 && (r != dsl_layer_in(l) || holds[r] != stream_at)) return fail("o_proj's skip is the layer input", g, B, attn);
      if (j == 4 && (r != DSL_RES0 || holds[r] != l * 8 + 2)) return fail("down_proj's skip is o_proj's output", g, B, attn);
      if ((j == 0 || j == 1 || j == 3) && r != DSL_NONE) return fail("no residual here", g, B, attn);
      holds[o] = l * 8 + j;
    }
    stream_at = l * 8 + 4;
  }
  if (holds[dsl_head_in()] != stream_at) return fail("lm_head input", g, B, attn);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "--total")) {
    for (int i = 2; i + 6 < argc; i += 7) {
      int64_t a[7];
      for (int k = 0; k < 7; ++k) a[k] = std::atoll(argv[i + k]);
      std::printf("%lld\n", (long long)dsl_make(a[0], a[1], a[2], a[3], a[4], a[5], a[6]).total);
    }
    return 0;
  }
  int bad = 0;
  for (const Geo& g : GEOS)
    for (int64_t B = 1; B <= DSL_MAX_B; ++B)
      for (int64_t splits : {0, 1, 2, 3, 7, 64}) {      // split partials of B * nh * splits * (hd + 2) floats, 0 = unsplit
        const int64_t attn = splits ? B * g.nh * splits * (g.hd + 2) + (splits == 3) : 0;
        bad += check(g, B, attn, 1) + check(g, B, attn, 2) + check(g, B, attn, 5);
      }
  if (bad) return 1;
  std::printf("OK\n");
  return 0;
}
