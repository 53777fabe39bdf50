// CPU check of attn_plan.h: sweeps sequence lengths and asserts what attn.hip relies on.
//   g++ -std=c++17 -I csrc/kernels csrc/kernels/attn_plan_check.cpp -o attn_plan_check && ./attn_plan_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "attn_plan.h"

using namespace mpa;

#define REQUIRE(c)                                                          \
  do {                                                                      \
    if (!(c)) {                                                             \
      std::printf("FAILED %s (line %d): S %d\n", #c, __LINE__, g.S);        \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

// element index of the last bf16 an operand read (row, col .. col + 7) touches in an LDS tile
static int frag_last(int row, int col) { return row * AT_PITCH + col + 7; }

static void check_seq(const AttnGeom& g) {
  REQUIRE(attn_geom_error(g) == nullptr);
  const AttnPlan p = attn_plan(g);
  REQUIRE(p.tiles >= 1 && p.tail >= 1 && p.tail <= AT_TILE);
  REQUIRE((p.tiles - 1) * AT_TILE + p.tail == g.S);
  REQUIRE(p.blocks == (int64_t)p.tiles * g.H * g.B);
  // every query row is owned by exactly one (tile, wave, lane % 16), every key column is one
  // (tile, sub-tile, lane group, register) of a streamed tile; positions >= S are masked
  std::vector<int> rows(g.S, 0), cols(g.S, 0);
  for (int tile = 0; tile < p.tiles; ++tile) {
    for (int w = 0; w < AT_WAVES; ++w)
      for (int i = 0; i < 16; ++i) {
        const int r = tile * AT_TILE + 16 * w + i;
        if (r < g.S) ++rows[r];
      }
    for (int t = 0; t < 4; ++t)
      for (int gq = 0; gq < 4; ++gq)
        for (int e = 0; e < 4; ++e) {
          const int c = tile * AT_TILE + at_acc_row(t, gq, e);
          REQUIRE(at_acc_row(t, gq, e) < AT_TILE);
          if (c < g.S) ++cols[c];
        }
  }
  for (int s = 0; s < g.S; ++s) REQUIRE(rows[s] == 1 && cols[s] == 1);
  // LDS budgets: what the kernels declare, under the static limit
  REQUIRE(p.lds_fwd == 4 * AT_TILE_BYTES && p.lds_fwd <= AT_LDS_LIMIT);
  REQUIRE(p.lds_dq == 3 * AT_TILE_BYTES && p.lds_dq <= AT_LDS_LIMIT);
  REQUIRE(p.lds_dkv == 4 * AT_TILE_BYTES + 512 && p.lds_dkv <= AT_LDS_LIMIT);
}

int main() {
  const AttnGeom g{1, 1, 1};
  // tile geometry, independent of S: staging writes and operand reads stay inside a tile, the
  // pitch keeps 16-B alignment, and the transposed order is the accumulator's
  REQUIRE(AT_PITCH % 8 == 0 && AT_PITCH >= AT_D + 8 && AT_THREADS * 2 * 8 == AT_TILE * AT_D);
  bool seen[AT_TILE] = {};
  for (int r = 0; r < AT_TILE; ++r) {
    const int pos = at_pos(r);
    REQUIRE(pos >= 0 && pos < AT_TILE && !seen[pos]);
    seen[pos] = true;
  }
  for (int hh = 0; hh < 2; ++hh)
    for (int gq = 0; gq < 4; ++gq)
      for (int e = 0; e < 8; ++e)  // operand element e of lane group gq, half hh
        REQUIRE(at_pos(at_acc_row(2 * hh + e / 4, gq, e % 4)) == 32 * hh + 8 * gq + e);
  for (int tid = 0; tid < AT_THREADS; ++tid)
    for (int pp = 0; pp < 2; ++pp) {
      const int r = (tid >> 3) + 32 * pp, c = (tid & 7) * 8;
      REQUIRE(r < AT_TILE && frag_last(r, c) < AT_TILE * AT_PITCH);      // row staging
      REQUIRE(frag_last(c + 7, at_pos(r) - 7) < AT_TILE * AT_PITCH);     // transposed staging
    }
  for (int t = 0; t < 4; ++t)
    for (int lane = 0; lane < 64; ++lane)
      for (int kk = 0; kk < 2; ++kk) {
        const int row = 16 * t + (lane & 15), col = 32 * kk + 8 * (lane >> 4);
        REQUIRE(col + 7 < AT_D && frag_last(row, col) < AT_TILE * AT_PITCH);
        REQUIRE((row * AT_PITCH + col) % 8 == 0);
      }
  // a wave's output patch [16][AT_PITCH] lies inside the first tile for every wave
  REQUIRE(AT_WAVES * 16 * AT_PITCH <= AT_TILE * AT_PITCH);
  // bank-conflict freedom of an operand read: 16 rows start at distinct 16-B bank groups
  bool bank[16] = {};
  for (int i = 0; i < 16; ++i) {
    const int grp = (i * AT_PITCH * 2 / 16) % 16;
    REQUIRE(!bank[grp]);
    bank[grp] = true;
  }

  long n = 0;
  for (int S = 1; S <= 1024; ++S, ++n) check_seq(AttnGeom{2, S, 3});
  for (int S : {1025, 2049, 4097, 16385, 65537}) {
    check_seq(AttnGeom{1, S, 1});
    ++n;
  }
  if (attn_plan(AttnGeom{256, 197, 12}).tiles != 4 || attn_plan(AttnGeom{1, 577, 12}).tiles != 10)
    return std::printf("vit plan\n"), 1;
  const AttnGeom bad[] = {{1, 0, 1}, {0, 5, 1}, {1, 5, 0}, {70000, 5, 1}, {4096, 4096, 12}};
  for (const AttnGeom& b : bad)
    if (!attn_geom_error(b)) return std::printf("accepted a refused geometry\n"), 1;
  // patchify: every output vector reads inside x, and each source vector exactly once
  for (const PatchGeom& pg : {PatchGeom{2, 32, 48, 8, 16}, PatchGeom{1, 16, 16, 4, 16},
                              PatchGeom{3, 8, 12, 2, 4}}) {
    if (patch_geom_error(pg)) return std::printf("patch geometry refused\n"), 1;
    const int64_t nvec = (int64_t)pg.B * pg.Hi * pg.Wi * pg.Cp / 8;
    std::vector<int> hit(nvec, 0);
    for (int64_t i = 0; i < nvec; ++i) {
      const int64_t s = patch_src(pg, i);
      if (s < 0 || s % 8 || s / 8 >= nvec) return std::printf("patch source out of range\n"), 1;
      ++hit[s / 8];
    }
    for (int64_t i = 0; i < nvec; ++i)
      if (hit[i] != 1) return std::printf("patch cover\n"), 1;
  }
  if (!patch_geom_error(PatchGeom{1, 20, 16, 8, 16}) || !patch_geom_error(PatchGeom{1, 6, 6, 1, 3}) ||
      !tok_geom_error(TokGeom{1, 5, 12}) || !tok_geom_error(TokGeom{1, 1, 8}))
    return std::printf("accepted a refused token geometry\n"), 1;
  std::printf("attn_plan_check sweep ok: %ld plans\n", n);
  return 0;
}
