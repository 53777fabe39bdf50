// CPU check of wattn_plan.h: sweeps window geometries and asserts what wattn.hip relies on.
//   g++ -std=c++17 -I csrc/kernels csrc/kernels/wattn_plan_check.cpp -o wattn_plan_check && ./wattn_plan_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "wattn_plan.h"

using namespace mpa;

#define REQUIRE(c)                                                                            \
  do {                                                                                        \
    if (!(c)) {                                                                               \
      std::printf("FAILED %s (line %d): B %d H %d map %d x %d ws %d shift %d\n", #c, __LINE__, \
                  g.B, g.H, g.Hf, g.Wf, g.ws, g.shift);                                       \
      std::exit(1);                                                                           \
    }                                                                                         \
  } while (0)

static void check_geom(const WattnGeom& g) {
  REQUIRE(wattn_geom_error(g) == nullptr);
  const WattnPlan p = wattn_plan(g);
  const int S2 = g.ws * g.ws, npix = g.B * g.Hf * g.Wf;
  REQUIRE(p.waves >= 1 && p.waves <= 4 && g.H % p.waves == 0 && p.groups * p.waves == g.H);
  for (int w = p.waves + 1; w <= 4; ++w) REQUIRE(g.H % w != 0);  // the largest divisor
  REQUIRE(p.nwin * S2 == npix && p.nbias == (2 * g.ws - 1) * (2 * g.ws - 1) && p.nbias <= WA_BIAS_MAX);
  // the walks partition the windows; the slab is capped
  REQUIRE(p.wpb >= 1 && p.rows >= 1 && p.rows <= WA_MAX_ROWS);
  REQUIRE((int64_t)(p.rows - 1) * p.wpb < p.nwin && (int64_t)p.rows * p.wpb >= p.nwin);
  REQUIRE(p.wpb == 1 || (int64_t)p.rows * p.groups <= WA_FILL_BLOCKS);  // CUs first, then walks
  REQUIRE(p.ws_floats == (int64_t)p.rows * g.H * p.nbias);
  REQUIRE(p.lds_fwd == p.waves * WA_FWD_BYTES && p.lds_bwd == p.waves * WA_BWD_BYTES);
  REQUIRE(p.lds_fwd <= AT_LDS_LIMIT && p.lds_bwd <= AT_LDS_LIMIT);
  // the cosine variant: the same grid and walks, two norm rows more LDS, one slab column more
  const WattnPlan c = wattn_plan(g, true);
  REQUIRE(c.waves == p.waves && c.groups == p.groups && c.nwin == p.nwin && c.wpb == p.wpb && c.rows == p.rows);
  REQUIRE(c.nbias == p.nbias && p.slab_cols == p.nbias && c.slab_cols == p.nbias + 1);
  REQUIRE(c.ws_floats == (int64_t)c.rows * g.H * c.slab_cols);
  REQUIRE(c.lds_fwd == p.waves * WA_FWD_COS_BYTES && c.lds_bwd == p.waves * WA_BWD_COS_BYTES);
  REQUIRE(c.lds_fwd <= AT_LDS_LIMIT && c.lds_bwd <= AT_LDS_LIMIT);

  // a labelled map, rolled by brute force: label[pixel] = region of the pixel's rolled position
  std::vector<int> rolled_region(npix, -1);
  for (int b = 0; b < g.B; ++b)
    for (int ry = 0; ry < g.Hf; ++ry)
      for (int rx = 0; rx < g.Wf; ++rx) {
        int by = 0, bx = 0;  // the published slices (0, -ws), (-ws, -shift), (-shift, end)
        if (g.shift) {
          by = ry >= g.Hf - g.shift ? 2 : (ry >= g.Hf - g.ws ? 1 : 0);
          bx = rx >= g.Wf - g.shift ? 2 : (rx >= g.Wf - g.ws ? 1 : 0);
        }
        const int y = (ry + g.shift) % g.Hf, x = (rx + g.shift) % g.Wf;  // roll by -shift
        rolled_region[(b * g.Hf + y) * g.Wf + x] = 3 * by + bx;
      }
  // every window token maps to a distinct in-range row; the windows cover the map once
  std::vector<int> hit(npix, 0);
  for (int win = 0; win < p.nwin; ++win)
    for (int n = 0; n < WA_N; ++n) {
      uint32_t info;
      const int row = wattn_token(g, win, n, &info);
      if (n >= S2) {
        REQUIRE(row == -1 && info == 0);
        continue;
      }
      REQUIRE(row >= 0 && row < npix);
      ++hit[row];
      REQUIRE((int)(info & 255) == n / g.ws && (int)((info >> 8) & 255) == n % g.ws);
      REQUIRE((int)(info >> 16) == rolled_region[row]);
    }
  for (int i = 0; i < npix; ++i) REQUIRE(hit[i] == 1);
}

int main() {
  WattnGeom g{1, 1, 1, 1, 1, 0};
  // layout constants: aligned sub-buffers, patches and the fold slice inside their tiles
  REQUIRE(WA_PITCH % 8 == 0 && WA_PITCH >= WA_N + 8 && WA_PPITCH % 8 == 0 && WA_PPITCH >= WA_D);
  REQUIRE(WA_FWD_BYTES % 16 == 0 && WA_BWD_BYTES % 16 == 0 && WA_TILE_BYTES % 16 == 0);
  REQUIRE(4 * WA_BWD_BYTES <= AT_LDS_LIMIT && 4 * WA_FWD_BYTES <= AT_LDS_LIMIT);
  REQUIRE(WA_FWD_COS_BYTES % 16 == 0 && WA_BWD_COS_BYTES % 16 == 0 && WA_NORM_BYTES == WA_N * 4);
  REQUIRE(4 * WA_BWD_COS_BYTES <= AT_LDS_LIMIT && 4 * WA_FWD_COS_BYTES <= AT_LDS_LIMIT);
  REQUIRE(16 * WA_PPITCH * 2 <= WA_TILE_BYTES);            // phase A's dQ patch in dOt
  REQUIRE(2 * 16 * WA_PPITCH * 2 <= WA_TILE_BYTES);        // phase B's dK and dV patches in Kt
  REQUIRE(16 * WA_FOLD_PITCH * 4 <= WA_TILE_BYTES && WA_FOLD_PITCH >= WA_N);  // the fold in Kt
  // transposed staging and operand reads stay inside a [32][WA_PITCH] tile
  for (int n = 0; n < WA_N; ++n)
    for (int d = 0; d < WA_D; ++d) REQUIRE(d * WA_PITCH + at_pos(n) < WA_D * WA_PITCH && at_pos(n) < WA_N);
  for (int lane = 0; lane < 64; ++lane)
    for (int dt = 0; dt < 2; ++dt)
      for (int hh = 0; hh < 2; ++hh) {
        const int row = 16 * dt + (lane & 15), col = 32 * hh + 8 * (lane >> 4);
        REQUIRE(row < WA_D && col + 7 < WA_N && (row * WA_PITCH + col) % 8 == 0);
      }
  // bank-conflict freedom of an operand read: 16 rows start at distinct 16-B bank groups
  bool bank[16] = {};
  for (int i = 0; i < 16; ++i) {
    const int grp = (i * WA_PITCH * 2 / 16) % 16;
    REQUIRE(!bank[grp]);
    bank[grp] = true;
  }

  long n = 0;
  for (int ws = 1; ws <= 8; ++ws) {
    // rel is a surjection onto 0 .. (2 ws - 1)^2 - 1, and the info words give the same index
    g = WattnGeom{1, 1, ws, ws, ws, 0};
    std::vector<int> seen((2 * ws - 1) * (2 * ws - 1), 0);
    for (int i = 0; i < ws * ws; ++i)
      for (int j = 0; j < ws * ws; ++j) {
        const int r = wattn_rel(ws, i / ws, i % ws, j / ws, j % ws);
        REQUIRE(r >= 0 && r < (int)seen.size());
        ++seen[r];
        uint32_t qi, kj;
        wattn_token(g, 0, i, &qi);
        wattn_token(g, 0, j, &kj);
        REQUIRE(wattn_rel_info(ws, qi, kj) == r);
        REQUIRE(wattn_rel_info(ws, 0, kj) >= 0 && wattn_rel_info(ws, qi, 0) < (int)seen.size());  // padded
      }
    for (int s : seen) REQUIRE(s > 0);
    for (int shift = 0; shift < ws; ++shift)
      for (int ny = 1; ny <= 3; ++ny)
        for (int nx = 1; nx <= 3; ++nx)
          for (int H : {1, 2, 3, 4, 5, 6, 12, 24}) {
            check_geom(WattnGeom{ny == 2 ? 3 : 1, H, ny * ws, nx * ws, ws, shift});
            ++n;
          }
  }
  // long walks: more windows than the fill target
  for (const WattnGeom& w : {WattnGeom{129, 1, 8, 8, 4, 1}, WattnGeom{65, 8, 8, 8, 4, 2},
                             WattnGeom{40, 3, 56, 56, 7, 3}}) {
    check_geom(w);
    g = w;
    REQUIRE(wattn_plan(w).wpb >= 2 && wattn_plan(w).rows >= 2);
    ++n;
  }
  // Swin-T's four stages at batch 256: 3-wave blocks for 3 and 6 heads, 4-wave for 12 and 24
  const int st[4][3] = {{3, 56, 3}, {6, 28, 3}, {12, 14, 4}, {24, 7, 4}};
  for (const auto& s : st) {
    g = WattnGeom{256, s[0], s[1], s[1], 7, s[1] > 7 ? 3 : 0};
    REQUIRE(wattn_geom_error(g) == nullptr && wattn_plan(g).waves == s[2]);
  }
  const WattnGeom bad[] = {{1, 1, 9, 9, 9, 0}, {1, 1, 15, 14, 7, 0}, {1, 1, 14, 15, 7, 0},
                           {1, 1, 14, 14, 7, 7}, {1, 1, 14, 14, 7, -1}, {0, 1, 7, 7, 7, 0},
                           {1, 0, 7, 7, 7, 0}, {4096, 24, 56, 56, 7, 3}};
  for (const WattnGeom& b : bad)
    if (!wattn_geom_error(b)) return std::printf("accepted a refused geometry\n"), 1;
  if (!wattn_geom_error(WattnGeom{1, 1, 7, 7, 7, 0}, 64)) return std::printf("accepted head dim 64\n"), 1;
  std::printf("wattn_plan_check sweep ok: %ld plans\n", n);
  return 0;
}
