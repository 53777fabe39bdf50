// CPU check of xattn_plan.h: sweeps cross-attention geometries and asserts what xattn.hip relies on.
//   g++ -std=c++17 -I csrc/kernels csrc/kernels/xattn_plan_check.cpp -o xattn_plan_check && ./xattn_plan_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "xattn_plan.h"

using namespace mpa;

#define REQUIRE(c)                                                                               \
  do {                                                                                           \
    if (!(c)) {                                                                                  \
      std::printf("FAILED %s (line %d): B %d H %d Sq %d Sk %d\n", #c, __LINE__, g.B, g.H, g.Sq, g.Sk); \
      std::exit(1);                                                                              \
    }                                                                                            \
  } while (0)

static void check_geom(const XattnGeom& g) {
  REQUIRE(xattn_geom_error(g) == nullptr);
  const XattnPlan p = xattn_plan(g);
  REQUIRE(p.tiles == (g.Sq + AT_TILE - 1) / AT_TILE && p.tpw >= 1 && p.walks >= 1);
  REQUIRE(p.walks <= XA_MAX_ROWS);
  // every query tile is covered exactly once by the walks, and no walk is empty
  std::vector<int> hit(p.tiles, 0);
  for (int w = 0; w < p.walks; ++w) {
    const int t0 = w * p.tpw, t1 = t0 + p.tpw < p.tiles ? t0 + p.tpw : p.tiles;
    REQUIRE(t0 < t1);
    for (int t = t0; t < t1; ++t) ++hit[t];
  }
  for (int t = 0; t < p.tiles; ++t) REQUIRE(hit[t] == 1);
  // CUs first, then walks
  REQUIRE(p.tpw == 1 || p.walks == 1 || (int64_t)p.walks * g.B * g.H <= XA_FILL_BLOCKS);
  REQUIRE(p.lds_fwd == XA_LDS_FWD && p.lds_bwd == XA_LDS_BWD);
  REQUIRE(p.lds_fwd <= AT_LDS_LIMIT && p.lds_bwd <= AT_LDS_LIMIT);
  REQUIRE(p.ws_floats == (int64_t)p.walks * g.B * g.H * 64 * 128);
  // the last element a block and the sum kernel address lies inside the slab
  const int64_t last_row = ((int64_t)(g.B - 1) * g.H + g.H - 1) * p.walks + p.walks - 1;
  REQUIRE(last_row * XA_SLAB_ROW + AT_TILE * AT_D + (int64_t)(g.Sk - 1) * AT_D + AT_D <= p.ws_floats);
}

int main() {
  XattnGeom g{1, 1, 1, 1};
  // layout constants: the seven backward tiles and the forward's three fit the static limit; a
  // wave's 16-row patch is a quarter of a tile; a slab row holds dK and dV of 64 keys
  REQUIRE(XA_LDS_BWD == 7 * AT_TILE_BYTES && XA_LDS_FWD == 3 * AT_TILE_BYTES);
  REQUIRE(AT_WAVES * 16 * AT_PITCH * 2 == AT_TILE_BYTES && AT_WAVES * 16 == AT_TILE);
  REQUIRE(XA_SLAB_ROW == 64 * 128 && XA_MAX_KEYS == AT_TILE);
  // staging and operand reads stay inside a tile: transposed columns (at_pos of a key, or a
  // query of the tile) and the 16-B fragments
  for (int r = 0; r < AT_TILE; ++r)
    for (int d = 0; d < AT_D; ++d) {
      REQUIRE(d * AT_PITCH + at_pos(r) < AT_TILE * AT_PITCH && at_pos(r) < AT_TILE);
      REQUIRE(r * AT_PITCH + d < AT_TILE * AT_PITCH);
    }
  for (int lane = 0; lane < 64; ++lane)
    for (int t = 0; t < 4; ++t)
      for (int hh = 0; hh < 2; ++hh) {
        const int row = 16 * t + (lane & 15), col = 32 * hh + 8 * (lane >> 4);
        REQUIRE(row < AT_TILE && col + 7 < AT_D && (row * AT_PITCH + col) % 8 == 0);
        for (int e = 0; e < 4; ++e) REQUIRE(at_acc_row(t, lane >> 4, e) < AT_TILE);
      }

  long n = 0;
  for (int B : {1, 2, 3, 8, 64, 256, 700})
    for (int H : {1, 2, 5, 8})
      for (int Sq : {1, 16, 17, 49, 64, 65, 128, 129, 196, 784, 3136, 4097, 9000})
        for (int Sk : {1, 16, 33, 49, 64}) {
          g = XattnGeom{B, Sq, Sk, H};
          if ((int64_t)B * Sq * H * AT_D >= (int64_t)1 << 31) {  // refused, not planned
            REQUIRE(xattn_geom_error(g) != nullptr);
            continue;
          }
          check_geom(g);
          ++n;
        }
  // PVT v2's four stages at batch 256 and the walks they get
  const int st[4][4] = {{1, 3136, 25, 2}, {2, 784, 13, 1}, {5, 196, 4, 1}, {8, 49, 1, 1}};
  for (const auto& s : st) {
    g = XattnGeom{256, s[1], 49, s[0]};
    const XattnPlan p = xattn_plan(g);
    std::printf("B 256 H %d Sq %d: tiles %d tpw %d walks %d\n", s[0], s[1], p.tiles, p.tpw, p.walks);
    REQUIRE(p.tpw == s[2] && p.walks == s[3]);
  }
  // the smallest geometry with two tiles in a walk, two slab rows and a short last walk
  g = XattnGeom{64, 129, 49, 4};
  {
    const XattnPlan p = xattn_plan(g);
    std::printf("B 64 H 4 Sq 129: tiles %d tpw %d walks %d ws_floats %lld\n", p.tiles, p.tpw, p.walks,
                (long long)p.ws_floats);
    REQUIRE(p.tiles == 3 && p.tpw == 2 && p.walks == 2 && p.tiles % p.tpw != 0);
  }
  const XattnGeom bad[] = {{1, 16, 65, 1}, {1, 0, 16, 1}, {1, 16, 0, 1}, {0, 16, 16, 1}, {1, 16, 16, 0},
                           {65536, 16, 16, 1}, {1, 16, 16, 65536}, {4096, 3136, 49, 8}, {65535, 1, 64, 512}};
  for (const XattnGeom& b : bad)
    if (!xattn_geom_error(b)) return std::printf("accepted a refused geometry\n"), 1;
  std::printf("xattn_plan_check sweep ok: %ld plans\n", n);
  return 0;
}
