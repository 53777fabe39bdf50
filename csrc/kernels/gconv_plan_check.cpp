// CPU check of gconv_plan.h: sweeps geometries and asserts what conv_group.hip relies on.
//   g++ -std=c++17 -I csrc/kernels csrc/kernels/gconv_plan_check.cpp -o gconv_plan_check && ./gconv_plan_check
#include <cstdio>
#include <cstdlib>

#include "gconv_plan.h"

using namespace mpa;

#define REQUIRE(c)                                                                          \
  do {                                                                                      \
    if (!(c)) {                                                                             \
      std::printf("FAILED %s (line %d): kind %d N %d H %d W %d C %d groups %d s %d\n", #c,  \
                  __LINE__, kind, g.N, g.H, g.W, g.C, g.groups, g.s);                       \
      std::exit(1);                                                                         \
    }                                                                                       \
  } while (0)

// 16 lanes (pixels i = 0 .. 15 of one MFMA) read the 16-B slot `slot(i)` each: all different
// mod 16, so the 16 reads of a ds_read_b128 quarter cover the 64 banks once
template <typename F>
static bool conflict_free(F slot) {
  unsigned seen = 0;
  for (int i = 0; i < 16; ++i) seen |= 1u << (slot(i) & 15);
  return seen == 0xffffu;
}

static void check(int kind, const GcGeom& g) {
  REQUIRE(gconv_geom_error(g) == nullptr);
  const GcPlan p = gconv_plan(kind, g);
  const int P = gc_out(g.H, g.s), Q = gc_out(g.W, g.s);
  const bool dg = kind == GC_DGRAD;
  // tiles: even origins and whole row pairs, full cover
  REQUIRE(p.th % 2 == 0 && p.tw == (p.gather ? 32 : 16));
  REQUIRE(p.tiles_h * p.th >= p.OH && (p.tiles_h - 1) * p.th < p.OH);
  REQUIRE(p.tiles_w * p.tw >= p.OW && (p.tiles_w - 1) * p.tw < p.OW);
  REQUIRE(p.OH == (dg ? g.H : P) && p.OW == (dg ? g.W : Q) && p.SH == (dg ? P : g.H) &&
          p.SW == (dg ? Q : g.W));
  REQUIRE(p.gather == (dg && g.s == 2) && p.split == (!dg && g.s == 2));
  // slabs: 16 channels, four per block, groups never straddle a block
  REQUIRE(p.slabs * GC_SLAB == g.C && p.chunks * GC_SPB >= p.slabs && (p.chunks - 1) * GC_SPB < p.slabs);
  REQUIRE(p.Cg * g.groups == g.C && (GC_SPB * GC_SLAB) % p.Cg == 0);
  // the staged tile holds every source pixel a tile's taps read, at a position inside it;
  // positions of the split layout are a permutation of the columns
  const int se = dg ? 1 : g.s;
  if (p.gather) {
    REQUIRE(p.sh_t == (p.th - 1 + 1) / 2 + 1 && p.sw_t == (p.tw - 1 + 1) / 2 + 1);
  } else {
    REQUIRE(p.sh_t == (p.th - 1) * se + 3 && p.sw_t == (p.tw - 1) * se + 3);
    unsigned long long seen = 0;
    for (int x = 0; x < p.sw_t; ++x) {
      const int pos = gc_pos(x, p.split, p.hc);
      REQUIRE(pos >= 0 && pos < p.sw_t && !((seen >> pos) & 1));
      seen |= 1ull << pos;
    }
  }
  // bank mapping: every tap's 16 pixels, at every channel vector, in 16 different slots mod 16
  for (int cv = 0; cv < 8; ++cv)
    for (int r = 0; r < (p.gather ? 2 : 3); ++r)
      for (int t = 0; t < (p.gather ? 2 : 3); ++t)
        for (int row = 0; row < (p.gather ? p.th / 2 : p.th); ++row) {
          auto slot = [&](int i) {
            const int col = p.gather ? i + t : gc_pos(i * se + t, p.split, p.hc);
            const int y = p.gather ? row + r : row * se + r;
            return (y * p.sw_t + col) * GC_PIX_SLOTS + cv;
          };
          REQUIRE(conflict_free(slot));
          REQUIRE(slot(15) < p.sh_t * p.sw_t * GC_PIX_SLOTS);
        }
  // LDS: two blocks per CU, room for the staged tiles and for the statistics reduction
  int need = p.sh_t * p.sw_t * GC_PIX_SLOTS * 16;
  if (kind == GC_WGRAD) {
    REQUIRE(p.dy_off * 16 == need);
    need += p.th * p.tw * GC_PIX_SLOTS * 16;
  }
  REQUIRE(p.lds_bytes >= need && p.lds_bytes <= GC_LDS_BUDGET && 2 * p.lds_bytes <= 160 * 1024);
  if (kind == GC_FWD) REQUIRE(p.lds_bytes >= GC_THREADS * 16 * 4);
  // grid and slab rows
  REQUIRE(p.imgs >= 1 && p.slices * p.imgs >= g.N && (p.slices - 1) * p.imgs < g.N);
  REQUIRE(kind == GC_WGRAD || (p.imgs == 1 && p.slices == g.N));
  REQUIRE(p.rows == p.slices * p.tiles_h * p.tiles_w && p.grid == (int64_t)p.rows * p.chunks);
  REQUIRE(p.grid > 0 && p.grid < ((int64_t)1 << 31));
  REQUIRE((int64_t)p.rows * gc_wrow(g) < ((int64_t)1 << 40));
  const int chunk = gc_fold_chunk(p.rows);
  REQUIRE((p.rows + chunk - 1) / chunk <= 64);
}

int main() {
  long n = 0;
  static const int sizes[] = {1, 2, 7, 8, 9, 14, 15, 16, 17, 28, 33, 56, 64};
  static const int chans[] = {16, 32, 48, 64, 128, 256, 512, 1024, 2048};
  static const int cgs[] = {4, 8, 16, 32};
  static const int batch[] = {1, 2, 5, 64, 256};
  for (int kind = 0; kind < 3; ++kind)
    for (int s = 1; s <= 2; ++s)
      for (int H : sizes)
        for (int W : sizes)
          for (int C : chans)
            for (int cg : cgs)
              for (int N : batch) {
                if (C % cg) continue;
                const GcGeom g{N, H, W, C, C, C / cg, 3, s};
                if (gconv_geom_error(g)) continue;
                check(kind, g);
                ++n;
              }
  // the 7 x 7 x 1024 tail still fills 256 CUs twice over at the training batch
  for (int kind = 0; kind < 3; ++kind) {
    const GcGeom a{256, 7, 7, 1024, 1024, 32, 3, 1}, b{256, 14, 14, 1024, 1024, 32, 3, 2};
    if (gconv_plan(kind, a).grid < 512 || gconv_plan(kind, b).grid < 512)
      return std::printf("grid\n"), 1;
  }
  const GcGeom bad[] = {{1, 8, 8, 8, 8, 4, 3, 1},     {1, 8, 8, 32, 32, 8, 5, 1},
                        {1, 8, 8, 32, 64, 8, 3, 1},   {1, 8, 8, 32, 32, 8, 3, 3},
                        {1, 8, 8, 64, 64, 1, 3, 1},   {1, 8, 8, 24, 24, 3, 3, 1},
                        {1, 8, 8, 32, 32, 32, 3, 1},  {1, 8, 8, 0, 0, 1, 3, 1}};
  for (const GcGeom& g : bad)
    if (!gconv_geom_error(g)) return std::printf("accepted a refused geometry\n"), 1;
  std::printf("gconv_plan_check sweep ok: %ld plans\n", n);
  return 0;
}
