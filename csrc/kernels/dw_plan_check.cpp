// CPU check of dw_plan.h: sweeps geometries and asserts what conv_dw.hip relies on.
//   g++ -std=c++17 -I csrc/kernels csrc/kernels/dw_plan_check.cpp -o dw_plan_check && ./dw_plan_check
#include <cstdio>
#include <cstdlib>

#include "dw_plan.h"

using namespace mpa;

#define REQUIRE(c)                                                                        \
  do {                                                                                    \
    if (!(c)) {                                                                           \
      std::printf("FAILED %s (line %d): kind %d N %d H %d W %d C %d k %d s %d\n", #c,     \
                  __LINE__, kind, g.N, g.H, g.W, g.C, g.k, g.s);                          \
      std::exit(1);                                                                       \
    }                                                                                     \
  } while (0)

static void check(int kind, const DwGeom& g) {
  REQUIRE(dw_geom_error(g) == nullptr);
  const DwPlan p = dw_plan(kind, g);
  const int P = dw_out(g.H, g.k, g.s), Q = dw_out(g.W, g.k, g.s);
  // tiles: even origins (the stride-2 gather), whole strips, full cover, 7 x 7 in one tile
  REQUIRE(p.th % 2 == 0 && p.tw % DW_STRIP == 0 && p.tw % 2 == 0);
  REQUIRE(p.tiles_h * p.th >= p.OH && (p.tiles_h - 1) * p.th < p.OH);
  REQUIRE(p.tiles_w * p.tw >= p.OW && (p.tiles_w - 1) * p.tw < p.OW);
  REQUIRE(p.OH == (kind == DW_DGRAD ? g.H : P) && p.SW == (kind == DW_DGRAD ? Q : g.W));
  if (p.OH <= 8 && p.OW <= 8) REQUIRE(p.th == 8 && p.tw == 8 && p.tiles_h * p.tiles_w == 1);
  // channel chunks cover C; every thread group is whole
  REQUIRE(p.cvb >= 1 && p.cvb <= DW_MAX_CVB && p.cvb * p.chunks >= g.C / 8 &&
          p.cvb * (p.chunks - 1) < g.C / 8);
  REQUIRE(DW_THREADS / p.cvb >= 1 && DW_THREADS / (p.cvb * g.k) >= 1);
  // the staged tile holds every source pixel a tile's taps read
  if (kind == DW_DGRAD && g.s == 2) {
    REQUIRE(p.sh_t >= (p.th - 1 + g.k / 2) / 2 + 2 && p.sw_t >= p.tw / 2 + 2);
  } else {
    const int se = kind == DW_DGRAD ? 1 : g.s;
    REQUIRE(p.sh_t >= (p.th - 1) * se + g.k && p.sw_t >= (p.tw - 1) * se + g.k);
  }
  REQUIRE(p.pitch >= p.sw_t * p.cvb && p.pitch < p.sw_t * p.cvb + 16);
  // LDS: inside the default dynamic limit, and large enough for the block reductions
  REQUIRE(p.lds_bytes <= 64 * 1024);
  REQUIRE(p.lds_bytes >= DW_THREADS * (kind == DW_WGRAD ? g.k * 8 : 16) * 4);
  REQUIRE(p.lds_bytes >= p.sh_t * p.pitch * 16 +
                             (kind == DW_WGRAD ? p.th * p.tw * p.cvb * 16 : g.k * g.k * p.cvb * 16));
  // grid and slab rows
  REQUIRE(p.imgs >= 1 && p.slices * p.imgs >= g.N && (p.slices - 1) * p.imgs < g.N);
  REQUIRE(kind == DW_WGRAD || (p.imgs == 1 && p.slices == g.N));
  REQUIRE(p.rows == p.slices * p.tiles_h * p.tiles_w && p.grid == (int64_t)p.rows * p.chunks);
  REQUIRE(p.grid > 0 && p.grid < ((int64_t)1 << 31));
  const int chunk = dw_fold_chunk(p.rows);
  REQUIRE((p.rows + chunk - 1) / chunk <= 64);
}

int main() {
  long n = 0;
  static const int sizes[] = {1, 2, 7, 8, 9, 14, 15, 16, 17, 28, 33, 56, 112};
  static const int chans[] = {8, 24, 32, 48, 72, 120, 144, 240, 480, 576, 1152, 4096};
  static const int batch[] = {1, 2, 5, 64, 256};
  for (int kind = 0; kind < 3; ++kind)
    for (int k = 3; k <= 7; k += 2)
      for (int s = 1; s <= 2; ++s)
        for (int H : sizes)
          for (int W : sizes)
            for (int C : chans)
              for (int N : batch) {
                const DwGeom g{N, H, W, C, k, s};
                if (dw_geom_error(g)) continue;
                check(kind, g);
                ++n;
              }
  // small layers still fill 256 CUs at the training batch
  for (int kind = 0; kind < 3; ++kind) {
    const DwGeom a{256, 7, 7, 1152, 3, 1}, b{256, 14, 14, 576, 5, 1};
    if (dw_plan(kind, a).grid < 512 || dw_plan(kind, b).grid < 512) return std::printf("grid\n"), 1;
  }
  // ConvNeXt's 7 x 7 layers at the training batch: forward and dgrad keep the 16 x 16 tile
  for (int kind = 0; kind < 2; ++kind) {
    const DwGeom a{256, 56, 56, 96, 7, 1}, b{256, 28, 28, 192, 7, 1};
    check(kind, a);
    check(kind, b);
    if (dw_plan(kind, a).th != 16 || dw_plan(kind, b).th != 16 || dw_plan(kind, b).cvb != 6)
      return std::printf("7x7 tile\n"), 1;
  }
  const DwGeom bad[] = {{1, 8, 8, 12, 3, 1}, {1, 8, 8, 8, 9, 1}, {1, 8, 8, 8, 7, 2},
                        {1, 8, 8, 8, 3, 3}, {1, 8, 8, 0, 3, 1}};
  for (const DwGeom& g : bad)
    if (!dw_geom_error(g)) return std::printf("accepted a refused geometry\n"), 1;
  std::printf("dw_plan_check sweep ok: %ld plans\n", n);
  return 0;
}
