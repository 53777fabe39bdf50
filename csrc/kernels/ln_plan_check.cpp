// CPU check of ln_plan.h: sweeps geometries and asserts what ln.hip relies on.
//   g++ -std=c++17 -I csrc/kernels csrc/kernels/ln_plan_check.cpp -o ln_plan_check && ./ln_plan_check
#include <cstdio>
#include <cstdlib>

#include "ln_plan.h"

using namespace mpa;

#define REQUIRE(c)                                                                 \
  do {                                                                             \
    if (!(c)) {                                                                    \
      std::printf("FAILED %s (line %d): M %d C %d\n", #c, __LINE__, g.M, g.C);     \
      std::exit(1);                                                                \
    }                                                                              \
  } while (0)

static void check_rows(const LnGeom& g) {
  REQUIRE(ln_geom_error(g) == nullptr);
  const LnPlan p = ln_plan(g);
  const int cv = g.C / 8;
  // L a power of two inside a wave, the row's vectors covered, no lane group wholly idle
  REQUIRE(p.L >= 1 && p.L <= 64 && (p.L & (p.L - 1)) == 0);
  REQUIRE(p.V >= 1 && p.V <= LN_MAX_V && p.L * p.V >= cv && p.L * (p.V - 1) < cv);
  REQUIRE(p.L == 1 || (p.L / 2) * LN_MAX_V < cv);
  REQUIRE(p.rpt * p.L == LN_THREADS);
  // slabs: whole trips, full cover, no empty block
  REQUIRE(p.trips >= 1 && p.slab == p.trips * p.rpt);
  REQUIRE((int64_t)p.rows * p.slab >= g.M && (int64_t)(p.rows - 1) * p.slab < g.M);
  REQUIRE(p.grid == p.rows && p.grid > 0);
  REQUIRE(p.trips >= LN_MIN_TRIPS || (int64_t)p.trips * p.rpt >= g.M);
  // LDS of the backward's fold, and the slab
  REQUIRE(8 * p.V * LN_THREADS * 4 <= 64 * 1024);
  REQUIRE(ln_bwd_ws_floats(g, true) == (int64_t)p.rows * 3 * g.C);
  const int chunk = ln_fold_chunk(p.rows);
  REQUIRE((p.rows + chunk - 1) / chunk <= LN_MAX_HEADS);
}

static void check_cols(const LnGeom& g) {
  REQUIRE(ln_col_error(g) == nullptr);
  const ColPlan p = ln_col_plan(g);
  const int cv = g.C / 8;
  REQUIRE(p.cvb >= 1 && p.cvb <= LN_COL_CVB && p.cvb * p.chunks >= cv && p.cvb * (p.chunks - 1) < cv);
  REQUIRE(p.nslots >= 1 && p.nslots * p.cvb <= LN_THREADS && p.cvb * 8 <= 8 * LN_THREADS);
  REQUIRE(p.trips >= 1 && p.slab == p.trips * p.nslots);
  REQUIRE((int64_t)p.rows * p.slab >= g.M && (int64_t)(p.rows - 1) * p.slab < g.M);
  REQUIRE(p.grid == (int64_t)p.rows * p.chunks && p.grid < ((int64_t)1 << 31));
  const int chunk = ln_fold_chunk(p.rows);
  REQUIRE((p.rows + chunk - 1) / chunk <= LN_MAX_HEADS);
}

int main() {
  long n = 0;
  static const int rows[] = {1, 2, 5, 37, 63, 64, 65, 98, 300, 1003, 4099, 12544, 20011,
                             50176, 200704, 802816};
  for (int C = 8; C <= 4096; C += 8)
    for (int M : rows) {
      const LnGeom g{M, C};
      if (ln_col_error(g)) continue;
      check_cols(g);
      ++n;
      if (ln_geom_error(g)) continue;
      check_rows(g);
      ++n;
    }
  // ConvNeXt's widths: no idle lane at three vectors per lane
  static const int dims[][2] = {{96, 4}, {192, 8}, {384, 16}, {768, 32}};
  for (auto& d : dims) {
    const LnPlan p = ln_plan(LnGeom{802816, d[0]});
    if (p.L != d[1] || p.V != 3 || p.grid < LN_FILL_BLOCKS) return std::printf("convnext plan\n"), 1;
  }
  if (ln_plan(LnGeom{20011, 96}).trips < 2 || ln_plan(LnGeom{20011, 96}).rows < 2)
    return std::printf("slab plan\n"), 1;
  const LnGeom bad[] = {{1, 12}, {1, 2056}, {0, 96}, {5, 0}, {1 << 24, 256}};
  for (const LnGeom& g : bad)
    if (!ln_geom_error(g)) return std::printf("accepted a refused geometry\n"), 1;
  std::printf("ln_plan_check sweep ok: %ld plans\n", n);
  return 0;
}
