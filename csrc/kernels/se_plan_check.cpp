// CPU check of se_plan.h: sweeps geometries and asserts what se.hip relies on.
//   g++ -std=c++17 -I csrc/kernels csrc/kernels/se_plan_check.cpp -o se_plan_check && ./se_plan_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "se_plan.h"

using namespace mpa;

#define REQUIRE(c)                                                                            \
  do {                                                                                        \
    if (!(c)) {                                                                               \
      std::printf("FAILED %s (line %d): N %d HW %d C %d Cs %d\n", #c, __LINE__, g.N, g.HW, g.C, \
                  Cs);                                                                        \
      std::exit(1);                                                                           \
    }                                                                                         \
  } while (0)

static void check(const SeGeom& g, int Cs) {
  REQUIRE(se_geom_error(g) == nullptr);
  const SePlan p = se_plan(g);
  const int cv = g.C / 8;
  // channel chunks cover C; a block has one pixel slot at least and a thread for every
  // (vector, slot)
  REQUIRE(p.cvb >= 1 && p.cvb <= SE_MAX_CVB && p.cvb * p.chunks >= cv && p.cvb * (p.chunks - 1) < cv);
  REQUIRE(p.nslots >= 1 && p.nslots * p.cvb <= SE_THREADS);
  // slabs cover every pixel exactly once, walked the way the kernel walks them
  REQUIRE(p.slabs >= 1 && p.pps >= 1 && p.slabs * p.pps >= g.HW && (p.slabs - 1) * p.pps < g.HW);
  std::vector<int> seen(g.HW, 0);
  for (int slab = 0; slab < p.slabs; ++slab) {
    const int p0 = slab * p.pps, p1 = g.HW < p0 + p.pps ? g.HW : p0 + p.pps;
    for (int slot = 0; slot < p.nslots; ++slot)
      for (int px = p0 + slot; px < p1; px += p.nslots) {
        REQUIRE(px >= 0 && px < g.HW);
        ++seen[px];
      }
  }
  for (int px = 0; px < g.HW; ++px) REQUIRE(seen[px] == 1);
  // partial rows: the last row the kernels index is inside the workspace
  REQUIRE(p.rows == g.N * p.slabs && p.grid == (int64_t)p.rows * p.chunks);
  REQUIRE(p.grid > 0 && p.grid < ((int64_t)1 << 31));
  for (int width = g.C; width <= 2 * g.C; width += g.C) {
    const int64_t last = ((int64_t)(g.N - 1) * p.slabs + (p.slabs - 1)) * width + width - 1;
    REQUIRE(se_ws_floats(g, width) == last + 1);
  }
  const int chunk = se_fold_chunk(p.rows), heads = (p.rows + chunk - 1) / chunk;
  REQUIRE(chunk >= 1 && heads >= 1 && heads <= SE_MAX_HEADS && (heads - 1) * chunk < p.rows);
  // gate kernels: LDS inside the default dynamic limit, a thread per channel vector, whole
  // lane groups
  if (Cs) {
    REQUIRE(se_gate_error(g.N, g.C, Cs) == nullptr);
    REQUIRE(se_gate_lds_bytes(g.C, Cs, true) <= 64 * 1024);
    REQUIRE(se_gate_lds_bytes(g.C, Cs, true) == (g.C + Cs + SE_THREADS * 8) * 4);
    REQUIRE(se_gate_lds_bytes(g.C, Cs, false) == (g.C + Cs) * 4);
    REQUIRE(g.C / 8 <= SE_THREADS && Cs / 8 <= SE_THREADS);
    for (int vec : {g.C / 8, Cs / 8}) {
      const int G = se_row_lanes(vec);
      REQUIRE(G >= 1 && G <= 64 && (G & (G - 1)) == 0 && (G >= vec || G == 64) && SE_THREADS % G == 0);
    }
  }
}

int main() {
  long n = 0;
  // MobileNetV3-Large at 224 x 224: every (H = W, expanded width, squeeze width or 0)
  static const int v3[][3] = {{112, 16, 0},  {112, 64, 0},  {56, 64, 0},   {56, 72, 0},  {28, 72, 24},
                              {28, 120, 32}, {28, 240, 0},  {14, 240, 0},  {14, 200, 0}, {14, 184, 0},
                              {14, 480, 120}, {14, 672, 168}, {7, 672, 168}, {7, 960, 240}, {1, 1280, 0}};
  for (const auto& l : v3)
    for (int N = 1; N <= 256; ++N) {
      check(SeGeom{N, l[0] * l[0], l[1]}, l[2]);
      ++n;
    }
  // the test shapes, and widths around the chunk and gate limits
  static const int extra[][4] = {{2, 64, 8, 8},      {3, 64, 72, 24},  {2, 1024, 24, 8},  {3, 49, 960, 240},
                                 {3, 784, 72, 24},   {2, 196, 8, 8},   {4, 196, 672, 168}, {4, 196, 120, 32},
                                 {1, 8, 1280, 0},    {1, 256, 1280, 0}, {5, 3, 1024, 1032}, {2, 1, 2048, 2048},
                                 {1, 1, 4096, 0},    {7, 100, 1032, 8}};
  for (const auto& e : extra) {
    check(SeGeom{e[0], e[1], e[2]}, e[3]);
    ++n;
  }
  // both ends of the network fill 256 CUs (four 4-wave blocks each) at the training batch
  if (se_plan(SeGeom{256, 49, 960}).grid < 1024 || se_plan(SeGeom{256, 784, 72}).grid < 1024)
    return std::printf("grid\n"), 1;
  const SeGeom bad[] = {{1, 64, 12}, {0, 64, 8}, {1, 0, 8}, {1, 64, 0}, {1 << 12, 1 << 12, 1 << 8}};
  for (const SeGeom& g : bad)
    if (!se_geom_error(g)) return std::printf("accepted a refused geometry\n"), 1;
  if (!se_gate_error(1, 4096, 8) || !se_gate_error(1, 64, 12) || !se_gate_error(1, 64, 0))
    return std::printf("accepted a refused gate\n"), 1;
  std::printf("se_plan_check sweep ok: %ld plans\n", n);
  return 0;
}
