// Launch planning of the channels-last LayerNorm / GELU / layer-scale kernels (ln.hip).
// Host-only arithmetic with no HIP types, so a CPU program (ln_plan_check.cpp) can include it
// and sweep its invariants.
//
// Row kernels (ln_fwd, ln_bwd): a row of C channels lives in the registers of L adjacent
// lanes (L a power of two <= 64); a lane holds V 16-B vectors (8 channels each) at a lane
// stride of L, vector l + v L of the row.  A block of LN_THREADS threads covers
// rpt = LN_THREADS / L adjacent rows per trip and walks a contiguous slab of `trips` trips.
// ln_bwd keeps per-lane fp32 sums of its 8 V channels over the slab, folds the block's rpt
// row slots through LDS in slot order and writes one slab row.
//
// Column kernels (gelu_bwd, scale_add_bwd): thread (vector, slot) owns one 16-B vector of a
// chunk of cvb channel vectors and walks its slab's rows slot, slot + nslots, ...; the slots
// are folded the same way.
//
// Slab rows are summed by a second launch in row order (folded to at most LN_MAX_HEADS heads
// first): no float atomics, bitwise repeatable.
#pragma once
#include <stdint.h>

namespace mpa {

constexpr int LN_THREADS = 256;
constexpr int LN_MAX_V = 4;            // 16-B vectors of a row per lane
constexpr int LN_MAX_C = 64 * LN_MAX_V * 8;  // 2048: a wave holds one row
constexpr int LN_FILL_BLOCKS = 1024;   // four 4-wave blocks per CU before slabs grow
constexpr int LN_MIN_TRIPS = 2;        // a block's operand loads and fold serve two trips at least
constexpr int LN_MAX_HEADS = 64;       // slab rows are folded to at most this many
constexpr int LN_COL_CVB = 64;         // column kernels: channel vectors per block (1 KiB rows)

struct LnGeom {
  int M, C;  // rows (N H W), channels
};

struct LnPlan {
  int L, V;          // lanes per row, vectors per lane
  int rpt;           // rows per block trip (LN_THREADS / L)
  int trips, slab;   // trips per block, rows per block (trips * rpt)
  int rows;          // slab rows a reducing launch writes (= blocks)
  int64_t grid;
};

struct ColPlan {
  int cvb, chunks;   // channel vectors per block, blocks along C
  int nslots;        // row slots per block (LN_THREADS / cvb)
  int trips, slab;   // rows per block = trips * nslots
  int rows;          // slab rows, each [C]
  int64_t grid;      // rows * chunks
};

// element-wise and column kernels: any C % 8 == 0
inline const char* ln_col_error(const LnGeom& g) {
  if (g.M < 1 || g.C < 8) return "empty tensor";
  if (g.C % 8) return "channels must be a multiple of 8";
  if ((int64_t)g.M * g.C >= (int64_t)1 << 31) return "tensor too large (2^31 elements)";
  return nullptr;
}

inline const char* ln_geom_error(const LnGeom& g) {
  if (const char* e = ln_col_error(g)) return e;
  if (g.C > LN_MAX_C) return "channels above 2048";
  return nullptr;
}

// trips per block: whole slabs of LN_MIN_TRIPS trips, more once the grid passes LN_FILL_BLOCKS
inline int ln_trips(int M, int per_trip, int chunks) {
  const int64_t b1 = ((int64_t)M + per_trip - 1) / per_trip;
  int64_t t = b1 * chunks / LN_FILL_BLOCKS;
  const int64_t least = b1 < LN_MIN_TRIPS ? b1 : LN_MIN_TRIPS;
  if (t < least) t = least;
  return (int)t;
}

// The smallest power of two L with L * LN_MAX_V vectors >= C / 8, then V = ceil(C / 8 / L):
// 96, 192, 384, 768 channels are L = 4, 8, 16, 32 at V = 3 with no idle lane; 2048 is a whole
// wave at V = 4; other widths mask their tail vectors (40 channels: L = 2, V = 3, one masked).
inline LnPlan ln_plan(const LnGeom& g) {
  LnPlan p{};
  const int cv = g.C / 8;
  p.L = 1;
  while (p.L * LN_MAX_V < cv) p.L *= 2;
  p.V = (cv + p.L - 1) / p.L;
  p.rpt = LN_THREADS / p.L;
  p.trips = ln_trips(g.M, p.rpt, 1);
  p.slab = p.trips * p.rpt;
  p.rows = (g.M + p.slab - 1) / p.slab;
  p.grid = p.rows;
  return p;
}

inline ColPlan ln_col_plan(const LnGeom& g) {
  ColPlan p{};
  const int cv = g.C / 8;
  p.chunks = (cv + LN_COL_CVB - 1) / LN_COL_CVB;
  p.cvb = (cv + p.chunks - 1) / p.chunks;
  p.nslots = LN_THREADS / p.cvb;
  p.trips = ln_trips(g.M, p.nslots, p.chunks);
  p.slab = p.trips * p.nslots;
  p.rows = (g.M + p.slab - 1) / p.slab;
  p.grid = (int64_t)p.rows * p.chunks;
  return p;
}

// slab rows are folded in chunks of ln_fold_chunk(rows) into each chunk's first row, then the
// heads are summed in row order
inline int ln_fold_chunk(int rows) {
  return rows > LN_MAX_HEADS ? (rows + LN_MAX_HEADS - 1) / LN_MAX_HEADS : 1;
}

// floats of the slab of ln_bwd ([rows][2 C], [3 C] with dpre_bias) and of a column kernel
inline int64_t ln_bwd_ws_floats(const LnGeom& g, bool dpre) {
  return (int64_t)ln_plan(g).rows * (dpre ? 3 : 2) * g.C;
}
inline int64_t ln_col_ws_floats(const LnGeom& g) { return (int64_t)ln_col_plan(g).rows * g.C; }

}  // namespace mpa
