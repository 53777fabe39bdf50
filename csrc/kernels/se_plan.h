// Launch planning of the squeeze-excite / activation-gate kernels (se.hip).  Host-only
// arithmetic with no HIP types, so a CPU program (se_plan_check.cpp) can include it and sweep
// its invariants.
//
// Streaming kernels (act_pool, act_gate_fwd, act_gate_bwd_pool / _sums / _dx): a block owns
// one image's pixel slab [p0, p1) x `cvb` channel vectors (8 channels, 16 B each).  Thread
// (vector, slot) keeps its channels' per-(image, channel) operands in registers and walks the
// slab's pixels slot, slot + nslots, ...  A reducing kernel sums its slots through LDS in slot
// order and writes one partial row per (image, slab).
//
// Gate kernels (se_gate, se_gate_bwd): one block per image, the image's [C] and [Cs] vectors
// in LDS.
#pragma once
#include <stdint.h>

namespace mpa {

constexpr int SE_THREADS = 256;
constexpr int SE_MAX_CVB = 128;      // channel vectors per block: two pixel slots at least
constexpr int SE_FILL_BLOCKS = 2048;  // eight 4-wave blocks per CU: two waves per SIMD
constexpr int SE_MIN_PIX = 4;        // pixels per slot below which a slab is not split further
constexpr int SE_MAX_WIDTH = 2048;   // gate kernels: C and Cs (one thread per channel vector)
constexpr int SE_MAX_HEADS = 64;     // column sums: rows are folded to at most this many

struct SeGeom {
  int N, HW, C;  // images, pixels per image, channels
};

struct SePlan {
  int cvb, chunks;   // channel vectors per block, blocks along C
  int nslots;        // pixel slots per block (SE_THREADS / cvb)
  int pps, slabs;    // pixels per slab, slabs per image
  int rows;          // partial rows a reducing launch writes: N * slabs, each [C] (or [2 C])
  int64_t grid;      // rows * chunks
};

inline const char* se_geom_error(const SeGeom& g) {
  if (g.N < 1 || g.HW < 1 || g.C < 8) return "empty tensor";
  if (g.C % 8) return "channels must be a multiple of 8";
  if ((int64_t)g.N * g.HW * g.C >= (int64_t)1 << 31) return "tensor too large (2^31 elements)";
  return nullptr;
}

inline const char* se_gate_error(int N, int C, int Cs) {
  if (N < 1 || C < 8 || Cs < 8) return "empty tensor";
  if (C % 8 || Cs % 8) return "channels and squeeze width must be multiples of 8";
  if (C > SE_MAX_WIDTH || Cs > SE_MAX_WIDTH) return "channels or squeeze width above 2048";
  return nullptr;
}

// Slabs per image: enough blocks to hold two waves on every SIMD (a streaming kernel hides
// its load latency with waves in flight), but no slab so short that a slot walks fewer than
// SE_MIN_PIX pixels - the per-thread operand loads and the block reduction are per slab.
// 7 x 7 x 960 at batch 256 (120 vectors, 2 slots): 7 slabs of 7 pixels, 1,792 blocks;
// 28 x 28 x 72 (9 vectors, 28 slots): 7 slabs of 112 pixels, 1,792 blocks.
inline SePlan se_plan(const SeGeom& g) {
  SePlan p{};
  const int cv = g.C / 8;
  p.chunks = (cv + SE_MAX_CVB - 1) / SE_MAX_CVB;
  p.cvb = (cv + p.chunks - 1) / p.chunks;
  p.nslots = SE_THREADS / p.cvb;
  const int64_t per = (int64_t)g.N * p.chunks;
  int64_t want = (SE_FILL_BLOCKS + per - 1) / per;
  const int64_t most = (g.HW + p.nslots * SE_MIN_PIX - 1) / (p.nslots * SE_MIN_PIX);
  if (want > most) want = most;
  if (want < 1) want = 1;
  p.pps = (int)((g.HW + want - 1) / want);
  p.slabs = (g.HW + p.pps - 1) / p.pps;
  p.rows = g.N * p.slabs;
  p.grid = (int64_t)p.rows * p.chunks;
  return p;
}

// floats of the partial rows of a reducing launch; width = C (pools) or 2 C (BN sums)
inline int64_t se_ws_floats(const SeGeom& g, int width) {
  return (int64_t)se_plan(g).rows * width;
}

// column sums over all rows (BN sums): rows are folded in chunks of se_fold_chunk(rows) into
// each chunk's first row, then the heads are summed in row order
inline int se_fold_chunk(int rows) {
  return rows > SE_MAX_HEADS ? (rows + SE_MAX_HEADS - 1) / SE_MAX_HEADS : 1;
}

// dynamic LDS of the gate kernels: the image's [C] and [Cs] fp32 vectors, and (backward) the
// slot reduction's 8 floats per thread
inline int se_gate_lds_bytes(int C, int Cs, bool bwd) {
  return (C + Cs) * 4 + (bwd ? SE_THREADS * 8 * 4 : 0);
}

// lanes that share one output row of a gate matrix-vector product: the power of two that
// covers the row's vec 16-B words, at most a wave
inline int se_row_lanes(int vec) {
  int g = 1;
  while (g < vec && g < 64) g *= 2;
  return g;
}

}  // namespace mpa
