// Launch planning and address arithmetic of the neighbourhood attention kernels (nattn.hip).
// Host-only arithmetic with no HIP types, so a CPU program (nattn_plan_check.cpp) can include
// it and sweep its invariants; the neighbourhood start, the key range of queries, the query
// range of keys and the bias index are AT_HD functions the kernels call.
//
// qkv [B Hf Wf][3][H][32] bf16 holds the in-projection's rows in natural token order.  Query
// (yi, xi) attends the 7 x 7 keys whose rows start at nattn_ni(yi, Hf) and columns at
// nattn_ni(xi, Wf): the start is clamped, not zero-padded, so every query has 49 keys.
//
// The map is cut into 8 x 8 tiles; a block of 4 waves owns one tile of one head.
//   nattn_fwd, nattn_dq   wave w owns query rows 2 w, 2 w + 1 of the tile (16 queries).  Its keys
//       are the rows nattn_ni(y) .. + 7 (8 sub-tiles, one key row each) by the 16 column slots
//       from nattn_ni(x0): at most 8 x 14 of them exist, the rest read as zero and are masked.
//   nattn_dkv             wave w owns the 4 x 4 key patch (w / 2, w % 2) of the tile.  Its queries
//       are the rows nattn_qlo(Y0) .. nattn_qhi(Y0 + 3) (at most 13, walked in pairs) by the 16
//       column slots from nattn_qlo(X0) (at most 13 used).  The attending set is not the mirror
//       of the key halo: clamping makes border keys popular, and a 2 x 8 patch would need up to
//       17 column slots (L = 22), which is why the patch is square.
// A sub-tile is ONE map row of 16 column slots, so slot -> coordinate is an add.
//
// nattn_dq walks `bpw` batch images of one tile position (the slot -> relative index map is the
// same for all of them), keeps the fp32 dS in registers, folds it to 169 bins through LDS and
// writes slab row (walk, tile); a second launch sums the rows in row order.
//
// Wave-private LDS (bytes): two stages of a transposed operand pair [32][NA_PITCH] bf16 and
// a [16][NA_PPITCH] output patch; the backward adds lse / delta of a query row pair.  The block
// shares the head's 169 bias floats and, in nattn_dq, the fold tile [64][NA_FOLD_PITCH] fp32
// (which overlays the wave regions after the walk).
//
// NA_FILL_BLOCKS, NA_MAX_WALKS and NA_HPB (heads per block) are first guesses: none of them
// was tuned by measurement.
#pragma once
#include <stdint.h>

#include "attn_plan.h"

namespace mpa {

constexpr int NA_D = 32;          // head dim
constexpr int NA_K = 7;           // neighbourhood edge
constexpr int NA_RPB = 13;        // 2 * NA_K - 1: edge of a head's bias table
constexpr int NA_NB = 169;        // floats of a head's bias table
constexpr int NA_TILE = 8;        // tile edge (queries in fwd / dq, keys in dkv)
constexpr int NA_SLOTS = 16;      // column slots of a sub-tile
constexpr int NA_SUB = 8;         // key-row sub-tiles of a query wave
constexpr int NA_QROWS = 14;      // query-row sub-tiles a key wave walks at most (7 pairs)
constexpr int NA_PITCH = 40;      // bf16 per row of a transposed pair tile [32][32]
constexpr int NA_PPITCH = 40;     // bf16 per row of an output patch [16][32]
constexpr int NA_FOLD_PITCH = 129;  // floats per query of the fold tile [64][128]
constexpr int NA_HPB = 1;         // heads per block (unmeasured)
constexpr int NA_FILL_BLOCKS = 512;  // dq blocks wanted before the walks lengthen (unmeasured)
constexpr int NA_MAX_WALKS = 16;     // walks per tile position: slab rows = tiles * walks (unmeasured)
constexpr int NA_PAIR_BYTES = NA_D * NA_PITCH * 2;    // 2560: one transposed [32][32] pair tile
constexpr int NA_PATCH_BYTES = 16 * NA_PPITCH * 2;    // 1280
constexpr int NA_FWD_WAVE = 2 * NA_PAIR_BYTES + NA_PATCH_BYTES;                      // Vt x 2 | o
constexpr int NA_DQ_WAVE = 2 * NA_PAIR_BYTES + NA_PATCH_BYTES;                       // Kt x 2 | dq
constexpr int NA_DKV_WAVE = 4 * NA_PAIR_BYTES + 2 * NA_PATCH_BYTES + 2 * 2 * 32 * 4;  // (Qt, dOt) x 2 | dk, dv | (lse, delta) x 2
constexpr int NA_FOLD_BYTES = 64 * NA_FOLD_PITCH * 4;  // 33024
constexpr int NA_FWD_BYTES = 4 * NA_FWD_WAVE + NA_NB * 4;
constexpr int NA_DQ_BYTES = (4 * NA_DQ_WAVE > NA_FOLD_BYTES ? 4 * NA_DQ_WAVE : NA_FOLD_BYTES) + NA_NB * 4;
constexpr int NA_DKV_BYTES = 4 * NA_DKV_WAVE + NA_NB * 4;

struct NattnGeom {
  int B, H, Hf, Wf;
};

struct NattnPlan {
  int ty, tx, tiles;   // ceil(Hf / 8), ceil(Wf / 8), their product (grid.x)
  int bpw, walks;      // batch images a dq block walks, walks per tile position (dq grid.z)
  int rows;            // slab rows per head: walks * tiles
  int lds_fwd, lds_dq, lds_dkv;  // static LDS bytes per block
  int64_t delta_floats;  // B H Hf Wf: delta, as lse
  int64_t ws_floats;     // delta, then the slab rows [rows][H][169]
};

// head_dim is the width of one head in qkv's columns (columns / (3 H))
inline const char* nattn_geom_error(const NattnGeom& g, int head_dim = NA_D) {
  if (head_dim != NA_D) return "head dim must be 32";
  if (g.B < 1 || g.H < 1) return "empty batch or no heads";
  if (g.Hf < NA_K || g.Wf < NA_K) return "the map must be at least 7 x 7";
  if (g.B > 65535 || g.H > 65535) return "batch or heads above 65535";
  if ((int64_t)g.B * g.Hf * g.Wf * 3 * g.H * NA_D >= (int64_t)1 << 31) return "tensor too large (2^31 elements)";
  return nullptr;
}

inline NattnPlan nattn_plan(const NattnGeom& g) {
  NattnPlan p{};
  p.ty = (g.Hf + NA_TILE - 1) / NA_TILE;
  p.tx = (g.Wf + NA_TILE - 1) / NA_TILE;
  p.tiles = p.ty * p.tx;
  // fill the CUs first (one image per block while the grid is below NA_FILL_BLOCKS), then
  // lengthen the walks; never more than NA_MAX_WALKS per tile position
  const int64_t per = (int64_t)p.tiles * g.H;
  int walks = (int)((NA_FILL_BLOCKS + per - 1) / per);
  if (walks > NA_MAX_WALKS) walks = NA_MAX_WALKS;
  if (walks > g.B) walks = g.B;
  p.bpw = (g.B + walks - 1) / walks;
  p.walks = (g.B + p.bpw - 1) / p.bpw;
  p.rows = p.walks * p.tiles;
  p.lds_fwd = NA_FWD_BYTES;
  p.lds_dq = NA_DQ_BYTES;
  p.lds_dkv = NA_DKV_BYTES;
  p.delta_floats = (int64_t)g.B * g.H * g.Hf * g.Wf;
  p.ws_floats = p.delta_floats + (int64_t)p.rows * g.H * NA_NB;
  return p;
}

// first key of the neighbourhood of query i on an axis of length L >= 7; i >= L gives L - 7
AT_HD inline int nattn_ni(int i, int L) {
  const int s = i - NA_K / 2;
  return s < 0 ? 0 : (s > L - NA_K ? L - NA_K : s);
}

// first / last query i (0 .. L - 1) whose neighbourhood holds key k (0 .. L - 1)
AT_HD inline int nattn_qlo(int k, int L) { (void)L; return k < NA_K ? 0 : k - NA_K / 2; }
AT_HD inline int nattn_qhi(int k, int L) { return k >= L - NA_K ? L - 1 : k + NA_K / 2; }

AT_HD inline bool nattn_in(int q, int k, int L) {
  const int s = nattn_ni(q, L);
  return k >= s && k < s + NA_K;
}

// bias index of query (yi, xi) and key (yj, xj) of its neighbourhood
AT_HD inline int nattn_rel(int yi, int xi, int yj, int xj) {
  return (yj - yi + NA_K - 1) * NA_RPB + (xj - xi + NA_K - 1);
}

// column of (sub-tile a of a pair, slot c) in a transposed pair tile: the second product's B
// operand is the first one's accumulator pair, lane group g holding slots 4 g .. 4 g + 3 of both
// sub-tiles side by side
AT_HD inline int nattn_pos(int a, int c) { return 8 * (c >> 2) + 4 * a + (c & 3); }

}  // namespace mpa
