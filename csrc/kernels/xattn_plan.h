// Launch planning of the short-key cross-attention kernels (xattn.hip).  Host-only arithmetic
// with no HIP types, so a CPU program (xattn_plan_check.cpp) can include it and sweep its
// invariants.
//
// q [B][Sq][H][64] and kv [B][Sk][2][H][64] bf16 (k rows, then v rows), 1 <= Sk <= 64: all keys
// and values of one (batch, head) fit in ONE 64-row LDS tile of attn_plan.h's layout, so a block
// stages them once and walks `tpw` consecutive 64-row query tiles, wave w owning rows 16 w ..
// 16 w + 15 of each.  No key streaming, no online rescale, no ring.
//
// Forward: grid (walks, H, B).  Backward: the same grid; a block keeps dK^T and dV^T of its walk
// in registers and writes them as one fp32 slab row [2][64 keys][64]; a second launch sums the
// `walks` rows of a (batch, head) in row order.
//
// LDS tiles (AT_TILE_BYTES = 9216 each, 64 rows of AT_PITCH bf16):
//   forward   K rows | V^T (at_pos order) | o patches (4 waves x 16 rows)
//   backward  K rows | V rows | K^T (at_pos order) | Q^T | dO^T | P^T | dS^T
//             Q^T / dO^T are [d][query of the tile], P^T / dS^T are [key][query of the tile],
//             rewritten for every tile; wave w's dQ patch lies in rows 16 w .. 16 w + 15 of P^T,
//             which only wave w reads (it owns those keys of dK / dV).
#pragma once
#include <stdint.h>

#include "attn_plan.h"

namespace mpa {

constexpr int XA_MAX_KEYS = AT_TILE;  // keys of a (batch, head): one LDS tile
constexpr int XA_LDS_FWD = 3 * AT_TILE_BYTES;
constexpr int XA_LDS_BWD = 7 * AT_TILE_BYTES;
constexpr int XA_SLAB_ROW = 2 * AT_TILE * AT_D;  // floats of a slab row: dK, dV [64 keys][64]
// Blocks of a grid before the walks lengthen: two 4-wave blocks per CU, what the backward's
// LDS lets a CU hold.  Not measured against other values (docs/NOTES.md holds the timings of
// this one).
constexpr int XA_FILL_BLOCKS = 512;
constexpr int XA_MAX_ROWS = 64;  // slab rows of a (batch, head) are capped here

struct XattnGeom {
  int B, Sq, Sk, H;
};

struct XattnPlan {
  int tiles;    // ceil(Sq / 64): query tiles of a (batch, head)
  int tpw;      // tiles a block walks
  int walks;    // ceil(tiles / tpw): grid.x, and the slab rows of a (batch, head)
  int lds_fwd, lds_bwd;  // static LDS bytes per block
  int64_t ws_floats;     // slab floats: walks * B * H * XA_SLAB_ROW
};

inline const char* xattn_geom_error(const XattnGeom& g) {
  if (g.B < 1 || g.H < 1 || g.Sq < 1 || g.Sk < 1) return "empty batch, sequence or no heads";
  if (g.Sk > XA_MAX_KEYS) return "at most 64 keys (Sk <= 64): larger key sets are not served";
  if (g.B > 65535 || g.H > 65535) return "batch or heads above 65535";
  if ((int64_t)g.B * g.Sq * g.H * AT_D >= (int64_t)1 << 31 ||
      (int64_t)g.B * g.Sk * 2 * g.H * AT_D >= (int64_t)1 << 31)
    return "tensor too large (2^31 elements)";
  return nullptr;
}

inline XattnPlan xattn_plan(const XattnGeom& g) {
  XattnPlan p{};
  p.tiles = (g.Sq + AT_TILE - 1) / AT_TILE;
  // fill the CUs first (one tile per block while the grid is below XA_FILL_BLOCKS), then
  // lengthen the walks; never more than XA_MAX_ROWS slab rows per (batch, head)
  int64_t rows = XA_FILL_BLOCKS / ((int64_t)g.B * g.H);
  if (rows < 1) rows = 1;
  if (rows > XA_MAX_ROWS) rows = XA_MAX_ROWS;
  p.tpw = (int)((p.tiles + rows - 1) / rows);
  p.walks = (p.tiles + p.tpw - 1) / p.tpw;
  p.lds_fwd = XA_LDS_FWD;
  p.lds_bwd = XA_LDS_BWD;
  p.ws_floats = (int64_t)p.walks * g.B * g.H * XA_SLAB_ROW;
  return p;
}

}  // namespace mpa
