// Launch planning and address arithmetic of the shifted-window attention kernels (wattn.hip).
// Host-only arithmetic with no HIP types, so a CPU program (wattn_plan_check.cpp) can include
// it and sweep its invariants; the token map, the relative-position index and the shift
// regions are AT_HD functions the kernels call.
//
// qkv [B Hf Wf][3][H][32] bf16 holds the in-projection's rows in natural token order.  The map
// is rolled by `shift` and cut into ws x ws windows only as addresses: token n = (wy, wx) of
// window (b, Y, X) is the row of map pixel ((Y ws + wy + shift) mod Hf, (X ws + wx + shift) mod
// Wf).  A window's ws^2 <= 64 tokens are padded to one 64 x 64 score tile that ONE wave owns
// for one head: no key streaming, no online rescale, no traffic between waves.  A block is
// W in {4, 3, 2, 1} waves, the largest dividing H, on adjacent heads of one window, so a token
// row's q (k, v) of the block is W * 64 contiguous bytes.
//
// Forward: grid (windows, H / W), one window per block.  Backward: grid (walks, H / W); a
// block walks `wpb` consecutive windows (across batch images: the bias gradient depends on
// (i, j) only), keeps its fp32 dS tile in registers over the walk, folds it ws^4 -> (2 ws - 1)^2
// through LDS at the end and writes one slab row [H][(2 ws - 1)^2]; a second launch sums the
// slab rows in row order.
//
// Wave-private LDS (bytes; WA_PITCH = 72 bf16 as in attn_plan.h, 32 rows per transposed tile):
//   forward   Vt 4608 | o patch 16 x 40 bf16 1280 | bias row 1024 | token rows 256 | info 256
//   backward  Kt 4608 | Qt 4608 | dOt 4608 | bias row 1024 | rows 256 | info 256 | lse 256 |
//             delta 256;   phase A's dQ patch lies in dOt (staged after phase A), phase B's dK
//             and dV patches and the bias-gradient fold (16 x 65 floats) lie in Kt.
//   cosine variant (wattn_cos_*): the rows' inverse norms follow, rk 256 in the forward (a
//             lane keeps its queries' in registers), rq 256 | rk 256 in the backward, whose
//             slab row gains one column per head, the temperature gradient.
#pragma once
#include <stdint.h>

#include "attn_plan.h"

namespace mpa {

constexpr int WA_D = 32;          // head dim
constexpr int WA_N = 64;          // padded tokens of a window (score tile edge)
constexpr int WA_PITCH = 72;      // bf16 per row of a transposed LDS tile
constexpr int WA_PPITCH = 40;     // bf16 per row of an output patch [16][32]
constexpr int WA_TILE_BYTES = WA_D * WA_PITCH * 2;   // 4608
constexpr int WA_BIAS_MAX = 256;  // floats of a head's bias row in LDS: (2 * 8 - 1)^2 = 225
constexpr int WA_FOLD_PITCH = 65; // floats per query row of the fold's [16][64] dS slice
constexpr int WA_FWD_BYTES = WA_TILE_BYTES + 16 * WA_PPITCH * 2 + WA_BIAS_MAX * 4 + 2 * WA_N * 4;
constexpr int WA_BWD_BYTES = 3 * WA_TILE_BYTES + WA_BIAS_MAX * 4 + 4 * WA_N * 4;
constexpr int WA_NORM_BYTES = WA_N * 4;  // cosine variant: the inverse norms of one operand's rows
constexpr int WA_FWD_COS_BYTES = WA_FWD_BYTES + WA_NORM_BYTES;
constexpr int WA_BWD_COS_BYTES = WA_BWD_BYTES + 2 * WA_NORM_BYTES;
constexpr int WA_FILL_BLOCKS = 512;  // two 4-wave blocks per CU before the walks lengthen
constexpr int WA_MAX_ROWS = 512;     // slab rows (per head group) are capped here

struct WattnGeom {
  int B, H, Hf, Wf, ws, shift;
};

struct WattnPlan {
  int waves;         // W: waves per block = heads per block
  int groups;        // H / W (grid.y)
  int nwin;          // B (Hf / ws) (Wf / ws): windows (forward grid.x)
  int wpb;           // windows a backward block walks
  int rows;          // slab rows = backward grid.x = ceil(nwin / wpb)
  int nbias;         // (2 ws - 1)^2
  int slab_cols;     // floats per head of a slab row: nbias, + 1 (temperature) in the cosine variant
  int lds_fwd, lds_bwd;  // static LDS bytes per block
  int64_t ws_floats;     // slab floats: rows * H * slab_cols
};

// head_dim is the width of one head in qkv's columns (columns / (3 H))
inline const char* wattn_geom_error(const WattnGeom& g, int head_dim = WA_D) {
  if (head_dim != WA_D) return "head dim must be 32";
  if (g.B < 1 || g.H < 1 || g.Hf < 1 || g.Wf < 1) return "empty batch, map or no heads";
  if (g.ws < 1 || g.ws * g.ws > WA_N) return "a window holds at most 64 tokens (ws^2 <= 64)";
  if (g.Hf % g.ws || g.Wf % g.ws) return "the map must be a multiple of the window";
  if (g.shift < 0 || g.shift >= g.ws) return "shift must be in [0, ws)";
  if (g.H > 65535) return "heads above 65535";
  if ((int64_t)g.B * g.Hf * g.Wf * 3 * g.H * WA_D >= (int64_t)1 << 31) return "tensor too large (2^31 elements)";
  return nullptr;
}

// cosine: the plan of wattn_cos_fwd / wattn_cos_bwd (same grid, larger LDS and slab rows)
inline WattnPlan wattn_plan(const WattnGeom& g, bool cosine = false) {
  WattnPlan p{};
  p.waves = g.H % 4 == 0 ? 4 : g.H % 3 == 0 ? 3 : g.H % 2 == 0 ? 2 : 1;
  p.groups = g.H / p.waves;
  p.nwin = g.B * (g.Hf / g.ws) * (g.Wf / g.ws);
  // fill the CUs first (one window per block while the grid is below WA_FILL_BLOCKS), then
  // lengthen the walks; never more than WA_MAX_ROWS slab rows
  int rows = WA_FILL_BLOCKS / p.groups;
  if (rows < 1) rows = 1;
  if (rows > WA_MAX_ROWS) rows = WA_MAX_ROWS;
  p.wpb = (p.nwin + rows - 1) / rows;
  p.rows = (p.nwin + p.wpb - 1) / p.wpb;
  p.nbias = (2 * g.ws - 1) * (2 * g.ws - 1);
  p.slab_cols = p.nbias + (cosine ? 1 : 0);
  p.lds_fwd = p.waves * (cosine ? WA_FWD_COS_BYTES : WA_FWD_BYTES);
  p.lds_bwd = p.waves * (cosine ? WA_BWD_COS_BYTES : WA_BWD_BYTES);
  p.ws_floats = (int64_t)p.rows * g.H * p.slab_cols;
  return p;
}

// relative-position index of query (yi, xi) and key (yj, xj) of a window
AT_HD inline int wattn_rel(int ws, int yi, int xi, int yj, int xj) {
  return (yi - yj + ws - 1) * (2 * ws - 1) + (xi - xj + ws - 1);
}

// band of coordinate c (rolled frame) of an axis of length L: [0, L - ws), [L - ws, L - shift),
// [L - shift, L); one band when nothing is shifted
AT_HD inline int wattn_band(int c, int L, int ws, int shift) {
  return shift == 0 ? 0 : (c < L - ws ? 0 : (c < L - shift ? 1 : 2));
}

// shift region 0..8 of rolled-frame pixel (ry, rx): tokens of different regions do not attend
AT_HD inline int wattn_region(const WattnGeom& g, int ry, int rx) {
  return 3 * wattn_band(ry, g.Hf, g.ws, g.shift) + wattn_band(rx, g.Wf, g.ws, g.shift);
}

// token n (0 .. 63) of window `win` (0 .. nwin - 1): its row of qkv / o, or -1 for a padded
// token (n >= ws^2), and info = wy | wx << 8 | region << 16 (0 for a padded token, which
// keeps every relative index it enters in range)
AT_HD inline int wattn_token(const WattnGeom& g, int win, int n, uint32_t* info) {
  *info = 0;
  if (n >= g.ws * g.ws) return -1;
  const int nwx = g.Wf / g.ws, nw = (g.Hf / g.ws) * nwx;
  const int b = win / nw, w = win - b * nw;
  const int Y = w / nwx, X = w - Y * nwx;
  const int wy = n / g.ws, wx = n - wy * g.ws;
  const int ry = Y * g.ws + wy, rx = X * g.ws + wx;   // rolled frame
  int y = ry + g.shift, x = rx + g.shift;
  if (y >= g.Hf) y -= g.Hf;
  if (x >= g.Wf) x -= g.Wf;
  *info = (uint32_t)wy | (uint32_t)wx << 8 | (uint32_t)wattn_region(g, ry, rx) << 16;
  return (b * g.Hf + y) * g.Wf + x;
}

// relative index from two info words
AT_HD inline int wattn_rel_info(int ws, uint32_t qi, uint32_t kj) {
  return wattn_rel(ws, (int)(qi & 255), (int)((qi >> 8) & 255), (int)(kj & 255), (int)((kj >> 8) & 255));
}

}  // namespace mpa
