// Launch planning of the fused multi-head attention kernels and the ViT token kernels
// (attn.hip).  Host-only arithmetic with no HIP types, so a CPU program (attn_plan_check.cpp)
// can include it and sweep its invariants.
//
// Packed input qkv [B][S][3][H][64] bf16 (the in-projection's rows), head dim 64 only.  All
// three attention kernels cut the sequence into tiles of AT_TILE = 64 positions: a block of
// AT_WAVES = 4 waves owns one tile of one (batch, head), wave w its rows 16 w .. 16 w + 15, and
// streams the tiles of the other axis through LDS.
//   attn_fwd      owns a query tile, streams key tiles (K rows, V transposed), two ring stages
//   attn_bwd_dq   owns a query tile, streams key tiles (K rows, V rows, K transposed)
//   attn_bwd_dkv  owns a key tile,   streams query tiles (Q, dO rows and transposed)
// An LDS tile is 64 rows of AT_PITCH = 72 bf16 (144 B): an MFMA operand read is lane (i, g) ->
// 16 B at row i, byte 16 g (+ 64), and 16 rows at a 144-B pitch start at 16 distinct
// multiples of 4 banks, so the 16 lanes of a read phase cover all 64 banks once.
//
// Transposed tiles hold position (tile row) r in column at_pos(r): the P / dS operand of the
// second MFMA is the first one's accumulator, lane group g holding rows 4 g .. 4 g + 3 of each
// 16-row sub-tile, and at_pos puts the eight rows a lane group holds of a 32-row half side by
// side, so the matching V / dO / Q / K fragment is one 16-B read.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define AT_HD __host__ __device__
#else
#define AT_HD
#endif

namespace mpa {

constexpr int AT_D = 64;         // head dim
constexpr int AT_TILE = 64;      // query rows / key columns per tile
constexpr int AT_WAVES = 4;
constexpr int AT_THREADS = 64 * AT_WAVES;
constexpr int AT_PITCH = 72;     // bf16 per LDS tile row
constexpr int AT_TILE_BYTES = AT_TILE * AT_PITCH * 2;  // 9216
constexpr int AT_LDS_LIMIT = 64 * 1024;                // static LDS of a block

struct AttnGeom {
  int B, S, H;
};

struct AttnPlan {
  int tiles;       // ceil(S / 64): query tiles (grid.x) and key tiles (loop), or the reverse
  int tail;        // valid positions of the last tile, 1..64
  int lds_fwd, lds_dq, lds_dkv;  // static LDS bytes per block
  int64_t blocks;  // tiles * H * B
};

inline const char* attn_geom_error(const AttnGeom& g) {
  if (g.S < 1) return "empty sequence";
  if (g.B < 1 || g.H < 1) return "empty batch or no heads";
  if (g.B > 65535 || g.H > 65535) return "batch or heads above 65535";
  if ((int64_t)g.B * g.S * 3 * g.H * AT_D >= (int64_t)1 << 31) return "tensor too large (2^31 elements)";
  return nullptr;
}

// column of tile row r in a transposed LDS tile (a bijection of 0..63)
inline constexpr int at_pos(int r) {
  return (r & 32) | (((r >> 2) & 3) << 3) | (((r >> 4) & 1) << 2) | (r & 3);
}

// tile row that lane group g's accumulator element (sub-tile t, register e) holds
inline constexpr int at_acc_row(int t, int g, int e) { return 16 * t + 4 * g + e; }

inline AttnPlan attn_plan(const AttnGeom& g) {
  AttnPlan p{};
  p.tiles = (g.S + AT_TILE - 1) / AT_TILE;
  p.tail = g.S - (p.tiles - 1) * AT_TILE;
  p.lds_fwd = 2 * 2 * AT_TILE_BYTES;                   // two stages of (K, Vt)
  p.lds_dq = 3 * AT_TILE_BYTES;                        // K, V, Kt
  p.lds_dkv = 4 * AT_TILE_BYTES + 2 * AT_TILE * 4;     // Q, dO, Qt, dOt, lse, delta
  p.blocks = (int64_t)p.tiles * g.H * g.B;
  return p;
}

// ------------------------------------------------------------------ token kernels
// patchify: x [B][Hi][Wi][Cp] -> rows [B (Hi/P) (Wi/P)][P P Cp]; one thread per 16-B vector
struct PatchGeom {
  int B, Hi, Wi, Cp, P;
};

inline const char* patch_geom_error(const PatchGeom& g) {
  if (g.B < 1 || g.Hi < 1 || g.Wi < 1 || g.Cp < 1 || g.P < 1) return "empty tensor";
  if (g.Hi % g.P || g.Wi % g.P) return "image size must be a multiple of the patch";
  if ((g.P * g.Cp) % 8) return "a patch row (P * C) must be a multiple of 8 elements";
  if ((int64_t)g.B * g.Hi * g.Wi * g.Cp >= (int64_t)1 << 31) return "tensor too large (2^31 elements)";
  return nullptr;
}

// source element of output vector i (8 elements): the run (row, ky) is contiguous in x
AT_HD inline int64_t patch_src(const PatchGeom& g, int64_t i) {
  const int rv = g.P * g.Cp / 8;              // vectors per (patch, ky) run
  const int64_t run = i / rv;
  const int v = (int)(i - run * rv);
  const int ky = (int)(run % g.P);
  const int64_t patch = run / g.P;
  const int nw = g.Wi / g.P, nh = g.Hi / g.P;
  const int px = (int)(patch % nw), py = (int)((patch / nw) % nh);
  const int64_t b = patch / ((int64_t)nw * nh);
  return ((b * g.Hi + (int64_t)py * g.P + ky) * g.Wi + (int64_t)px * g.P) * g.Cp + (int64_t)v * 8;
}

// tokens: x [B][T][D], T = 1 + Np, D % 8 == 0
struct TokGeom {
  int B, T, D;
};

inline const char* tok_geom_error(const TokGeom& g) {
  if (g.B < 1 || g.T < 2 || g.D < 8) return "empty tensor";
  if (g.D % 8) return "width must be a multiple of 8";
  if ((int64_t)g.B * g.T * g.D >= (int64_t)1 << 31) return "tensor too large (2^31 elements)";
  return nullptr;
}

}  // namespace mpa
