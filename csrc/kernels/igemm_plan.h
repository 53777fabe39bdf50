// Launch planning of the implicit-GEMM engine: from a launch's arguments and the process's
// switches to the kernel that runs (family and template arguments), its grid, its split
// count, the fields it needs set in the argument struct, the follow-up launch (split-K
// finalize / split reduce) and the workspace all of that writes.  This header is the only
// place a GEMM launch is decided; igemm.hip and igemm_dma.hip launch what it returns.  Only
// igemm_args.h and the C++ standard library: no HIP, no globals, no environment, so
// igemm_plan_check.cpp runs every function here on the CPU (tests/test_igemm_plan_cpu.py).
//
// The 3x3 halo and 7x7 stem paths (halo_plan.h, conv_stem.hip) take precedence over a GEMM
// plan; the callers in igemm.hip ask them first.
#pragma once
#include <cstdio>
#include <string>

#include "igemm_args.h"

namespace mpa {

constexpr int BK = 32;  // K extent of one tile step (one v_mfma_f32_16x16x32_bf16)

// Staging engine for 16-B-granular operands: 0 = register-staged (igemm.hip),
// 1 = tuned default: LDS-DMA (igemm_dma.hip) for the rows GEMMs (fwd / dgrad / linear);
//     for wgrad the 8-wave generic DMA tile where it wins (wgrad_big), the incremental
//     DMA kernel where it applies, register staging elsewhere,
// 2 = LDS-DMA for every GEMM.
// dma_uni: the uniform-tap / incremental fast paths of the LDS-DMA engine.  kpad: 16-B but
// not 32-granular channel counts run the uniform-tap kernel with each tap's K padded to 32.
// force_*: tile override for measurement (zeros: the heuristics); applies to both plans
// (rows and wgrad, BM x BN of the respective GEMM) when the tile exists for the engine.
struct GemmSwitches {
  int engine = 1;
  bool dma_uni = true;
  bool kpad = true;
  int force_bm = 0, force_bn = 0, force_splits = 0;
};

// ---------------------------------------------------------------------------- tiles
// Every instantiated (BM, BN, WM, WN) per kernel family; a block has WM * WN waves.  The
// dispatchers in the .hip files cover exactly these rows.
struct Tile {
  int bm, bn, wm, wn;
  constexpr int block() const { return wm * wn * 64; }
};
struct TileSize {  // a tuned, forced or candidate tile (zeros: none)
  int bm, bn;
};

constexpr Tile kRowsRegTiles[] = {{128, 128, 2, 2}, {256, 64, 4, 1}, {128, 32, 4, 1}};
// the LDS-DMA engine adds the 8-wave 256x256 and the 256x128 / 128x64 tiles (256x256 is
// reachable through force_bm / force_bn only; tools/bench_kernels.py sweep measures it
// slower than 128x128 on every ResNet layer: it leaves the grid under one block per CU or
// forces split-K, whose fp32 partial slab costs more than the tile saves)
constexpr Tile kRowsDmaTiles[] = {{256, 256, 2, 4}, {256, 128, 2, 2}, {128, 128, 2, 2},
                                  {256, 64, 4, 1},  {128, 64, 2, 2},  {128, 32, 4, 1}};
constexpr Tile kWgradRegTiles[] = {{64, 128, 2, 2}, {128, 128, 2, 2}};
constexpr Tile kWgradDmaTiles[] = {{256, 256, 2, 4}, {128, 256, 2, 4}, {64, 256, 2, 4},
                                   {128, 128, 2, 2}, {64, 128, 2, 2}};
// incremental kernel for the 4-wave tiles; the 8-wave tiles keep the generic kernel (the
// extra per-lane pixel state costs them their second block per CU: 124 -> 166 VGPR)
constexpr Tile kWgradIncTiles[] = {{128, 128, 2, 2}, {64, 128, 2, 2}};

template <int N>
inline const Tile* find_tile(const Tile (&tiles)[N], int bm, int bn) {
  for (const Tile& t : tiles)
    if (t.bm == bm && t.bn == bn) return &t;
  return nullptr;
}
inline const Tile* rows_tile(int bm, int bn, bool dma) {
  return dma ? find_tile(kRowsDmaTiles, bm, bn) : find_tile(kRowsRegTiles, bm, bn);
}
inline const Tile* wgrad_tile(int bm, int bn, bool dma) {
  return dma ? find_tile(kWgradDmaTiles, bm, bn) : find_tile(kWgradRegTiles, bm, bn);
}

// ------------------------------------------------------------------- tuner candidates
constexpr TileSize kRowsCands[] = {{128, 128}, {256, 128}, {128, 64}, {256, 64}, {128, 32},
                                   {256, 256}};

// The 8-wave 256 x 256 rows tile is not an autotuner candidate: same-box A/B, round 3 -
// ResNet-18 b1024 47.73k/47.89k vs 47.67k/47.85k img/s, Inception 7.24k vs 7.26k,
// ResNet-34 25.35k vs 25.39k (noise) - for a longer first-step tuning pass.
inline bool rows_cand_ok(TileSize c, int N) {
  if (c.bm == 256 && c.bn == 256) return false;
  if (c.bn == 128 && N <= 64) return false;  // half-empty tiles
  if (c.bn == 64 && (N <= 32 || N > 1024)) return false;
  if (c.bn == 32 && N > 32) return false;
  return true;
}

constexpr TileSize kWgradCands[] = {{64, 128}, {128, 128}, {64, 256}, {128, 256}, {256, 256}};

inline bool wgrad_cand_ok(TileSize c, const WGradArgs& a) {
  if (c.bm > 64 && a.Kout <= 64) return false;  // half-empty tiles
  if (c.bn == 256 && a.Ncols <= 128) return false;
  return true;
}

// ------------------------------------------------------------------------- tuner keys
// One key per GEMM shape; data-parallel ranks exchange the "key -> BMxBN" table, so the
// text is an interface.  Ktot: the launch's K after padding (plan_rows).
inline std::string rows_key(const IGemmArgs& a, int Ktot, bool bkc, bool split) {
  char k[256];
  snprintf(k, sizeof k, "rows%d%d M%d N%d K%d a%dx%dx%d o%dx%d U%d,%d O%d,%d T%d s%d b%d r%d p%d",
           (int)bkc, (int)split, a.M, a.N, Ktot, a.aH, a.aW, a.aC, a.oH, a.oW, a.Uh, a.Uw,
           a.Oh, a.Ow, a.T, a.stap, a.beta, a.relu, a.nphase);
  std::string key(k);
  for (int i = 0; i < a.nphase; ++i)
    key += " " + std::to_string(a.ph[i].M) + "," + std::to_string(a.ph[i].Ktot);
  return key;
}

inline std::string wgrad_key(const WGradArgs& a) {
  char k[200];
  snprintf(k, sizeof k, "wgrad K%d N%d P%d x%dx%dx%d o%dx%d f%dx%d s%d,%d p%d,%d", a.Kout, a.Ncols,
           a.Mpix, a.H, a.W, a.C, a.P, a.Q, a.R, a.S, a.sh, a.sw, a.ph, a.pw);
  return k;
}

// ======================================================================================
//  rows GEMMs (conv forward / dgrad / linear)
// ======================================================================================
inline bool rows_dma(int vw, const GemmSwitches& sw) { return vw == 8 && sw.engine >= 1; }

// byte extents of the rows kernel's operands: the uniform-tap kernel addresses both with
// 32-bit offsets
inline bool rows_uni_fits(const IGemmArgs& a, bool bkc) {
  const PhaseDesc* d = a.nphase > 0 ? &a.ph[0] : nullptr;
  const int64_t hw = d ? (int64_t)d->oH * d->oW : (int64_t)a.oH * a.oW;
  const int64_t m = d ? d->M : a.M;
  const int64_t nimg = hw > 0 ? (m + hw - 1) / hw : 0;
  const int64_t abytes = nimg * a.aH * a.aW * a.aC * 2;
  const int64_t bbytes = (bkc ? (int64_t)a.N : (int64_t)a.aC * a.RS) * a.ldb * 2;
  const int64_t b2bytes = (int64_t)a.N * a.ldb2 * 2;
  return abytes < (1ll << 31) && bbytes < (1ll << 31) && b2bytes < (1ll << 31);
}

// the LDS-DMA engine runs the uniform-tap kernel (every 32-wide K step lies inside one tap)
inline bool rows_uni_ok(const IGemmArgs& a, bool bkc, bool kpad, const GemmSwitches& sw) {
  return (a.aC % BK == 0 || a.stap || (kpad && bkc)) && sw.dma_uni && rows_uni_fits(a, bkc);
}

// 16-B but not 32-granular channel counts (Inception 48 / 80): the launch runs the
// uniform-tap kernel with each tap's K padded to 32 (kpad off: the generic gather kernel)
inline bool rows_kpad_ok(const IGemmArgs& a, bool bkc, int vw, const GemmSwitches& sw) {
  return rows_dma(vw, sw) && sw.kpad && bkc && sw.dma_uni && !a.stap && a.nphase == 0 &&
         a.aC % BK != 0 && a.aC % 8 == 0 && rows_uni_fits(a, bkc);
}

// a second GEMM source is read only by the uniform-tap kernel's phase form with K-contiguous
// B: true exactly when plan_rows_phases names that kernel
inline bool rows_uni_src2_ok(const IGemmArgs& a, bool bkc, const GemmSwitches& sw) {
  return bkc && a.nphase > 0 && !a.stap && a.aC % BK == 0 && rows_uni_ok(a, bkc, false, sw);
}
inline bool dgrad_src2_ok(const IGemmArgs& a, int vw, bool bkc, const GemmSwitches& sw) {
  return rows_dma(vw, sw) && a.nphase > 0 && a.nphase <= MAXPH && rows_uni_src2_ok(a, bkc, sw);
}

inline int choose_bn(int N) {
  if (N <= 32) return 32;
  if (N <= 64 || (N % 128 != 0 && N % 64 == 0 && N < 256)) return 64;
  return 128;
}

// Split-K for grids smaller than the chip (< 256 tiles): each split stores its partial
// tile with plain 16-B stores into a [splits][M][N] fp32 slab and splitk_finalize sums
// them (+bias, ReLU, bf16, BN statistics) - no atomics.  Slab traffic is
// 2 * splits * M * N * 4 bytes, small next to the GEMM for these deep-K shapes.
inline int choose_splits(int tiles, int ktiles) {
  if (tiles >= 256 || ktiles < 16) return 1;
  int s = (512 + tiles - 1) / tiles;
  s = std::min(s, ktiles / 8);
  s = std::min(s, 64);
  return std::max(s, 1);
}

// even K-tile shares: no split is empty
inline void finish_split_plan(int ktiles, int& splits, int& per_split) {
  per_split = ktiles > 0 ? (ktiles + splits - 1) / splits : 1;
  splits = ktiles > 0 ? (ktiles + per_split - 1) / per_split : 1;
}

// tile and split count of an M x N x Ktot rows GEMM.  tuned: a tile chosen by the autotuner
// (zeros: the heuristic); force_bm / force_bn win.
struct RowsTiling {
  Tile tile;
  int tiles_n, tiles_total, splits, ktiles_per_split;
};
inline RowsTiling rows_tiling(int M, int N, int Ktot, bool allow_split, bool dma,
                              const GemmSwitches& sw, TileSize tuned) {
  int BN = choose_bn(N);
  // 64-wide GEMMs: the DMA engine's 128x64 tile (36 KiB ring, 4 blocks/CU) beats 256x64
  // (60 KiB, 2 blocks/CU) on every ResNet-18 64-channel layer by 8-20 % (tile sweep)
  int BM = (BN == 64 && !dma) ? 256 : 128;
  const int ktiles = (Ktot + BK - 1) / BK;
  if (tuned.bm && tuned.bn && rows_tile(tuned.bm, tuned.bn, dma)) { BM = tuned.bm; BN = tuned.bn; }
  if (sw.force_bm && sw.force_bn && rows_tile(sw.force_bm, sw.force_bn, dma)) {
    BM = sw.force_bm;
    BN = sw.force_bn;
  }
  RowsTiling t{};
  t.tile = *rows_tile(BM, BN, dma);
  t.tiles_n = (N + BN - 1) / BN;
  t.tiles_total = (M + BM - 1) / BM * t.tiles_n;
  t.splits = allow_split ? choose_splits(t.tiles_total, ktiles) : 1;
  if (allow_split && sw.force_splits > 0) t.splits = std::min(sw.force_splits, std::max(ktiles, 1));
  finish_split_plan(ktiles, t.splits, t.ktiles_per_split);
  return t;
}

// split-K partials [splits][M][N], sized for whichever engine ends up running the launch
inline int64_t rows_ws_floats(int M, int N, int Ktot, const GemmSwitches& sw) {
  int64_t best = 0;
  for (int dma = 0; dma < 2; ++dma) {
    const RowsTiling t = rows_tiling(M, N, Ktot, true, dma == 1, sw, TileSize{});
    if (t.splits > 1) best = std::max(best, (int64_t)t.splits * M * N);
  }
  return best;
}

// statistics slab rows: one per 128-row M-tile (the smallest BM of any plan), per halo /
// stem block or per splitk_finalize block row (<= slab_rows_max), then the [2][N] sums
inline int64_t slab_rows_max(int M) {
  return std::max<int64_t>((M + 127) / 128, std::max(64, HALO_MAX_ROWS));
}
inline int64_t slab_floats(int M, int N) { return slab_rows_max(M) * 2 * N + 2 * N; }

// dgrad + fused BN-backward reduction: dense slab rows, one per (phase, M-tile)
inline int64_t bnred_slab_floats(int M, int N, int nphase) {
  const int64_t rows = std::max<int64_t>((int64_t)((M + 127) / 128 + 1) * std::max(nphase, 1),
                                         HALO_MAX_ROWS);
  return rows * 2 * N;
}

enum class RowsFamily { Reg, Dma, DmaUni };  // igemm_rows_kernel, igemm_rows_dma(_uni)_kernel

struct RowsLaunch {
  RowsFamily family;
  int BM, BN, WM, WN, VW;  // (VW: register family only; the LDS-DMA kernels read 16 B)
  bool BKC, SPLIT, PH;
  int grid_x, splits, block;  // grid (grid_x, 1, splits)
  // fields of IGemmArgs the kernel reads that the plan decides (apply)
  int Ktot, kpad, tiles_n, tiles_total, ktiles_per_split;
  int nphase, ph_tiles[MAXPH];
  bool to_ws;              // the kernel stores fp32 partials [splits][M][N] into the workspace
  int fin_cw, fin_gx, fin_gy;  // splitk_finalize_kernel<fin_cw>, grid (gx, gy); cw 0: none
  int slab_rows;           // statistics-slab rows written: M-tiles (per phase, summed: the
                           // rows a fused BN-backward reduction runs over) or finalize rows
  void apply(IGemmArgs& a) const {
    a.Ktot = Ktot;
    a.kpad = kpad;
    a.tiles_n = tiles_n;
    a.tiles_total = tiles_total;
    a.ktiles_per_split = ktiles_per_split;
    for (int i = 0; i < nphase; ++i) a.ph[i].tiles = ph_tiles[i];
  }
};

namespace plan_detail {
inline RowsLaunch rows_launch(const IGemmArgs& a, int Ktot, int kpad, const Tile& t, bool bkc, int vw,
                              bool dma, bool ph, int splits, const GemmSwitches& sw) {
  RowsLaunch p{};
  p.family = !dma ? RowsFamily::Reg
                  : rows_uni_ok(a, bkc, kpad != 0, sw) ? RowsFamily::DmaUni : RowsFamily::Dma;
  p.BM = t.bm; p.BN = t.bn; p.WM = t.wm; p.WN = t.wn;
  p.VW = dma || vw == 8 ? 8 : vw == 4 ? 4 : 1;
  p.BKC = bkc;
  p.SPLIT = splits > 1;
  p.PH = ph;
  p.splits = splits;
  p.block = t.block();
  p.Ktot = Ktot;
  p.kpad = kpad;
  return p;
}
}  // namespace plan_detail

// padded K of a launch plan_rows pads (0: it does not); the tuner's key carries it
inline int rows_kpad_ktot(const IGemmArgs& a, bool bkc, int vw, const GemmSwitches& sw) {
  return rows_kpad_ok(a, bkc, vw, sw) ? a.T * ((a.aC + BK - 1) / BK) * BK : 0;
}

// One rows GEMM (a.nphase == 0).  allow_split: the caller holds rows_ws_floats(M, N, Ktot)
// floats of workspace; a padded-K launch never splits (the workspace was sized for the
// unpadded K).  dma: the engine, rows_dma(vw, sw) for every caller but the fused
// BN-backward dgrad, whose callers guarantee the LDS-DMA engine and which never pads.
inline RowsLaunch plan_rows_on(const IGemmArgs& a, bool bkc, int vw, bool allow_split, bool dma,
                               bool pad, const GemmSwitches& sw, TileSize tuned) {
  const int kp = pad ? rows_kpad_ktot(a, bkc, vw, sw) : 0;
  if (kp) allow_split = false;
  if (!dma) tuned = TileSize{};
  const RowsTiling t = rows_tiling(a.M, a.N, kp ? kp : a.Ktot, allow_split, dma, sw, tuned);
  RowsLaunch p = plan_detail::rows_launch(a, kp ? kp : a.Ktot, kp ? 1 : a.kpad, t.tile, bkc, vw, dma,
                                          false, t.splits, sw);
  p.tiles_n = t.tiles_n;
  p.tiles_total = t.tiles_total;
  p.ktiles_per_split = t.ktiles_per_split;
  p.grid_x = t.tiles_total;
  p.to_ws = t.splits > 1;
  p.slab_rows = (a.M + t.tile.bm - 1) / t.tile.bm;
  if (t.splits > 1) {
    // ~512+ blocks (two rows in flight per thread), at most one slab row per block row
    const int cw = a.N <= 32 ? 32 : 64, rp = 256 / cw, gx = (a.N + cw - 1) / cw;
    p.fin_cw = cw;
    p.fin_gx = gx;
    p.fin_gy = (int)std::min<int64_t>(
        slab_rows_max(a.M),
        std::max(1, std::min((a.M + 2 * rp - 1) / (2 * rp), (1024 + gx - 1) / gx)));
    p.slab_rows = p.fin_gy;
  }
  return p;
}
inline RowsLaunch plan_rows(const IGemmArgs& a, bool bkc, int vw, bool allow_split,
                            const GemmSwitches& sw, TileSize tuned) {
  return plan_rows_on(a, bkc, vw, allow_split, rows_dma(vw, sw), true, sw, tuned);
}

// All stride phases of a strided conv's dgrad in ONE launch on the LDS-DMA engine
// (0 < a.nphase <= MAXPH): the tile of the largest phase; tile g of the launch belongs to
// phase g % nphase, phases padded to the longest tile count; never split.
inline RowsLaunch plan_rows_phases(const IGemmArgs& a, bool bkc, const GemmSwitches& sw,
                                   TileSize tuned) {
  int M = 0, Ktot = 0;
  for (int i = 0; i < a.nphase; ++i) {
    M = std::max(M, a.ph[i].M);
    Ktot = std::max(Ktot, a.ph[i].Ktot);
  }
  const RowsTiling t = rows_tiling(M, a.N, Ktot, false, true, sw, tuned);
  RowsLaunch p = plan_detail::rows_launch(a, a.Ktot, a.kpad, t.tile, bkc, 8, true, true, 1, sw);
  p.tiles_n = (a.N + t.tile.bn - 1) / t.tile.bn;
  p.nphase = a.nphase;
  int most = 0;
  for (int i = 0; i < a.nphase; ++i) {
    const int mts = (a.ph[i].M + t.tile.bm - 1) / t.tile.bm;
    p.ph_tiles[i] = mts * p.tiles_n;
    most = std::max(most, p.ph_tiles[i]);
    p.slab_rows += mts;
  }
  p.tiles_total = most * a.nphase;
  p.ktiles_per_split = 1 << 30;
  p.grid_x = p.tiles_total;
  return p;
}

// ======================================================================================
//  weight-gradient GEMMs
// ======================================================================================
// incremental pixel walk applicable: one wrap per step suffices, 32-bit offsets, and
// 16-B granular operands on both sides (callers guarantee Kout % 8 == 0, C % 8 == 0)
inline bool wgrad_inc_ok(const WGradArgs& a, const GemmSwitches& sw) {
  return sw.dma_uni && (BK / a.Q) + 1 <= a.P && a.Ncols >= 8 && a.Kout >= 8 &&
         (int64_t)a.Mpix / (a.P * a.Q) * a.H * a.W * a.C < (1ll << 31);
}

struct WInc {   // per-launch scalar constants of the incremental kernel's pixel walk
  int dq_s, dp_s;          // sw * (32 % Q), sh * (32 / Q): per-step ow*sw / oh*sh advance
  int qwrap, pwrap;        // Q * sw, P * sh: wrap thresholds of ow*sw and oh*sh
  int step_off;            // input offset advance per step (no wrap)
  int qwrap_off, pwrap_off;  // extra input offset on a column / image wrap
};
inline WInc wgrad_inc(const WGradArgs& a) {
  WInc w;
  w.dq_s = a.sw * (BK % a.Q);
  w.dp_s = a.sh * (BK / a.Q);
  w.qwrap = a.Q * a.sw;
  w.pwrap = a.P * a.sh;
  w.step_off = (w.dp_s * a.W + w.dq_s) * a.C;
  w.qwrap_off = (a.sh * a.W - a.Q * a.sw) * a.C;
  w.pwrap_off = (a.H - a.P * a.sh) * a.W * a.C;
  return w;
}

// big: the 8-wave 128x256 LDS-DMA tile (measured +20..40 % over the 4-wave tiles for
// Kout >= 256 and for the stem's tiny-output / huge-pixel-count reduction)
inline bool wgrad_big(const WGradArgs& a, bool dma_ok) {
  return dma_ok && (a.Kout >= 256 || ((int64_t)a.Kout * a.Ncols <= 32768 && a.Mpix >= (1 << 20)));
}

// split over pixels: ~512 blocks (2 per CU), >= 16 K-steps per split, slab <= 64 MiB
// (16 Mi floats); stem-shaped reductions target ~1024 blocks instead
struct WGradTiling {
  Tile tile;
  int tiles_n, tiles_total, splits, ktiles_per_split;
};
inline WGradTiling wgrad_tiling(int Kout, int Ncols, int Mpix, bool dma, bool big,
                                const GemmSwitches& sw, TileSize tuned_tile) {
  int BM = (Kout <= 64) ? 64 : 128;
  int BN = 128;
  // few 128-row tiles (e.g. a 1x1 downsample: Ncols = C_in): halve BM for parallelism
  if (dma && BM == 128 && ((Kout + 127) / 128) * ((Ncols + 127) / 128) < 4) BM = 64;
  if (big) BN = 256, BM = (Kout <= 64) ? 64 : 128;  // 64-row stems: no half-empty tile
  const bool tuned = tuned_tile.bm && tuned_tile.bn && wgrad_tile(tuned_tile.bm, tuned_tile.bn, dma);
  if (tuned) { BM = tuned_tile.bm; BN = tuned_tile.bn; }
  const bool forced = sw.force_bm && sw.force_bn;
  if (forced && wgrad_tile(sw.force_bm, sw.force_bn, dma)) {
    BM = sw.force_bm;
    BN = sw.force_bn;
  }
  WGradTiling t{};
  const int tiles_m = (Kout + BM - 1) / BM;
  const int ktiles = (Mpix + BK - 1) / BK;
  // stem-shaped reductions (64 output rows, 129..256 columns, >= 1M pixels): two 64x128
  // column tiles x 512 splits instead of one 64x256 tile x 512 splits
  // (profiles/stem_sweep_b512.txt, batch 512: 64x128/s512 439.4 us, 64x128/s1024 449.2 us,
  // 64x256/s512 493.7 us). 512 splits keep the fp32 slab at 29 MB (1024: 58.7 MB).
  const bool stem2 = big && BM == 64 && BN == 256 && !forced && !tuned && Ncols > 128 && Ncols <= 256;
  if (stem2) BN = 128;
  t.tile = *wgrad_tile(BM, BN, dma);
  t.tiles_n = (Ncols + BN - 1) / BN;
  t.tiles_total = tiles_m * t.tiles_n;
  t.splits = std::max(1, ((stem2 ? 1024 : 512) + t.tiles_total - 1) / t.tiles_total);
  t.splits = std::min(t.splits, std::max(1, ktiles / 16));
  if (sw.force_splits > 0) t.splits = std::min(sw.force_splits, std::max(ktiles, 1));
  const int64_t out = (int64_t)Kout * Ncols;
  t.splits = (int)std::min<int64_t>(t.splits, std::max<int64_t>(1, (16ll << 20) / out));
  finish_split_plan(ktiles, t.splits, t.ktiles_per_split);
  return t;
}

// split partials [splits][Kout][Ncols] of the GEMM plans (the halo and stem kernels size
// their own): register, DMA, DMA big tile
inline int64_t wgrad_gemm_ws_floats(int Kout, int Ncols, int Mpix, const GemmSwitches& sw) {
  int64_t best = 0;
  for (int dma = 0; dma < 3; ++dma) {
    const WGradTiling t = wgrad_tiling(Kout, Ncols, Mpix, dma >= 1, dma == 2, sw, TileSize{});
    if (t.splits > 1) best = std::max(best, (int64_t)t.splits * Kout * Ncols);
  }
  return best;
}

// igemm_wgrad_kernel, igemm_wgrad_dma_kernel, igemm_wgrad_dma_inc_kernel
enum class WGradFamily { Reg, Dma, DmaInc };
enum class WGradReduce { None, Vector, Scalar };  // wgrad_reduce_kernel / _scalar_kernel

struct WGradLaunch {
  WGradFamily family;
  int BM, BN, WM, WN, VWA, VWB;  // (VWA / VWB: register family only)
  int grid_x, splits, block;     // grid (grid_x, 1, splits)
  int tiles_n, tiles_total, ktiles_per_split;  // fields of WGradArgs (apply)
  WInc inc;                      // DmaInc only
  WGradReduce reduce;            // sums the split slab into dw
  int reduce_blocks;
  void apply(WGradArgs& a) const {
    a.tiles_n = tiles_n;
    a.tiles_total = tiles_total;
    a.ktiles_per_split = ktiles_per_split;
  }
};

// block count of wgrad_reduce_kernel over n = Kout * Ncols floats (n % 4 == 0)
inline int wgrad_reduce_blocks(int64_t n) { return (int)std::max<int64_t>(1, (n / 4 + 63) / 64); }

// One weight-gradient GEMM.  tuned: the autotuner's tile (LDS-DMA-capable launches only).
inline WGradLaunch plan_wgrad(const WGradArgs& a, int vwa, int vwb, const GemmSwitches& sw,
                              TileSize tuned) {
  const bool dma_ok = vwa == 8 && vwb == 8 && sw.engine >= 1;
  if (!dma_ok) tuned = TileSize{};
  const bool big = (tuned.bm && tuned.bn) ? tuned.bn == 256 : wgrad_big(a, dma_ok);
  // engine 1: big 8-wave tile where it wins, else the incremental-pixel DMA kernel
  // (tools/bench_kernels.py sweep: equal or faster than register staging on every
  // ResNet-18 wgrad shape it covers), else register staging
  const bool dma = big || (dma_ok && (sw.engine == 2 || wgrad_inc_ok(a, sw)));
  const WGradTiling t = wgrad_tiling(a.Kout, a.Ncols, a.Mpix, dma, big, sw, tuned);
  WGradLaunch p{};
  const bool inc = dma && wgrad_inc_ok(a, sw) && find_tile(kWgradIncTiles, t.tile.bm, t.tile.bn);
  p.family = !dma ? WGradFamily::Reg : inc ? WGradFamily::DmaInc : WGradFamily::Dma;
  p.BM = t.tile.bm; p.BN = t.tile.bn; p.WM = t.tile.wm; p.WN = t.tile.wn;
  p.VWA = dma || vwa == 8 ? 8 : vwa == 4 ? 4 : 1;
  p.VWB = dma || vwb != 1 ? 8 : 1;
  p.grid_x = t.tiles_total;
  p.splits = t.splits;
  p.block = t.tile.block();
  p.tiles_n = t.tiles_n;
  p.tiles_total = t.tiles_total;
  p.ktiles_per_split = t.ktiles_per_split;
  if (inc) p.inc = wgrad_inc(a);
  if (t.splits > 1) {
    const int64_t n = (int64_t)a.Kout * a.Ncols;
    if (n % 4 == 0) {  // float4 path: 16-B aligned split rows
      p.reduce = WGradReduce::Vector;
      p.reduce_blocks = wgrad_reduce_blocks(n);
    } else {
      p.reduce = WGradReduce::Scalar;
      p.reduce_blocks = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 4096));
    }
  }
  return p;
}

}  // namespace mpa
