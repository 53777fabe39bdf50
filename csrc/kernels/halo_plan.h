// Launch planner of the halo-staged 3x3 / stride-1 kernels (conv_halo.hip): the tile
// constants, the plan structs the kernels take by value, and two pure functions that map a
// launch's arguments, the process switches and the CU count to the one kernel instance
// that runs it (or to none: the implicit GEMM takes the launch).  Only the C++ standard
// library: csrc/kernels/halo_plan_check.cpp sweeps it on the CPU.  conv_halo.hip launches
// what a plan names and decides nothing itself, so "will the halo engine take this" and
// "which instance runs" are one evaluation.
#pragma once
#include <algorithm>
#include <stdint.h>

#include "igemm_args.h"

namespace mpa {

constexpr int HB_BM = 256, HB_BN = 64, HB_NW = 4;
constexpr int HB_HIW = 9;                       // halo DMA instructions per wave per chunk
constexpr int HB_HPX = 16 * HB_NW * HB_HIW;     // 576 halo pixels per chunk
constexpr int HB_HBYTES = HB_HPX * 64;          // 36 KiB
constexpr int HB_WIW = 9;                       // weight DMA instructions per wave per chunk
constexpr int HB_WBYTES = 9 * HB_BN * 64;       // 36 KiB: [tap][64 cols][32 k]
constexpr int HB_RED = HB_NW * HB_BN * 2 * 4;   // epilogue cross-wave statistics
constexpr int HB_COLS = 4 * HB_BN * 4;          // per-column epilogue operands [4][64]
constexpr int HB_LDS = 2 * HB_HBYTES + 2 * HB_WBYTES + HB_RED + HB_COLS;  // 150,528 B
constexpr int HB_BM7 = 448;                     // pixels of an MI = 7 tile
constexpr int HB_HPX7 = 640;                    // its halo stage (pixels)

struct HaloPlan {
  int w2;               // halo row pitch P: W + 1 (one shared zero column) rounded up to 8
  int btoff[9];         // tap t = (dh + 1) * 3 + (dw + 1): byte offset bt * aC * 2 of its
                        // weight row segment (the host orders any 3x3 tap table this way)
  uint32_t mag_w, mag_w2, mag_h1, mag_hw;  // floor(2^32 / d) + 1: exact n / d for n*d < 2^32
  int tiles_m, tiles_total, cc;
  uint32_t a_bytes, b_bytes;
  int hiw;              // (256-pixel tiles) halo DMA instructions per producer wave and item:
                        // the slots any tile of this geometry reads (halo_need), <= HB_HIW
};

// Epilogue flavours (compile-time, so the kernels' fused epilogue is one straight-line block)
enum : int { EP_RELU = 1, EP_BETA = 2, EP_BNRED = 4, EP_STATS = 8, EP_BIAS = 16 };

struct StripPlan {
  int tr, tw, p;            // tile rows / columns, LDS pitch (pixels)
  int hiw;                  // halo DMA instructions per producer wave per item (<= 9)
  int tiles_c, tiles_img;   // column strips per row band, tiles per image
  int tiles_total, cc;
  uint32_t mag_tw, mag_p, mag_tc, mag_timg;  // floor(2^32 / d) + 1 (0: d == 1)
  int btoff[9];
  uint32_t a_bytes, b_bytes;
  int ch, cw;               // tap-set centre shift: output (i, j) reads input rows / cols
                            // i + ch - 1 .. i + ch + 1 (same conv 0, valid 1, its dgrad -1)
};

constexpr int HW_BM = 128;                    // pixels per tile
constexpr int HW_HIW = 7;                     // halo DMA instructions per wave per chunk
constexpr int HW_HPX = 16 * 4 * HW_HIW;       // 448 halo pixels
constexpr int HW_HBYTES = HW_HPX * 64;        // 28 KiB per chunk
constexpr int HW_DBYTES = HW_BM * 64 * 2;     // 16 KiB: dy tile, 4 k-steps x [32 px][64 k]
constexpr int HW_STAGE = HW_DBYTES + 2 * HW_HBYTES;  // 72 KiB
constexpr int HW_LDS = 2 * HW_STAGE;                 // 147,456 B

struct HaloWPlan {
  int toff[9];
  int w2;  // halo row pitch in pixels: W + 2 rounded up to 16 (see the B-address note)
  uint32_t mag_w, mag_w2, mag_h1, mag_hw;
  int tiles_m, parts, kparts, Z;
  uint32_t dy_bytes, x_bytes;
  // STRIP: tiles of tr rows x tw columns of one image (w2 = tw + 2 rounded up to 16), for
  // images too wide for the 128-pixel linear tiles' halo (VGG 224^2 / 112^2)
  int tr, tw, tiles_c, tiles_img;
  uint32_t mag_tw, mag_tc, mag_timg;  // (0: divisor 1)
  // XCD-grouped block order (grid % 8 == 0): logical block L = xcd * (grid / 8) + slot, so
  // one XCD's blocks are consecutive (z, part) ids - they share z lanes and cover a run of
  // partitions, and each staged dy / x tile is read into that XCD's L2 by the blocks that
  // consume it, instead of every XCD fetching every x (or dy) panel
  int xmap;
};

// ------------------------------------------------------------------------ geometry
inline uint32_t magic(uint32_t d) { return (uint32_t)((1ull << 32) / d + 1); }

// halo row pitch: W pixels + one zero column shared by consecutive rows (a row's right
// border is the next row's left border), rounded up to 8 pixels
inline int halo_pitch(int W) { return (W + 1 + 7) / 8 * 8; }
inline int halo_wgrad_pitch(int W) { return (W + 2 + 15) / 16 * 16; }

// Halo slots (pixels of pitch-P rows) that the taps of any linear tile of BM pixels reach:
// the rows the tile touches, 2 halo rows and the image separators it crosses (+1: with
// P == W + 1 the last slot's right border is the next pixel).  One expression for the
// admission checks (the stage must hold it) and for the geometry-sized fetch (nothing at
// or past it is read: tools/halo_index_check.py proves that for every tile).
inline int64_t halo_need(int BM, int H, int W, int P) {
  const int64_t HW = (int64_t)H * W;
  const int64_t rows = (BM - 1 + W - 1) / W + 1;
  const int64_t seps = (BM - 1) / HW + 1;
  return (rows + 2 + seps) * P + (P == W + 1 ? 1 : 0);
}

// 16-slot DMA instructions per wave (4 DMA waves, slot blocks dealt round-robin) that
// cover `need` slots, at most the stage's hiw_max (trim off: the whole stage)
inline int halo_dma_count(int64_t need, int hiw_max, bool trim) {
  if (!trim) return hiw_max;
  const int64_t blocks = (need + 15) / 16;
  return (int)std::min<int64_t>(hiw_max, (blocks + 3) / 4);
}

// Halo DMA instructions per wave and chunk of the 4-wave linear-tile weight gradient on
// H x W images: the smallest instantiated count (HT) that covers the slots a tile reads.
// Instantiated next to the pitch: 4 of 7 at pitch 16 (ResNet layer3), 5 of 7 at pitch 32
// (layer2).
inline int halo_wgrad_dma_count(int H, int W, bool trim) {
  const int W2 = halo_wgrad_pitch(W);
  const int64_t need = halo_need(HW_BM, H, W, W2);
  if (need > HW_HPX) return HW_HIW;  // (ONECH / strip tiles: whole stages)
  const int c = halo_dma_count(need, HW_HIW, trim);
  if (W2 == 16 && c <= 4) return 4;
  if (W2 == 32 && c <= 5) return 5;
  return HW_HIW;
}

// epilogue flavour of a launch; -1: not instantiated (the implicit GEMM runs it)
inline int halo_epi(const IGemmArgs& a) {
  int e = 0;
  // fused BN reduction: the z-mask form only (y is never read; see EpiIn)
  if (a.ep_bnred)
    return (a.beta || a.relu || a.bias || a.ep_y || !a.ep_gamma || !a.ep_beta || !a.ep_mean ||
            !a.ep_rstd)
               ? -1
               : EP_BNRED;
  if (a.relu) e |= EP_RELU;
  if (a.beta) e |= EP_BETA;
  if (a.stats) e |= EP_STATS;
  if (a.bias) e |= EP_BIAS;
  switch (e) {
    case 0: case EP_BETA: case EP_STATS: case EP_BIAS | EP_RELU: case EP_BIAS | EP_STATS:
      return e;
    default:
      return -1;
  }
}

// centre shift (ch, cw) of a 3x3 stride-1 tap set: the taps Oh + dh cover ch-1 .. ch+1 (same
// conv 0; valid conv 1; the valid conv's dgrad, padding 2, -1) and the output is the input
// less 2*ch rows / 2*cw columns
inline bool tap_shift(const IGemmArgs& a, int& ch, int& cw) {
  int mh = 1 << 20, mw = 1 << 20;
  for (int t = 0; t < 9; ++t) {
    mh = std::min(mh, a.Oh + a.taps.dh[t]);
    mw = std::min(mw, a.Ow + a.taps.dw[t]);
  }
  ch = mh + 1;
  cw = mw + 1;
  if (ch < -1 || ch > 1 || cw < -1 || cw > 1) return false;
  int seen = 0;  // every relative (dh, dw) in {-1,0,1}^2 exactly once
  for (int t = 0; t < 9; ++t) {
    const int dh = a.Oh + a.taps.dh[t] - ch, dw = a.Ow + a.taps.dw[t] - cw;
    if (dh < -1 || dh > 1 || dw < -1 || dw > 1) return false;
    seen |= 1 << ((dh + 1) * 3 + dw + 1);
  }
  return seen == 511 && a.oH == a.aH - 2 * ch && a.oW == a.aW - 2 * cw;
}

// persistent grid: G8 blocks per XCD, a multiple of tiles_n (fixed column tile per block)
inline int halo_grid(int cus, int tiles_total, int tiles_n) {
  int g8 = std::min(std::min(cus, HALO_MAX_ROWS) / 8, (tiles_total + 7) / 8);
  g8 = std::max(tiles_n, g8 / tiles_n * tiles_n);
  return 8 * g8;
}

// ------------------------------------------------------------------------ switches
// The process-wide MPA_HALO* switches (conv_halo.hip holds the one object) as a parameter
struct HaloSwitches {
  bool halo = true;   // MPA_HALO=0: the implicit GEMM runs every launch
  bool trim = true;   // geometry-sized halo fetch (off: every launch fetches the whole stage)
  bool wres = true;   // MPA_HALO_WRES=0: no resident-weight variant
  bool mi7 = true;    // MPA_HALO_MI7=0: 256-pixel tiles for the resident-weight layers
  bool wxmap = true;  // MPA_HALO_WXMAP=0: plain weight-gradient block order
  bool wprod = true;  // MPA_HALO_WPROD=0: 4-wave weight gradients (MFMA waves issue the DMAs)
  int strip = 1;      // MPA_HALO_STRIP: 0 off; 1 images too wide for the linear tiles; 2 also
                      // the resident-weight layers whose strips leave room for a third stage
};

// --------------------------------------------------------------- forward / stride-1 dgrad
enum class HaloKind { None, Linear256, Linear448, Strip };

// One instance of conv3_halo_kernel<wres, epi, full, nj, MI> (Linear256: MI 4, Linear448:
// MI 7) or conv3_strip_kernel<wres, epi, ns, nj>, its grid and block, and its plan struct
struct HaloLaunch {
  HaloKind kind;
  int epi;       // EP_* flavour
  bool wres;     // the 64 x 9 x C weight tile stays resident (one column tile, C <= 64)
  bool full;     // (linear) no tile ends past M: branch-free epilogue everywhere
  int nj;        // 16-column fragments per wave: 4 (64-wide column tiles), 2 (N == 32)
  int ns;        // (strip) ring stages
  int grid, threads;
  int tiles_n, tiles_total;  // for IGemmArgs
  HaloPlan lin;
  StripPlan strip;
};

// The flavours instantiated for a column-tile width: 64-wide tiles take every flavour
// halo_epi returns; the one 32-wide tile (DenseNet's growth-rate convs, Inception's
// Conv2d_2a) plain and statistics, and on strip tiles also accumulate and the BN link
inline bool halo_epi_instantiated(int epi, bool n32, bool strip) {
  if (epi < 0) return false;
  if (!n32 || epi == 0 || epi == EP_STATS) return true;
  return strip && (epi == EP_BETA || epi == EP_BNRED);
}

// TR x TW tiles of one output image (TW = W, or W split into equal strips of <= 128
// columns), the largest TR whose (TR + 2)-row halo fits the DMA count; false: no tiling
// keeps half the MFMA rows live or fits the ring
inline bool strip_plan(const IGemmArgs& a, int ch, int cw, bool wres, int tiles_n, StripPlan& h,
                       int& ns) {
  const int W = a.oW, H = a.oH;  // tiles cover the output image
  if (W < 8) return false;
  h.ch = ch;
  h.cw = cw;
  const int nstrip = (W + 127) / 128;
  const int TW = (W + nstrip - 1) / nstrip;
  int TR = std::max(1, std::min(H, HB_BM / TW));
  const int P = (TW + 2 + 7) / 8 * 8;
  while (TR > 1 && ((TR + 2) * P + 63) / 64 > HB_HIW) --TR;
  const int hiw = ((TR + 2) * P + 63) / 64;
  if (hiw > HB_HIW || 2 * TR * TW < HB_BM) return false;  // at least half the MFMA rows live
  h.tr = TR;
  h.tw = TW;
  h.p = P;
  h.hiw = hiw;
  h.tiles_c = (W + TW - 1) / TW;
  h.tiles_img = ((H + TR - 1) / TR) * h.tiles_c;
  h.cc = a.aC / 32;
  const int nimg = a.M / (H * W);  // (output pixels per image)
  const int lds = 2 * HB_HBYTES + 2 * HB_WBYTES;
  ns = 2;
  if (wres && 3 * hiw * 4096 + h.cc * HB_WBYTES <= lds) ns = 3;
  if (ns * hiw * 4096 + (wres ? h.cc : ns) * HB_WBYTES > lds) return false;
  h.mag_tw = magic(TW);
  h.mag_p = magic(P);
  h.mag_tc = h.tiles_c > 1 ? magic(h.tiles_c) : 0u;
  h.mag_timg = h.tiles_img > 1 ? magic(h.tiles_img) : 0u;
  h.tiles_total = nimg * h.tiles_img * tiles_n;
  return (int64_t)nimg * h.tiles_img < (1 << 24);
}

// Order of the decisions: (1) the launch is a dense 3x3 / stride-1 GEMM the engine can
// address, in a flavour halo_epi knows; (2) strip tiles, when the switch allows them and
// either the linear tiles cannot hold the image (wide images, shifted tap sets, a 32-wide
// flavour only the strip kernel has) or MPA_HALO_STRIP=2 gives a resident-weight layer a
// third stage; (3) else linear tiles: 448 pixels for whole-row resident-weight tiles, else
// 256; (4) the persistent grid.  B must be K-contiguous with the tap map in a.taps.bt.
inline HaloLaunch plan_halo(const IGemmArgs& a, const HaloSwitches& sw, int cus) {
  HaloLaunch L{};
  L.kind = HaloKind::None;
  if (!sw.halo || a.nphase > 0 || a.stap || a.T != 9 || a.Uh != 1 || a.Uw != 1) return L;
  if (a.aC % 32 != 0 || a.M <= 0 || a.oH <= 0 || a.oW <= 0) return L;
  const int epi = halo_epi(a);
  const bool n32 = a.N == 32;
  if ((a.N % HB_BN != 0 && !n32) || !halo_epi_instantiated(epi, n32, true)) return L;
  // dense [M][ldc] output (stride-1 geometry), 32-bit element offsets in the epilogue
  if (a.dH != a.oH || a.dW != a.oW || a.Uoh != 1 || a.Uow != 1 || a.Poh != 0 || a.Pow != 0)
    return L;
  if ((int64_t)a.M * a.ldc >= (1ll << 31) || a.ldc < a.N) return L;
  if (a.Ktot != 9 * a.aC) return L;
  int ch, cw;
  if (!tap_shift(a, ch, cw)) return L;
  const int64_t HW = (int64_t)a.aH * a.aW, OHW = (int64_t)a.oH * a.oW;
  if (a.M % OHW != 0) return L;
  const int64_t a_bytes = (int64_t)(a.M / OHW) * HW * a.aC * 2, b_bytes = (int64_t)a.N * a.ldb * 2;
  if (a_bytes >= (1ll << 31) || b_bytes >= (1ll << 31)) return L;
  // linear tiles: the same-conv tap set, images the 16-bit slot arithmetic and the pitch
  // hold, and the halo slots of any 256-pixel tile fit the stage
  const int W2 = halo_pitch(a.aW);
  const bool linear = ch == 0 && cw == 0 && HW + HB_BM < 65536 && a.aW + 2 <= 255 &&
                      halo_need(HB_BM, a.aH, a.aW, W2) <= HB_HPX &&
                      halo_epi_instantiated(epi, n32, false);
  L.epi = epi;
  L.nj = n32 ? 2 : 4;
  L.tiles_n = (a.N + HB_BN - 1) / HB_BN;
  L.wres = sw.wres && L.tiles_n == 1 && a.aC / 32 <= 2;
  int btoff[9];  // raster (dh, dw) order, whatever order the table had
  for (int t = 0; t < 9; ++t)
    btoff[(a.Oh + a.taps.dh[t] - ch + 1) * 3 + (a.Ow + a.taps.dw[t] - cw + 1)] =
        a.taps.bt[t] * a.aC * 2;
  StripPlan sp{};
  int ns = 0;
  if (sw.strip >= 1 && strip_plan(a, ch, cw, L.wres, L.tiles_n, sp, ns) &&
      (!linear || (sw.strip >= 2 && ns == 3))) {
    L.kind = HaloKind::Strip;
    L.ns = ns;
    L.threads = 512;
    std::copy(btoff, btoff + 9, sp.btoff);
    sp.a_bytes = (uint32_t)a_bytes;
    sp.b_bytes = (uint32_t)b_bytes;
    L.strip = sp;
    L.tiles_total = sp.tiles_total;
  } else if (linear) {
    // 448-pixel tiles (MI = 7): one resident 64-wide weight tile, plain or statistics
    // epilogue (the accumulate / BN-link flavours spill 92-102 B/lane at 448 pixels), tiles
    // of whole image rows that never cross an image and whose (448 / W + 2)-slot halo fits
    // the 640-pixel stage
    const bool mi7 = sw.mi7 && L.wres && a.N == HB_BN && (epi == 0 || epi == EP_STATS) &&
                     HW % HB_BM7 == 0 && HB_BM7 % a.aW == 0 && a.M % HB_BM7 == 0 &&
                     (HB_BM7 / a.aW + 2) * W2 <= HB_HPX7;
    L.kind = mi7 ? HaloKind::Linear448 : HaloKind::Linear256;
    L.full = mi7 || a.M % HB_BM == 0;
    L.threads = mi7 ? 256 : 512;
    HaloPlan& h = L.lin;
    h.w2 = W2;
    std::copy(btoff, btoff + 9, h.btoff);
    h.mag_w = magic(a.aW);
    h.mag_w2 = magic(W2);
    h.mag_h1 = magic(a.aH + 1);
    h.mag_hw = magic(a.aH * a.aW);
    h.cc = a.aC / 32;
    h.hiw = halo_dma_count(halo_need(HB_BM, a.aH, a.aW, W2), HB_HIW, sw.trim);
    h.tiles_m = mi7 ? a.M / HB_BM7 : (a.M + HB_BM - 1) / HB_BM;
    h.tiles_total = h.tiles_m * L.tiles_n;
    h.a_bytes = (uint32_t)a_bytes;
    h.b_bytes = (uint32_t)b_bytes;
    L.tiles_total = h.tiles_total;
  } else {
    return L;
  }
  L.grid = halo_grid(cus, L.tiles_total, L.tiles_n);
  return L;
}

// ------------------------------------------------------------------------ weight gradient
enum class HaloWKind { None, Linear, OneChunk, Strip };

// One instance of conv3_halo_wgrad_kernel<w2t, kind == OneChunk, kind == Strip, prod, km,
// ht>, its grid and block, and its plan struct
struct HaloWLaunch {
  HaloWKind kind;
  bool prod;    // producer-wave (8-wave) block: linear and one-chunk tiles under MPA_HALO_WPROD
  int km;       // 16-row k fragments per partition: 4; 2 when Kout == 32 (producer form only)
  int w2t;      // compile-time pitch of the 4-wave linear tiles (16 / 32 / 48 / 64), else 0
  int ht;       // halo DMAs per wave and chunk: geometry-sized where instantiated, else 7
  int grid, threads;
  HaloWPlan plan;
};

// strip tiling of the weight gradient (images too wide for the linear tiles): the TR x TW
// tile (TR * TW <= 128 pixels) minimising tiles x (128 MFMA rows + staged halo pixels)
inline bool halo_wgrad_strip_plan(const WGradArgs& a, HaloWPlan& h) {
  const int OH = a.P, OW = a.Q;  // tiles cover dy (the conv output)
  const int64_t nimg = a.Mpix / ((int64_t)OH * OW);
  int64_t best = -1;
  for (int n = 1; n <= OW; ++n) {
    const int tw = (OW + n - 1) / n;
    if (tw > 126 || (n > 1 && (OW + tw - 1) / tw != n)) continue;
    if (tw < 8) break;
    const int pitch = (tw + 2 + 15) / 16 * 16;
    int tr = std::max(1, std::min(OH, HW_BM / tw));
    while (tr > 1 && (tr + 2) * pitch > HW_HPX) --tr;
    if ((tr + 2) * pitch > HW_HPX) continue;
    const int64_t tiles = nimg * ((OH + tr - 1) / tr) * n;
    const int64_t cost = tiles * (HW_BM + (tr + 2) * pitch);
    if (best < 0 || cost < best) {
      best = cost;
      h.tr = tr;
      h.tw = tw;
      h.w2 = pitch;
      h.tiles_c = n;
      h.tiles_img = ((OH + tr - 1) / tr) * n;
      h.tiles_m = (int)tiles;
    }
  }
  if (best < 0 || h.tiles_m <= 0) return false;
  h.mag_tw = magic(h.tw);
  h.mag_tc = h.tiles_c > 1 ? magic(h.tiles_c) : 0u;
  h.mag_timg = h.tiles_img > 1 ? magic(h.tiles_img) : 0u;
  return true;
}

// Order of the decisions: (1) a 3x3 / stride-1 conv with pad 0 or 1 whose operands the
// engine can address; (2) linear 128-pixel tiles for same convs whose halo fits a chunk's
// stage - or both chunk areas, when the partition has one 32-channel chunk (OneChunk);
// (3) else strip tiles, when the switch allows them (pad 0: its dy is the smaller image);
// (4) the form: producer waves for linear and one-chunk tiles under MPA_HALO_WPROD, else
// 4-wave blocks with the pitch and the geometry-sized DMA count where instantiated;
// (5) Z blocks per 64 x 64 partition out of the CUs.
inline HaloWLaunch plan_halo_wgrad(const WGradArgs& a, const HaloSwitches& sw, int cus) {
  HaloWLaunch L{};
  L.kind = HaloWKind::None;
  if (!sw.halo || a.R != 3 || a.S != 3 || a.sh != 1 || a.sw != 1) return L;
  if (a.ph < 0 || a.ph > 1 || a.pw < 0 || a.pw > 1) return L;
  if (a.P != a.H + 2 * a.ph - 2 || a.Q != a.W + 2 * a.pw - 2 || a.P <= 0 || a.Q <= 0) return L;
  // 64 x 64 partitions; a 32-wide remainder in either dimension is zero-filled
  if (a.C % 32 != 0 || a.Kout % 32 != 0) return L;
  const int64_t PQ = (int64_t)a.P * a.Q;
  if (a.Mpix % PQ != 0) return L;
  const int64_t x_bytes = a.Mpix / PQ * a.H * a.W * a.C * 2;
  const int64_t dy_bytes = (int64_t)a.Mpix * a.Kout * 2;
  if (x_bytes >= (1ll << 31) || dy_bytes >= (1ll << 31)) return L;
  HaloWPlan& h = L.plan;
  const int64_t need = halo_need(HW_BM, a.H, a.W, halo_wgrad_pitch(a.W));
  if (a.ph == 1 && a.pw == 1 && (int64_t)a.H * a.W + HW_BM < 65536 && a.W + 2 <= 255 &&
      need <= (a.C == 32 ? 2 : 1) * HW_HPX) {
    L.kind = need > HW_HPX ? HaloWKind::OneChunk : HaloWKind::Linear;
    h.w2 = halo_wgrad_pitch(a.W);
    h.mag_w = magic(a.W);
    h.mag_h1 = magic(a.H + 1);
    h.mag_hw = magic(a.H * a.W);
    h.tiles_m = (a.Mpix + HW_BM - 1) / HW_BM;
  } else if (sw.strip >= 1 && halo_wgrad_strip_plan(a, h)) {
    L.kind = HaloWKind::Strip;
  } else {
    return L;
  }
  for (int t = 0; t < 9; ++t) h.toff[t] = (t / 3 - 1) * h.w2 + (t % 3 - 1);
  h.mag_w2 = magic(h.w2);
  h.kparts = (a.Kout + 63) / 64;
  h.parts = h.kparts * ((a.C + 63) / 64);
  h.Z = std::max(1, std::min(std::min(cus, HALO_MAX_ROWS) / h.parts, h.tiles_m));
  h.dy_bytes = (uint32_t)dy_bytes;
  h.x_bytes = (uint32_t)x_bytes;
  L.grid = h.parts * h.Z;
  h.xmap = sw.wxmap && L.grid % 8 == 0;
  // (8-wave forms use the run-time pitch: with a compile-time pitch the MFMA waves' hoisted
  // tap addresses spill past their 256 registers)
  L.prod = sw.wprod && L.kind != HaloWKind::Strip;
  L.threads = L.prod ? 512 : 256;
  L.km = L.prod && a.Kout == 32 ? 2 : 4;
  const bool rr = L.kind == HaloWKind::Linear && !L.prod;  // the 4-wave linear form
  L.w2t = rr && h.w2 <= 64 ? h.w2 : 0;
  L.ht = rr ? halo_wgrad_dma_count(a.H, a.W, sw.trim) : HW_HIW;
  return L;
}

}  // namespace mpa
