// Launch planning of the depthwise conv kernels (conv_dw.hip): tile, channel chunk, LDS
// pitch and grid of one launch.  Host-only arithmetic with no HIP types, so a CPU program
// (dw_plan_check.cpp) can include it and sweep its invariants.
//
// A block owns `cvb` channel vectors (8 channels, 16 B each) x a th x tw tile of "output"
// pixels of one image: z pixels in the forward, dx pixels in dgrad, dy pixels in the weight
// gradient.  It stages the source tile it reads (x halo / dy window) in LDS as
// [sh_t][pitch] 16-B slots, pixel-major with the chunk's vectors adjacent.
#pragma once
#include <stdint.h>

namespace mpa {

constexpr int DW_THREADS = 256;
constexpr int DW_STRIP = 4;           // adjacent output columns one thread computes (fwd / dgrad)
constexpr int DW_MAX_CVB = 8;         // channel vectors per block (128 B per pixel)
constexpr int DW_MAX_CVB7 = 6;        // 7 x 7: a 16 x 16 tile's 22 x 22 halo fits the LDS budget
constexpr int DW_LDS_BUDGET = 64 * 1024;  // two blocks per CU
constexpr int DW_FILL_BLOCKS = 512;   // prefer the smaller tile below two blocks per CU
constexpr int DW_WGRAD_BLOCKS = 2048;  // weight gradient: images are grouped above this grid

enum DwKind { DW_FWD = 0, DW_DGRAD = 1, DW_WGRAD = 2 };

struct DwGeom {
  int N, H, W, C;  // the conv's input x
  int k, s;        // kernel size (3 | 5 | 7), stride (1 | 2; 7 x 7: 1); padding k / 2
};

struct DwPlan {
  int th, tw;            // tile of output pixels (multiples of 2 and DW_STRIP)
  int OH, OW;            // extent the tiles cover (z / dx / dy)
  int SH, SW;            // extent of the staged tensor (x / dy / x)
  int tiles_h, tiles_w;
  int cvb, chunks;       // channel vectors per block, blocks along C
  int sh_t, sw_t;        // staged tile in pixels
  int pitch;             // staged row pitch in 16-B slots (>= sw_t * cvb)
  int imgs, slices;      // weight gradient: images per block, blocks along N (else 1, N)
  int rows;              // slab rows the launch writes (statistics / weight-gradient partials)
  int64_t grid;
  int lds_bytes;
};

inline int dw_out(int n, int k, int s) { return (n + 2 * (k / 2) - k) / s + 1; }

inline const char* dw_geom_error(const DwGeom& g) {
  if (g.N < 1 || g.H < 1 || g.W < 1 || g.C < 8) return "empty tensor";
  if (g.C % 8) return "channels must be a multiple of 8";
  if (g.k != 3 && g.k != 5 && g.k != 7) return "kernel size must be 3, 5 or 7";
  if (g.s != 1 && g.s != 2) return "stride must be 1 or 2";
  if (g.k == 7 && g.s != 1) return "a 7 x 7 kernel runs at stride 1 only";
  if (dw_out(g.H, g.k, g.s) < 1 || dw_out(g.W, g.k, g.s) < 1) return "empty output";
  if ((int64_t)g.N * g.H * g.W * g.C >= (int64_t)1 << 31) return "tensor too large (2^31 elements)";
  return nullptr;
}

// Staged tile extent along one axis for t output pixels.  Forward, weight gradient and the
// stride-1 dgrad (a stride-1 conv with flipped taps) read (t - 1) s + k source pixels; the
// stride-2 dgrad reads dy pixels t0 / 2 - 1 .. (t0 + t - 1 + k / 2) / 2, t / 2 + 2 of them.
inline int dw_stage(int kind, int t, int k, int s) {
  if (kind == DW_DGRAD) return s == 1 ? t + k - 1 : t / 2 + 2;
  return (t - 1) * s + k;
}

// Row pitch: adjacent lanes are adjacent channel vectors of one pixel and then the same
// column of the next tile row, rs source rows further.  With rs * pitch = cvb (mod 16) sixteen
// adjacent lanes read sixteen different 16-B slots mod 256 B: no LDS bank conflict.  Where
// that has no solution (odd cvb, even rs) cvb + 1 leaves a one-slot gap instead.
inline int dw_pitch(int sw_t, int cvb, int rs) {
  const int base = sw_t * cvb;
  for (int want = cvb; want <= cvb + 1; ++want)
    for (int pad = 0; pad < 16; ++pad)
      if ((rs * (base + pad)) % 16 == want % 16) return base + pad;
  return base;
}

inline int dw_lds_bytes(int kind, const DwPlan& p, int k) {
  const int wts = k * k * p.cvb * 16;
  int b = p.sh_t * p.pitch * 16 + wts;
  if (kind == DW_WGRAD) b = p.sh_t * p.pitch * 16 + p.th * p.tw * p.cvb * 16;
  // the block reduction that follows reuses the space: fwd statistics 16 floats per thread,
  // weight gradient k * 8 floats per thread
  const int red = DW_THREADS * (kind == DW_WGRAD ? k * 8 : 16) * 4;
  return b > red ? b : red;
}

inline DwPlan dw_plan(int kind, const DwGeom& g) {
  DwPlan p{};
  const int P = dw_out(g.H, g.k, g.s), Q = dw_out(g.W, g.k, g.s);
  const bool dg = kind == DW_DGRAD;
  p.OH = dg ? g.H : P;
  p.OW = dg ? g.W : Q;
  p.SH = dg ? P : g.H;
  p.SW = dg ? Q : g.W;
  const int cv = g.C / 8;
  // 7 x 7: at 8 vectors a 16 x 16 tile stages 22 x 22 x 128 B + 6 KiB of weights, over the
  // budget, and the 8 x 8 fallback stages 3.06 x its own pixels against 1.89 x; at 6 vectors
  // (96 channels, ConvNeXt's widths are multiples) the large tile takes 51 KiB
  const int max_cvb = g.k == 7 ? DW_MAX_CVB7 : DW_MAX_CVB;
  p.chunks = (cv + max_cvb - 1) / max_cvb;
  p.cvb = (cv + p.chunks - 1) / p.chunks;  // even split: 9 vectors run as 5 + 4, not 8 + 1
  static const int cand[2][2] = {{16, 16}, {8, 8}};
  for (int i = 0; i < 2; ++i) {
    p.th = cand[i][0];
    p.tw = cand[i][1];
    p.tiles_h = (p.OH + p.th - 1) / p.th;
    p.tiles_w = (p.OW + p.tw - 1) / p.tw;
    p.sh_t = dw_stage(kind, p.th, g.k, g.s);
    p.sw_t = dw_stage(kind, p.tw, g.k, g.s);
    p.pitch = dw_pitch(p.sw_t, p.cvb, dg ? 1 : g.s);
    p.lds_bytes = dw_lds_bytes(kind, p, g.k);
    const int64_t blocks = (int64_t)g.N * p.chunks * p.tiles_h * p.tiles_w;
    // the large tile where it fits in LDS twice per CU, still fills the device and is not
    // mostly outside the image; else the small one (one 7 x 7 image)
    if (p.lds_bytes <= DW_LDS_BUDGET && blocks >= DW_FILL_BLOCKS && p.OH > p.th / 2 &&
        p.OW > p.tw / 2)
      break;
  }
  p.imgs = 1;
  p.slices = g.N;
  if (kind == DW_WGRAD) {
    // several images per block above DW_WGRAD_BLOCKS blocks (fewer partial rows to reduce),
    // and two at least so a block's weight-independent setup is shared
    const int64_t per_img = (int64_t)p.chunks * p.tiles_h * p.tiles_w;
    int64_t imgs = (per_img * g.N + DW_WGRAD_BLOCKS - 1) / DW_WGRAD_BLOCKS;
    if (imgs < 2) imgs = 2;
    if (imgs > g.N) imgs = g.N;
    p.imgs = (int)imgs;
    p.slices = (g.N + p.imgs - 1) / p.imgs;
  }
  p.rows = p.slices * p.tiles_h * p.tiles_w;
  p.grid = (int64_t)p.rows * p.chunks;
  return p;
}

// Weight-gradient slab reduction: rows are folded in chunks of dw_fold_chunk(rows) into each
// chunk's first row (at most 64 heads), then the heads are summed.
inline int dw_fold_chunk(int rows) { return rows > 64 ? (rows + 63) / 64 : 1; }

}  // namespace mpa
