// Launch planning of the grouped 3x3 conv kernels (conv_group.hip): tile, slab chunk, LDS
// layout and grid of one launch.  Host-only arithmetic with no HIP types, so a CPU program
// (gconv_plan_check.cpp) can include it and sweep its invariants.
//
// A slab is 16 adjacent channels.  With Cg = C / groups in {4, 8, 16} dividing 16, output
// channels [16j, 16j + 16) read exactly input channels [16j, 16j + 16): the conv is
// block-diagonal in slabs and one v_mfma_f32_16x16x32_bf16 takes 16 pixels x one slab, its
// K = 32 being two taps x 16 channels.  With Cg = 32 a slab reads its group's 32 channels and
// K = 32 is one tap.
//
// A block is four waves; wave w owns slab 4 * chunk + w for a th x tw tile of "output" pixels
// of one image (z pixels in the forward, dx pixels in dgrad, dy pixels in the weight
// gradient).  An MFMA's 16 pixels are 16 adjacent tile columns of one tile row, or, in the
// stride-2 dgrad (a gather by output parity), the 16 columns of one parity of a 32-wide tile.
// The block stages the source tile it reads in LDS as [sh_t][sw_t] pixels of GC_PIX_SLOTS
// 16-B slots each: 8 channel vectors of the chunk's 64 channels and one slot of padding.
#pragma once
#include <stdint.h>

namespace mpa {

constexpr int GC_THREADS = 256;
constexpr int GC_SLAB = 16;            // channels of a slab
constexpr int GC_SPB = 4;              // slabs per block (one per wave): 64 channels, 128 B per pixel
constexpr int GC_PIX_SLOTS = 9;        // 16-B slots per staged pixel: odd, so 16 adjacent pixels
                                       // start in 16 different slots mod 16 (256 B of banks)
constexpr int GC_LDS_BUDGET = 64 * 1024;  // two blocks per CU
constexpr int GC_WGRAD_BLOCKS = 1024;  // weight gradient: images are grouped above this grid

enum GcKind { GC_FWD = 0, GC_DGRAD = 1, GC_WGRAD = 2 };

struct GcGeom {
  int N, H, W;     // the conv's input x
  int C, K;        // input / output channels
  int groups;
  int k, s;        // kernel size, stride; padding 1
};

struct GcPlan {
  int th, tw;            // tile of output pixels
  int OH, OW;            // extent the tiles cover (z / dx / dy)
  int SH, SW;            // extent of the staged tensor (x / dy / x)
  int tiles_h, tiles_w;
  int Cg, slabs, chunks; // channels per group, slabs of the tensor, blocks along C
  int gather;            // the stride-2 dgrad
  int sh_t, sw_t;        // staged tile in pixels
  int split, hc;         // stride-2 conv: columns staged even-first; hc = number of even columns
  int dy_off;            // weight gradient: 16-B slot where the staged dy tile starts
  int imgs, slices;      // weight gradient: images per block, blocks along N (else 1, N)
  int rows;              // slab rows the launch writes (statistics / weight-gradient partials)
  int64_t grid;
  int lds_bytes;
};

inline int gc_out(int n, int s) { return (n - 1) / s + 1; }  // 3x3, padding 1

inline const char* gconv_geom_error(const GcGeom& g) {
  if (g.N < 1 || g.H < 1 || g.W < 1 || g.C < 1 || g.K < 1 || g.groups < 1) return "empty tensor";
  if (g.k != 3) return "grouped conv: kernel size must be 3";
  if (g.s != 1 && g.s != 2) return "grouped conv: stride must be 1 or 2";
  if (g.C != g.K) return "grouped conv: in_channels must equal out_channels";
  if (g.C % GC_SLAB) return "grouped conv: channels must be a multiple of 16";
  if (g.C % g.groups) return "grouped conv: channels must be a multiple of groups";
  const int cg = g.C / g.groups;
  if (cg != 4 && cg != 8 && cg != 16 && cg != 32)
    return "grouped conv: channels per group must be 4, 8, 16 or 32";
  if ((int64_t)g.N * g.H * g.W * g.C >= (int64_t)1 << 31) return "tensor too large (2^31 elements)";
  return nullptr;
}

// Staged column x of a tile sits at position gc_pos(x): under stride 2 the even columns come
// first, so the 16 pixels of one tap (columns 2 i + t) are 16 adjacent positions as they are
// under stride 1, and GC_PIX_SLOTS being odd makes both free of bank conflicts.
inline int gc_pos(int x, int split, int hc) { return split ? (x & 1) * hc + (x >> 1) : x; }

inline GcPlan gconv_plan(int kind, const GcGeom& g) {
  GcPlan p{};
  const int P = gc_out(g.H, g.s), Q = gc_out(g.W, g.s);
  const bool dg = kind == GC_DGRAD;
  p.OH = dg ? g.H : P;
  p.OW = dg ? g.W : Q;
  p.SH = dg ? P : g.H;
  p.SW = dg ? Q : g.W;
  p.Cg = g.C / g.groups;
  p.slabs = g.C / GC_SLAB;
  p.chunks = (p.slabs + GC_SPB - 1) / GC_SPB;
  p.gather = dg && g.s == 2;
  p.split = !dg && g.s == 2;
  if (p.gather) {  // dx tile 8 x 32 reads dy rows h0/2 .. h0/2 + th/2, columns likewise
    p.th = 8;
    p.tw = 32;
    p.sh_t = p.th / 2 + 1;
    p.sw_t = p.tw / 2 + 1;
  } else {
    const int se = dg ? 1 : g.s;
    p.th = se == 1 ? 8 : 4;
    p.tw = 16;
    p.sh_t = (p.th - 1) * se + 3;
    p.sw_t = (p.tw - 1) * se + 3;
  }
  p.hc = (p.sw_t + 1) / 2;
  p.tiles_h = (p.OH + p.th - 1) / p.th;
  p.tiles_w = (p.OW + p.tw - 1) / p.tw;
  const int src_slots = p.sh_t * p.sw_t * GC_PIX_SLOTS;
  p.dy_off = src_slots;
  int slots = src_slots;
  if (kind == GC_WGRAD) slots += p.th * p.tw * GC_PIX_SLOTS;
  p.lds_bytes = slots * 16;
  // the forward's statistics reduction reuses the space: 16 floats per thread
  if (kind == GC_FWD && p.lds_bytes < GC_THREADS * 16 * 4) p.lds_bytes = GC_THREADS * 16 * 4;
  p.imgs = 1;
  p.slices = g.N;
  if (kind == GC_WGRAD) {
    const int64_t per_img = (int64_t)p.chunks * p.tiles_h * p.tiles_w;
    int64_t imgs = (per_img * g.N + GC_WGRAD_BLOCKS - 1) / GC_WGRAD_BLOCKS;
    if (imgs < 2) imgs = 2;
    if (imgs > g.N) imgs = g.N;
    p.imgs = (int)imgs;
    p.slices = (g.N + p.imgs - 1) / p.imgs;
  }
  p.rows = p.slices * p.tiles_h * p.tiles_w;
  p.grid = (int64_t)p.rows * p.chunks;
  return p;
}

// floats of one weight-gradient partial row: the stored weight [C][3][3][Cg]
inline int64_t gc_wrow(const GcGeom& g) { return (int64_t)g.C * 9 * (g.C / g.groups); }

// Weight-gradient slab reduction: rows are folded in chunks of gc_fold_chunk(rows) into each
// chunk's first row (at most 64 heads), then the heads are summed.
inline int gc_fold_chunk(int rows) { return rows > 64 ? (rows + 63) / 64 : 1; }

}  // namespace mpa
