// Grouped 3x3 convolution for gfx950 on v_mfma_f32_16x16x32_bf16: forward (with the BN
// statistics of the stored output from the epilogue), input gradient and weight gradient.
// NHWC bf16, cin == cout == C, C % 16 == 0, Cg = C / groups in {4, 8, 16, 32}, padding 1,
// stride 1 or 2, weight stored [C][3][3][Cg] (layers.Conv2d groups).  Plan: gconv_plan.h.
//
// The packing is slab-diagonal.  A slab is 16 adjacent channels; with Cg dividing 16 the 16
// output channels of a slab read exactly its 16 input channels, so one MFMA computes 16
// pixels x one slab with K = 32 = two taps x 16 channels:
//
//   weights  A[i][k]: i = output channel of the slab, k = 16 * (tap of the pair) + input
//            channel; lane (i, q = lane / 16) holds k = 8 q .. 8 q + 7, that is tap q / 2 and
//            the channel half q % 2.  The slab's compact weight is expanded to the dense
//            16 x 16 per tap (zeros where the input channel's group is not the output
//            channel's) while the fragment is built, in registers, never in memory.
//   pixels   B[k][j]: j = pixel; the lane's operand is one 16-B ds_read_b128 of pixel
//            j * stride + tap offset from the LDS halo tile.
//   output   D[i][j]: a lane holds 4 adjacent channels of one pixel.  Two pixel groups are
//            exchanged between the lane pairs (q, q ^ 1) so every lane stores 16 B.
//
// Nine taps are four two-tap MFMAs and one whose upper K half is zero in the weights (its
// pixel operand re-reads tap 8).  Cg = 32: a slab reads its group's 32 channels, K = 32 is
// one tap, nine dense MFMAs; the two slabs of a group read the same staged vectors.
//
// A block is four waves, wave w owns slab 4 * chunk + w of a th x tw pixel tile of one image.
// The block stages the source tile once (zero outside the image: no tap tests a border); a
// wave builds its slab's weight fragments once and keeps them in registers.  Reductions
// (statistics, weight gradient) go block -> slab row -> fixed-order sum: no float atomics.
#include <type_traits>

#include "api.h"
#include "common.h"
#include "gconv_plan.h"

namespace mpa {
namespace {

struct GcArgs {
  const bf16_t* src;    // staged tensor [N][SH][SW][C]: x (fwd, wgrad) / dy (dgrad)
  const bf16_t* src2;   // wgrad: dy [N][OH][OW][C]
  const bf16_t* w;      // [C][9][Cg]
  bf16_t* dst;          // fwd z / dgrad dx [N][OH][OW][C]
  float* slab;          // fwd statistics [rows][2 C] / wgrad partials [rows][C 9 Cg]
  const float* shift;   // fwd statistics shift [C] or null
  int N, C, slabs;
  int OH, OW, SH, SW;
  int th, tw, tiles_w, tiles;
  int chunks, sh_t, sw_t, hc, dy_off, imgs;
};

enum { GC_CONV = 0, GC_FLIP = 1, GC_GATHER = 2 };  // forward / stride-1 dgrad / stride-2 dgrad

// Tap order of the fragments.  Cg <= 16: fragment m holds taps seq[2 m] (K half 0) and
// seq[2 m + 1] (K half 1), -1 = zero half.  The gather order keeps each output parity's taps
// together: (even row, even column) tap 4; (even, odd) 3 5; (odd, even) 1 7; (odd, odd) 0 2 6 8.
__device__ constexpr int gc_seq(bool gather, int j) {
  const int conv[10] = {0, 1, 2, 3, 4, 5, 6, 7, 8, -1};
  const int gat[10] = {4, -1, 3, 5, 1, 7, 0, 2, 6, 8};
  return gather ? gat[j] : conv[j];
}
// Cg == 32: fragment m is one tap
__device__ constexpr int gc_tap32(bool gather, int m) {
  const int gat[9] = {4, 3, 5, 1, 7, 0, 2, 6, 8};
  return gather ? gat[m] : m;
}

// LDS tile [rows][cols] pixels of GC_PIX_SLOTS slots <- src[n][y0 ..][x0 ..][c0 .. c0 + 64),
// zero outside the image and past C; adjacent lanes copy adjacent 16-B vectors (128 B per
// pixel).  SPLIT: column x at position gc_pos(x) (even columns first).
template <bool SPLIT>
__device__ __forceinline__ void gc_stage(uint4* lds, const bf16_t* __restrict__ src, int n, int y0,
                                         int x0, int SH, int SW, int C, int c0, int rows,
                                         int cols, int hc) {
  const int per_row = cols * 8;
  for (int e = threadIdx.x; e < rows * per_row; e += GC_THREADS) {
    const int ly = e / per_row, rem = e - ly * per_row;
    const int lx = rem >> 3, cv = rem & 7;
    const int gy = y0 + ly, gx = x0 + lx;
    uint4 v = make_uint4(0, 0, 0, 0);
    if ((unsigned)gy < (unsigned)SH && (unsigned)gx < (unsigned)SW && c0 + cv * 8 < C)
      v = *(const uint4*)(src + (((size_t)n * SH + gy) * SW + gx) * C + c0 + cv * 8);
    const int pos = SPLIT ? (lx & 1) * hc + (lx >> 1) : lx;
    lds[(ly * cols + pos) * GC_PIX_SLOTS + cv] = v;
  }
}

// One lane's 8 K elements of a slab's weight fragment for stored tap `tap` (-1: zeros).
//  forward (DG = false): row i = output channel 16 slab + i, K element = input channel
//  dgrad   (DG = true):  row i = dx (input) channel 16 slab + i, K element = dy (output) channel
template <int CG, bool DG>
__device__ __forceinline__ bf16x8 gc_wfrag(const bf16_t* __restrict__ w, int slab, int tap,
                                           int lane) {
  const int i = lane & 15, q = lane >> 4;
  s16x8 r = {0, 0, 0, 0, 0, 0, 0, 0};
  if (tap >= 0) {
    if constexpr (CG == 32) {
      const int gb = (slab * 16) & ~31;  // the group's first channel
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const size_t idx = DG ? ((size_t)(gb + 8 * q + e) * 9 + tap) * 32 + (slab * 16 + i - gb)
                              : ((size_t)(slab * 16 + i) * 9 + tap) * 32 + 8 * q + e;
        r[e] = (short)w[idx];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int o = 8 * (q & 1) + e;
        if (o / CG == i / CG) {
          const size_t idx = DG ? ((size_t)(slab * 16 + o) * 9 + tap) * CG + i % CG
                                : ((size_t)(slab * 16 + i) * 9 + tap) * CG + o % CG;
          r[e] = (short)w[idx];
        }
      }
    }
  }
  return __builtin_bit_cast(bf16x8, r);
}

__device__ __forceinline__ f32x4 gc_mfma(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// Forward (MODE GC_CONV), stride-1 dgrad (GC_FLIP: the forward's loop over dy with flipped
// taps and transposed group blocks) and stride-2 dgrad (GC_GATHER) of one tile.
//  gather: dx[h][w] = sum over the taps with h + 1 - r and w + 1 - t even of
//          dy[(h + 1 - r) / 2][(w + 1 - t) / 2] w[r][t]^T.  Tile origins are even and an MFMA's
//          16 pixels are the columns of one parity of one row, so the taps of a pixel group
//          are compile-time: 1 / 2 / 2 / 4 of them by (row, column) parity.
template <int CG, int S, int MODE>
__global__ __launch_bounds__(GC_THREADS) void gc_conv_kernel(GcArgs a) {
  extern __shared__ uint4 smem[];
  constexpr bool GATHER = MODE == GC_GATHER, DG = MODE != GC_CONV;
  constexpr int NF = CG == 32 ? 9 : 5;
  constexpr bool SPLIT = MODE == GC_CONV && S == 2;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, q = lane >> 4;
  int b = blockIdx.x;
  const int tile = b % a.tiles;
  b /= a.tiles;
  const int chunk = b % a.chunks, n = b / a.chunks;
  const int oh0 = (tile / a.tiles_w) * a.th, ow0 = (tile % a.tiles_w) * a.tw;
  const int c0 = chunk * (GC_SPB * GC_SLAB);
  const int slab = chunk * GC_SPB + wave;
  const bool active = slab < a.slabs;
  const int sw_t = a.sw_t;

  gc_stage<SPLIT>(smem, a.src, n, GATHER ? oh0 / 2 : oh0 * S - 1, GATHER ? ow0 / 2 : ow0 * S - 1,
                  a.SH, a.SW, a.C, c0, a.sh_t, sw_t, a.hc);

  // the lane's channel vector of a staged pixel, and per fragment its tap's slot offset
  const int cv = CG == 32 ? (wave & ~1) * 2 + q : wave * 2 + (q & 1);
  bf16x8 wf[NF];
  int toff[NF];
  if (active) {
#pragma unroll
    for (int m = 0; m < NF; ++m) {
      int tap, rd;  // stored tap of the weights (-1: zero half), tap whose pixel is read
      if constexpr (CG == 32) {
        tap = rd = gc_tap32(GATHER, m);
      } else {
        tap = (q >> 1) ? gc_seq(GATHER, 2 * m + 1) : gc_seq(GATHER, 2 * m);
        rd = tap < 0 ? gc_seq(GATHER, 2 * m) : tap;
      }
      const int r = rd / 3, t = rd - 3 * r;
      int px;
      if constexpr (GATHER) px = (r == 0) * sw_t + (t == 0);
      else if constexpr (SPLIT) px = r * sw_t + (t & 1) * a.hc + (t >> 1);
      else px = r * sw_t + t;
      toff[m] = px * GC_PIX_SLOTS;
      wf[m] = gc_wfrag<CG, DG>(a.w, slab, (MODE == GC_FLIP && tap >= 0) ? 8 - tap : tap, lane);
    }
  }
  __syncthreads();

  float st[16], sft[8];
#pragma unroll
  for (int j = 0; j < 16; ++j) st[j] = 0.f;
  const int cst = slab * 16 + 4 * (q & ~1);  // the 8 channels this lane stores
#pragma unroll
  for (int j = 0; j < 8; ++j) sft[j] = (!DG && active && a.shift) ? a.shift[cst + j] : 0.f;

  if (active) {
    const uint4* lb = smem + li * GC_PIX_SLOTS + cv;
    auto group = [&](const uint4* base, auto m0c, auto m1c) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int m = decltype(m0c)::value; m < decltype(m1c)::value; ++m) {
        const uint4 v = base[toff[m]];
        acc = gc_mfma(wf[m], __builtin_bit_cast(bf16x8, v), acc);
      }
      return acc;
    };
    // pixel groups A and B of one slab: lanes with even q store 8 channels of A's pixel,
    // lanes with odd q 8 channels of B's
    auto store = [&](const f32x4& fa, const f32x4& fb, int oyA, int oxA, int oyB, int oxB) {
      const uint32_t a0 = pack2(fa[0], fa[1]), a1 = pack2(fa[2], fa[3]);
      const uint32_t b0 = pack2(fb[0], fb[1]), b1 = pack2(fb[2], fb[3]);
      const bool odd = q & 1;
      const uint32_t r0 = __shfl_xor(odd ? a0 : b0, 16, 64);
      const uint32_t r1 = __shfl_xor(odd ? a1 : b1, 16, 64);
      const uint4 v = odd ? make_uint4(r0, r1, b0, b1) : make_uint4(a0, a1, r0, r1);
      const int oy = odd ? oyB : oyA, ox = odd ? oxB : oxA;
      if (oy < a.OH && ox < a.OW) {
        *(uint4*)(a.dst + (((size_t)n * a.OH + oy) * a.OW + ox) * a.C + cst) = v;
        if (!DG && a.slab) {  // statistics of the stored (rounded) output
          float zf[8];
          unpack8(v, zf);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float d = zf[j] - sft[j];
            st[j] += d;
            st[8 + j] = fmaf(d, d, st[8 + j]);
          }
        }
      }
    };
    using I0 = std::integral_constant<int, 0>;
    using IN = std::integral_constant<int, NF>;
    if constexpr (!GATHER) {
      const int rstep = S * sw_t * GC_PIX_SLOTS;
      for (int rp = 0; rp < a.th; rp += 2) {
        const f32x4 fa = group(lb + rp * rstep, I0{}, IN{});
        const f32x4 fb = group(lb + (rp + 1) * rstep, I0{}, IN{});
        store(fa, fb, oh0 + rp, ow0 + li, oh0 + rp + 1, ow0 + li);
      }
    } else {
      // fragments of the four parities: [0, E1) [E1, E2) [E2, E3) [E3, NF)
      constexpr int E1 = 1, E2 = CG == 32 ? 3 : 2, E3 = CG == 32 ? 5 : 3;
      using I1 = std::integral_constant<int, E1>;
      using I2 = std::integral_constant<int, E2>;
      using I3 = std::integral_constant<int, E3>;
      for (int rp = 0; rp < a.th; rp += 2) {
        const uint4* base = lb + (rp >> 1) * sw_t * GC_PIX_SLOTS;
        const f32x4 f00 = group(base, I0{}, I1{});
        const f32x4 f01 = group(base, I1{}, I2{});
        store(f00, f01, oh0 + rp, ow0 + 2 * li, oh0 + rp, ow0 + 2 * li + 1);
        const f32x4 f10 = group(base, I2{}, I3{});
        const f32x4 f11 = group(base, I3{}, IN{});
        store(f10, f11, oh0 + rp + 1, ow0 + 2 * li, oh0 + rp + 1, ow0 + 2 * li + 1);
      }
    }
  }

  if (!DG && a.slab) {
    // block reduction in lane order through LDS, then one slab row (n, tile) per block:
    // columns [0, C) shifted sums, [C, 2C) shifted sums of squares.  Lanes with q / 2 == h
    // hold channels 8 h .. 8 h + 7 of their wave's slab.
    __syncthreads();
    float* red = (float*)smem;
#pragma unroll
    for (int j = 0; j < 16; ++j) red[tid * 16 + j] = st[j];
    __syncthreads();
    if (tid < 128) {
      const int w = tid >> 5, kind = (tid >> 4) & 1, c = tid & 15;
      const int l0 = w * 64 + 32 * (c >> 3);
      float s = 0.f;
      for (int l = 0; l < 32; ++l) s += red[(l0 + l) * 16 + kind * 8 + (c & 7)];
      const int sl = chunk * GC_SPB + w;
      if (sl < a.slabs)
        a.slab[((size_t)n * a.tiles + tile) * (2 * a.C) + kind * a.C + sl * 16 + c] = s;
    }
  }
}

// Weight gradient.  Per slab dWdense[k][tap][c] = sum_pix dy[pix][k] x[pix * S + tap][c]: an
// MFMA whose K = 32 is pixels (two tile rows of 16).  Both operands are pixel-major in LDS
// and read with ds_read_b64_tr_b16: within 16 lanes, lane l addresses pixel l / 4 and the
// 8-B channel chunk l % 4 and receives channel l of the four pixels.  Nine accumulators per
// slab (Cg = 32: eighteen, the group's two input halves).  A block owns 4 slabs x a tile of dy
// pixels x `imgs` images, keeps the diagonal Cg x Cg blocks and writes one partial row.
template <int CG, int S>
__global__ __launch_bounds__(GC_THREADS) void gc_wgrad_kernel(GcArgs a) {
  extern __shared__ uint4 smem[];
  constexpr int NB = CG == 32 ? 2 : 1;
  constexpr bool SPLIT = S == 2;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, g = lane >> 4;
  int b = blockIdx.x;
  const int tile = b % a.tiles;
  b /= a.tiles;
  const int chunk = b % a.chunks, slice = b / a.chunks;
  const int oh0 = (tile / a.tiles_w) * a.th, ow0 = (tile % a.tiles_w) * a.tw;
  const int c0 = chunk * (GC_SPB * GC_SLAB);
  const int slab = chunk * GC_SPB + wave;
  const bool active = slab < a.slabs;
  const int sw_t = a.sw_t;
  uint4* xs = smem;
  uint4* ds = smem + a.dy_off;
  constexpr int PB = GC_PIX_SLOTS * 16;  // bytes per staged pixel

  // K element 8 g + e of a step (tile rows rp, rp + 1) is the pixel (rp + g / 2, 8 (g % 2) + e);
  // this lane addresses e = li / 4 (and + 4) and the channel chunk li % 4
  const int prow = g >> 1, pcol = 8 * (g & 1) + (li >> 2);
  const int dy_b = (prow * a.tw + pcol) * PB + wave * 32 + 8 * (li & 3);
  const int x_b = (prow * S * sw_t + pcol) * PB + (CG == 32 ? (wave & ~1) * 32 : wave * 32) +
                  8 * (li & 3);
  int xoff[9];
#pragma unroll
  for (int t9 = 0; t9 < 9; ++t9) {
    const int r = t9 / 3, t = t9 % 3;
    xoff[t9] = (SPLIT ? r * sw_t + (t & 1) * a.hc + (t >> 1) : r * sw_t + t) * PB;
  }

  f32x4 acc[NB][9];
#pragma unroll
  for (int h = 0; h < NB; ++h)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[h][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto tr8 = [&](const char* p0) {  // K elements e and e + 4: four pixels further
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, p0));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, p0 + 4 * PB));
    s16x8 r;
    r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
    r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
    return __builtin_bit_cast(bf16x8, r);
  };

  const int n1 = min(a.N, (slice + 1) * a.imgs);
  for (int n = slice * a.imgs; n < n1; ++n) {
    __syncthreads();  // the previous image's readers are done
    gc_stage<SPLIT>(xs, a.src, n, oh0 * S - 1, ow0 * S - 1, a.SH, a.SW, a.C, c0, a.sh_t, sw_t,
                    a.hc);
    gc_stage<false>(ds, a.src2, n, oh0, ow0, a.OH, a.OW, a.C, c0, a.th, a.tw, 0);
    __syncthreads();
    if (active) {
      for (int rp = 0; rp < a.th; rp += 2) {
        const bf16x8 af = tr8((const char*)ds + rp * a.tw * PB + dy_b);
        const char* xb = (const char*)xs + rp * S * sw_t * PB + x_b;
#pragma unroll
        for (int t9 = 0; t9 < 9; ++t9)
#pragma unroll
          for (int h = 0; h < NB; ++h)
            acc[h][t9] = gc_mfma(af, tr8(xb + xoff[t9] + h * 32), acc[h][t9]);
      }
    }
  }

  // D[k][c]: this lane holds dy channels k = 4 g + r of the slab and x channel c = li
  if (active) {
    const size_t wrow = (size_t)a.C * 9 * CG;
    float* out = a.slab + (size_t)(slice * a.tiles + tile) * wrow;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = 4 * g + r;
      float* ok = out + (size_t)(slab * 16 + k) * 9 * CG;
      if constexpr (CG == 32) {  // both slabs of a group see its input halves 0 and 1
#pragma unroll
        for (int h = 0; h < NB; ++h)
#pragma unroll
          for (int t9 = 0; t9 < 9; ++t9) ok[t9 * CG + 16 * h + li] = acc[h][t9][r];
      } else {
        if (li / CG == k / CG) {
#pragma unroll
          for (int t9 = 0; t9 < 9; ++t9) ok[t9 * CG + li % CG] = acc[0][t9][r];
        }
      }
    }
  }
}

// slab [S][W]: rows [r0, r0 + chunk) summed into row r0 (four interleaved chains, fixed order)
__global__ __launch_bounds__(256) void gc_fold_kernel(float* __restrict__ slab, int S, int W,
                                                      int chunk) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= W) return;
  const int r0 = blockIdx.y * chunk, r1 = min(S, r0 + chunk);
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  int r = r0;
  for (; r + 3 < r1; r += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) s[u] += slab[(size_t)(r + u) * W + w];
  }
  for (; r < r1; ++r) s[0] += slab[(size_t)r * W + w];
  slab[(size_t)r0 * W + w] = (s[0] + s[1]) + (s[2] + s[3]);
}

// out[w] (+)= the heads' sum in row order
__global__ __launch_bounds__(256) void gc_final_kernel(const float* __restrict__ slab, int heads,
                                                       int rstep, int W, float* __restrict__ out,
                                                       int overwrite) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= W) return;
  float s = 0.f;
  for (int h = 0; h < heads; ++h) s += slab[(size_t)h * rstep * W + w];
  out[w] = overwrite ? s : out[w] + s;
}

GcArgs gc_args(const GcGeom& g, const GcPlan& p) {
  GcArgs a{};
  a.N = g.N;
  a.C = g.C;
  a.slabs = p.slabs;
  a.OH = p.OH; a.OW = p.OW; a.SH = p.SH; a.SW = p.SW;
  a.th = p.th; a.tw = p.tw; a.tiles_w = p.tiles_w; a.tiles = p.tiles_h * p.tiles_w;
  a.chunks = p.chunks; a.sh_t = p.sh_t; a.sw_t = p.sw_t; a.hc = p.hc; a.dy_off = p.dy_off;
  a.imgs = p.imgs;
  return a;
}

template <typename Kern>
void gc_launch(Kern kern, const GcArgs& a, const GcPlan& p, hipStream_t s) {
  static_assert(GC_LDS_BUDGET <= 64 * 1024, "dynamic LDS above 64 KiB needs the opt-in attribute");
  hipLaunchKernelGGL(kern, dim3((unsigned)p.grid), dim3(GC_THREADS), p.lds_bytes, s, a);
  MPA_CHECK_LAUNCH();
}

template <int CG>
void gc_conv_dispatch(int kind, int stride, const GcArgs& a, const GcPlan& p, hipStream_t s) {
  if (kind == GC_FWD) {
    if (stride == 1) gc_launch(gc_conv_kernel<CG, 1, GC_CONV>, a, p, s);
    else gc_launch(gc_conv_kernel<CG, 2, GC_CONV>, a, p, s);
  } else if (kind == GC_DGRAD) {
    if (stride == 1) gc_launch(gc_conv_kernel<CG, 1, GC_FLIP>, a, p, s);
    else gc_launch(gc_conv_kernel<CG, 1, GC_GATHER>, a, p, s);
  } else {
    if (stride == 1) gc_launch(gc_wgrad_kernel<CG, 1>, a, p, s);
    else gc_launch(gc_wgrad_kernel<CG, 2>, a, p, s);
  }
}

void gc_dispatch(int kind, const GcGeom& g, const GcArgs& a, const GcPlan& p, hipStream_t s) {
  switch (p.Cg) {
    case 4: gc_conv_dispatch<4>(kind, g.s, a, p, s); break;
    case 8: gc_conv_dispatch<8>(kind, g.s, a, p, s); break;
    case 16: gc_conv_dispatch<16>(kind, g.s, a, p, s); break;
    default: gc_conv_dispatch<32>(kind, g.s, a, p, s); break;
  }
}

}  // namespace

int64_t gconv_fwd_ws_floats(const GcGeom& g) {
  return ((int64_t)gconv_plan(GC_FWD, g).rows + 1) * 2 * g.C;
}

void gconv_fwd(const bf16_raw* x, const bf16_raw* w, const GcGeom& g, bf16_raw* z, float* stats,
               const float* shift, float* ws, hipStream_t s) {
  const GcPlan p = gconv_plan(GC_FWD, g);
  GcArgs a = gc_args(g, p);
  a.src = x;
  a.w = w;
  a.dst = z;
  a.slab = stats ? ws : nullptr;
  a.shift = shift;
  gc_dispatch(GC_FWD, g, a, p, s);
  if (stats)  // ws = slab [rows][2C] | sums [2C]
    slab_stats(ws, p.rows, g.C, shift, g.N * p.OH * p.OW, ws + (size_t)p.rows * 2 * g.C, stats, s);
}

void gconv_dgrad(const bf16_raw* dy, const bf16_raw* w, const GcGeom& g, bf16_raw* dx,
                 hipStream_t s) {
  const GcPlan p = gconv_plan(GC_DGRAD, g);
  GcArgs a = gc_args(g, p);
  a.src = dy;
  a.w = w;
  a.dst = dx;
  gc_dispatch(GC_DGRAD, g, a, p, s);
}

int64_t gconv_wgrad_ws_floats(const GcGeom& g) {
  return (int64_t)gconv_plan(GC_WGRAD, g).rows * gc_wrow(g);
}

void gconv_wgrad(const bf16_raw* dy, const bf16_raw* x, const GcGeom& g, float* dw, bool overwrite,
                 float* ws, hipStream_t s) {
  const GcPlan p = gconv_plan(GC_WGRAD, g);
  GcArgs a = gc_args(g, p);
  a.src = x;
  a.src2 = dy;
  a.slab = ws;
  gc_dispatch(GC_WGRAD, g, a, p, s);
  const int W = (int)gc_wrow(g);
  const int chunk = gc_fold_chunk(p.rows);
  const int heads = (p.rows + chunk - 1) / chunk;
  if (chunk > 1)
    hipLaunchKernelGGL(gc_fold_kernel, dim3((W + 255) / 256, heads), dim3(256), 0, s, ws, p.rows,
                       W, chunk);
  hipLaunchKernelGGL(gc_final_kernel, dim3((W + 255) / 256), dim3(256), 0, s, ws, heads, chunk, W,
                     dw, overwrite ? 1 : 0);
  MPA_CHECK_LAUNCH();
}

}  // namespace mpa
