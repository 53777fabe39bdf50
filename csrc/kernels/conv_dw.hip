// Depthwise convolution for gfx950: forward (with the BN statistics of the stored output from
// the epilogue), input gradient and weight gradient.  NHWC bf16, C % 8 == 0, k in {3, 5, 7},
// stride in {1, 2} (7 x 7: stride 1), padding k / 2, weight stored [C][k][k] (layers.Conv2d groups == C).
//
// A depthwise conv does k^2 MACs per loaded element: it is bound by memory and LDS, and an
// MFMA formulation would be block-diagonal (1/16 of the array busy).  So these are VALU
// kernels built around data movement (plan: dw_plan.h):
//
//  * a lane owns one 16-B vector (8 channels) of a pixel, adjacent lanes adjacent vectors:
//    every global access is a coalesced 16-B access along C;
//  * a block owns cvb channel vectors x a th x tw tile of output pixels of one image and
//    stages the source tile it reads once in LDS ([rows][pitch] 16-B slots, zero outside the
//    image), so no tap touches global memory and no border test is left in the tap loops;
//  * the chunk's weights ([cvb * 8][k^2] bf16, one contiguous global range) are transposed
//    into LDS as [tap][cvb * 8], so a lane reads its 8 channels of a tap as one 16-B word and
//    weights stay packed (4 VGPRs per tap) until they are used;
//  * forward / dgrad: a thread computes DW_STRIP = 4 adjacent output columns; per tap row it
//    loads the (DW_STRIP - 1) s + k source vectors once into a register window that the four
//    outputs slide over (13 LDS reads per 20 taps x 4 outputs at k = 5, s = 1);
//  * reductions (statistics, weight gradient) go block -> slab row -> fixed-order sum: no
//    float atomics, bitwise repeatable.
#include "api.h"
#include "common.h"
#include "dw_plan.h"

namespace mpa {
namespace {

struct DwArgs {
  const bf16_t* src;    // staged tensor [N][SH][SW][C]: x (fwd, wgrad) / dy (dgrad)
  const bf16_t* src2;   // wgrad: dy [N][OH][OW][C]
  const bf16_t* w;      // [C][k * k]
  bf16_t* dst;          // fwd z / dgrad dx [N][OH][OW][C]
  const bf16_t* accum;  // dgrad: added in fp32 before the one rounding (may alias dst)
  float* slab;          // fwd statistics [rows][2 C] / wgrad partials [rows][C k k]
  const float* shift;   // fwd statistics shift [C] or null
  int N, C, CV;
  int OH, OW, SH, SW;
  int th, tw, tiles_w, tiles;
  int cvb, chunks, sh_t, sw_t, pitch, imgs;
};

// A tap row's LDS reads stay inside that row: without the fence the compiler hoists the
// strip-invariant weights out of the strip loop as unpacked fp32 (25 taps x 8 channels = 200
// VGPRs at k = 5, which spills), and loads every row's window up front.  Fenced, a row holds
// its window, one packed tap and the 32 accumulators.
#define DW_ROW_FENCE() asm volatile("" ::: "memory")

__device__ __forceinline__ void fma8(float* acc, const uint4& x, const float* wf) {
  float xf[8];
  unpack8(x, xf);
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = fmaf(xf[j], wf[j], acc[j]);
}

// LDS tile [rows][pitch] <- src[n][y0 .. y0 + rows)[x0 .. x0 + cols)[chunk], zero outside
// the image and past the last channel vector; adjacent lanes copy adjacent 16-B vectors
__device__ __forceinline__ void stage_tile(uint4* lds, const bf16_t* __restrict__ src, int n,
                                           int y0, int x0, int SH, int SW, int C, int c0v, int CV,
                                           int rows, int cols, int cvb, int pitch) {
  const int per_row = cols * cvb;
  for (int e = threadIdx.x; e < rows * per_row; e += DW_THREADS) {
    const int ly = e / per_row, rem = e - ly * per_row;
    const int lx = rem / cvb, cv = rem - lx * cvb;
    const int gy = y0 + ly, gx = x0 + lx;
    uint4 v = make_uint4(0, 0, 0, 0);
    if ((unsigned)gy < (unsigned)SH && (unsigned)gx < (unsigned)SW && c0v + cv < CV)
      v = *(const uint4*)(src + (((size_t)n * SH + gy) * SW + gx) * C + (size_t)(c0v + cv) * 8);
    lds[ly * pitch + lx * cvb + cv] = v;
  }
}

// wl[tap][cvb * 8] <- w[c0 .. c0 + cvb * 8)[tap] (flip: tap k^2 - 1 - t, the stride-1 dgrad)
template <int KK, bool FLIP>
__device__ __forceinline__ void stage_weights(bf16_t* wl, const bf16_t* __restrict__ w, int C,
                                              int c0v, int cvb) {
  const int c0 = c0v * 8, cw = cvb * 8;
  for (int e = threadIdx.x; e < cw * KK; e += DW_THREADS) {
    const int cl = e / KK, t = e - cl * KK;
    const bf16_t v = (c0 + cl < C) ? w[(size_t)(c0 + cl) * KK + t] : (bf16_t)0;
    wl[(FLIP ? KK - 1 - t : t) * cw + cl] = v;
  }
}

// Forward (DG = false) and input gradient (DG = true) of one tile.
//  fwd:        z[oh][ow]  = sum_{r,t} x[oh S + r - p][ow S + t - p] w[r][t]
//  dgrad S=1:  dx[h][w]   = sum_{r,t} dy[h + r - p][w + t - p] w[k-1-r][k-1-t]  (taps flipped
//              while staging, so the loop is the forward's)
//  dgrad S=2:  dx[h][w]   = sum over the taps with h + p - r and w + p - t even of
//              dy[(h + p - r) / 2][(w + p - t) / 2] w[r][t]: tile origins are even, so a
//              strip's column parities are compile-time and a row's tap parity is (row + p) & 1
template <int K, int S, bool DG>
__global__ __launch_bounds__(DW_THREADS) void dw_conv_kernel(DwArgs a) {
  extern __shared__ uint4 smem[];
  constexpr int KK = K * K, PAD = K / 2;
  constexpr bool GATHER = DG && S == 2;
  constexpr int SE = DG ? 1 : S;                       // source step per output pixel
  constexpr int NX = GATHER ? 4 : (DW_STRIP - 1) * SE + K;  // register window per tap row
  uint4* xs = smem;
  bf16_t* wl = (bf16_t*)(smem + a.sh_t * a.pitch);
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int tile = b % a.tiles;
  b /= a.tiles;
  const int chunk = b % a.chunks, n = b / a.chunks;
  const int oh0 = (tile / a.tiles_w) * a.th, ow0 = (tile % a.tiles_w) * a.tw;
  const int c0v = chunk * a.cvb, cvb = a.cvb, pitch = a.pitch;
  const int y0 = GATHER ? oh0 / 2 - 1 : oh0 * SE - PAD;
  const int x0 = GATHER ? ow0 / 2 - 1 : ow0 * SE - PAD;
  stage_tile(xs, a.src, n, y0, x0, a.SH, a.SW, a.C, c0v, a.CV, a.sh_t, a.sw_t, cvb, pitch);
  stage_weights<KK, DG && S == 1>(wl, a.w, a.C, c0v, cvb);
  __syncthreads();

  const int cv = tid % cvb, slot = tid / cvb, nslots = DW_THREADS / cvb;
  const bool on = slot < nslots && c0v + cv < a.CV;
  const int nstrips = a.th * (a.tw / DW_STRIP);
  const size_t cofs = (size_t)(c0v + cv) * 8;
  float st[16], sft[8];
#pragma unroll
  for (int j = 0; j < 16; ++j) st[j] = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) sft[j] = (!DG && on && a.shift) ? a.shift[cofs + j] : 0.f;

  if (on) {
    // adjacent slots take adjacent tile rows of one strip column (dw_pitch's bank layout)
    for (int si = slot; si < nstrips; si += nslots) {
      const int row = si % a.th, col4 = si / a.th;
      const int oh = oh0 + row, ow = ow0 + col4 * DW_STRIP;
      if (oh >= a.OH || ow >= a.OW) continue;
      float acc[DW_STRIP][8];
#pragma unroll
      for (int o = 0; o < DW_STRIP; ++o)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[o][j] = 0.f;
      if constexpr (!GATHER) {
        const uint4* xb = xs + (row * SE) * pitch + (col4 * DW_STRIP * SE) * cvb + cv;
#pragma unroll 1
        for (int r = 0; r < K; ++r) {
          DW_ROW_FENCE();
          uint4 xv[NX];
#pragma unroll
          for (int j = 0; j < NX; ++j) xv[j] = xb[r * pitch + j * cvb];
#pragma unroll
          for (int t = 0; t < K; ++t) {
            float wf[8];
            unpack8(*(const uint4*)(wl + ((r * K + t) * cvb + cv) * 8), wf);
#pragma unroll
            for (int o = 0; o < DW_STRIP; ++o) fma8(acc[o], xv[o * SE + t], wf);
          }
        }
      } else {
        const int rp = (row + PAD) & 1;
        const uint4* xb = xs + (col4 * 2) * cvb + cv;
#pragma unroll 1
        for (int i = 0; i < (K + 1) / 2; ++i) {
          const int r = rp + 2 * i;
          if (r < K) {
            DW_ROW_FENCE();
            const int lr = ((row + PAD - r) >> 1) + 1;
            uint4 xv[NX];
#pragma unroll
            for (int j = 0; j < NX; ++j) xv[j] = xb[lr * pitch + j * cvb];
#pragma unroll
            for (int t = 0; t < K; ++t) {
              float wf[8];
              unpack8(*(const uint4*)(wl + ((r * K + t) * cvb + cv) * 8), wf);
#pragma unroll
              for (int o = 0; o < DW_STRIP; ++o)
                if (((o + PAD - t) & 1) == 0) fma8(acc[o], xv[(o + PAD - t) / 2 + 1], wf);
            }
          }
        }
      }
      const size_t base = (((size_t)n * a.OH + oh) * a.OW + ow) * a.C + cofs;
#pragma unroll
      for (int o = 0; o < DW_STRIP; ++o) {
        if (ow + o >= a.OW) break;
        bf16_t* p = a.dst + base + (size_t)o * a.C;
        if (DG && a.accum) {  // fp32 sum, one rounding
          float pf[8];
          unpack8(*(const uint4*)(a.accum + base + (size_t)o * a.C), pf);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[o][j] += pf[j];
        }
        const uint4 v = pack8(acc[o]);
        *(uint4*)p = v;
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
    }
  }

  if (!DG && a.slab) {
    // block reduction in slot order through LDS, then one slab row (n, tile) per block:
    // columns [0, C) shifted sums, [C, 2C) shifted sums of squares
    __syncthreads();
    float* red = (float*)smem;
#pragma unroll
    for (int j = 0; j < 16; ++j) red[tid * 16 + j] = st[j];
    __syncthreads();
    if (tid < cvb * 16) {
      const int v = tid >> 4, j = tid & 15;
      float s = 0.f;
      for (int q = 0; q < nslots; ++q) s += red[(q * cvb + v) * 16 + j];
      if (c0v + v < a.CV) {
        const int c = (c0v + v) * 8 + (j & 7);
        a.slab[((size_t)n * a.tiles + tile) * (2 * a.C) + (j < 8 ? c : a.C + c)] = s;
      }
    }
  }
}

// Weight gradient: dw[c][r][t] = sum_{n,p,q} dy[n][p][q][c] x[n][p S + r - pad][q S + t - pad][c].
// A block owns cvb channel vectors x a th x tw tile of dy pixels x `imgs` images; per image it
// stages the x halo tile and the dy tile (both zero outside the image, so the loops carry no
// border test).  Thread (vector, tap row r, slot) keeps the k x 8 accumulators of its tap row
// and walks the slot's dy pixels; the slots are summed through LDS in slot order and the
// block writes one partial row [cvb * 8][k * k] of the slab.
template <int K, int S>
__global__ __launch_bounds__(DW_THREADS) void dw_wgrad_kernel(DwArgs a) {
  extern __shared__ uint4 smem[];
  constexpr int KK = K * K, PAD = K / 2;
  uint4* xs = smem;
  uint4* ds = smem + a.sh_t * a.pitch;
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int tile = b % a.tiles;
  b /= a.tiles;
  const int chunk = b % a.chunks, slice = b / a.chunks;
  const int oh0 = (tile / a.tiles_w) * a.th, ow0 = (tile % a.tiles_w) * a.tw;
  const int c0v = chunk * a.cvb, cvb = a.cvb, pitch = a.pitch;
  const int cv = tid % cvb, r = (tid / cvb) % K, slot = tid / (cvb * K);
  const int nslots = DW_THREADS / (cvb * K);
  const bool on = slot < nslots;
  const int npix = a.th * a.tw;
  float acc[K][8];
#pragma unroll
  for (int t = 0; t < K; ++t)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[t][j] = 0.f;

  const int n1 = min(a.N, (slice + 1) * a.imgs);
  for (int n = slice * a.imgs; n < n1; ++n) {
    __syncthreads();  // the previous image's readers are done
    stage_tile(xs, a.src, n, oh0 * S - PAD, ow0 * S - PAD, a.SH, a.SW, a.C, c0v, a.CV, a.sh_t,
               a.sw_t, cvb, pitch);
    stage_tile(ds, a.src2, n, oh0, ow0, a.OH, a.OW, a.C, c0v, a.CV, a.th, a.tw, cvb,
               a.tw * cvb);
    __syncthreads();
    if (on) {
      for (int pix = slot; pix < npix; pix += nslots) {
        const int py = pix / a.tw, px = pix - py * a.tw;
        float df[8];
        unpack8(ds[pix * cvb + cv], df);
        const uint4* xb = xs + (py * S + r) * pitch + (px * S) * cvb + cv;
#pragma unroll
        for (int t = 0; t < K; ++t) fma8(acc[t], xb[t * cvb], df);
      }
    }
  }

  __syncthreads();
  float* red = (float*)smem;  // [thread][k][8]
#pragma unroll
  for (int t = 0; t < K; ++t)
#pragma unroll
    for (int j = 0; j < 8; ++j) red[tid * (K * 8) + t * 8 + j] = acc[t][j];
  __syncthreads();
  const int row = slice * a.tiles + tile;
  for (int e = tid; e < cvb * 8 * KK; e += DW_THREADS) {
    const int cl = e / KK, tap = e - cl * KK;
    const int rr = tap / K, t = tap - rr * K, v = cl >> 3, j = cl & 7;
    float s = 0.f;
    for (int q = 0; q < nslots; ++q) s += red[((q * K + rr) * cvb + v) * (K * 8) + t * 8 + j];
    const int c = c0v * 8 + cl;
    if (c < a.C) a.slab[(size_t)row * a.C * KK + (size_t)c * KK + tap] = s;
  }
}

// slab [S][W]: rows [r0, r0 + chunk) summed into row r0 (four interleaved chains, fixed order)
__global__ __launch_bounds__(256) void dw_fold_kernel(float* __restrict__ slab, int S, int W,
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
__global__ __launch_bounds__(256) void dw_final_kernel(const float* __restrict__ slab, int heads,
                                                       int rstep, int W, float* __restrict__ out,
                                                       int overwrite) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= W) return;
  float s = 0.f;
  for (int h = 0; h < heads; ++h) s += slab[(size_t)h * rstep * W + w];
  out[w] = overwrite ? s : out[w] + s;
}

DwArgs dw_args(const DwGeom& g, const DwPlan& p) {
  DwArgs a{};
  a.N = g.N;
  a.C = g.C;
  a.CV = g.C / 8;
  a.OH = p.OH; a.OW = p.OW; a.SH = p.SH; a.SW = p.SW;
  a.th = p.th; a.tw = p.tw; a.tiles_w = p.tiles_w; a.tiles = p.tiles_h * p.tiles_w;
  a.cvb = p.cvb; a.chunks = p.chunks; a.sh_t = p.sh_t; a.sw_t = p.sw_t; a.pitch = p.pitch;
  a.imgs = p.imgs;
  return a;
}

template <typename Kern>
void dw_launch(Kern kern, const DwArgs& a, const DwPlan& p, hipStream_t s) {
  static_assert(DW_LDS_BUDGET <= 64 * 1024, "dynamic LDS above 64 KiB needs the opt-in attribute");
  hipLaunchKernelGGL(kern, dim3((unsigned)p.grid), dim3(DW_THREADS), p.lds_bytes, s, a);
  MPA_CHECK_LAUNCH();
}

template <bool DG>
void dw_conv_dispatch(const DwGeom& g, const DwArgs& a, const DwPlan& p, hipStream_t s) {
  if (g.k == 3 && g.s == 1) dw_launch(dw_conv_kernel<3, 1, DG>, a, p, s);
  else if (g.k == 3) dw_launch(dw_conv_kernel<3, 2, DG>, a, p, s);
  else if (g.k == 7) dw_launch(dw_conv_kernel<7, 1, DG>, a, p, s);
  else if (g.s == 1) dw_launch(dw_conv_kernel<5, 1, DG>, a, p, s);
  else dw_launch(dw_conv_kernel<5, 2, DG>, a, p, s);
}

}  // namespace

int64_t dwconv_fwd_ws_floats(const DwGeom& g) {
  return ((int64_t)dw_plan(DW_FWD, g).rows + 1) * 2 * g.C;
}

void dwconv_fwd(const bf16_raw* x, const bf16_raw* w, const DwGeom& g, bf16_raw* z, float* stats,
                const float* shift, float* ws, hipStream_t s) {
  const DwPlan p = dw_plan(DW_FWD, g);
  DwArgs a = dw_args(g, p);
  a.src = x;
  a.w = w;
  a.dst = z;
  a.slab = stats ? ws : nullptr;
  a.shift = shift;
  dw_conv_dispatch<false>(g, a, p, s);
  if (stats)  // ws = slab [rows][2C] | sums [2C]
    slab_stats(ws, p.rows, g.C, shift, g.N * p.OH * p.OW, ws + (size_t)p.rows * 2 * g.C, stats, s);
}

void dwconv_dgrad(const bf16_raw* dy, const bf16_raw* w, const DwGeom& g, bf16_raw* dx,
                  const bf16_raw* accum, hipStream_t s) {
  const DwPlan p = dw_plan(DW_DGRAD, g);
  DwArgs a = dw_args(g, p);
  a.src = dy;
  a.w = w;
  a.dst = dx;
  a.accum = accum;
  dw_conv_dispatch<true>(g, a, p, s);
}

int64_t dwconv_wgrad_ws_floats(const DwGeom& g) {
  return (int64_t)dw_plan(DW_WGRAD, g).rows * g.C * g.k * g.k;
}

void dwconv_wgrad(const bf16_raw* dy, const bf16_raw* x, const DwGeom& g, float* dw,
                  bool overwrite, float* ws, hipStream_t s) {
  const DwPlan p = dw_plan(DW_WGRAD, g);
  DwArgs a = dw_args(g, p);
  a.src = x;
  a.src2 = dy;
  a.slab = ws;
  if (g.k == 3 && g.s == 1) dw_launch(dw_wgrad_kernel<3, 1>, a, p, s);
  else if (g.k == 3) dw_launch(dw_wgrad_kernel<3, 2>, a, p, s);
  else if (g.k == 7) dw_launch(dw_wgrad_kernel<7, 1>, a, p, s);
  else if (g.s == 1) dw_launch(dw_wgrad_kernel<5, 1>, a, p, s);
  else dw_launch(dw_wgrad_kernel<5, 2>, a, p, s);
  const int W = g.C * g.k * g.k;
  const int chunk = dw_fold_chunk(p.rows);
  const int heads = (p.rows + chunk - 1) / chunk;
  if (chunk > 1)
    hipLaunchKernelGGL(dw_fold_kernel, dim3((W + 255) / 256, heads), dim3(256), 0, s, ws, p.rows,
                       W, chunk);
  hipLaunchKernelGGL(dw_final_kernel, dim3((W + 255) / 256), dim3(256), 0, s, ws, heads, chunk, W,
                     dw, overwrite ? 1 : 0);
  MPA_CHECK_LAUNCH();
}

}  // namespace mpa
