// Implicit-GEMM convolution / linear engine on CDNA4 MFMA (gfx950, wave64).
//
// One engine serves every GEMM-shaped op the reference reaches through ATen
// (SURVEY.md §2.7 K1/K2/K3/K9): conv forward, conv dgrad, conv wgrad and Linear
// fwd/dgrad/wgrad.  Activations are NHWC bf16, conv weights KRSC bf16, accumulation fp32
// on v_mfma_f32_16x16x32_bf16.
//
//  * fwd / dgrad kernel ("igemm_rows"): GEMM rows = output pixels (gathered im2col rows of
//    an NHWC tensor, K-contiguous), GEMM cols = output channels.  A per-launch TAP TABLE
//    (dh, dw, weight-tap) describes the gather, so one kernel covers every kernel shape
//    (7x7, 11x11, 1x7/7x1 asymmetric, 1x1) and, for dgrad, every stride phase of a strided
//    conv (sub-pixel decomposition: each output phase is a stride-1 conv over the valid
//    taps only - no zero-stuffed MFMA work).  Weights are read K-contiguous (fwd, [K][RSC])
//    or N-contiguous (dgrad: B(kk=(tap,k), n=c) = w[k][tap][c]) through the hardware
//    transpose read ds_read_b64_tr_b16 - no transposed weight copy is ever materialised.
//    Epilogue: +bias, ReLU, bf16 store of 4 consecutive channels per lane (the MFMA is
//    issued with the channel operand first so each lane owns 4 adjacent channels), and
//    per-channel BatchNorm sum / sum-of-squares reduced in-wave and added with one fp32
//    atomic per channel per wave (K4's statistics pass disappears).
//  * wgrad kernel ("igemm_wgrad"): GEMM rows = output channels, cols = (r,s,c), reduction
//    over pixels.  Both operands are pixel-major in memory, so both are staged
//    [pixel][channel] in LDS and read as MFMA fragments with ds_read_b64_tr_b16.  Split-K
//    over pixels with fp32 atomic accumulation straight into the flat gradient arena.
//
// LDS images are XOR-swizzled so fragment reads are bank-conflict free (derivation in
// docs/KERNELS.md); staging is register double-buffered: global loads for tile k+1 are in
// flight while tile k's MFMAs run, one barrier per K-step.  Blocks are remapped so tiles
// sharing an operand panel land on the same XCD (private L2).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include "igemm_common.h"
#include "halo_plan.h"

namespace mpa {

// Occupancy target (waves per SIMD) of the MFMA kernels in this file: 3 fits every tile in
// <= 168 VGPRs with no spills (accumulators move from AGPRs to VGPRs); 4 (<= 128 VGPRs)
// spills a few registers on the large tiles.
constexpr int MFMA_OCC = 3;

// ======================================================================================
//  fwd / dgrad kernel
// ======================================================================================
template <int BM, int BN, int WM, int WN, int VW, bool BKC, bool SPLIT>
__global__ __launch_bounds__(256, MFMA_OCC) void igemm_rows_kernel(IGemmArgs p) {
  constexpr int NA = BM / 64;                 // A chunks / thread
  constexpr int A_BYTES = BM * 64;
  constexpr int B_BYTES = BN * 64;
  constexpr int STAGE = A_BYTES + B_BYTES;
  constexpr int TM = BM / WM / 16;
  constexpr int TN = BN / WN / 16;
  constexpr int NB_KC = (BN * 4 + 255) / 256;  // B chunks / thread (K-contig)
  constexpr int CPR = BN / 8;                  // N-contig: chunks per k-row
  constexpr int NB_MN = (BK * CPR + 255) / 256;
  constexpr int NB = BKC ? NB_KC : NB_MN;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;

  const int tile = block_tile(p.tiles_total);
  const int mt = tile / p.tiles_n, nt = tile % p.tiles_n;
  const int m0 = mt * BM, n0 = nt * BN;

  const int ktiles = (p.Ktot + BK - 1) / BK;
  const int kbeg = block_split() * p.ktiles_per_split;
  const int kend = min(ktiles, kbeg + p.ktiles_per_split);

  // ---- per-thread A rows (fixed for the whole K loop)
  const int akc = tid & 3;
  int a_img[NA], a_bh[NA], a_bw[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int m = m0 + (tid >> 2) + 64 * i;
    if (m < p.M) {
      const int hw = p.oH * p.oW;
      const int img = (int)fdiv((uint32_t)m, p.fd_hw);
      const int r = m - img * hw;
      const int oh = (int)fdiv((uint32_t)r, p.fd_ow);
      const int ow = r - oh * p.oW;
      a_img[i] = img * p.aH * p.aW;
      a_bh[i] = oh * p.Uh + p.Oh;
      a_bw[i] = ow * p.Uw + p.Ow;
    } else {
      a_img[i] = -1;
      a_bh[i] = 0;
      a_bw[i] = 0;
    }
  }

  u32x4 ra[NA], rb[NB];

  auto load_A = [&](int kt) {
    const int kk0 = kt * BK + akc * 8;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      if constexpr (VW == 8) {
        const int t = kk0 / p.aC;
        const int c = kk0 - t * p.aC;
        bool ok = (a_img[i] >= 0) && (kk0 < p.Ktot);
        int ih = 0, iw = 0;
        if (ok) {
          ih = a_bh[i] + p.taps.dh[t];
          iw = a_bw[i] + p.taps.dw[t];
          ok = (unsigned)ih < (unsigned)p.aH && (unsigned)iw < (unsigned)p.aW;
        }
        ra[i] = ld_chunk<8>(p.A + (size_t)(a_img[i] + ih * p.aW + iw) * p.aC + c, ok ? 8 : 0);
      } else {
        constexpr int SUB = (VW == 4) ? 2 : 8;
        constexpr int SW = 8 / SUB;
        uint16_t e[8];
#pragma unroll
        for (int s = 0; s < SUB; ++s) {
          const int kk = kk0 + s * SW;
          const int t = kk / p.aC;
          const int c = kk - t * p.aC;
          bool ok = (a_img[i] >= 0) && (kk < p.Ktot);
          int ih = 0, iw = 0;
          if (ok) {
            ih = a_bh[i] + p.taps.dh[t];
            iw = a_bw[i] + p.taps.dw[t];
            ok = (unsigned)ih < (unsigned)p.aH && (unsigned)iw < (unsigned)p.aW;
          }
          const bf16_t* src = p.A + (size_t)(a_img[i] + ih * p.aW + iw) * p.aC + c;
          if constexpr (SW == 4) {
            u32x2 v = u32x2{0u, 0u};
            if (ok) v = *(const u32x2*)src;
            e[4 * s] = v.x & 0xffff; e[4 * s + 1] = v.x >> 16;
            e[4 * s + 2] = v.y & 0xffff; e[4 * s + 3] = v.y >> 16;
          } else {
            e[s] = ok ? src[0] : (uint16_t)0;
          }
        }
        ra[i] = u32x4_make(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16),
                           e[6] | (e[7] << 16));
      }
    }
  };

  auto load_B = [&](int kt) {
    if constexpr (BKC) {
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int c = tid + 256 * i;
        const int row = c >> 2, kc = c & 3;
        const int n = n0 + row;
        const int kk = kt * BK + kc * 8;
        if constexpr (VW == 1) {
          uint16_t e[8];
#pragma unroll
          for (int j = 0; j < 8; ++j)
            e[j] = (row < BN && n < p.N && kk + j < p.Ktot) ? p.B[(size_t)n * p.ldb + kk + j] : 0;
          rb[i] = u32x4_make(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16),
                             e[6] | (e[7] << 16));
        } else {
          const bool ok = (row < BN) && (n < p.N);
          int kb = kk;
          if (VW == 8 && p.b_tapmap && kk < p.Ktot) {  // weight-tap row map (dgrad, wT)
            const int t = kk / p.aC;
            kb = p.taps.bt[t] * p.aC + (kk - t * p.aC);
          }
          rb[i] = ld_chunk<VW>(p.B + (size_t)n * p.ldb + kb, ok ? nvalid(kk, p.Ktot) : 0);
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int c = tid + 256 * i;
        const int krow = c / CPR, cc = c % CPR;
        const int kk = kt * BK + krow;
        const int n = n0 + cc * 8;
        const bool ok = (krow < BK) && (kk < p.Ktot) && (n < p.N);
        int t = 0, k = 0;
        if (ok) {
          t = kk / p.aC;
          k = kk - t * p.aC;
        }
        rb[i] = ld_chunk<VW>(p.B + ((size_t)k * p.RS + p.taps.bt[t]) * p.ldb + n,
                              ok ? nvalid(n, p.N) : 0);
      }
    }
  };

  auto store_tiles = [&](char* st) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int row = (tid >> 2) + 64 * i;
      *LDS_PTR(u32x4, st + kc_off(row, akc)) = ra[i];
    }
    char* bimg = st + A_BYTES;
    if constexpr (BKC) {
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int c = tid + 256 * i;
        const int row = c >> 2, kc = c & 3;
        if (row < BN) *LDS_PTR(u32x4, bimg + kc_off(row, kc)) = rb[i];
      }
    } else {
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int c = tid + 256 * i;
        const int krow = c / CPR, cc = c % CPR;
        if (krow < BK) *LDS_PTR(u32x4, bimg + mn_off<BN>(krow, cc * 8)) = rb[i];
      }
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int wrow0 = wm * (BM / WM);
  const int wcol0 = wn * (BN / WN);

  if (kbeg < kend) {
    load_A(kbeg);
    load_B(kbeg);
    store_tiles(smem);
    __syncthreads();
    int cur = 0;
    for (int kt = kbeg; kt < kend; ++kt) {
      const bool more = kt + 1 < kend;
      if (more) {
        load_A(kt + 1);
        load_B(kt + 1);
      }
      const char* st = smem + cur * STAGE;
      const char* bimg = st + A_BYTES;
      bf16x8 af[TM], bfr[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = frag_kc(st, wrow0 + i * 16 + (lane & 15), lane);
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        if constexpr (BKC) bfr[j] = frag_kc(bimg, wcol0 + j * 16 + (lane & 15), lane);
        else bfr[j] = frag_mn<BN>(bimg, wcol0 + j * 16, lane);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mfma16(bfr[j], af[i], acc[i][j]);
      if (more) store_tiles(smem + (cur ^ 1) * STAGE);
      __syncthreads();
      cur ^= 1;
    }
  }
  rows_epilogue<BM, BN, WM, WN, SPLIT>(p, acc, smem, mt, m0, n0, wm, wrow0, wcol0, tid,
                                       RowsGeom{p.M, p.oH, p.oW, p.Poh, p.Pow, p.fd_hw, p.fd_ow});
}

// ======================================================================================
//  wgrad kernel: dW[m = kout][n = (r,s,c)] += sum_pix dy[pix][m] * im2col(x)[pix][n]
// ======================================================================================
template <int BM, int BN, int WM, int WN, int VWA, int VWB>
__global__ __launch_bounds__(256, MFMA_OCC) void igemm_wgrad_kernel(WGradArgs p) {
  constexpr int A_BYTES = BK * BM * 2;
  constexpr int B_BYTES = BK * BN * 2;
  constexpr int STAGE = A_BYTES + B_BYTES;
  constexpr int CPRA = BM / 8, CPRB = BN / 8;
  constexpr int NA = (BK * CPRA + 255) / 256;
  constexpr int NB = (BK * CPRB + 255) / 256;
  constexpr int TM = BM / WM / 16;
  constexpr int TN = BN / WN / 16;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;

  const int tile = xcd_remap(blockIdx.x, p.tiles_total);
  const int mt = tile / p.tiles_n, nt = tile % p.tiles_n;
  const int m0 = mt * BM, n0 = nt * BN;
  const int ktiles = (p.Mpix + BK - 1) / BK;
  const int kbeg = blockIdx.z * p.ktiles_per_split;
  const int kend = min(ktiles, kbeg + p.ktiles_per_split);
  if (kbeg >= kend) return;

  // ---- B column decode (fixed per thread): n -> (r, s, c)
  constexpr int NE = (VWB == 1) ? 8 : 1;
  int b_dh[NB][NE], b_dw[NB][NE], b_c[NB][NE];
  bool b_ok[NB][NE];
  // pixel iterators (incremental), one per B chunk
  int pix_img[NB], pix_oh[NB], pix_ow[NB];
  const int PQ = p.P * p.Q;
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int c = tid + 256 * i;
    const int krow = c / CPRB, cc = c % CPRB;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int n = n0 + cc * 8 + e;
      const int tap = n / p.C;
      const int ch = n - tap * p.C;
      const int r = tap / p.S, s = tap - (tap / p.S) * p.S;
      b_dh[i][e] = r - p.ph;
      b_dw[i][e] = s - p.pw;
      b_c[i][e] = ch;
      b_ok[i][e] = (krow < BK) && (n < p.Ncols);
    }
    const int pix = kbeg * BK + krow;
    const int img = pix / PQ;
    const int rr = pix - img * PQ;
    pix_img[i] = img;
    pix_oh[i] = rr / p.Q;
    pix_ow[i] = rr - (rr / p.Q) * p.Q;
  }

  u32x4 ra[NA], rb[NB];

  auto load_A = [&](int kt) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int c = tid + 256 * i;
      const int krow = c / CPRA, cc = c % CPRA;
      const int pix = kt * BK + krow;
      const int m = m0 + cc * 8;
      const bool ok = (krow < BK) && (pix < p.Mpix);
      ra[i] = ld_chunk<VWA>(p.dy + (size_t)pix * p.Kout + m, ok ? nvalid(m, p.Kout) : 0);
    }
  };

  auto load_B = [&](int kt) {
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int c = tid + 256 * i;
      const int krow = c / CPRB;
      const int pix = kt * BK + krow;
      const bool pok = (krow < BK) && (pix < p.Mpix);
      const int bh = pix_oh[i] * p.sh, bw = pix_ow[i] * p.sw;
      const size_t ibase = (size_t)pix_img[i] * p.H * p.W;
      if constexpr (VWB == 1) {
        uint16_t e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int ih = bh + b_dh[i][j], iw = bw + b_dw[i][j];
          const bool ok = pok && b_ok[i][j] && (unsigned)ih < (unsigned)p.H &&
                          (unsigned)iw < (unsigned)p.W;
          e[j] = ok ? p.x[(ibase + ih * p.W + iw) * p.C + b_c[i][j]] : (uint16_t)0;
        }
        rb[i] = u32x4_make(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16),
                           e[6] | (e[7] << 16));
      } else {
        const int ih = bh + b_dh[i][0], iw = bw + b_dw[i][0];
        const bool ok = pok && b_ok[i][0] && (unsigned)ih < (unsigned)p.H &&
                        (unsigned)iw < (unsigned)p.W;
        rb[i] = ld_chunk<VWB>(p.x + (ibase + ih * p.W + iw) * p.C + b_c[i][0], ok ? 8 : 0);
      }
      // advance this chunk's pixel by BK for the next K-step
      int ow = pix_ow[i] + BK, oh = pix_oh[i], img = pix_img[i];
      while (ow >= p.Q) { ow -= p.Q; ++oh; }
      while (oh >= p.P) { oh -= p.P; ++img; }
      pix_ow[i] = ow; pix_oh[i] = oh; pix_img[i] = img;
    }
  };

  auto store_tiles = [&](char* st) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int c = tid + 256 * i;
      const int krow = c / CPRA, cc = c % CPRA;
      if (krow < BK) *LDS_PTR(u32x4, st + mn_off<BM>(krow, cc * 8)) = ra[i];
    }
    char* bimg = st + A_BYTES;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int c = tid + 256 * i;
      const int krow = c / CPRB, cc = c % CPRB;
      if (krow < BK) *LDS_PTR(u32x4, bimg + mn_off<BN>(krow, cc * 8)) = rb[i];
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int wrow0 = wm * (BM / WM);
  const int wcol0 = wn * (BN / WN);

  load_A(kbeg);
  load_B(kbeg);
  store_tiles(smem);
  __syncthreads();
  int cur = 0;
  for (int kt = kbeg; kt < kend; ++kt) {
    const bool more = kt + 1 < kend;
    if (more) {
      load_A(kt + 1);
      load_B(kt + 1);
    }
    const char* st = smem + cur * STAGE;
    const char* bimg = st + A_BYTES;
    bf16x8 af[TM], bfr[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) af[i] = frag_mn<BM>(st, wrow0 + i * 16, lane);
#pragma unroll
    for (int j = 0; j < TN; ++j) bfr[j] = frag_mn<BN>(bimg, wcol0 + j * 16, lane);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = mfma16(bfr[j], af[i], acc[i][j]);
    if (more) store_tiles(smem + (cur ^ 1) * STAGE);
    __syncthreads();
    cur ^= 1;
  }
  wgrad_epilogue<BM, BN, WM, WN>(p, acc, m0, n0, wrow0, wcol0, lane);

}

// dw[i] += sum_z slab[z][i] (dw[i] = ... when overwrite).  A block owns 64 float4 columns; its 4 waves sum disjoint
// quarters of the splits (4 float4 loads in flight per lane), then reduce through LDS.
// With ~100 splits of a small layer (ResNet-18 layer1: 64 x 576 outputs) a
// one-thread-per-column walk over the splits ran at ~0.6 TB/s on 36 blocks.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slab, int S,
                                                            int64_t n, float* __restrict__ dw,
                                                            int overwrite) {
  __shared__ f32x4 red[4][64];
  const int64_t n4 = n / 4;
  const int64_t c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int g = threadIdx.x >> 6;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  if (c < n4) {
    const f32x4* src = (const f32x4*)slab + c;
    const int64_t stride = n4;  // one split = n4 float4
    int z = g;
    for (; z + 12 < S; z += 16) {
      const f32x4 a = src[(int64_t)z * stride], b = src[(int64_t)(z + 4) * stride];
      const f32x4 d = src[(int64_t)(z + 8) * stride], e = src[(int64_t)(z + 12) * stride];
      acc += (a + b) + (d + e);
    }
    for (; z < S; z += 4) acc += src[(int64_t)z * stride];
  }
  red[g][threadIdx.x & 63] = acc;
  __syncthreads();
  if (g == 0 && c < n4) {
    const int t = threadIdx.x;
    f32x4 v = overwrite ? f32x4{0.f, 0.f, 0.f, 0.f} : ((f32x4*)dw)[c];
    v += (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    ((f32x4*)dw)[c] = v;
  }
}

// any n (split rows not 16-B aligned when n % 4 != 0): one thread per element
__global__ __launch_bounds__(256) void wgrad_reduce_scalar_kernel(const float* __restrict__ slab,
                                                                   int S, int64_t n,
                                                                   float* __restrict__ dw,
                                                                   int overwrite) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float a = overwrite ? 0.f : dw[i];
    for (int z = 0; z < S; ++z) a += slab[(size_t)z * n + i];
    dw[i] = a;
  }
}

// ----------------------------------------------------------- split-K finalize (fp32->bf16)
// Sums the S split partials [S][M][N] (+ the existing output when beta).  A block owns CW
// columns (CW = 32 for 32-wide GEMMs, so no lane idles) and 256 / CW rows per pass, rows
// strided by gridDim.y; two rows per thread are in flight per pass (the S loads of both are
// independent).  Statistics go to the per-block-row slab [gridDim.y][2N].  (The round-2
// form, 64 columns x 4 rows per block and at most 64 block rows, left a 32-wide 12,544-row
// finalize at 59 us: 64 blocks, half their lanes idle, one dependent row at a time.)
template <int CW>
__global__ __launch_bounds__(256) void splitk_finalize_kernel(
    const float* __restrict__ ws, int S, bf16_t* __restrict__ out, int M, int N,
    const float* __restrict__ bias, int relu, float* __restrict__ slab,
    const float* __restrict__ shift, float* __restrict__ sums, int beta) {
  constexpr int RP = 256 / CW;
  __shared__ float red[2][256];
  const int n = blockIdx.x * CW + (threadIdx.x % CW);
  const int r0 = blockIdx.y * RP + threadIdx.x / CW;
  const int rstep = gridDim.y * RP;
  const size_t MN = (size_t)M * N;
  float s = 0.f, q = 0.f;
  const float b = (bias && n < N) ? bias[n] : 0.f;
  const float k = (shift && n < N) ? shift[n] : 0.f;
  auto fin = [&](int m, float v) {
    if (beta) v += bf2f(out[(size_t)m * N + n]);
    if (relu) v = fmaxf(v, 0.f);
    const bf16_t o = f2bf(v);
    out[(size_t)m * N + n] = o;
    const float rv = bf2f(o) - k;
    s += rv;
    q += rv * rv;
  };
  if (n < N) {
    int m = r0;
    for (; m + rstep < M; m += 2 * rstep) {
      float v0 = b, v1 = b;
      const float* w0 = ws + (size_t)m * N + n;
      const float* w1 = w0 + (size_t)rstep * N;
      for (int z = 0; z < S; ++z) {
        v0 += w0[z * MN];
        v1 += w1[z * MN];
      }
      fin(m, v0);
      fin(m + rstep, v1);
    }
    if (m < M) {
      float v = b;
      for (int z = 0; z < S; ++z) v += ws[z * MN + (size_t)m * N + n];
      fin(m, v);
    }
  }
  if (slab) {
    if (blockIdx.y == 0 && threadIdx.x < CW && n < N) {  // start value of the slab reduction
      sums[n] = 0.f;
      sums[N + n] = 0.f;
    }
    red[0][threadIdx.x] = s;
    red[1][threadIdx.x] = q;
    __syncthreads();
    if (threadIdx.x < CW && n < N) {
      const int t = threadIdx.x;
      float a0 = 0.f, a1 = 0.f;
#pragma unroll
      for (int r = 0; r < RP; ++r) {
        a0 += red[0][t + r * CW];
        a1 += red[1][t + r * CW];
      }
      slab[(size_t)blockIdx.y * 2 * N + n] = a0;
      slab[(size_t)blockIdx.y * 2 * N + N + n] = a1;
    }
  }
}

// ======================================================================================
//  host-side launch logic: the process's switches, the tile autotuner's state, and the
//  launch of a plan.  What runs is decided in igemm_plan.h.
// ======================================================================================
// The one GemmSwitches object.  MPA_IGEMM_ENGINE=0|1|2 sets the engine's start value (read
// at the first use), MPA_DMA_UNI=0 / MPA_KPAD=0 turn those paths off; igemm_set_engine,
// igemm_set_dma_uni and igemm_force_tile switch at run time (A/B benchmarks, cross-checking
// tests, tools/bench_kernels.py).
static bool env_on(const char* e) { return !(e && e[0] == '0'); }  // (set to 0: off)
static GemmSwitches g_sw = [] {
  GemmSwitches sw;
  sw.engine = -1;
  sw.dma_uni = env_on(getenv("MPA_DMA_UNI"));
  sw.kpad = env_on(getenv("MPA_KPAD"));
  return sw;
}();
static const GemmSwitches& switches() {
  if (g_sw.engine < 0) {
    const char* e = getenv("MPA_IGEMM_ENGINE");
    g_sw.engine = e ? std::min(2, std::max(0, atoi(e))) : 1;
  }
  return g_sw;
}
int igemm_engine() { return switches().engine; }
void igemm_set_engine(int e) { g_sw.engine = std::min(2, std::max(0, e)); }
void igemm_set_dma_uni(int on) { g_sw.dma_uni = on != 0; }
bool igemm_stap_ok() { return switches().dma_uni && switches().engine >= 1; }
void igemm_force_tile(int bm, int bn, int splits) {
  g_sw.force_bm = bm; g_sw.force_bn = bn; g_sw.force_splits = splits;
}

int64_t igemm_ws_floats(int M, int N, int Ktot) { return rows_ws_floats(M, N, Ktot, switches()); }
int64_t igemm_slab_floats(int M, int N) { return slab_floats(M, N); }
int64_t igemm_bnred_slab_floats(int M, int N, int nphase) { return bnred_slab_floats(M, N, nphase); }
int64_t igemm_wgrad_ws_floats(int Kout, int Ncols, int Mpix) {
  int64_t best = conv3_halo_wgrad_ws_floats(Kout, Ncols);
  if (Kout == 64 && Ncols == 224) best = std::max(best, stem_wgrad_ws_floats());
  return std::max(best, wgrad_gemm_ws_floats(Kout, Ncols, Mpix, switches()));
}
bool igemm_dgrad_src2_ok(const IGemmArgs& a, int vw, bool bkc) {
  return dgrad_src2_ok(a, vw, bkc, switches());
}

// ---------------------------------------------------------------------- tile autotuner
// The static plans (rows_tiling / wgrad_tiling) were fitted on a few shapes and miss by
// 10-25 % elsewhere (tools/bench_kernels.py sweep at batch 512: layer4's strided conv runs
// 24 % faster on 256x128, layer2's strided wgrad 10 % faster on 128x256, layer3's 15 %
// faster on 128x128).  Like cudnn.benchmark, the first launch of each GEMM shape on the
// LDS-DMA engine times every eligible tile on scratch outputs (a warm-up run, then 3 timed
// ones) and caches the fastest; later launches reuse it.  The sweep costs a few ms once per
// shape (the warm-up steps of a training run), is skipped while a HIP graph is being
// captured (the static plan runs then) and is off with MPA_TUNE=0.  Tiles never change a
// result's summation order except through the split-K count, which candidates may not
// raise past the caller's workspace.
static bool g_tune = env_on(getenv("MPA_TUNE"));
void igemm_set_tune(int on) { g_tune = on != 0; }
// Drain the whole device before timing a tuner candidate (single GPU: side / branch
// streams may still run kernels whose overlap would bias the choice).  Off under data
// parallelism (parallel/dist.py init_world): the drain would also wait for the overlapped
// RCCL all-reduces of the first step; the compute stream alone is synchronized then.
static bool g_tune_drain = true;
void igemm_set_tune_drain(int on) { g_tune_drain = on != 0; }

static std::mutex g_tune_mu;
static std::map<std::string, TileSize> g_tuned;
// held for a whole tuning pass (scratch growth + candidate launches + timing): a second
// host thread tuning on the same device must not free the scratch buffer that this
// thread's candidate kernels are still writing
static std::mutex g_tune_pass_mu;

static bool stream_capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}

// grow-only per-device scratch for the candidates' outputs
static char* tune_scratch(size_t bytes) {
  static char* buf[64] = {};
  static size_t cap[64] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (bytes > cap[dev]) {
    if (buf[dev]) (void)hipFree(buf[dev]);
    buf[dev] = nullptr;
    cap[dev] = 0;
    if (hipMalloc(&buf[dev], bytes) != hipSuccess) return nullptr;
    cap[dev] = bytes;
  }
  return buf[dev];
}

// Timing of one tuner candidate: the device is drained first (the first training step tunes
// while side / branch streams may still run other kernels, whose overlap would bias the
// choice - an intermittent 3x slower SqueezeNet step in round 5), then the best of two
// rounds of three launches.  Tuning only runs on a shape's first launch outside a capture.
template <class F>
static float time_launches(F&& fn, hipStream_t s) {
  if (g_tune_drain) (void)hipDeviceSynchronize();
  else (void)hipStreamSynchronize(s);
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  fn();
  float best = 1e30f;
  for (int r = 0; r < 2; ++r) {
    (void)hipEventRecord(e0, s);
    for (int i = 0; i < 3; ++i) fn();
    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    best = std::min(best, ms / 3.f);
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return best;
}

static bool tuned_lookup(const std::string& key, TileSize& t) {
  std::lock_guard<std::mutex> lock(g_tune_mu);
  auto it = g_tuned.find(key);
  if (it == g_tuned.end()) return false;
  t = it->second;
  return true;
}
static void tuned_store(const std::string& key, TileSize t) {
  std::lock_guard<std::mutex> lock(g_tune_mu);
  g_tuned[key] = t;
}

// number of tuned shapes and a readable dump ("key -> BMxBN" lines) for diagnostics
std::string igemm_tuned_table() {
  std::lock_guard<std::mutex> lock(g_tune_mu);
  std::string out;
  for (const auto& kv : g_tuned)
    out += kv.first + " -> " + std::to_string(kv.second.bm) + "x" + std::to_string(kv.second.bn) + "\n";
  return out;
}

// load a table in igemm_tuned_table()'s format ("key -> BMxBN" lines); replace: drop every
// entry first.  Data-parallel ranks adopt rank 0's table this way, so every rank runs the
// same tiles (parallel/comm.py agree_tuned_tiles).  Returns the entries loaded.
int igemm_tuned_load(const std::string& table, bool replace) {
  std::lock_guard<std::mutex> lock(g_tune_mu);
  if (replace) g_tuned.clear();
  int n = 0;
  size_t pos = 0;
  while (pos < table.size()) {
    size_t end = table.find('\n', pos);
    if (end == std::string::npos) end = table.size();
    const std::string line = table.substr(pos, end - pos);
    pos = end + 1;
    const size_t arrow = line.rfind(" -> ");
    if (arrow == std::string::npos) continue;
    int bm = 0, bn = 0;
    if (sscanf(line.c_str() + arrow + 4, "%dx%d", &bm, &bn) != 2 || bm <= 0 || bn <= 0) continue;
    g_tuned[line.substr(0, arrow)] = TileSize{bm, bn};
    ++n;
  }
  return n;
}

// The autotuned tile of the GEMM shape `make_key()` names (zeros: keep the heuristic).
// `plan(c, run)` plans candidate c on scratch outputs (tune_scratch) and fills the Run that
// `launch(run)` then launches; Skip: the candidate is not eligible (its tile does not exist
// for the launch, or its split slab would not fit the caller's workspace); Stop: no scratch
// memory - the pass is abandoned, nothing is stored and the heuristic tile runs.
enum class Cand { Skip, Stop, Ready };
struct RowsRun {
  RowsLaunch p;
  IGemmArgs a;
  float *ws, *slab;
};
struct WGradRun {
  WGradLaunch p;
  WGradArgs a;
};
template <class Run, class Key, int N, class Plan, class Launch>
static TileSize tuned_tile(Key&& make_key, const TileSize (&cands)[N], hipStream_t s, Plan&& plan,
                           Launch&& launch) {
  TileSize best_tile{0, 0};
  if (!g_tune || deterministic() || (g_sw.force_bm && g_sw.force_bn) || stream_capturing(s))
    return best_tile;
  const std::string key = make_key();
  if (tuned_lookup(key, best_tile)) return best_tile;
  std::lock_guard<std::mutex> pass(g_tune_pass_mu);
  if (tuned_lookup(key, best_tile)) return best_tile;  // tuned by another thread meanwhile
  float best = 1e30f;
  Run run{};
  for (const TileSize& c : cands) {
    const Cand r = plan(c, run);
    if (r == Cand::Stop) return TileSize{0, 0};
    if (r == Cand::Skip) continue;
    const float t = time_launches([&] { launch(run); }, s);
    if (t < best) { best = t; best_tile = c; }
  }
  if (best_tile.bm) tuned_store(key, best_tile);
  return best_tile;
}

// ------------------------------------------------------------------------ rows launches
[[noreturn]] void no_kernel(const char* what, int bm, int bn, int wm, int wn, int x, int y) {
  fprintf(stderr, "%s: no kernel for the planned tile %dx%d (%dx%d waves; %d, %d)\n", what, bm, bn,
          wm, wn, x, y);
  abort();
}

template <int BM, int BN, int WM, int WN, bool BKC, bool SPLIT>
static void launch_rows_reg(const RowsLaunch& p, const IGemmArgs& a, hipStream_t s) {
  const dim3 grid(p.grid_x, 1, p.splits), block(p.block);
  switch (p.VW) {
    case 8: hipLaunchKernelGGL((igemm_rows_kernel<BM, BN, WM, WN, 8, BKC, SPLIT>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((igemm_rows_kernel<BM, BN, WM, WN, 4, BKC, SPLIT>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((igemm_rows_kernel<BM, BN, WM, WN, 1, BKC, SPLIT>), grid, block, 0, s, a);
  }
}

template <int BM, int BN, int WM, int WN>
static void launch_rows_reg_tile(const RowsLaunch& p, const IGemmArgs& a, hipStream_t s) {
  if (p.BKC) {
    if (p.SPLIT) launch_rows_reg<BM, BN, WM, WN, true, true>(p, a, s);
    else launch_rows_reg<BM, BN, WM, WN, true, false>(p, a, s);
  } else {
    if (p.SPLIT) launch_rows_reg<BM, BN, WM, WN, false, true>(p, a, s);
    else launch_rows_reg<BM, BN, WM, WN, false, false>(p, a, s);
  }
}

// register family: the rows of kRowsRegTiles
static void igemm_rows_reg(const RowsLaunch& p, const IGemmArgs& a0, hipStream_t s) {
  IGemmArgs a = a0;
  igemm_set_fastdiv(a);
  switch (p.BM * 1000 + p.BN) {
    case 128128: launch_rows_reg_tile<128, 128, 2, 2>(p, a, s); break;
    case 256064: launch_rows_reg_tile<256, 64, 4, 1>(p, a, s); break;
    case 128032: launch_rows_reg_tile<128, 32, 4, 1>(p, a, s); break;
    default: no_kernel("igemm_rows_reg", p.BM, p.BN, p.WM, p.WN, p.VW, 0);
  }
}

// the planned kernel alone (the plan's argument fields set)
static void launch_rows_kernel(const RowsLaunch& p, IGemmArgs a, hipStream_t s) {
  p.apply(a);
  if (p.family == RowsFamily::Reg) igemm_rows_reg(p, a, s);
  else igemm_rows_dma(p, a, s);
}

// One planned rows GEMM with its follow-ups.  `a.stats` (if set) receives the finalized
// per-column statistics [mean(N), var(N)] (biased variance, from sums shifted by
// a.stats_shift); `slab` is a workspace of igemm_slab_floats(M, N) floats, its rows first,
// then the [2][N] sums; `ws` holds the split-K partials when the plan splits.
static void launch_rows(const RowsLaunch& p, IGemmArgs a, float* ws, float* slab, hipStream_t s) {
  void* final_out = a.C;
  float* stats = a.stats;
  float* sums = stats ? slab + slab_rows_max(a.M) * 2 * a.N : nullptr;
  a.stats = stats ? slab : nullptr;
  a.stats_sums = sums;
  if (p.to_ws) {
    a.C = ws;
    a.ldc = a.N;
  }
  launch_rows_kernel(p, a, s);
  if (p.fin_cw) {
    const dim3 grid(p.fin_gx, p.fin_gy);
    if (p.fin_cw == 32)
      hipLaunchKernelGGL(splitk_finalize_kernel<32>, grid, dim3(256), 0, s, ws, p.splits,
                         (bf16_t*)final_out, a.M, a.N, a.bias, a.relu,
                         stats ? slab : (float*)nullptr, a.stats_shift, sums, a.beta);
    else
      hipLaunchKernelGGL(splitk_finalize_kernel<64>, grid, dim3(256), 0, s, ws, p.splits,
                         (bf16_t*)final_out, a.M, a.N, a.bias, a.relu,
                         stats ? slab : (float*)nullptr, a.stats_shift, sums, a.beta);
  }
  if (stats) slab_stats(slab, p.slab_rows, a.N, a.stats_shift, a.M, sums, stats, s, a.stats_ld);
}

static void run_rows(IGemmArgs a, bool bkc, int vw, float* ws, float* slab, hipStream_t s) {
  const GemmSwitches& sw = switches();
  const bool dma = rows_dma(vw, sw);
  if (dma && bkc && conv_stem_ok(a)) {  // 7x7 pixel-pair stem: row-staged direct conv
    float* stats = a.stats;
    float* sums = stats ? slab + slab_rows_max(a.M) * 2 * a.N : nullptr;
    a.stats = stats ? slab : nullptr;
    const int rows = conv_stem(a, s);
    if (stats) slab_stats(slab, rows, a.N, a.stats_shift, a.M, sums, stats, s, a.stats_ld);
    return;
  }
  const HaloLaunch halo = dma && bkc ? conv3_halo_plan(a) : HaloLaunch{};
  if (halo.kind != HaloKind::None) {  // 3x3 / stride 1: halo-staged direct conv
    float* stats = a.stats;
    float* sums = stats ? slab + slab_rows_max(a.M) * 2 * a.N : nullptr;
    a.stats = stats ? slab : nullptr;
    a.stats_sums = sums;
    const int rows = conv3_halo(a, halo, s);
    if (stats) slab_stats(slab, rows, a.N, a.stats_shift, a.M, sums, stats, s, a.stats_ld);
    return;
  }
  // (a padded-K launch never splits: the caller's workspace was sized for the unpadded K)
  const int kp = rows_kpad_ktot(a, bkc, vw, sw);
  const int Ktot = kp ? kp : a.Ktot;
  if (kp) ws = nullptr;
  const bool allow_split = ws != nullptr;
  TileSize tuned{0, 0};
  if (dma && a.M > 0)
    tuned = tuned_tile<RowsRun>(
        [&] { return rows_key(a, Ktot, bkc, allow_split); }, kRowsCands, s,
        [&](TileSize c, RowsRun& r) {
          if (!rows_cand_ok(c, a.N)) return Cand::Skip;
          r.p = plan_rows(a, bkc, vw, allow_split, sw, c);
          if (r.p.BM != c.bm || r.p.BN != c.bn) return Cand::Skip;
          const int64_t ws_cap = allow_split ? rows_ws_floats(a.M, a.N, Ktot, sw) : 0;
          if (r.p.splits > 1 && (int64_t)r.p.splits * a.M * a.N > ws_cap) return Cand::Skip;
          const int64_t cbytes = ((int64_t)a.M * std::max(a.ldc, a.N) * 2 + 255) / 256 * 256;
          const int64_t sbytes = (slab_floats(a.M, a.N) + 2 * a.N) * 4;
          const int64_t wbytes = r.p.splits > 1 ? (int64_t)r.p.splits * a.M * a.N * 4 : 0;
          char* scr = tune_scratch(cbytes + sbytes + wbytes + 512);
          if (!scr) return Cand::Stop;
          r.a = a;
          r.a.C = scr;
          r.slab = (float*)(scr + cbytes);
          if (a.stats) r.a.stats = r.slab + slab_floats(a.M, a.N);  // [2][N] after the slab
          r.a.stats_ld = 0;
          r.ws = allow_split ? (float*)(scr + cbytes + sbytes) : nullptr;
          return Cand::Ready;
        },
        [&](const RowsRun& r) { launch_rows(r.p, r.a, r.ws, r.slab, s); });
  launch_rows(plan_rows(a, bkc, vw, allow_split, sw, tuned), a, ws, slab, s);
}

// `ws` holds igemm_ws_floats(M, N, Ktot) floats for the split-K partials (nullptr disables
// split-K, e.g. for strided output mappings); `slab`: see launch_rows.
void igemm_rows(IGemmArgs a, int vw, float* ws, float* slab, hipStream_t s) {
  run_rows(a, true, vw, ws, slab, s);
}

void igemm_rows_dgrad(IGemmArgs a, int vw, float* ws, hipStream_t s, bool bkc) {
  a.stats = nullptr;
  a.nphase = 0;
  run_rows(a, bkc, vw, ws, nullptr, s);
}

// dgrad + fused BN-backward reduction (LDS-DMA engine only: one launch, dense slab rows)
void igemm_rows_dgrad_bnred(IGemmArgs a, int vw, bool bkc, float* slab, float* sums,
                            hipStream_t s) {
  (void)vw;  // callers guarantee 16-B granular operands (LDS-DMA engine)
  a.bias = nullptr;
  a.relu = 0;
  a.stats_shift = nullptr;
  a.ep_bnred = 1;
  a.stats = slab;
  a.stats_sums = sums;
  if (a.nphase == 0 && bkc) {
    IGemmArgs t = a;
    if (t.ep_gamma && t.ep_beta) t.ep_y = nullptr;  // the halo kernel's z-mask form
    const HaloLaunch halo = conv3_halo_plan(t);
    if (halo.kind != HaloKind::None) {
      const int rows = conv3_halo(t, halo, s);
      slab_reduce(slab, rows, 2 * a.N, sums, false, s);
      return;
    }
  }
  const RowsLaunch p = a.nphase > 0
                           ? plan_rows_phases(a, bkc, switches(), TileSize{0, 0})
                           : plan_rows_on(a, bkc, 8, false, true, false, switches(), TileSize{0, 0});
  launch_rows_kernel(p, a, s);
  slab_reduce(slab, p.slab_rows, 2 * a.N, sums, false, s);
}

// All stride phases in ONE launch on the LDS-DMA engine: a stride-2 conv's dgrad is 4
// GEMMs of a quarter of the pixels each; launched separately each fills a fraction of the
// 256 CUs (ResNet-18 layer4 at batch 256: 196 tiles per phase), merged they fill it.
void igemm_rows_dgrad_phases(IGemmArgs a, int vw, hipStream_t s, bool bkc) {
  const GemmSwitches& sw = switches();
  a.stats = nullptr;
  a.bias = nullptr;
  if (a.nphase <= 0) return;
  if (a.A2 && !dgrad_src2_ok(a, vw, bkc, sw)) {
    fprintf(stderr, "igemm_rows_dgrad_phases: second source on an ineligible launch\n");
    abort();
  }
  if (rows_dma(vw, sw) && a.nphase <= MAXPH) {
    // the tuner times the merged launch per candidate tile
    const TileSize tuned = tuned_tile<RowsRun>(
        [&] { return rows_key(a, a.Ktot, bkc, false); }, kRowsCands, s,
        [&](TileSize c, RowsRun& r) {
          if (!rows_cand_ok(c, a.N)) return Cand::Skip;
          r.p = plan_rows_phases(a, bkc, sw, c);
          if (r.p.BM != c.bm || r.p.BN != c.bn || r.p.tiles_total <= 0) return Cand::Skip;
          const int64_t hw0 = std::max(1, a.ph[0].oH * a.ph[0].oW);
          const int64_t rows = (a.ph[0].M + hw0 - 1) / hw0 * a.dH * a.dW;  // dx pixels
          char* scr = tune_scratch(rows * std::max(a.ldc, a.N) * 2 + 256);
          if (!scr) return Cand::Stop;
          r.a = a;
          r.a.C = scr;
          return Cand::Ready;
        },
        [&](const RowsRun& r) { launch_rows_kernel(r.p, r.a, s); });
    const RowsLaunch p = plan_rows_phases(a, bkc, sw, tuned);
    if (p.tiles_total > 0) {
      launch_rows_kernel(p, a, s);
      return;
    }
  }
  for (int i = 0; i < a.nphase; ++i) {  // one launch per phase
    const PhaseDesc& d = a.ph[i];
    IGemmArgs b = a;
    b.nphase = 0;
    b.M = d.M; b.oH = d.oH; b.oW = d.oW; b.Ktot = d.Ktot; b.T = d.T;
    b.Poh = d.Poh; b.Pow = d.Pow;
    for (int t = 0; t < d.T; ++t) {
      b.taps.dh[t] = a.taps.dh[d.tap0 + t];
      b.taps.dw[t] = a.taps.dw[d.tap0 + t];
      b.taps.bt[t] = a.taps.bt[d.tap0 + t];
    }
    run_rows(b, bkc, vw, nullptr, nullptr, s);
  }
}

// ----------------------------------------------------------------------- wgrad launches
template <int BM, int BN, int WM, int WN>
static void launch_wgrad_reg(const WGradLaunch& p, const WGradArgs& a, hipStream_t s) {
  const dim3 grid(p.grid_x, 1, p.splits), block(p.block);
  switch (p.VWA * 10 + p.VWB) {
    case 81: hipLaunchKernelGGL((igemm_wgrad_kernel<BM, BN, WM, WN, 8, 1>), grid, block, 0, s, a); break;
    case 41: hipLaunchKernelGGL((igemm_wgrad_kernel<BM, BN, WM, WN, 4, 1>), grid, block, 0, s, a); break;
    case 11: hipLaunchKernelGGL((igemm_wgrad_kernel<BM, BN, WM, WN, 1, 1>), grid, block, 0, s, a); break;
    case 88: hipLaunchKernelGGL((igemm_wgrad_kernel<BM, BN, WM, WN, 8, 8>), grid, block, 0, s, a); break;
    case 48: hipLaunchKernelGGL((igemm_wgrad_kernel<BM, BN, WM, WN, 4, 8>), grid, block, 0, s, a); break;
    case 18: hipLaunchKernelGGL((igemm_wgrad_kernel<BM, BN, WM, WN, 1, 8>), grid, block, 0, s, a); break;
    default: no_kernel("igemm_wgrad_reg", p.BM, p.BN, p.WM, p.WN, p.VWA, p.VWB);
  }
}

// register family: the rows of kWgradRegTiles
static void igemm_wgrad_reg(const WGradLaunch& p, const WGradArgs& a, hipStream_t s) {
  switch (p.BM * 1000 + p.BN) {
    case 64128: launch_wgrad_reg<64, 128, 2, 2>(p, a, s); break;
    case 128128: launch_wgrad_reg<128, 128, 2, 2>(p, a, s); break;
    default: no_kernel("igemm_wgrad_reg", p.BM, p.BN, p.WM, p.WN, p.VWA, p.VWB);
  }
}

// sums the z split partials of a.slab into a.dw (n = Kout * Ncols, n % 4 == 0)
static void wgrad_reduce(const WGradArgs& a, int z, hipStream_t s) {
  const int64_t n = (int64_t)a.Kout * a.Ncols;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(wgrad_reduce_blocks(n)), dim3(256), 0, s, a.slab, z, n,
                     a.dw, a.overwrite);
}

void igemm_stem_pool_wgrad(WGradArgs a, StemPoolArgs q, hipStream_t s) {
  wgrad_reduce(a, stem_pool_wgrad(a, q, s), s);
}

// one planned weight-gradient GEMM and its split reduction
static void launch_wgrad(const WGradLaunch& p, WGradArgs a, hipStream_t s) {
  p.apply(a);
  if (p.family == WGradFamily::Reg) igemm_wgrad_reg(p, a, s);
  else igemm_wgrad_dma(p, a, s);
  const int64_t n = (int64_t)a.Kout * a.Ncols;
  if (p.reduce == WGradReduce::Vector)
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(p.reduce_blocks), dim3(256), 0, s, a.slab, p.splits,
                       n, a.dw, a.overwrite);
  else if (p.reduce == WGradReduce::Scalar)
    hipLaunchKernelGGL(wgrad_reduce_scalar_kernel, dim3(p.reduce_blocks), dim3(256), 0, s, a.slab,
                       p.splits, n, a.dw, a.overwrite);
}

void igemm_wgrad(WGradArgs a, int vwa, int vwb, hipStream_t s) {
  const GemmSwitches& sw = switches();
  const HaloWLaunch halo = sw.engine >= 1 ? conv3_halo_wgrad_plan(a) : HaloWLaunch{};
  if (halo.kind != HaloWKind::None) {  // 3x3 / stride 1: halo-staged (Ncols = 9C, C % 32 == 0)
    wgrad_reduce(a, conv3_halo_wgrad(a, halo, s), s);
    return;
  }
  if (sw.engine >= 1 && stem_wgrad_ok(a)) {  // pixel-pair 7x7 stem: halo-staged
    wgrad_reduce(a, stem_wgrad(a, s), s);
    return;
  }
  // autotuned tile of a (non-halo) weight-gradient GEMM; candidates run on a scratch slab
  // and a scratch dw, and may not need more split slab than the caller allocated
  TileSize tuned{0, 0};
  if (vwa == 8 && vwb == 8 && sw.engine >= 1 && a.Mpix > 0)
    tuned = tuned_tile<WGradRun>(
        [&] { return wgrad_key(a); }, kWgradCands, s,
        [&](TileSize c, WGradRun& r) {
          if (!wgrad_cand_ok(c, a)) return Cand::Skip;
          r.p = plan_wgrad(a, vwa, vwb, sw, c);
          if (r.p.BM != c.bm || r.p.BN != c.bn) return Cand::Skip;
          const int64_t out = (int64_t)a.Kout * a.Ncols;
          if (r.p.splits > 1 && r.p.splits * out > igemm_wgrad_ws_floats(a.Kout, a.Ncols, a.Mpix))
            return Cand::Skip;
          char* scr = tune_scratch((size_t)(out + (r.p.splits > 1 ? r.p.splits * out : 0)) * 4 + 256);
          if (!scr) return Cand::Stop;
          r.a = a;
          r.a.dw = (float*)scr;
          r.a.slab = a.slab ? (float*)scr + out : nullptr;
          return Cand::Ready;
        },
        [&](const WGradRun& r) { launch_wgrad(r.p, r.a, s); });
  launch_wgrad(plan_wgrad(a, vwa, vwb, sw, tuned), a, s);
}

}  // namespace mpa
