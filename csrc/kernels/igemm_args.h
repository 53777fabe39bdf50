// Plain-data argument structs of the GEMM / conv launchers: no HIP, no torch, only the C++
// standard library, so host-side planning code (halo_plan.h) and its stand-alone checks
// compile without a GPU toolchain.  api.h includes this file.
#pragma once
#include <algorithm>
#include <stdint.h>

namespace mpa {

typedef uint16_t bf16_raw;
// statistics-slab rows of a persistent launch (halo and stem kernels): one per block
constexpr int HALO_MAX_ROWS = 256;
constexpr int MAXT = 128;  // max taps in one implicit-GEMM launch (11x11 = 121)

struct Taps {
  short dh[MAXT];
  short dw[MAXT];
  short bt[MAXT];
};

// One stride phase of a merged dgrad launch: its output sub-grid (oH x oW pixels at
// rows/cols Poh + Uoh*i, Pow + Uow*j of dx), its taps [tap0, tap0 + T) of the shared table,
// and its tile count.  Tile g of the launch belongs to phase g % nphase (phases interleaved
// so every XCD's contiguous share of the tile list holds an equal mix of long and short
// phases), local tile g / nphase; phases are padded to the longest tile count.
// n / d for 0 <= n < 2^31 as one multiply-high and a shift (Granlund-Montgomery: m =
// ceil(2^(31 + l) / d), l = ceil(log2 d)); m == 0 encodes d == 1.  The rows kernels split
// a pixel index into (image, row, column) with these instead of two 32-bit integer divisions
// (~40 VALU each) per row in the prologue and again in the epilogue.
struct FastDiv {
  uint32_t m, s;
};
inline FastDiv make_fastdiv(uint32_t d) {
  if (d <= 1) return FastDiv{0u, 0u};
  const uint32_t l = 32u - (uint32_t)__builtin_clz(d - 1u);
  return FastDiv{(uint32_t)(((1ull << (31 + l)) + d - 1) / d), l - 1u};
}

constexpr int MAXPH = 16;
struct PhaseDesc {
  int M, oH, oW, Ktot, tap0, T, Poh, Pow, tiles;
  FastDiv fd_hw, fd_ow;  // oH * oW, oW (set by the launchers: igemm_set_fastdiv)
};

// implicit GEMM whose rows are pixels of a gathered NHWC tensor (conv fwd / dgrad / linear)
struct IGemmArgs {
  const bf16_raw* A;
  int aH, aW, aC;
  int oH, oW;
  int M;
  int Uh, Uw, Oh, Ow;
  int T;
  int Ktot;
  const bf16_raw* B;
  int N;
  int RS;
  int ldb;
  void* C;
  int ldc;
  int dH, dW, Uoh, Uow, Poh, Pow;
  const float* bias;
  float* stats;              // [2][N]: finalized (mean, biased var) of the bf16 output
  const float* stats_shift;  // per-column shift K for the sums (BN running mean) or null
  float* stats_sums;         // [2][N] final sums: zeroed by the epilogue's mt == 0 blocks
  int stats_ld;              // row stride of the finalized [2][N] statistics (0: N)
  int relu;
  int ktiles_per_split;
  int tiles_n;
  int tiles_total;
  Taps taps;
  int nphase;             // > 0: merged stride-phase dgrad launch (igemm_rows_dgrad_phases)
  PhaseDesc ph[MAXPH];
  int b_tapmap;           // K-contiguous B whose rows are indexed by weight tap: B element of
                          // GEMM k = (t, c) is B[n][taps.bt[t] * aC + c] (dgrad from the
                          // transposed weight [C][RS][K]); 0: B[n][k]
  // fused BN-backward reduction (dgrad epilogue, ep_bnred = 1): the GEMM output v is the
  // gradient dy of a ReLU(BN(z)) whose z / y / mean / rstd are given (same layout as C);
  // the epilogue writes g = dy * (y > 0) and slab-reduces (sum g, sum g * (z - mean) * rstd)
  // per column into `stats` exactly like the forward statistics (row `stat` of the slab)
  int ep_bnred;
  const bf16_raw* ep_z;
  const bf16_raw* ep_y;
  const float* ep_mean;
  const float* ep_rstd;
  // ep_gamma / ep_beta (optional): the 3x3/s1 halo kernel then recomputes the ReLU mask
  // from z exactly as bn_fwd_train rounded y (bf16(fma(z, gamma*rstd, fma(-mean,
  // gamma*rstd, beta))) > 0) and never reads y; the implicit GEMM always reads ep_y
  const float* ep_gamma;
  const float* ep_beta;
  // ep_gacc (dense_gacc.hip only): no output is written; gamma*rstd * g is ADDED into
  // ep_gacc (same row stride ldc as ep_z; bf16 with one rounding, or fp32 when
  // ep_gacc_f32) - the DenseNet block gradient, whose per-channel BN-backward corrections
  // are deferred (bn_defer_step)
  void* ep_gacc;
  int ep_gacc_f32;
  int stap;               // 8-channel "super-tap" forward: each tap entry = 4 adjacent kernel
                          // columns (dw .. dw+3, weight taps bt .. bt+ns-1), Ktot = 32 * T
  int beta;               // 1: accumulate, C = acc + C (bf16 read-add-write, one rounding):
                          // a second gradient contribution lands in the first one's buffer
  FastDiv fd_hw, fd_ow;   // oH * oW, oW (igemm_set_fastdiv, right before a launch)
  // second GEMM source (merged stride-phase dgrad, uniform-tap LDS-DMA kernel only): tap
  // entries with bt & TAP_SRC2 read A2 (same pixel grid and channel count as A) and B2
  // (K-contiguous, row stride ldb2) - the dgrad of a second conv that reads the same input
  // with the same stride (ResNet's 1x1/s2 shortcut) lands as extra K of the phase its
  // taps belong to, so dx is written once
  const bf16_raw* A2;
  const bf16_raw* B2;
  int ldb2;
  // kpad (uniform-tap LDS-DMA kernel, K-contiguous B): aC is 16-B but not 32-granular
  // (Inception's 48 / 80 channels): every tap's K is padded to a multiple of 32, Ktot =
  // T * round32(aC), and the chunks past aC read zeros
  int kpad;
  // accumulate (beta = 1) from ep_res instead of the old C, masked by the ReLU bit mask
  // ep_rmask (bit e % 8 of byte e / 8 for element e): a residual block's shortcut gradient
  // dy * (y > 0) added in the conv1 dgrad epilogue without being written first (halo
  // kernels only; dense [M][N] rows)
  const bf16_raw* ep_res;
  const uint8_t* ep_rmask;
};
constexpr short TAP_SRC2 = 0x2000;

// fill the FastDiv fields of a rows launch (and of its stride phases)
inline void igemm_set_fastdiv(IGemmArgs& a) {
  a.fd_hw = make_fastdiv((uint32_t)std::max(1, a.oH * a.oW));
  a.fd_ow = make_fastdiv((uint32_t)std::max(1, a.oW));
  for (int i = 0; i < a.nphase && i < MAXPH; ++i) {
    a.ph[i].fd_hw = make_fastdiv((uint32_t)std::max(1, a.ph[i].oH * a.ph[i].oW));
    a.ph[i].fd_ow = make_fastdiv((uint32_t)std::max(1, a.ph[i].oW));
  }
}

struct WGradArgs {
  const bf16_raw* dy;
  const bf16_raw* x;
  float* dw;
  float* slab;  // split partials [splits][Kout][Ncols] (igemm_wgrad_ws_floats), or null
  int Kout, C, H, W, P, Q, R, S, sh, sw, ph, pw;
  int Mpix;
  int Ncols;
  int ktiles_per_split;
  int tiles_n, tiles_total;
  int overwrite;  // 1: dw holds nothing to keep (first gradient since zero_grad): store, no
                  // read-modify-write of the fp32 arena
};

}  // namespace mpa
