// MFMA fragment, LDS tile and output-patch helpers of the attention kernels on
// v_mfma_f32_16x16x32_bf16 (attn.hip, xattn.hip).  Device code; the layout they implement is
// described in attn_plan.h.
#pragma once
#include "common.h"
#include "attn_plan.h"

namespace mpa {
namespace {

constexpr int TILE = AT_TILE * AT_PITCH;  // bf16 elements of an LDS tile

__device__ __forceinline__ f32x4 at_mfma(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ bf16x8 as_frag(uint4 v) { return __builtin_bit_cast(bf16x8, v); }

// 16-B operand fragment: row `row`, columns col .. col + 7 of an LDS tile
__device__ __forceinline__ bf16x8 frag(const bf16_t* tile, int row, int col) {
  return *(const bf16x8*)(tile + row * AT_PITCH + col);
}

__device__ __forceinline__ uint4 ld16(const bf16_t* p) { return *(const uint4*)p; }

// rows row0 .. row0 + 63 of a [.][64] operand (row stride `stride`) into registers: thread tid
// holds vector (tid & 7) of rows (tid >> 3) and (tid >> 3) + 32; rows >= S read as zero
__device__ __forceinline__ void tile_load(const bf16_t* base, size_t stride, int row0, int S,
                                          int tid, uint4 (&v)[2]) {
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int row = row0 + (tid >> 3) + 32 * p;
    v[p] = row < S ? ld16(base + (size_t)row * stride + (tid & 7) * 8) : make_uint4(0, 0, 0, 0);
  }
}

__device__ __forceinline__ void tile_store_rows(bf16_t* tile, int tid, const uint4 (&v)[2]) {
#pragma unroll
  for (int p = 0; p < 2; ++p)
    *(uint4*)(tile + ((tid >> 3) + 32 * p) * AT_PITCH + (tid & 7) * 8) = v[p];
}

// transposed: element (r, d) to tile[d][at_pos(r)]
__device__ __forceinline__ void tile_store_tr(bf16_t* tile, int tid, const uint4 (&v)[2]) {
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int pos = at_pos((tid >> 3) + 32 * p), d0 = (tid & 7) * 8;
    const uint32_t w[4] = {v[p].x, v[p].y, v[p].z, v[p].w};
#pragma unroll
    for (int e = 0; e < 8; ++e)
      tile[(d0 + e) * AT_PITCH + pos] = (bf16_t)(w[e >> 1] >> (16 * (e & 1)));
  }
}

// the second products' B operands from four accumulator sub-tiles: half hh holds sub-tiles
// 2 hh and 2 hh + 1 (tile rows at_acc_row(t, g, e), columns at_pos of them)
__device__ __forceinline__ void pack_halves(const float (&p)[4][4], bf16x8 (&b)[2]) {
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    const float f[8] = {p[2 * hh][0], p[2 * hh][1], p[2 * hh][2], p[2 * hh][3],
                        p[2 * hh + 1][0], p[2 * hh + 1][1], p[2 * hh + 1][2], p[2 * hh + 1][3]};
    b[hh] = as_frag(pack8(f));
  }
}

// acc[dt][r] = X^T[16 dt + 4 g + r][i] of the wave's 16 owned rows i: to the wave's LDS patch
// [16][AT_PITCH] as row i, columns 16 dt + 4 g ..
__device__ __forceinline__ void patch_write(bf16_t* patch, const f32x4 (&acc)[4], float scale,
                                            int lane) {
  const int i = lane & 15, g = lane >> 4;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    uint2 w;
    w.x = pack2(acc[dt][0] * scale, acc[dt][1] * scale);
    w.y = pack2(acc[dt][2] * scale, acc[dt][3] * scale);
    *(uint2*)(patch + i * AT_PITCH + 16 * dt + 4 * g) = w;
  }
}

// the patch's rows to global rows row0 .. row0 + 15 (< S) with 16-B stores
__device__ __forceinline__ void patch_flush(const bf16_t* patch, bf16_t* base, size_t stride,
                                            int row0, int S, int lane) {
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int r = (lane >> 3) + 8 * p, c = lane & 7;
    if (row0 + r < S)
      *(uint4*)(base + (size_t)(row0 + r) * stride + c * 8) = *(const uint4*)(patch + r * AT_PITCH + c * 8);
  }
}

__device__ __forceinline__ float group_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float group_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

}  // namespace
}  // namespace mpa
