// Swin V2's continuous position bias for gfx950: the table the cosine window-attention kernels
// (wattn.hip) read, bias[h][t] = 16 sigmoid(w2[h, :] . relu(w1 coord_t + b1)), from a 2 -> 512 -> H
// MLP over the log-spaced relative coordinates, and the MLP's gradients.  All fp32: the table is
// written head-major in the layout wattn_cos_fwd reads and never exists in bf16.
//
//  * coord_t is computed from t: entry t = (dy + ws - 1) (2 ws - 1) + (dx + ws - 1) of the
//    (2 ws - 1)^2 offsets has, per axis, x = 8 d / (ws - 1) and coord = sign(x) log2(1 + |x|) / 3
//    (torchvision's relative_coords_table); no coordinate buffer is read.
//  * Forward: one wave per table entry.  A lane holds 8 hidden units (lane + 64 k) in registers;
//    per head one 8-term partial and a 6-step xor-shuffle sum, lane 0 stores.
//  * Backward: one lane per hidden unit, 8 waves per pass, two passes (blockIdx.y) that share
//    nothing.  dz[h][t] = dbias[h][t] b (1 - b / 16) comes from the stored table b = 16 sigmoid(z),
//    at wave-uniform addresses.  Pass 0 loops heads outside and entries inside: dw2[h][u] = sum_t
//    dz[h][t] hid_t[u], the hidden unit recomputed from two multiply-adds.  Pass 1 loops entries
//    outside and heads inside: dhid = sum_h dz[h][t] w2[h][u], gated by the unit's sign, summed
//    into db1[u] and dw1[u][0..1].  Every sum is one thread's register in a fixed order: no
//    atomics, no workspace, bitwise repeatable.
#include "api.h"
#include "common.h"

namespace mpa {
namespace {

constexpr int CPB_PER_LANE = CPB_HIDDEN / 64;

// log-spaced coordinate of offset d (-(ws - 1) .. ws - 1) of one axis
__device__ __forceinline__ float cpb_coord(int d, int ws) {
  const float x = (float)d / (float)(ws - 1) * 8.0f;
  return copysignf(log2f(fabsf(x) + 1.0f) / 3.0f, x);
}

// grid (2 ws - 1)^2 blocks of one wave
__global__ __launch_bounds__(64) void cpb_fwd_kernel(const float* __restrict__ w1,
                                                     const float* __restrict__ b1,
                                                     const float* __restrict__ w2,
                                                     float* __restrict__ bias, int H, int ws) {
  const int lane = threadIdx.x, t = blockIdx.x, rw = 2 * ws - 1, T = rw * rw;
  const float cy = cpb_coord(t / rw - (ws - 1), ws), cx = cpb_coord(t % rw - (ws - 1), ws);
  float hid[CPB_PER_LANE];
#pragma unroll
  for (int k = 0; k < CPB_PER_LANE; ++k) {
    const int u = lane + 64 * k;
    const float2 w = make_float2(w1[2 * u], w1[2 * u + 1]);
    hid[k] = fmaxf(fmaf(w.x, cy, fmaf(w.y, cx, b1[u])), 0.f);
  }
  for (int h = 0; h < H; ++h) {
    float z = 0.f;
#pragma unroll
    for (int k = 0; k < CPB_PER_LANE; ++k) z = fmaf(w2[(size_t)h * CPB_HIDDEN + lane + 64 * k], hid[k], z);
    z = wave_sum(z);
    if (lane == 0) bias[(size_t)h * T + t] = 16.0f / (1.0f + expf(-z));
  }
}

// grid (CPB_HIDDEN / 64, 2) blocks of one wave: thread = hidden unit, blockIdx.y = pass
__global__ __launch_bounds__(64) void cpb_bwd_kernel(const float* __restrict__ dbias,
                                                     const float* __restrict__ bias,
                                                     const float* __restrict__ w1,
                                                     const float* __restrict__ b1,
                                                     const float* __restrict__ w2,
                                                     float* __restrict__ dw1, float* __restrict__ db1,
                                                     float* __restrict__ dw2, int H, int ws,
                                                     int overwrite) {
  const int u = blockIdx.x * 64 + threadIdx.x, rw = 2 * ws - 1, T = rw * rw;
  const float2 w = make_float2(w1[2 * u], w1[2 * u + 1]);
  const float b = b1[u];
  if (blockIdx.y == 0) {
    for (int h = 0; h < H; ++h) {
      float acc = 0.f;
      for (int t = 0; t < T; ++t) {
        const float cy = cpb_coord(t / rw - (ws - 1), ws), cx = cpb_coord(t % rw - (ws - 1), ws);
        const float hid = fmaxf(fmaf(w.x, cy, fmaf(w.y, cx, b)), 0.f);
        const float bv = bias[(size_t)h * T + t];
        acc = fmaf(dbias[(size_t)h * T + t] * bv * (1.0f - bv * 0.0625f), hid, acc);
      }
      float* out = dw2 + (size_t)h * CPB_HIDDEN + u;
      *out = overwrite ? acc : *out + acc;
    }
  } else {
    float gy = 0.f, gx = 0.f, gb = 0.f;
    for (int t = 0; t < T; ++t) {
      const float cy = cpb_coord(t / rw - (ws - 1), ws), cx = cpb_coord(t % rw - (ws - 1), ws);
      float dh = 0.f;
      for (int h = 0; h < H; ++h) {
        const float bv = bias[(size_t)h * T + t];
        dh = fmaf(dbias[(size_t)h * T + t] * bv * (1.0f - bv * 0.0625f), w2[(size_t)h * CPB_HIDDEN + u], dh);
      }
      if (fmaf(w.x, cy, fmaf(w.y, cx, b)) > 0.f) {
        gb += dh;
        gy = fmaf(dh, cy, gy);
        gx = fmaf(dh, cx, gx);
      }
    }
    dw1[2 * u] = overwrite ? gy : dw1[2 * u] + gy;
    dw1[2 * u + 1] = overwrite ? gx : dw1[2 * u + 1] + gx;
    db1[u] = overwrite ? gb : db1[u] + gb;
  }
}

}  // namespace

void cpb_fwd(const float* w1, const float* b1, const float* w2, int H, int ws, float* bias,
             hipStream_t s) {
  const int T = (2 * ws - 1) * (2 * ws - 1);
  hipLaunchKernelGGL(cpb_fwd_kernel, dim3((unsigned)T), dim3(64), 0, s, w1, b1, w2, bias, H, ws);
  MPA_CHECK_LAUNCH();
}

void cpb_bwd(const float* dbias, const float* bias, const float* w1, const float* b1, const float* w2,
             int H, int ws, float* dw1, float* db1, float* dw2, bool overwrite, hipStream_t s) {
  hipLaunchKernelGGL(cpb_bwd_kernel, dim3(CPB_HIDDEN / 64, 2), dim3(64), 0, s, dbias, bias, w1, b1, w2,
                     dw1, db1, dw2, H, ws, overwrite ? 1 : 0);
  MPA_CHECK_LAUNCH();
}

}  // namespace mpa
