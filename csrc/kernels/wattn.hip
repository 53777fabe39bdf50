// Shifted-window attention (forward, backward) on v_mfma_f32_16x16x32_bf16 for gfx950: Swin's
// softmax(q k^T 32^-1/2 + bias[h][rel(i, j)] + mask(i, j)) v over every ws x ws window of the
// cyclically shifted map.  Plan, address arithmetic and LDS map: wattn_plan.h.
//
//  * Roll, window partition and window reverse are address arithmetic only: qkv
//    [B Hf Wf][3][H][32] is read, and o / dqkv are written, at the row wattn_token() gives.
//    The bias index and the shift mask come from the per-token info word (wy, wx, region);
//    no index tensor, mask tensor or copy of an activation exists.
//  * One wave owns one (window, head): the padded 64 x 64 score tile is four 16-query
//    sub-tiles of four MFMAs each (head dim 32 is one k-step), both operands 16-B fragments
//    straight from global.  As in attn.hip the tile is computed transposed to the rows the
//    lane owns, so a lane holds 16 scores of ONE row per sub-tile, softmax statistics are 16
//    register operations and two xor shuffles, and P / dS rounded to bf16 are already the B
//    operand of the second product; its A operand is staged transposed in at_pos() order in
//    wave-private LDS.
//  * Backward, one kernel, two phases.  A (S^T layout, lane owns a query): P^T from lse,
//    dP^T = V dO^T, delta_i = sum_j P_ij dP_ij (o is not an input), dS^T, dQ^T = K^T dS^T
//    32^-1/2.  B (S layout, lane owns a key): P and dS again from lse and the parked delta,
//    dV^T = dO^T P, dK^T = Q^T dS 32^-1/2.  No atomics, no dQ / dKV split.
//  * dbias: the wave sums its fp32 dS tile in registers over the block's walk of windows,
//    folds it ws^4 -> (2 ws - 1)^2 through LDS in a fixed order into one slab row, and
//    wattn_dbias_kernel sums the slab rows in row order: bitwise repeatable.
//  * Accumulators, softmax state and dbias are fp32; the row sum uses the unrounded P.
//  * Cosine variant (COS, Swin V2): s = tau_h (q^ . k^) + bias + mask, q^ = q / max(|q|, 1e-12),
//    tau_h = exp(min(logit_scale[h], ln 100)).  The first MFMA stays on the raw bf16 q and k; a
//    row's inverse norm is an fp32 sum of the 32 elements its four lanes already hold (two xor
//    shuffles), kept in registers for the rows a lane owns and in 64 floats of wave-private LDS
//    for the rows it meets in the accumulator, and multiplies the fp32 accumulator: no
//    normalised operand is ever rounded or stored.  Backward: with c = q^ . k^ recomputed the
//    same way, t_i = sum_j dS_ij c_ij and u_j = sum_i dS_ij c_ij are row sums beside delta;
//    tau and the other side's inverse norm are folded into dS before it is rounded to the MFMA
//    operand, and the own inverse norm and the projection term (t_i q^_i, u_j k^_j) are applied
//    in fp32 to the accumulator before the patch is written; the own row's columns come from
//    its fragments by lane permutes.  The temperature gradient sum_i t_i is a register over
//    the walk and one more column of the slab row.
#include "api.h"
#include "common.h"
#include "wattn_plan.h"

namespace mpa {
namespace {

constexpr float WA_SCALE = 0.17677669529663687f;  // 32^-1/2 as one fp32 rounding
constexpr float WA_LOGIT_MAX = 4.605170185988092f;  // ln 100: the clamp of logit_scale
constexpr float WA_NORM_EPS = 1e-12f;

struct WattnArgs {
  const bf16_t* qkv;
  const bf16_t* d_o;
  const float* bias;    // [H][(2 ws - 1)^2]
  const float* logit_scale;  // cosine variant: [H]
  const float* lse_in;
  bf16_t* out;          // forward: o; backward: dqkv
  float* lse;           // forward: [nwin][H][ws^2]
  float* slab;          // backward: [rows][H][(2 ws - 1)^2]
  WattnGeom g;
  int nwin, wpb;
};

__device__ __forceinline__ f32x4 wa_mfma(uint4 a, uint4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                 __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// 16-B operand fragment: row `row`, columns col .. col + 7 of a transposed LDS tile
__device__ __forceinline__ uint4 wa_frag(const bf16_t* tile, int row, int col) {
  return *(const uint4*)(tile + row * WA_PITCH + col);
}

__device__ __forceinline__ float wa_group_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float wa_group_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// fragments of token rows 16 t + i of one operand (lane (i, g): columns 8 g .. 8 g + 7),
// straight from global; padded tokens (row < 0) read as zero
__device__ __forceinline__ void wa_load(const bf16_t* base, size_t stride, const int* rows_s, int i,
                                        int g, uint4 (&f)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int row = rows_s[16 * t + i];
    f[t] = row >= 0 ? *(const uint4*)(base + (size_t)row * stride + 8 * g) : make_uint4(0, 0, 0, 0);
  }
}

// the same fragments transposed into a wave tile: element (n = 16 t + i, d = 8 g + e) to
// tile[d][at_pos(n)]
__device__ __forceinline__ void wa_store_tr(bf16_t* tile, int i, int g, const uint4 (&f)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int pos = at_pos(16 * t + i);
    const uint32_t w[4] = {f[t].x, f[t].y, f[t].z, f[t].w};
#pragma unroll
    for (int e = 0; e < 8; ++e)
      tile[(8 * g + e) * WA_PITCH + pos] = (bf16_t)(w[e >> 1] >> (16 * (e & 1)));
  }
}

// the second products' B operands from four accumulator sub-tiles (attn.hip's pack_halves)
__device__ __forceinline__ void wa_pack(const float (&p)[4][4], uint4 (&b)[2]) {
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    const float f[8] = {p[2 * hh][0], p[2 * hh][1], p[2 * hh][2], p[2 * hh][3],
                        p[2 * hh + 1][0], p[2 * hh + 1][1], p[2 * hh + 1][2], p[2 * hh + 1][3]};
    b[hh] = pack8(f);
  }
}

// acc[dt][r] = X^T[16 dt + 4 g + r][i] of 16 owned rows i: to the patch [16][WA_PPITCH]
__device__ __forceinline__ void wa_patch_write(bf16_t* patch, const f32x4 (&acc)[2], float scale,
                                               int i, int g) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    uint2 w;
    w.x = pack2(acc[dt][0] * scale, acc[dt][1] * scale);
    w.y = pack2(acc[dt][2] * scale, acc[dt][3] * scale);
    *(uint2*)(patch + i * WA_PPITCH + 16 * dt + 4 * g) = w;
  }
}

// the patch's 16 rows (tokens n0 .. n0 + 15) to their global rows, one 16-B store per lane
__device__ __forceinline__ void wa_patch_flush(const bf16_t* patch, bf16_t* base, size_t stride,
                                               const int* rows_s, int n0, int lane) {
  const int r = lane >> 2, c = lane & 3;
  const int row = rows_s[n0 + r];
  if (row >= 0)
    *(uint4*)(base + (size_t)row * stride + 8 * c) = *(const uint4*)(patch + r * WA_PPITCH + 8 * c);
}

// score of query info qi and key info kj: the scale is one fp32 rounding, then two fp32 adds
__device__ __forceinline__ float wa_score(float s, const float* bias_s, int ws, uint32_t qi,
                                          uint32_t kj) {
  const float b = bias_s[wattn_rel_info(ws, qi, kj)];
  const float m = (qi >> 16) != (kj >> 16) ? -100.f : 0.f;
  return s * WA_SCALE + b + m;
}

// cosine variant: inverse norms of the four token rows 16 t + i whose fragments the lanes (i, 0..3)
// hold: 32-term fp32 sum of squares (8 in the lane, then two xor shuffles), on all four lanes
__device__ __forceinline__ void wa_inv_norms(const uint4 (&f)[4], float (&rn)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    float e[8];
    unpack8(f[t], e);
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) ss = fmaf(e[j], e[j], ss);
    rn[t] = 1.0f / fmaxf(sqrtf(wa_group_sum(ss)), WA_NORM_EPS);  // (a zero row: 1e12, times 0)
  }
}

// columns 16 dt + 4 g + r (an accumulator's) of the lane's own row i, as fp32, from the row's
// fragments: lane (i, g') holds columns 8 g' .. 8 g' + 7, so they are one half of the fragment
// of lane (i, 2 dt + g / 2)
__device__ __forceinline__ void wa_own_cols(const uint4& f, int i, int g, float (&o)[2][4]) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    const int src = i + 16 * (2 * dt + (g >> 1));
    const uint32_t x = (uint32_t)__shfl((int)f.x, src, 64), y = (uint32_t)__shfl((int)f.y, src, 64);
    const uint32_t z = (uint32_t)__shfl((int)f.z, src, 64), w = (uint32_t)__shfl((int)f.w, src, 64);
    const uint32_t lo = (g & 1) ? z : x, hi = (g & 1) ? w : y;
    o[dt][0] = __uint_as_float(lo << 16);
    o[dt][1] = __uint_as_float(lo & 0xffff0000u);
    o[dt][2] = __uint_as_float(hi << 16);
    o[dt][3] = __uint_as_float(hi & 0xffff0000u);
  }
}

// acc = rn (acc - coef x): the own inverse norm and the projection term of dQ / dK, in fp32
__device__ __forceinline__ void wa_project(f32x4 (&acc)[2], const uint4& f, float rn, float coef,
                                           int i, int g) {
  float x[2][4];
  wa_own_cols(f, i, g, x);
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[dt][r] = rn * (acc[dt][r] - coef * x[dt][r]);
}

// cosine score from c = q^ . k^: the temperature, then the same two fp32 adds
__device__ __forceinline__ float wa_score_cos(float c, float tau, const float* bias_s, int ws,
                                              uint32_t qi, uint32_t kj) {
  const float b = bias_s[wattn_rel_info(ws, qi, kj)];
  const float m = (qi >> 16) != (kj >> 16) ? -100.f : 0.f;
  return tau * c + b + m;
}

// ------------------------------------------------------------------------------ forward
// grid (windows, H / W), block W waves: wave w owns head blockIdx.y W + w of window blockIdx.x
template <int W, bool COS>
__global__ __launch_bounds__(64 * W) void wattn_fwd_kernel(WattnArgs a) {
  constexpr int WBYTES = COS ? WA_FWD_COS_BYTES : WA_FWD_BYTES;  // a wave's LDS
  __shared__ __attribute__((aligned(16))) unsigned char lds[W * WBYTES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
  const int win = blockIdx.x, H = a.g.H, h = blockIdx.y * W + wave;
  const int ws = a.g.ws, S2 = ws * ws, nb = (2 * ws - 1) * (2 * ws - 1);
  bf16_t* Vt = (bf16_t*)(lds + wave * WBYTES);
  bf16_t* patch = Vt + WA_D * WA_PITCH;
  float* bias_s = (float*)(patch + 16 * WA_PPITCH);
  int* rows_s = (int*)(bias_s + WA_BIAS_MAX);
  uint32_t* info = (uint32_t*)(rows_s + WA_N);
  {
    uint32_t inf;
    rows_s[lane] = wattn_token(a.g, win, lane, &inf);
    info[lane] = inf;
  }
  for (int j = lane; j < nb; j += 64) bias_s[j] = a.bias[(size_t)h * nb + j];
  __syncthreads();
  const size_t hs = (size_t)H * WA_D, rs = 3 * hs;
  const bf16_t* qb = a.qkv + (size_t)h * WA_D;
  uint4 qf[4], kf[4];
  {
    uint4 vf[4];
    wa_load(qb, rs, rows_s, i, g, qf);
    wa_load(qb + hs, rs, rows_s, i, g, kf);
    wa_load(qb + 2 * hs, rs, rows_s, i, g, vf);
    wa_store_tr(Vt, i, g, vf);
  }
  float* rk_s = (float*)(info + WA_N);  // (COS) inverse norms of the key rows
  float rqv[4] = {0.f, 0.f, 0.f, 0.f}, tau = 0.f;
  if constexpr (COS) {
    float rkv[4];
    tau = expf(fminf(a.logit_scale[h], WA_LOGIT_MAX));
    wa_inv_norms(qf, rqv);
    wa_inv_norms(kf, rkv);
    if (g == 0) {
#pragma unroll
      for (int t = 0; t < 4; ++t) rk_s[16 * t + i] = rkv[t];
    }
  }
  __syncthreads();
#pragma unroll
  for (int qs = 0; qs < 4; ++qs) {
    if (16 * qs < S2) {  // (block-uniform) wholly padded query sub-tiles are skipped
      const uint32_t qi = info[16 * qs + i];
      float p[4][4];
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f32x4 st = wa_mfma(kf[t], qf[qs], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int nk = at_acc_row(t, g, r);
          if constexpr (COS)
            p[t][r] = nk < S2 ? wa_score_cos(st[r] * rqv[qs] * rk_s[nk], tau, bias_s, ws, qi, info[nk])
                              : -INFINITY;
          else
            p[t][r] = nk < S2 ? wa_score(st[r], bias_s, ws, qi, info[nk]) : -INFINITY;
          mx = fmaxf(mx, p[t][r]);
        }
      }
      const float m = wa_group_max(mx);  // (finite: key 0 is never padded)
      float rsum = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p[t][r] = expf(p[t][r] - m);
          rsum += p[t][r];
        }
      const float l = wa_group_sum(rsum);
      uint4 pb[2];
      wa_pack(p, pb);
      f32x4 acc[2];
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
          acc[dt] = wa_mfma(wa_frag(Vt, 16 * dt + i, 32 * hh + 8 * g), pb[hh], acc[dt]);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[dt][r] = acc[dt][r] / l;
      }
      wa_patch_write(patch, acc, 1.0f, i, g);
      __syncthreads();
      wa_patch_flush(patch, a.out + (size_t)h * WA_D, hs, rows_s, 16 * qs, lane);
      if (g == 0 && 16 * qs + i < S2)
        a.lse[((size_t)win * H + h) * S2 + 16 * qs + i] = m + logf(l);
      __syncthreads();
    }
  }
}

// ----------------------------------------------------------------------------- backward
// grid (walks, H / W): the block walks windows blockIdx.x wpb .. + wpb - 1 (< nwin)
template <int W, bool COS>
__global__ __launch_bounds__(64 * W) void wattn_bwd_kernel(WattnArgs a) {
  constexpr int WBYTES = COS ? WA_BWD_COS_BYTES : WA_BWD_BYTES;  // a wave's LDS
  __shared__ __attribute__((aligned(16))) unsigned char lds[W * WBYTES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
  const int H = a.g.H, h = blockIdx.y * W + wave;
  const int ws = a.g.ws, S2 = ws * ws, rw = 2 * ws - 1, nb = rw * rw;
  bf16_t* Kt = (bf16_t*)(lds + wave * WBYTES);
  bf16_t* Qt = Kt + WA_D * WA_PITCH;
  bf16_t* Dt = Qt + WA_D * WA_PITCH;
  float* bias_s = (float*)(Dt + WA_D * WA_PITCH);
  int* rows_s = (int*)(bias_s + WA_BIAS_MAX);
  uint32_t* info = (uint32_t*)(rows_s + WA_N);
  float* lse_s = (float*)(info + WA_N);
  float* del_s = lse_s + WA_N;
  float* rq_s = del_s + WA_N;  // (COS) inverse norms of the query and the key rows
  float* rk_s = rq_s + WA_N;
  float tau = 0.f, dtau = 0.f;  // (COS) the lane's part of sum_i t_i over the walk
  if constexpr (COS) tau = expf(fminf(a.logit_scale[h], WA_LOGIT_MAX));
  for (int j = lane; j < nb; j += 64) bias_s[j] = a.bias[(size_t)h * nb + j];
  const size_t hs = (size_t)H * WA_D, rs = 3 * hs;
  const bf16_t* qb = a.qkv + (size_t)h * WA_D;
  bf16_t* dq = a.out + (size_t)h * WA_D;
  float dsacc[4][4][4];  // the walk's fp32 dS tile: [query sub-tile][key sub-tile][register]
#pragma unroll
  for (int qs = 0; qs < 4; ++qs)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) dsacc[qs][t][r] = 0.f;

  const int w0 = blockIdx.x * a.wpb, w1 = min(w0 + a.wpb, a.nwin);
  for (int win = w0; win < w1; ++win) {
    __syncthreads();  // the previous window's LDS reads are done
    {
      uint32_t inf;
      rows_s[lane] = wattn_token(a.g, win, lane, &inf);
      info[lane] = inf;
      // padded query rows: lse = +inf makes every P zero, delta stays 0
      lse_s[lane] = lane < S2 ? a.lse_in[((size_t)win * H + h) * S2 + lane] : INFINITY;
      del_s[lane] = 0.f;
    }
    __syncthreads();
    uint4 qf[4], kf[4], vf[4], df[4];
    wa_load(qb, rs, rows_s, i, g, qf);
    wa_load(qb + hs, rs, rows_s, i, g, kf);
    wa_load(qb + 2 * hs, rs, rows_s, i, g, vf);
    wa_load(a.d_o + (size_t)h * WA_D, hs, rows_s, i, g, df);
    wa_store_tr(Kt, i, g, kf);
    float rqv[4] = {0.f, 0.f, 0.f, 0.f}, rkv[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (COS) {
      wa_inv_norms(qf, rqv);
      wa_inv_norms(kf, rkv);
      if (g == 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          rq_s[16 * t + i] = rqv[t];
          rk_s[16 * t + i] = rkv[t];
        }
      }
    }
    __syncthreads();

    // phase A: S^T layout, the lane owns query 16 qs + i and holds keys 16 t + 4 g + r
#pragma unroll
    for (int qs = 0; qs < 4; ++qs) {
      if (16 * qs < S2) {
        const uint32_t qi = info[16 * qs + i];
        const float lse = lse_s[16 * qs + i];
        float pv[4][4], ds[4][4], cc[4][4];
        float dsum = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const f32x4 st = wa_mfma(kf[t], qf[qs], f32x4{0.f, 0.f, 0.f, 0.f});
          const f32x4 dp = wa_mfma(vf[t], df[qs], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int nk = at_acc_row(t, g, r);
            if constexpr (COS) {
              cc[t][r] = st[r] * rqv[qs] * rk_s[nk];
              pv[t][r] = nk < S2 ? expf(wa_score_cos(cc[t][r], tau, bias_s, ws, qi, info[nk]) - lse) : 0.f;
            } else {
              pv[t][r] = nk < S2 ? expf(wa_score(st[r], bias_s, ws, qi, info[nk]) - lse) : 0.f;
            }
            ds[t][r] = dp[r];
            dsum = fmaf(pv[t][r], dp[r], dsum);
          }
        }
        const float delta = wa_group_sum(dsum);
        float tsum = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            ds[t][r] = pv[t][r] * (ds[t][r] - delta);
            dsacc[qs][t][r] += ds[t][r];
            if constexpr (COS) {  // t_i, then tau and the key's inverse norm into the operand
              tsum = fmaf(ds[t][r], cc[t][r], tsum);
              ds[t][r] *= tau * rk_s[at_acc_row(t, g, r)];
            }
          }
        uint4 dsb[2];
        wa_pack(ds, dsb);
        f32x4 acc[2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int hh = 0; hh < 2; ++hh)
            acc[dt] = wa_mfma(wa_frag(Kt, 16 * dt + i, 32 * hh + 8 * g), dsb[hh], acc[dt]);
        }
        if (g == 0) del_s[16 * qs + i] = delta;
        if constexpr (COS) {
          dtau += tsum;
          wa_project(acc, qf[qs], rqv[qs], tau * wa_group_sum(tsum) * rqv[qs], i, g);
        }
        wa_patch_write(Dt, acc, COS ? 1.0f : WA_SCALE, i, g);  // (dOt is staged after this phase)
        __syncthreads();
        wa_patch_flush(Dt, dq, rs, rows_s, 16 * qs, lane);
        __syncthreads();
      }
    }
    wa_store_tr(Qt, i, g, qf);
    wa_store_tr(Dt, i, g, df);
    __syncthreads();

    // phase B: S layout, the lane owns key 16 ks + i and holds queries 16 t + 4 g + r
    bf16_t* pk = Kt;                      // (K transposed is dead after phase A)
    bf16_t* pvv = Kt + 16 * WA_PPITCH;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      if (16 * ks < S2) {
        const uint32_t kj = info[16 * ks + i];
        const bool kon = 16 * ks + i < S2;
        float pv[4][4], ds[4][4];
        float usum = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const f32x4 st = wa_mfma(qf[t], kf[ks], f32x4{0.f, 0.f, 0.f, 0.f});
          const f32x4 dp = wa_mfma(df[t], vf[ks], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int nq = at_acc_row(t, g, r);
            if constexpr (COS) {  // u_j, then tau and the query's inverse norm into the operand
              const float c = st[r] * rq_s[nq] * rkv[ks];
              pv[t][r] = kon ? expf(wa_score_cos(c, tau, bias_s, ws, info[nq], kj) - lse_s[nq]) : 0.f;
              ds[t][r] = pv[t][r] * (dp[r] - del_s[nq]);
              usum = fmaf(ds[t][r], c, usum);
              ds[t][r] *= tau * rq_s[nq];
            } else {
              pv[t][r] = kon ? expf(wa_score(st[r], bias_s, ws, info[nq], kj) - lse_s[nq]) : 0.f;
              ds[t][r] = pv[t][r] * (dp[r] - del_s[nq]);
            }
          }
        }
        uint4 pb[2], dsb[2];
        wa_pack(pv, pb);
        wa_pack(ds, dsb);
        f32x4 accv[2], acck[2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          accv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
          acck[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int hh = 0; hh < 2; ++hh) {
            accv[dt] = wa_mfma(wa_frag(Dt, 16 * dt + i, 32 * hh + 8 * g), pb[hh], accv[dt]);
            acck[dt] = wa_mfma(wa_frag(Qt, 16 * dt + i, 32 * hh + 8 * g), dsb[hh], acck[dt]);
          }
        }
        if constexpr (COS)
          wa_project(acck, kf[ks], rkv[ks], tau * wa_group_sum(usum) * rkv[ks], i, g);
        wa_patch_write(pk, acck, COS ? 1.0f : WA_SCALE, i, g);
        wa_patch_write(pvv, accv, 1.0f, i, g);
        __syncthreads();
        wa_patch_flush(pk, dq + hs, rs, rows_s, 16 * ks, lane);
        wa_patch_flush(pvv, dq + 2 * hs, rs, rows_s, 16 * ks, lane);
        __syncthreads();
      }
    }
  }

  // fold ws^4 -> (2 ws - 1)^2: one 16-query slice of the dS tile at a time through LDS; output
  // lane + 64 rr adds the slice's entries of its (dy, dx) in query order
  float* fold = (float*)Kt;  // [16][WA_FOLD_PITCH]
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int qs = 0; qs < 4; ++qs) {
    if (16 * qs < S2) {
      __syncthreads();
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) fold[i * WA_FOLD_PITCH + at_acc_row(t, g, r)] = dsacc[qs][t][r];
      __syncthreads();
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int idx = lane + 64 * rr;
        if (idx < nb) {
          const int dy = idx / rw - (ws - 1), dx = idx % rw - (ws - 1);
          for (int ii = 0; ii < 16; ++ii) {
            const int q = 16 * qs + ii;
            if (q >= S2) break;
            const int yj = (int)(info[q] & 255) - dy, xj = (int)((info[q] >> 8) & 255) - dx;
            if (yj >= 0 && yj < ws && xj >= 0 && xj < ws) sum[rr] += fold[ii * WA_FOLD_PITCH + yj * ws + xj];
          }
        }
      }
    }
  }
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int idx = lane + 64 * rr;
    if (idx < nb) a.slab[((size_t)blockIdx.x * H + h) * (nb + (COS ? 1 : 0)) + idx] = sum[rr];
  }
  if constexpr (COS) {  // the slab row's last column: sum_i t_i of the walk
    const float d = wave_sum(dtau);
    if (lane == 0) a.slab[((size_t)blockIdx.x * H + h) * (nb + 1) + nb] = d;
  }
}

// dbias[h][idx] (+)= the slab rows' sum in row order: one thread per element
__global__ __launch_bounds__(256) void wattn_dbias_kernel(const float* __restrict__ slab,
                                                          float* __restrict__ dbias, int rows, int n,
                                                          int overwrite) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  float s = 0.f;
  for (int r = 0; r < rows; ++r) s += slab[(size_t)r * n + idx];
  dbias[idx] = overwrite ? s : dbias[idx] + s;
}

// the cosine variant's second launch: slab rows [H][nb + 1] summed in row order; column nb is
// d tau_h, and d logit_scale_h = d tau_h tau_h below the clamp, 0 at it
__global__ __launch_bounds__(256) void wattn_cos_dbias_kernel(const float* __restrict__ slab,
                                                              const float* __restrict__ logit_scale,
                                                              float* __restrict__ dbias,
                                                              float* __restrict__ dlogit, int rows, int H,
                                                              int nb, int overwrite) {
  const int idx = blockIdx.x * 256 + threadIdx.x, n = H * (nb + 1);
  if (idx >= n) return;
  float s = 0.f;
  for (int r = 0; r < rows; ++r) s += slab[(size_t)r * n + idx];
  const int h = idx / (nb + 1), j = idx - h * (nb + 1);
  float* out = dbias + h * nb + j;
  if (j == nb) {
    const float ls = logit_scale[h];
    s = ls < WA_LOGIT_MAX ? s * expf(ls) : 0.f;
    out = dlogit + h;
  }
  *out = overwrite ? s : *out + s;
}

template <int W, bool COS>
void launch_fwd(const WattnArgs& a, const WattnPlan& p, hipStream_t s) {
  hipLaunchKernelGGL((wattn_fwd_kernel<W, COS>), dim3((unsigned)p.nwin, (unsigned)p.groups), dim3(64 * W), 0,
                     s, a);
}
template <int W, bool COS>
void launch_bwd(const WattnArgs& a, const WattnPlan& p, hipStream_t s) {
  hipLaunchKernelGGL((wattn_bwd_kernel<W, COS>), dim3((unsigned)p.rows, (unsigned)p.groups), dim3(64 * W), 0,
                     s, a);
}

}  // namespace

int64_t wattn_ws_floats(const WattnGeom& g) { return wattn_plan(g).ws_floats; }

void wattn_fwd(const bf16_raw* qkv, const float* bias, const WattnGeom& g, bf16_raw* o, float* lse,
               hipStream_t s) {
  const WattnPlan p = wattn_plan(g);
  WattnArgs a{};
  a.qkv = qkv; a.bias = bias; a.out = o; a.lse = lse; a.g = g; a.nwin = p.nwin; a.wpb = 1;
  switch (p.waves) {
    case 4: launch_fwd<4, false>(a, p, s); break;
    case 3: launch_fwd<3, false>(a, p, s); break;
    case 2: launch_fwd<2, false>(a, p, s); break;
    default: launch_fwd<1, false>(a, p, s); break;
  }
  MPA_CHECK_LAUNCH();
}

void wattn_cos_fwd(const bf16_raw* qkv, const float* logit_scale, const float* bias,
                   const WattnGeom& g, bf16_raw* o, float* lse, hipStream_t s) {
  const WattnPlan p = wattn_plan(g, true);
  WattnArgs a{};
  a.qkv = qkv; a.bias = bias; a.logit_scale = logit_scale; a.out = o; a.lse = lse; a.g = g;
  a.nwin = p.nwin; a.wpb = 1;
  switch (p.waves) {
    case 4: launch_fwd<4, true>(a, p, s); break;
    case 3: launch_fwd<3, true>(a, p, s); break;
    case 2: launch_fwd<2, true>(a, p, s); break;
    default: launch_fwd<1, true>(a, p, s); break;
  }
  MPA_CHECK_LAUNCH();
}

void wattn_bwd(const bf16_raw* d_o, const bf16_raw* qkv, const float* lse, const float* bias,
               const WattnGeom& g, bf16_raw* dqkv, float* dbias, bool overwrite, float* ws,
               hipStream_t s) {
  const WattnPlan p = wattn_plan(g);
  WattnArgs a{};
  a.qkv = qkv; a.d_o = d_o; a.bias = bias; a.lse_in = lse; a.out = dqkv; a.slab = ws; a.g = g;
  a.nwin = p.nwin; a.wpb = p.wpb;
  switch (p.waves) {
    case 4: launch_bwd<4, false>(a, p, s); break;
    case 3: launch_bwd<3, false>(a, p, s); break;
    case 2: launch_bwd<2, false>(a, p, s); break;
    default: launch_bwd<1, false>(a, p, s); break;
  }
  const int n = g.H * p.nbias;
  hipLaunchKernelGGL(wattn_dbias_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ws,
                     dbias, p.rows, n, overwrite ? 1 : 0);
  MPA_CHECK_LAUNCH();
}

int64_t wattn_cos_ws_floats(const WattnGeom& g) { return wattn_plan(g, true).ws_floats; }

void wattn_cos_bwd(const bf16_raw* d_o, const bf16_raw* qkv, const float* lse, const float* logit_scale,
                   const float* bias, const WattnGeom& g, bf16_raw* dqkv, float* dbias, float* dlogit,
                   bool overwrite, float* ws, hipStream_t s) {
  const WattnPlan p = wattn_plan(g, true);
  WattnArgs a{};
  a.qkv = qkv; a.d_o = d_o; a.bias = bias; a.logit_scale = logit_scale; a.lse_in = lse; a.out = dqkv;
  a.slab = ws; a.g = g; a.nwin = p.nwin; a.wpb = p.wpb;
  switch (p.waves) {
    case 4: launch_bwd<4, true>(a, p, s); break;
    case 3: launch_bwd<3, true>(a, p, s); break;
    case 2: launch_bwd<2, true>(a, p, s); break;
    default: launch_bwd<1, true>(a, p, s); break;
  }
  const int n = g.H * p.slab_cols;
  hipLaunchKernelGGL(wattn_cos_dbias_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ws,
                     logit_scale, dbias, dlogit, p.rows, g.H, p.nbias, overwrite ? 1 : 0);
  MPA_CHECK_LAUNCH();
}

}  // namespace mpa
