// Neighbourhood attention (forward, backward) on v_mfma_f32_16x16x32_bf16 for gfx950: NAT's
// o_i = sum_j softmax_j(q_i . k_j 32^-1/2 + rpb[h][yj - yi + 6][xj - xi + 6]) v_j over the 7 x 7
// keys whose start is clamped to the map (nattn_ni).  Plan, address arithmetic and LDS map:
// nattn_plan.h.
//
//  * No gathered key or value tensor exists: qkv [B Hf Wf][3][H][32] is read in place.  A block
//    owns an 8 x 8 tile of one head; a sub-tile of the score tile is ONE map row of 16 column
//    slots, so a slot's coordinates, the neighbourhood mask and the bias index are adds and
//    compares on registers.  A head's 169 bias floats sit in LDS.
//  * Forward and dQ: wave w owns query rows 2 w, 2 w + 1 of the tile, 16 queries, and meets 8
//    key rows by 16 slots.  As in wattn.hip the tile is computed transposed (S^T = K Q^T, one
//    MFMA per key row since head dim 32 is one k-step), so a lane holds all 32 scores of ONE
//    query per group, the softmax is single-pass in registers with two xor shuffles, and P / dS
//    rounded to bf16 are already the B operand of the second product.
//  * Both products' first operands are 16-B fragments straight from global memory (the rows a
//    tile's waves share come from L1 / L2).  The second product's A operand (V, K, or Q and dO
//    transposed) is staged by the wave itself from the fragments it holds, one row pair [32][32]
//    at a time in two ring stages of wave-private LDS: no wave waits for another's data.  The
//    issue's plan was one block-wide 14 x 14 halo tile; a wave's pairs start at a row of either
//    parity of that tile, which would split every operand read in two, and the dK / dV side
//    needs up to 17 x 17 queries per tile (33 KB per operand).  Not compared by measurement.
//  * Backward, two attention kernels, no atomics.  nattn_dq (the forward's geometry): P from
//    lse, dP^T = V dO^T, delta_i = sum_j P dP (written for the second kernel), dS^T, dQ^T = K^T
//    dS^T 32^-1/2.  nattn_dkv: wave w owns a 4 x 4 key patch in the S = Q K^T layout (a lane
//    owns a key) and walks the query rows that attend it in pairs: dV^T += dO^T P, dK^T += Q^T dS
//    32^-1/2 in registers; no softmax state, so any number of pairs works.
//  * drpb: a dq block walks one tile position over `bpw` batch images, sums its fp32 dS in
//    registers (the slot -> relative index map is the same for all of them), folds 64 x 128
//    slots to 169 bins through LDS in query order and writes one slab row; nattn_drpb_kernel
//    sums the slab rows in row order: bitwise repeatable.
//  * Queries and keys of a partial tile are computed on zeros (lse = +inf) and never stored.
//  * Accumulators, softmax state and drpb are fp32; the row sum uses the unrounded P.
#include "api.h"
#include "common.h"
#include "nattn_plan.h"

namespace mpa {
namespace {

constexpr float NA_SCALE = 0.17677669529663687f;  // 32^-1/2 as one fp32 rounding
constexpr int NA_PAIR = NA_D * NA_PITCH;          // bf16 elements of a transposed pair tile

struct NattnArgs {
  const bf16_t* qkv;
  const bf16_t* d_o;
  const float* rpb;       // [H][169]
  const float* lse_in;    // [B][H][Hf Wf]
  const float* delta_in;  // dkv: [B][H][Hf Wf]
  bf16_t* out;            // forward: o; backward: dqkv
  float* lse;             // forward
  float* delta;           // dq
  float* slab;            // dq: [walks][tiles][H][169]
  NattnGeom g;
  int tx, tiles, bpw;
};

__device__ __forceinline__ f32x4 na_mfma(uint4 a, uint4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                 __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ float na_group_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}
__device__ __forceinline__ float na_group_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}

// columns 8 g .. 8 g + 7 of one operand of the token at (y, x) >= 0 of an image whose rows
// start at `base` (row stride `stride`); a token outside the map reads as zero
__device__ __forceinline__ uint4 na_load(const bf16_t* base, size_t stride, const NattnGeom& gm, int y,
                                         int x, int g) {
  return y < gm.Hf && x < gm.Wf ? *(const uint4*)(base + ((size_t)y * gm.Wf + x) * stride + 8 * g)
                                : make_uint4(0, 0, 0, 0);
}

// a fragment (slot i of sub-tile a of a pair, columns 8 g ..) transposed into a pair tile
__device__ __forceinline__ void na_store_tr(bf16_t* tile, int a, int i, int g, const uint4& f) {
  const int pos = nattn_pos(a, i);
  const uint32_t w[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
  for (int e = 0; e < 8; ++e) tile[(8 * g + e) * NA_PITCH + pos] = (bf16_t)(w[e >> 1] >> (16 * (e & 1)));
}

__device__ __forceinline__ uint4 na_frag(const bf16_t* tile, int row, int col) {
  return *(const uint4*)(tile + row * NA_PITCH + col);
}

// the second product's B operand from an accumulator pair
__device__ __forceinline__ uint4 na_pack(const float (&p0)[4], const float (&p1)[4]) {
  const float f[8] = {p0[0], p0[1], p0[2], p0[3], p1[0], p1[1], p1[2], p1[3]};
  return pack8(f);
}

// acc[dt][r] = X^T[16 dt + 4 g + r][i] of 16 owned rows i: to the patch [16][NA_PPITCH]
__device__ __forceinline__ void na_patch_write(bf16_t* patch, const f32x4 (&acc)[2], float scale, int i,
                                               int g) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    uint2 w;
    w.x = pack2(acc[dt][0] * scale, acc[dt][1] * scale);
    w.y = pack2(acc[dt][2] * scale, acc[dt][3] * scale);
    *(uint2*)(patch + i * NA_PPITCH + 16 * dt + 4 * g) = w;
  }
}

// patch row lane / 4 to the token at (y, x) if it is in the map, one 16-B store per lane
__device__ __forceinline__ void na_patch_flush(const bf16_t* patch, bf16_t* base, size_t stride,
                                               const NattnGeom& gm, int y, int x, int lane) {
  if (y < gm.Hf && x < gm.Wf)
    *(uint4*)(base + ((size_t)y * gm.Wf + x) * stride + 8 * (lane & 3)) =
        *(const uint4*)(patch + (lane >> 2) * NA_PPITCH + 8 * (lane & 3));
}

// what a lane of a query wave (forward, dq) knows about its query and the wave's key slots
struct QueryLane {
  int yq, xq;    // the lane's query (may lie outside the map in a partial tile)
  bool on;       // it is in the map
  int yc, xc;    // clamped into the map: the mask's and the bias index's coordinates
  int ny, nx;    // its neighbourhood's first row, column
  int ky0, kx0;  // the wave's first key row, the tile's first key column
};

__device__ __forceinline__ QueryLane na_query_lane(const NattnGeom& gm, int ty, int tx, int wave, int i) {
  QueryLane q;
  q.yq = NA_TILE * ty + 2 * wave + (i >> 3);
  q.xq = NA_TILE * tx + (i & 7);
  q.on = q.yq < gm.Hf && q.xq < gm.Wf;
  q.yc = min(q.yq, gm.Hf - 1);
  q.xc = min(q.xq, gm.Wf - 1);
  q.ny = nattn_ni(q.yc, gm.Hf);
  q.nx = nattn_ni(q.xc, gm.Wf);
  q.ky0 = nattn_ni(NA_TILE * ty + 2 * wave, gm.Hf);
  q.kx0 = nattn_ni(NA_TILE * tx, gm.Wf);
  return q;
}

// score of the lane's query and the key at slot (t, c): the scale is one fp32 rounding, then
// one fp32 add; -inf outside the query's 7 x 7
__device__ __forceinline__ float na_score(float s, const float* bias_s, const QueryLane& q, int t, int c) {
  const int Y = q.ky0 + t, X = q.kx0 + c;
  const bool ok = Y >= q.ny && Y < q.ny + NA_K && X >= q.nx && X < q.nx + NA_K;
  const float b = bias_s[ok ? nattn_rel(q.yc, q.xc, Y, X) : 0];
  return ok ? s * NA_SCALE + b : -INFINITY;
}

// ------------------------------------------------------------------------------ forward
// grid (tiles, H, B), 4 waves
__global__ __launch_bounds__(256) void nattn_fwd_kernel(NattnArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[NA_FWD_BYTES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
  const int ty = blockIdx.x / a.tx, tx = blockIdx.x - ty * a.tx, h = blockIdx.y, b = blockIdx.z;
  const NattnGeom gm = a.g;
  const int H = gm.H, HW = gm.Hf * gm.Wf;
  bf16_t* Vt = (bf16_t*)(lds + wave * NA_FWD_WAVE);
  bf16_t* patch = Vt + 2 * NA_PAIR;
  float* bias_s = (float*)(lds + 4 * NA_FWD_WAVE);
  for (int j = threadIdx.x; j < NA_NB; j += 256) bias_s[j] = a.rpb[(size_t)h * NA_NB + j];
  const QueryLane q = na_query_lane(gm, ty, tx, wave, i);
  const size_t hs = (size_t)H * NA_D, rs = 3 * hs;
  const bf16_t* qb = a.qkv + (size_t)b * HW * rs + (size_t)h * NA_D;
  const uint4 qf = q.on ? na_load(qb, rs, gm, q.yq, q.xq, g) : make_uint4(0, 0, 0, 0);
  uint4 kf[NA_SUB], vf[NA_SUB];
#pragma unroll
  for (int t = 0; t < NA_SUB; ++t) {
    kf[t] = na_load(qb + hs, rs, gm, q.ky0 + t, q.kx0 + i, g);
    vf[t] = na_load(qb + 2 * hs, rs, gm, q.ky0 + t, q.kx0 + i, g);
  }
  __syncthreads();
  float p[NA_SUB][4];
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < NA_SUB; ++t) {
    const f32x4 st = na_mfma(kf[t], qf, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[t][r] = na_score(st[r], bias_s, q, t, 4 * g + r);
      mx = fmaxf(mx, p[t][r]);
    }
  }
  const float m = na_group_max(mx);  // (finite: 49 keys of every query are unmasked)
  float rsum = 0.f;
#pragma unroll
  for (int t = 0; t < NA_SUB; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[t][r] = expf(p[t][r] - m);
      rsum += p[t][r];
    }
  const float l = na_group_sum(rsum);
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int mm = 0; mm < NA_SUB / 2; ++mm) {
    bf16_t* vt = Vt + (mm & 1) * NA_PAIR;
    na_store_tr(vt, 0, i, g, vf[2 * mm]);
    na_store_tr(vt, 1, i, g, vf[2 * mm + 1]);
    __syncthreads();
    const uint4 pb = na_pack(p[2 * mm], p[2 * mm + 1]);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) acc[dt] = na_mfma(na_frag(vt, 16 * dt + i, 8 * g), pb, acc[dt]);
  }
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[dt][r] = acc[dt][r] / l;
  na_patch_write(patch, acc, 1.0f, i, g);
  __syncthreads();
  const int rr = lane >> 2;
  na_patch_flush(patch, a.out + (size_t)b * HW * hs + (size_t)h * NA_D, hs, gm,
                 NA_TILE * ty + 2 * wave + (rr >> 3), NA_TILE * tx + (rr & 7), lane);
  if (g == 0 && q.on) a.lse[((size_t)b * H + h) * HW + q.yq * gm.Wf + q.xq] = m + logf(l);
}

// ----------------------------------------------------------------------------- backward, dQ
// grid (tiles, H, walks): the block walks images blockIdx.z bpw .. + bpw - 1 (< B) of its tile
__global__ __launch_bounds__(256) void nattn_dq_kernel(NattnArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[NA_DQ_BYTES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
  const int ty = blockIdx.x / a.tx, tx = blockIdx.x - ty * a.tx, h = blockIdx.y;
  const NattnGeom gm = a.g;
  const int H = gm.H, HW = gm.Hf * gm.Wf;
  bf16_t* Kt = (bf16_t*)(lds + wave * NA_DQ_WAVE);
  bf16_t* patch = Kt + 2 * NA_PAIR;
  float* bias_s = (float*)(lds + NA_DQ_BYTES - NA_NB * 4);
  for (int j = threadIdx.x; j < NA_NB; j += 256) bias_s[j] = a.rpb[(size_t)h * NA_NB + j];
  const QueryLane q = na_query_lane(gm, ty, tx, wave, i);
  const size_t hs = (size_t)H * NA_D, rs = 3 * hs;
  float dsacc[NA_SUB][4];  // the walk's fp32 dS: [key-row sub-tile][register]
#pragma unroll
  for (int t = 0; t < NA_SUB; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) dsacc[t][r] = 0.f;
  __syncthreads();

  const int b0 = blockIdx.z * a.bpw, b1 = min(b0 + a.bpw, gm.B);
  for (int b = b0; b < b1; ++b) {
    const bf16_t* qb = a.qkv + (size_t)b * HW * rs + (size_t)h * NA_D;
    const bf16_t* dob = a.d_o + (size_t)b * HW * hs + (size_t)h * NA_D;
    const size_t tok = ((size_t)b * H + h) * HW + (size_t)q.yc * gm.Wf + q.xc;
    const uint4 qf = q.on ? na_load(qb, rs, gm, q.yq, q.xq, g) : make_uint4(0, 0, 0, 0);
    const uint4 df = q.on ? na_load(dob, hs, gm, q.yq, q.xq, g) : make_uint4(0, 0, 0, 0);
    const float lse = q.on ? a.lse_in[tok] : INFINITY;  // (+inf: every P of a query outside the map is 0)
    uint4 kf[NA_SUB];
    float pv[NA_SUB][4], ds[NA_SUB][4];
    float dsum = 0.f;
#pragma unroll
    for (int t = 0; t < NA_SUB; ++t) {
      kf[t] = na_load(qb + hs, rs, gm, q.ky0 + t, q.kx0 + i, g);
      const uint4 vf = na_load(qb + 2 * hs, rs, gm, q.ky0 + t, q.kx0 + i, g);
      const f32x4 st = na_mfma(kf[t], qf, f32x4{0.f, 0.f, 0.f, 0.f});
      const f32x4 dp = na_mfma(vf, df, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pv[t][r] = expf(na_score(st[r], bias_s, q, t, 4 * g + r) - lse);
        ds[t][r] = dp[r];
        dsum = fmaf(pv[t][r], dp[r], dsum);
      }
    }
    const float delta = na_group_sum(dsum);
    if (g == 0 && q.on) a.delta[tok] = delta;
#pragma unroll
    for (int t = 0; t < NA_SUB; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ds[t][r] = pv[t][r] * (ds[t][r] - delta);
        dsacc[t][r] += ds[t][r];
      }
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int mm = 0; mm < NA_SUB / 2; ++mm) {
      bf16_t* kt = Kt + (mm & 1) * NA_PAIR;
      na_store_tr(kt, 0, i, g, kf[2 * mm]);
      na_store_tr(kt, 1, i, g, kf[2 * mm + 1]);
      __syncthreads();
      const uint4 dsb = na_pack(ds[2 * mm], ds[2 * mm + 1]);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) acc[dt] = na_mfma(na_frag(kt, 16 * dt + i, 8 * g), dsb, acc[dt]);
    }
    na_patch_write(patch, acc, NA_SCALE, i, g);
    __syncthreads();
    const int rr = lane >> 2;
    na_patch_flush(patch, a.out + (size_t)b * HW * rs + (size_t)h * NA_D, rs, gm,
                   NA_TILE * ty + 2 * wave + (rr >> 3), NA_TILE * tx + (rr & 7), lane);
  }

  // fold 64 queries x 128 slots -> 169 bins: thread (dy, dx) adds its entries in query order
  __syncthreads();
  float* fold = (float*)lds;  // [64][NA_FOLD_PITCH], over the waves' regions (not the bias)
#pragma unroll
  for (int t = 0; t < NA_SUB; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) fold[(16 * wave + i) * NA_FOLD_PITCH + 16 * t + 4 * g + r] = dsacc[t][r];
  __syncthreads();
  if (threadIdx.x < NA_NB) {
    const int dy = (int)threadIdx.x / NA_RPB - (NA_K - 1), dx = (int)threadIdx.x % NA_RPB - (NA_K - 1);
    float s = 0.f;
    for (int n = 0; n < 64; ++n) {
      const int y = NA_TILE * ty + (n >> 3), x = NA_TILE * tx + (n & 7), Y = y + dy, X = x + dx;
      if (y < gm.Hf && x < gm.Wf && nattn_in(y, Y, gm.Hf) && nattn_in(x, X, gm.Wf)) {
        const int t = Y - nattn_ni(NA_TILE * ty + 2 * (n >> 4), gm.Hf), c = X - q.kx0;
        s += fold[n * NA_FOLD_PITCH + 16 * t + c];
      }
    }
    a.slab[(((size_t)blockIdx.z * a.tiles + blockIdx.x) * H + h) * NA_NB + threadIdx.x] = s;
  }
}

// ------------------------------------------------------------------------- backward, dK / dV
// grid (tiles, H, B): wave w owns the 4 x 4 key patch (w / 2, w % 2) of the tile
__global__ __launch_bounds__(256) void nattn_dkv_kernel(NattnArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[NA_DKV_BYTES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
  const int ty = blockIdx.x / a.tx, tx = blockIdx.x - ty * a.tx, h = blockIdx.y, b = blockIdx.z;
  const NattnGeom gm = a.g;
  const int H = gm.H, Hf = gm.Hf, Wf = gm.Wf, HW = Hf * Wf;
  bf16_t* QD = (bf16_t*)(lds + wave * NA_DKV_WAVE);  // two stages of (Qt, dOt)
  bf16_t* pk = QD + 4 * NA_PAIR;
  bf16_t* pvv = pk + 16 * NA_PPITCH;
  float* ld_s = (float*)(pvv + 16 * NA_PPITCH);      // two stages of (lse [2][16], delta [2][16])
  float* bias_s = (float*)(lds + 4 * NA_DKV_WAVE);
  for (int j = threadIdx.x; j < NA_NB; j += 256) bias_s[j] = a.rpb[(size_t)h * NA_NB + j];
  const int Y0 = NA_TILE * ty + 4 * (wave >> 1), X0 = NA_TILE * tx + 4 * (wave & 1);
  const int Yk = Y0 + (i >> 2), Xk = X0 + (i & 3);   // the lane's key
  const bool kon = Yk < Hf && Xk < Wf;
  const int qy0 = nattn_qlo(min(Y0, Hf - 1), Hf), qx0 = nattn_qlo(min(X0, Wf - 1), Wf);
  int npairs = 0;  // block-uniform: the longer of the tile's two patch rows
#pragma unroll
  for (int py = 0; py < 2; ++py) {
    const int ya = min(NA_TILE * ty + 4 * py, Hf - 1), yb = min(NA_TILE * ty + 4 * py + 3, Hf - 1);
    npairs = max(npairs, (nattn_qhi(yb, Hf) - nattn_qlo(ya, Hf) + 2) / 2);
  }
  const size_t hs = (size_t)H * NA_D, rs = 3 * hs;
  const bf16_t* qb = a.qkv + (size_t)b * HW * rs + (size_t)h * NA_D;
  const bf16_t* dob = a.d_o + (size_t)b * HW * hs + (size_t)h * NA_D;
  const size_t hb = ((size_t)b * H + h) * HW;
  const uint4 kf = kon ? na_load(qb + hs, rs, gm, Yk, Xk, g) : make_uint4(0, 0, 0, 0);
  const uint4 vf = kon ? na_load(qb + 2 * hs, rs, gm, Yk, Xk, g) : make_uint4(0, 0, 0, 0);
  f32x4 accv[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  f32x4 acck[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  for (int mm = 0; mm < npairs; ++mm) {
    const int y = qy0 + 2 * mm;
    bf16_t* Qt = QD + (mm & 1) * 2 * NA_PAIR;
    bf16_t* Dt = Qt + NA_PAIR;
    float* ls = ld_s + (mm & 1) * 64;
    uint4 qf[2], df[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      qf[s] = na_load(qb, rs, gm, y + s, qx0 + i, g);
      df[s] = na_load(dob, hs, gm, y + s, qx0 + i, g);
      na_store_tr(Qt, s, i, g, qf[s]);
      na_store_tr(Dt, s, i, g, df[s]);
    }
    {  // lanes 0..31: lse of (row lane / 16, slot lane % 16), +inf outside the map; 32..63: delta
      const int yy = y + ((lane >> 4) & 1), xx = qx0 + (lane & 15);
      const bool on = yy < Hf && xx < Wf;
      const float* src = lane < 32 ? a.lse_in : a.delta_in;
      ls[lane] = on ? src[hb + (size_t)yy * Wf + xx] : (lane < 32 ? INFINITY : 0.f);
    }
    __syncthreads();
    float pv[2][4], ds[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const f32x4 st = na_mfma(qf[s], kf, f32x4{0.f, 0.f, 0.f, 0.f});
      const f32x4 dp = na_mfma(df[s], vf, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int yq = y + s, xq = qx0 + 4 * g + r;
        const bool ok = kon && yq < Hf && xq < Wf && nattn_in(yq, Yk, Hf) && nattn_in(xq, Xk, Wf);
        const float bias = bias_s[ok ? nattn_rel(yq, xq, Yk, Xk) : 0];
        pv[s][r] = ok ? expf(st[r] * NA_SCALE + bias - ls[16 * s + 4 * g + r]) : 0.f;
        ds[s][r] = pv[s][r] * (dp[r] - ls[32 + 16 * s + 4 * g + r]);
      }
    }
    const uint4 pb = na_pack(pv[0], pv[1]), dsb = na_pack(ds[0], ds[1]);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      accv[dt] = na_mfma(na_frag(Dt, 16 * dt + i, 8 * g), pb, accv[dt]);
      acck[dt] = na_mfma(na_frag(Qt, 16 * dt + i, 8 * g), dsb, acck[dt]);
    }
  }
  na_patch_write(pk, acck, NA_SCALE, i, g);
  na_patch_write(pvv, accv, 1.0f, i, g);
  __syncthreads();
  const int rr = lane >> 2;
  bf16_t* dk = a.out + (size_t)b * HW * rs + hs + (size_t)h * NA_D;
  na_patch_flush(pk, dk, rs, gm, Y0 + (rr >> 2), X0 + (rr & 3), lane);
  na_patch_flush(pvv, dk + hs, rs, gm, Y0 + (rr >> 2), X0 + (rr & 3), lane);
}

// drpb[h][idx] (+)= the slab rows' sum in row order: one thread per element
__global__ __launch_bounds__(256) void nattn_drpb_kernel(const float* __restrict__ slab,
                                                         float* __restrict__ drpb, int rows, int n,
                                                         int overwrite) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  float s = 0.f;
  for (int r = 0; r < rows; ++r) s += slab[(size_t)r * n + idx];
  drpb[idx] = overwrite ? s : drpb[idx] + s;
}

}  // namespace

int64_t nattn_ws_floats(const NattnGeom& g) { return nattn_plan(g).ws_floats; }

void nattn_fwd(const bf16_raw* qkv, const float* rpb, const NattnGeom& g, bf16_raw* o, float* lse,
               hipStream_t s) {
  const NattnPlan p = nattn_plan(g);
  NattnArgs a{};
  a.qkv = qkv; a.rpb = rpb; a.out = o; a.lse = lse; a.g = g; a.tx = p.tx; a.tiles = p.tiles;
  hipLaunchKernelGGL(nattn_fwd_kernel, dim3((unsigned)p.tiles, (unsigned)g.H, (unsigned)g.B), dim3(256), 0,
                     s, a);
  MPA_CHECK_LAUNCH();
}

void nattn_bwd(const bf16_raw* d_o, const bf16_raw* qkv, const float* lse, const float* rpb,
               const NattnGeom& g, bf16_raw* dqkv, float* drpb, bool overwrite, float* ws,
               hipStream_t s) {
  const NattnPlan p = nattn_plan(g);
  NattnArgs a{};
  a.qkv = qkv; a.d_o = d_o; a.rpb = rpb; a.lse_in = lse; a.out = dqkv; a.g = g;
  a.delta = ws; a.delta_in = ws; a.slab = ws + p.delta_floats;
  a.tx = p.tx; a.tiles = p.tiles; a.bpw = p.bpw;
  hipLaunchKernelGGL(nattn_dq_kernel, dim3((unsigned)p.tiles, (unsigned)g.H, (unsigned)p.walks), dim3(256),
                     0, s, a);
  hipLaunchKernelGGL(nattn_dkv_kernel, dim3((unsigned)p.tiles, (unsigned)g.H, (unsigned)g.B), dim3(256), 0,
                     s, a);
  const int n = g.H * NA_NB;
  hipLaunchKernelGGL(nattn_drpb_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.slab, drpb,
                     p.rows, n, overwrite ? 1 : 0);
  MPA_CHECK_LAUNCH();
}

}  // namespace mpa
