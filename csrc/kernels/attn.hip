// Fused multi-head self-attention (forward, backward) on v_mfma_f32_16x16x32_bf16 and the ViT
// token kernels, for gfx950.  Plan and LDS layout: attn_plan.h.
//
// qkv [B][S][3][H][64] bf16 is the in-projection's output; q, k and v of head h are read in
// place (row stride 3 H 64).  Scores and probabilities live in registers only.
//
//  * Every score tile is computed TRANSPOSED with respect to the tile its block owns: the
//    forward and attn_bwd_dq (owning 16 query rows per wave) compute S^T = K Q^T, attn_bwd_dkv
//    (owning 16 key rows per wave) computes S = Q K^T.  The MFMA's C layout (lane (i, g), i =
//    lane % 16, g = lane / 16, holds rows 4 g .. 4 g + 3 of column i) then gives every lane 16
//    scores of ONE owned row i per 64-wide streamed tile, so
//      - the online-softmax state (running max, running sum), lse and delta are one scalar
//        per lane, the accumulator rescale is a per-lane multiply, and the row reductions are
//        16 register operations and two xor shuffles (16, 32);
//      - P (or dS), rounded to bf16, is already the B operand of the second product
//        O^T = V^T P^T (dV^T = dO^T P, dK^T = Q^T dS, dQ^T = K^T dS^T): no LDS round trip.  Its
//        k axis runs over streamed rows in the order at_pos(), and the other operand is staged
//        transposed in that order, so its fragment is one 16-B LDS read.
//  * All accumulators are fp32; P and dS are rounded to bf16 only as MFMA operands; the row
//    sum uses the unrounded P.  The scale 1/8 is applied to the fp32 scores (exact).
//  * No atomics: dK / dV and dQ come from two kernels that each recompute P from lse.
//    delta_i = sum_d dO_id O_id is computed in fp32 where the dO rows are loaded.
#include "api.h"
#include "common.h"
#include "attn_plan.h"
#include "attn_frag.h"

namespace mpa {
namespace {

struct AttnArgs {
  const bf16_t* qkv;
  const bf16_t* o;
  const bf16_t* d_o;
  const float* lse_in;
  bf16_t* out;  // forward: o [B][S][H 64]; backward: dqkv
  float* lse;   // forward: [B][H][S]
  int S, H;
};

// ------------------------------------------------------------------------------ forward
// grid (query tiles, H, B).  K rows and V transposed stream through a two-stage LDS ring: the
// next tile's global loads are issued before the current tile's MFMAs and land in the other
// stage after them, one barrier per tile.
__global__ __launch_bounds__(AT_THREADS) void attn_fwd_kernel(AttnArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t lds[4 * TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z, S = a.S;
  const size_t rs = (size_t)3 * a.H * AT_D, hs = (size_t)a.H * AT_D;
  const bf16_t* qb = a.qkv + (size_t)b * S * rs + (size_t)h * AT_D;
  const bf16_t* kb = qb + hs;
  const bf16_t* vb = kb + hs;
  const int q0 = blockIdx.x * AT_TILE + wave * 16, qrow = q0 + i;
  const bool active = q0 < S;  // (wave-uniform)
  bf16x8 qf[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
    qf[kk] = as_frag(qrow < S ? ld16(qb + (size_t)qrow * rs + 32 * kk + 8 * g)
                              : make_uint4(0, 0, 0, 0));
  float m = -INFINITY, l = 0.f;
  f32x4 acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nkt = (S + AT_TILE - 1) / AT_TILE;
  uint4 kr[2], vr[2];
  tile_load(kb, rs, 0, S, tid, kr);
  tile_load(vb, rs, 0, S, tid, vr);
  tile_store_rows(lds, tid, kr);
  tile_store_tr(lds + TILE, tid, vr);
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const bf16_t* Ks = lds + (kt & 1) * 2 * TILE;
    const bf16_t* Vt = Ks + TILE;
    const bool more = kt + 1 < nkt;
    if (more) {
      tile_load(kb, rs, (kt + 1) * AT_TILE, S, tid, kr);
      tile_load(vb, rs, (kt + 1) * AT_TILE, S, tid, vr);
    }
    if (active) {
      float p[4][4];
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        f32x4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) st = at_mfma(frag(Ks, 16 * t + i, 32 * kk + 8 * g), qf[kk], st);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // LDS holds zeros for keys >= S, whose score 0 must not enter the maximum or the sum
          const bool on = kt * AT_TILE + at_acc_row(t, g, r) < S;
          p[t][r] = on ? st[r] * 0.125f : -INFINITY;
          mx = fmaxf(mx, p[t][r]);
        }
      }
      const float mn = fmaxf(m, group_max(mx));  // (finite: a tile's first key is < S)
      const float alpha = expf(m - mn);
      float rsum = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p[t][r] = expf(p[t][r] - mn);
          rsum += p[t][r];
        }
      l = fmaf(l, alpha, group_sum(rsum));
      m = mn;
      bf16x8 pb[2];
      pack_halves(p, pb);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        acc[dt] *= alpha;
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
          acc[dt] = at_mfma(frag(Vt, 16 * dt + i, 32 * hh + 8 * g), pb[hh], acc[dt]);
      }
    }
    if (more) {
      bf16_t* nK = lds + ((kt + 1) & 1) * 2 * TILE;
      tile_store_rows(nK, tid, kr);
      tile_store_tr(nK + TILE, tid, vr);
    }
    __syncthreads();
  }

  // o = acc / l through the wave's LDS patch (the ring is free after the last barrier)
  bf16_t* patch = lds + wave * 16 * AT_PITCH;
  if (active) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[dt][r] = acc[dt][r] / l;
    patch_write(patch, acc, 1.0f, lane);
  }
  __syncthreads();
  if (active) {
    patch_flush(patch, a.out + (size_t)b * S * hs + (size_t)h * AT_D, hs, q0, S, lane);
    if (g == 0 && qrow < S) a.lse[((size_t)b * a.H + h) * S + qrow] = m + logf(l);
  }
}

// ------------------------------------------------------------------------- backward: dQ
// grid (query tiles, H, B); the wave's Q and dO fragments, lse and delta stay in registers;
// K rows, V rows and K transposed stream through LDS.  dQ = (dS K) / 8.
__global__ __launch_bounds__(AT_THREADS) void attn_bwd_dq_kernel(AttnArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t lds[3 * TILE];
  bf16_t* Ks = lds;
  bf16_t* Vs = lds + TILE;
  bf16_t* Kt = lds + 2 * TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z, S = a.S;
  const size_t rs = (size_t)3 * a.H * AT_D, hs = (size_t)a.H * AT_D;
  const bf16_t* qb = a.qkv + (size_t)b * S * rs + (size_t)h * AT_D;
  const bf16_t* kb = qb + hs;
  const bf16_t* vb = kb + hs;
  const size_t ob = (size_t)b * S * hs + (size_t)h * AT_D;
  const int q0 = blockIdx.x * AT_TILE + wave * 16, qrow = q0 + i;
  const bool active = q0 < S, rowok = qrow < S;
  bf16x8 qf[2], dof[2];
  float dsum = 0.f;
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const uint4 z = make_uint4(0, 0, 0, 0);
    const int col = 32 * kk + 8 * g;
    const uint4 dv = rowok ? ld16(a.d_o + ob + (size_t)qrow * hs + col) : z;
    const uint4 ov = rowok ? ld16(a.o + ob + (size_t)qrow * hs + col) : z;
    qf[kk] = as_frag(rowok ? ld16(qb + (size_t)qrow * rs + col) : z);
    dof[kk] = as_frag(dv);
    float df[8], of[8];
    unpack8(dv, df);
    unpack8(ov, of);
#pragma unroll
    for (int e = 0; e < 8; ++e) dsum = fmaf(df[e], of[e], dsum);
  }
  const float delta = group_sum(dsum);
  // (rows >= S: lse = +inf makes every P zero)
  const float lse = rowok ? a.lse_in[((size_t)b * a.H + h) * S + qrow] : INFINITY;
  f32x4 acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nkt = (S + AT_TILE - 1) / AT_TILE;
  for (int kt = 0; kt < nkt; ++kt) {
    uint4 kr[2], vr[2];
    tile_load(kb, rs, kt * AT_TILE, S, tid, kr);
    tile_load(vb, rs, kt * AT_TILE, S, tid, vr);
    __syncthreads();  // the previous tile's reads are done
    tile_store_rows(Ks, tid, kr);
    tile_store_rows(Vs, tid, vr);
    tile_store_tr(Kt, tid, kr);
    __syncthreads();
    if (!active) continue;
    float ds[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f32x4 st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        st = at_mfma(frag(Ks, 16 * t + i, 32 * kk + 8 * g), qf[kk], st);
        dp = at_mfma(frag(Vs, 16 * t + i, 32 * kk + 8 * g), dof[kk], dp);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool on = kt * AT_TILE + at_acc_row(t, g, r) < S;
        const float p = on ? expf(st[r] * 0.125f - lse) : 0.f;
        ds[t][r] = p * (dp[r] - delta);
      }
    }
    bf16x8 dsb[2];
    pack_halves(ds, dsb);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
        acc[dt] = at_mfma(frag(Kt, 16 * dt + i, 32 * hh + 8 * g), dsb[hh], acc[dt]);
  }
  __syncthreads();
  bf16_t* patch = lds + wave * 16 * AT_PITCH;
  if (active) patch_write(patch, acc, 0.125f, lane);
  __syncthreads();
  if (active) patch_flush(patch, a.out + (size_t)b * S * rs + (size_t)h * AT_D, rs, q0, S, lane);
}

// -------------------------------------------------------------------- backward: dK, dV
// grid (key tiles, H, B); the wave's K and V fragments stay in registers; Q and dO (rows and
// transposed), lse and delta of a query tile stream through LDS.
// dV = P^T dO, dK = (dS^T Q) / 8; query rows >= S carry lse = +inf, so P = 0.
__global__ __launch_bounds__(AT_THREADS) void attn_bwd_dkv_kernel(AttnArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t lds[4 * TILE];
  __shared__ float lse_s[AT_TILE], del_s[AT_TILE];
  bf16_t* Qs = lds;
  bf16_t* Ds = lds + TILE;
  bf16_t* Qt = lds + 2 * TILE;
  bf16_t* Dt = lds + 3 * TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z, S = a.S;
  const size_t rs = (size_t)3 * a.H * AT_D, hs = (size_t)a.H * AT_D;
  const bf16_t* qb = a.qkv + (size_t)b * S * rs + (size_t)h * AT_D;
  const bf16_t* kb = qb + hs;
  const bf16_t* vb = kb + hs;
  const bf16_t* dob = a.d_o + (size_t)b * S * hs + (size_t)h * AT_D;
  const bf16_t* oub = a.o + (size_t)b * S * hs + (size_t)h * AT_D;
  const float* lseb = a.lse_in + ((size_t)b * a.H + h) * S;
  const int k0 = blockIdx.x * AT_TILE + wave * 16, krow = k0 + i;
  const bool active = k0 < S;
  bf16x8 kf[2], vf[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const uint4 z = make_uint4(0, 0, 0, 0);
    kf[kk] = as_frag(krow < S ? ld16(kb + (size_t)krow * rs + 32 * kk + 8 * g) : z);
    vf[kk] = as_frag(krow < S ? ld16(vb + (size_t)krow * rs + 32 * kk + 8 * g) : z);
  }
  f32x4 accv[4], acck[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    accv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    acck[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const int nqt = (S + AT_TILE - 1) / AT_TILE;
  for (int qt = 0; qt < nqt; ++qt) {
    uint4 qr[2], dr[2], orr[2];
    tile_load(qb, rs, qt * AT_TILE, S, tid, qr);
    tile_load(dob, hs, qt * AT_TILE, S, tid, dr);
    tile_load(oub, hs, qt * AT_TILE, S, tid, orr);
    // delta of rows (tid >> 3) (+ 32): the row's eight vectors sit in eight adjacent lanes
    float dl[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      float df[8], of[8], s = 0.f;
      unpack8(dr[p], df);
      unpack8(orr[p], of);
#pragma unroll
      for (int e = 0; e < 8; ++e) s = fmaf(df[e], of[e], s);
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 4, 64);
      dl[p] = s;
    }
    __syncthreads();  // the previous tile's reads are done
    tile_store_rows(Qs, tid, qr);
    tile_store_rows(Ds, tid, dr);
    tile_store_tr(Qt, tid, qr);
    tile_store_tr(Dt, tid, dr);
    if ((tid & 7) == 0) {
      del_s[tid >> 3] = dl[0];
      del_s[(tid >> 3) + 32] = dl[1];
    }
    if (tid < AT_TILE) lse_s[tid] = qt * AT_TILE + tid < S ? lseb[qt * AT_TILE + tid] : INFINITY;
    __syncthreads();
    if (!active) continue;
    float pv[4][4], ds[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f32x4 st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        st = at_mfma(frag(Qs, 16 * t + i, 32 * kk + 8 * g), kf[kk], st);
        dp = at_mfma(frag(Ds, 16 * t + i, 32 * kk + 8 * g), vf[kk], dp);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = at_acc_row(t, g, r);
        pv[t][r] = expf(st[r] * 0.125f - lse_s[q]);
        ds[t][r] = pv[t][r] * (dp[r] - del_s[q]);
      }
    }
    bf16x8 pb[2], dsb[2];
    pack_halves(pv, pb);
    pack_halves(ds, dsb);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        accv[dt] = at_mfma(frag(Dt, 16 * dt + i, 32 * hh + 8 * g), pb[hh], accv[dt]);
        acck[dt] = at_mfma(frag(Qt, 16 * dt + i, 32 * hh + 8 * g), dsb[hh], acck[dt]);
      }
  }
  __syncthreads();
  bf16_t* pk = Qs + wave * 16 * AT_PITCH;
  bf16_t* pvv = Ds + wave * 16 * AT_PITCH;
  if (active) {
    patch_write(pk, acck, 0.125f, lane);
    patch_write(pvv, accv, 1.0f, lane);
  }
  __syncthreads();
  if (active) {
    bf16_t* ob = a.out + (size_t)b * S * rs + (size_t)h * AT_D;
    patch_flush(pk, ob + hs, rs, k0, S, lane);
    patch_flush(pvv, ob + 2 * hs, rs, k0, S, lane);
  }
}

// ------------------------------------------------------------------------ token kernels
__global__ __launch_bounds__(256) void patchify_kernel(const bf16_t* __restrict__ x,
                                                       bf16_t* __restrict__ out, PatchGeom g,
                                                       int64_t nvec) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  st_stream(out + i * 8, ld_stream(x + patch_src(g, i)));
}

// the inverse permutation: vector i of the rows back to its place in x
__global__ __launch_bounds__(256) void unpatchify_kernel(const bf16_t* __restrict__ rows,
                                                         bf16_t* __restrict__ x, PatchGeom g,
                                                         int64_t nvec) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  st_stream(x + patch_src(g, i), ld_stream(rows + i * 8));
}

__device__ __forceinline__ void ld8f(const float* p, float* f) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
  f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

// x[b][0] = cls + pos[0]; x[b][1 + i] = patch[b][i] + pos[1 + i]: fp32 add, one rounding
__global__ __launch_bounds__(256) void tokens_fwd_kernel(const bf16_t* __restrict__ patch,
                                                         const float* __restrict__ cls,
                                                         const float* __restrict__ pos,
                                                         bf16_t* __restrict__ x, TokGeom g,
                                                         int64_t nvec) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  const int dv = g.D / 8;
  const int d8 = (int)(i % dv), t = (int)((i / dv) % g.T);
  const int64_t b = i / ((int64_t)dv * g.T);
  float v[8], pf[8];
  if (t == 0) ld8f(cls + d8 * 8, v);
  else unpack8(ld_stream(patch + ((b * (g.T - 1) + t - 1) * g.D + d8 * 8)), v);
  ld8f(pos + (size_t)t * g.D + d8 * 8, pf);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] += pf[j];
  st_stream(x + i * 8, pack8(v));
}

// thread (t, vector): dpos[t] (+)= sum_b dx[b][t] in batch order (fp32), dpatch = dx[:, 1:];
// the t = 0 threads also write dcls.  One thread owns a column's whole sum: fixed order.
__global__ __launch_bounds__(256) void tokens_bwd_kernel(const bf16_t* __restrict__ dx,
                                                         bf16_t* __restrict__ dpatch,
                                                         float* __restrict__ dcls,
                                                         float* __restrict__ dpos, TokGeom g,
                                                         int overwrite) {
  const int dv = g.D / 8;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= g.T * dv) return;
  const int t = i / dv, d8 = i - t * dv;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int b = 0; b < g.B; ++b) {
    const uint4 w = ld_stream(dx + ((size_t)b * g.T + t) * g.D + d8 * 8);
    if (t > 0) st_stream(dpatch + ((size_t)b * (g.T - 1) + t - 1) * g.D + d8 * 8, w);
    float f[8];
    unpack8(w, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] += f[j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float* o = dpos + (size_t)t * g.D + d8 * 8 + j;
    *o = overwrite ? s[j] : *o + s[j];
    if (t == 0) {
      float* c = dcls + d8 * 8 + j;
      *c = overwrite ? s[j] : *c + s[j];
    }
  }
}

AttnArgs attn_args(const AttnGeom& g) {
  AttnArgs a{};
  a.S = g.S;
  a.H = g.H;
  return a;
}

dim3 attn_grid(const AttnGeom& g) {
  return dim3((unsigned)attn_plan(g).tiles, (unsigned)g.H, (unsigned)g.B);
}

}  // namespace

void attn_fwd(const bf16_raw* qkv, const AttnGeom& g, bf16_raw* o, float* lse, hipStream_t s) {
  AttnArgs a = attn_args(g);
  a.qkv = qkv; a.out = o; a.lse = lse;
  hipLaunchKernelGGL(attn_fwd_kernel, attn_grid(g), dim3(AT_THREADS), 0, s, a);
  MPA_CHECK_LAUNCH();
}

void attn_bwd(const bf16_raw* d_o, const bf16_raw* qkv, const bf16_raw* o, const float* lse,
              const AttnGeom& g, bf16_raw* dqkv, hipStream_t s) {
  AttnArgs a = attn_args(g);
  a.qkv = qkv; a.o = o; a.d_o = d_o; a.lse_in = lse; a.out = dqkv;
  hipLaunchKernelGGL(attn_bwd_dkv_kernel, attn_grid(g), dim3(AT_THREADS), 0, s, a);
  hipLaunchKernelGGL(attn_bwd_dq_kernel, attn_grid(g), dim3(AT_THREADS), 0, s, a);
  MPA_CHECK_LAUNCH();
}

void patchify(const bf16_raw* x, const PatchGeom& g, bf16_raw* rows, hipStream_t s) {
  const int64_t nvec = (int64_t)g.B * g.Hi * g.Wi * g.Cp / 8;
  hipLaunchKernelGGL(patchify_kernel, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, s, x,
                     rows, g, nvec);
  MPA_CHECK_LAUNCH();
}

void unpatchify(const bf16_raw* rows, const PatchGeom& g, bf16_raw* x, hipStream_t s) {
  const int64_t nvec = (int64_t)g.B * g.Hi * g.Wi * g.Cp / 8;
  hipLaunchKernelGGL(unpatchify_kernel, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, s,
                     rows, x, g, nvec);
  MPA_CHECK_LAUNCH();
}

void tokens_fwd(const bf16_raw* patch, const float* cls, const float* pos, const TokGeom& g,
                bf16_raw* x, hipStream_t s) {
  const int64_t nvec = (int64_t)g.B * g.T * (g.D / 8);
  hipLaunchKernelGGL(tokens_fwd_kernel, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, s,
                     patch, cls, pos, x, g, nvec);
  MPA_CHECK_LAUNCH();
}

void tokens_bwd(const bf16_raw* dx, const TokGeom& g, bf16_raw* dpatch, float* dcls, float* dpos,
                bool overwrite, hipStream_t s) {
  const int n = g.T * (g.D / 8);
  hipLaunchKernelGGL(tokens_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dx,
                     dpatch, dcls, dpos, g, overwrite ? 1 : 0);
  MPA_CHECK_LAUNCH();
}

}  // namespace mpa
