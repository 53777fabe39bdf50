// Cross-attention with a short key set (forward, backward) on v_mfma_f32_16x16x32_bf16, for
// gfx950: PVT v2's spatial-reduction attention.  Plan and LDS map: xattn_plan.h.
//
// q [B][Sq][H][64] and kv [B][Sk][2][H][64] bf16 are read in place, 1 <= Sk <= 64.  All keys and
// values of a (batch, head) are ONE tile of attn_plan.h's layout: a block stages it once and
// walks query tiles, so nothing of attn.hip's key loop is left: no ring, no running maximum, no
// accumulator rescale.  What streams is Q (and dO, o) from global memory straight into MFMA
// fragments, the next tile's loads issued before the current tile's MFMAs.
//
//  * Scores are computed transposed, S^T = K Q^T, as in attn.hip: lane (i, g) holds the 16
//    scores of query row i for keys at_acc_row(t, g, r), so the softmax is max, exp, sum over 16
//    registers and two xor shuffles, and P (dS), rounded to bf16, is already the B operand of
//    O^T = V^T P^T (dQ^T = K^T dS^T) with V^T (K^T) staged in at_pos order.
//  * Keys j >= Sk hold zeros in LDS; their scores are masked out of the maximum and the sum
//    (a score of 0 is not a masked score).
//  * Backward, one attention pass: per tile a wave recomputes P from lse, forms delta = sum_d
//    dO o in fp32 where both are loaded, dP, dS and its rows' dQ, which is complete (all keys
//    are here).  dK and dV contract over queries, the axis the lanes of S^T do not hold, so the
//    waves exchange bf16 P^T, dS^T, Q^T and dO^T through LDS once per tile, and wave w then owns
//    keys 16 w .. 16 w + 15 of dK^T = Q^T dS and dV^T = dO^T P, accumulated in registers over the
//    walk.  S is computed once.
//  * No atomics: a block writes its dK^T / dV^T as one fp32 slab row, and xattn_dkv_sum_kernel
//    sums the rows of a (batch, head) in row order, scales dK by 1/8 and rounds to bf16 once.
#include "api.h"
#include "common.h"
#include "xattn_plan.h"
#include "attn_frag.h"

namespace mpa {
namespace {

struct XattnArgs {
  const bf16_t* q;
  const bf16_t* kv;
  const bf16_t* o;
  const bf16_t* d_o;
  const float* lse_in;
  bf16_t* out;  // forward: o [B][Sq][H 64]; backward: dq
  float* lse;   // forward: [B][H][Sq]
  float* slab;  // backward: [B][H][walks][2][64][64]
  int Sq, Sk, H, tiles, tpw;
};

// the two fragments (columns 32 kk + 8 g ..) of row `row` of a [.][64] operand; rows >= S are zero
__device__ __forceinline__ void row_load(const bf16_t* base, size_t stride, int row, int S, int g,
                                         uint4 (&v)[2]) {
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
    v[kk] = row < S ? ld16(base + (size_t)row * stride + 32 * kk + 8 * g) : make_uint4(0, 0, 0, 0);
}

// a lane's row fragments to column `col` of a transposed tile: element d of the row to tile[d][col]
__device__ __forceinline__ void row_store_tr(bf16_t* tile, int col, int g, const uint4 (&v)[2]) {
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const uint32_t w[4] = {v[kk].x, v[kk].y, v[kk].z, v[kk].w};
#pragma unroll
    for (int e = 0; e < 8; ++e)
      tile[(32 * kk + 8 * g + e) * AT_PITCH + col] = (bf16_t)(w[e >> 1] >> (16 * (e & 1)));
  }
}

// a lane's 16 accumulator values (keys at_acc_row(t, g, r)) to column `col` of a [key][.] tile
__device__ __forceinline__ void acc_store_tr(bf16_t* tile, int col, int g, const float (&p)[4][4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) tile[at_acc_row(t, g, r) * AT_PITCH + col] = f2bf(p[t][r]);
}

// ------------------------------------------------------------------------------ forward
// grid (walks, H, B): K rows and V transposed staged once, then `tpw` query tiles.
__global__ __launch_bounds__(AT_THREADS) void xattn_fwd_kernel(XattnArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t lds[3 * TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z, Sq = a.Sq, Sk = a.Sk;
  const size_t hs = (size_t)a.H * AT_D, ks = 2 * hs;
  const bf16_t* Ks = lds;
  const bf16_t* Vt = lds + TILE;
  bf16_t* patch = lds + 2 * TILE + wave * 16 * AT_PITCH;
  const bf16_t* qb = a.q + (size_t)b * Sq * hs + (size_t)h * AT_D;
  const bf16_t* kb = a.kv + (size_t)b * Sk * ks + (size_t)h * AT_D;
  bf16_t* ob = a.out + (size_t)b * Sq * hs + (size_t)h * AT_D;
  float* lseb = a.lse + ((size_t)b * a.H + h) * Sq;
  const int t0 = blockIdx.x * a.tpw, t1 = min(a.tiles, t0 + a.tpw);

  uint4 kr[2], vr[2], qn[2];
  tile_load(kb, ks, 0, Sk, tid, kr);
  tile_load(kb + hs, ks, 0, Sk, tid, vr);
  row_load(qb, hs, t0 * AT_TILE + wave * 16 + i, Sq, g, qn);
  tile_store_rows(lds, tid, kr);
  tile_store_tr(lds + TILE, tid, vr);
  __syncthreads();

  for (int t = t0; t < t1; ++t) {
    const int q0 = t * AT_TILE + wave * 16, qrow = q0 + i;
    const bool active = q0 < Sq;  // (wave-uniform)
    const bf16x8 qf[2] = {as_frag(qn[0]), as_frag(qn[1])};
    if (t + 1 < t1) row_load(qb, hs, qrow + AT_TILE, Sq, g, qn);
    f32x4 acc[4];
    float m = 0.f, l = 1.f;
    if (active) {
      float p[4][4];
      float mx = -INFINITY;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        f32x4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) st = at_mfma(frag(Ks, 16 * s + i, 32 * kk + 8 * g), qf[kk], st);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p[s][r] = at_acc_row(s, g, r) < Sk ? st[r] * 0.125f : -INFINITY;
          mx = fmaxf(mx, p[s][r]);
        }
      }
      m = group_max(mx);  // (finite: key 0 is valid)
      float rsum = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p[s][r] = expf(p[s][r] - m);
          rsum += p[s][r];
        }
      l = group_sum(rsum);
      bf16x8 pb[2];
      pack_halves(p, pb);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
          acc[dt] = at_mfma(frag(Vt, 16 * dt + i, 32 * hh + 8 * g), pb[hh], acc[dt]);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[dt][r] = acc[dt][r] / l;
      }
      patch_write(patch, acc, 1.0f, lane);
    }
    __syncthreads();  // the patch is wave-private: the barrier orders its write and its reads
    if (active) {
      patch_flush(patch, ob, hs, q0, Sq, lane);
      if (g == 0 && qrow < Sq) lseb[qrow] = m + logf(l);
    }
  }
}

// ----------------------------------------------------------------------------- backward
// grid (walks, H, B).  Per tile: phase A (wave w owns query rows 16 w ..) P, dS, dQ; exchange
// through LDS; phase B (wave w owns keys 16 w ..) dK^T, dV^T += over the tile's 64 queries.
__global__ __launch_bounds__(AT_THREADS) void xattn_bwd_kernel(XattnArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t lds[7 * TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z, Sq = a.Sq, Sk = a.Sk;
  const size_t hs = (size_t)a.H * AT_D, ks = 2 * hs;
  const bf16_t* Ks = lds;
  const bf16_t* Vs = lds + TILE;
  const bf16_t* Kt = lds + 2 * TILE;
  bf16_t* Qt = lds + 3 * TILE;
  bf16_t* Dt = lds + 4 * TILE;
  bf16_t* Pt = lds + 5 * TILE;
  bf16_t* St = lds + 6 * TILE;
  bf16_t* patch = Pt + wave * 16 * AT_PITCH;  // (rows only this wave reads in phase B)
  const size_t qofs = (size_t)b * Sq * hs + (size_t)h * AT_D;
  const bf16_t* qb = a.q + qofs;
  const bf16_t* dob = a.d_o + qofs;
  const bf16_t* oub = a.o + qofs;
  const bf16_t* kb = a.kv + (size_t)b * Sk * ks + (size_t)h * AT_D;
  const float* lseb = a.lse_in + ((size_t)b * a.H + h) * Sq;
  const int t0 = blockIdx.x * a.tpw, t1 = min(a.tiles, t0 + a.tpw);
  const int col = wave * 16 + i;           // phase A: this lane's query of the tile
  const bool kown = wave * 16 < Sk;        // phase B: this wave owns valid keys (wave-uniform)

  uint4 kr[2], vr[2], qn[2], dn[2], on[2];
  tile_load(kb, ks, 0, Sk, tid, kr);
  tile_load(kb + hs, ks, 0, Sk, tid, vr);
  const int first = t0 * AT_TILE + col;
  row_load(qb, hs, first, Sq, g, qn);
  row_load(dob, hs, first, Sq, g, dn);
  row_load(oub, hs, first, Sq, g, on);
  // (rows >= Sq: lse = +inf makes every P zero)
  float lse_n = first < Sq ? lseb[first] : INFINITY;
  tile_store_rows(lds, tid, kr);
  tile_store_rows(lds + TILE, tid, vr);
  tile_store_tr(lds + 2 * TILE, tid, kr);
  f32x4 acck[4], accv[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    acck[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    accv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  __syncthreads();

  for (int t = t0; t < t1; ++t) {
    const int q0 = t * AT_TILE + wave * 16, qrow = q0 + i;
    const bool active = q0 < Sq;  // (wave-uniform)
    const uint4 qr[2] = {qn[0], qn[1]}, dr[2] = {dn[0], dn[1]};
    const bf16x8 qf[2] = {as_frag(qr[0]), as_frag(qr[1])}, dof[2] = {as_frag(dr[0]), as_frag(dr[1])};
    const float lse = lse_n;
    float dsum = 0.f;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      float df[8], of[8];
      unpack8(dr[kk], df);
      unpack8(on[kk], of);
#pragma unroll
      for (int e = 0; e < 8; ++e) dsum = fmaf(df[e], of[e], dsum);
    }
    const float delta = group_sum(dsum);
    if (t + 1 < t1) {
      const int nrow = qrow + AT_TILE;
      row_load(qb, hs, nrow, Sq, g, qn);
      row_load(dob, hs, nrow, Sq, g, dn);
      row_load(oub, hs, nrow, Sq, g, on);
      lse_n = nrow < Sq ? lseb[nrow] : INFINITY;
    }

    // phase A
    float pv[4][4], ds[4][4];
    f32x4 accq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) accq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (active) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        f32x4 st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          st = at_mfma(frag(Ks, 16 * s + i, 32 * kk + 8 * g), qf[kk], st);
          dp = at_mfma(frag(Vs, 16 * s + i, 32 * kk + 8 * g), dof[kk], dp);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          pv[s][r] = at_acc_row(s, g, r) < Sk ? expf(st[r] * 0.125f - lse) : 0.f;
          ds[s][r] = pv[s][r] * (dp[r] - delta);
        }
      }
      bf16x8 dsb[2];
      pack_halves(ds, dsb);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
          accq[dt] = at_mfma(frag(Kt, 16 * dt + i, 32 * hh + 8 * g), dsb[hh], accq[dt]);
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) pv[s][r] = ds[s][r] = 0.f;
    }

    __syncthreads();  // the previous tile's phase B reads and dQ flush are done
    row_store_tr(Qt, col, g, qr);
    row_store_tr(Dt, col, g, dr);
    acc_store_tr(Pt, col, g, pv);
    acc_store_tr(St, col, g, ds);
    __syncthreads();

    // phase B: B operands are this wave's key rows of P^T / dS^T, k axis = the tile's queries
    if (kown) {
      bf16x8 pb[2], sb[2];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        pb[hh] = frag(Pt, col, 32 * hh + 8 * g);
        sb[hh] = frag(St, col, 32 * hh + 8 * g);
      }
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          accv[dt] = at_mfma(frag(Dt, 16 * dt + i, 32 * hh + 8 * g), pb[hh], accv[dt]);
          acck[dt] = at_mfma(frag(Qt, 16 * dt + i, 32 * hh + 8 * g), sb[hh], acck[dt]);
        }
    }
    // dQ = (dS K) / 8 through the wave's patch (after its own reads of those P^T rows)
    if (active) patch_write(patch, accq, 0.125f, lane);
    __syncthreads();  // the patch is wave-private: the barrier orders its write and its reads
    if (active) patch_flush(patch, a.out + qofs, hs, q0, Sq, lane);
  }

  // acc[dt][r] = X^T[16 dt + 4 g + r][key col]: four floats of the key's slab row; keys >= Sk
  // are never written
  if (kown && col < Sk) {
    float* row = a.slab + (((size_t)b * a.H + h) * gridDim.x + blockIdx.x) * XA_SLAB_ROW +
                 (size_t)col * AT_D;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      *(f32x4*)(row + 16 * dt + 4 * g) = acck[dt];
      *(f32x4*)(row + AT_TILE * AT_D + 16 * dt + 4 * g) = accv[dt];
    }
  }
}

// thread = one 16-B vector of dkv [B][Sk][2][H][64]: the slab rows of its (batch, head) in row
// order, dK scaled by 1/8 (exact), one rounding
__global__ __launch_bounds__(256) void xattn_dkv_sum_kernel(const float* __restrict__ slab,
                                                            bf16_t* __restrict__ dkv, int Sk, int H,
                                                            int walks, int64_t nvec) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nvec) return;
  const int d8 = (int)(v & 7);
  int64_t r = v >> 3;
  const int h = (int)(r % H);
  r /= H;
  const int which = (int)(r & 1);
  r >>= 1;
  const int key = (int)(r % Sk);
  const int64_t b = r / Sk;
  const float* src = slab + ((b * H + h) * walks) * XA_SLAB_ROW + (size_t)which * AT_TILE * AT_D +
                     (size_t)key * AT_D + d8 * 8;
  float s[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = 0.f;
  for (int w = 0; w < walks; ++w) {
    const f32x4 lo = *(const f32x4*)(src + (size_t)w * XA_SLAB_ROW);
    const f32x4 hi = *(const f32x4*)(src + (size_t)w * XA_SLAB_ROW + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] += lo[j];
      s[4 + j] += hi[j];
    }
  }
  const float scale = which == 0 ? 0.125f : 1.0f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] *= scale;
  *(uint4*)(dkv + v * 8) = pack8(s);
}

XattnArgs xattn_args(const XattnGeom& g, const XattnPlan& p) {
  XattnArgs a{};
  a.Sq = g.Sq; a.Sk = g.Sk; a.H = g.H; a.tiles = p.tiles; a.tpw = p.tpw;
  return a;
}

}  // namespace

void xattn_fwd(const bf16_raw* q, const bf16_raw* kv, const XattnGeom& g, bf16_raw* o, float* lse,
               hipStream_t s) {
  const XattnPlan p = xattn_plan(g);
  XattnArgs a = xattn_args(g, p);
  a.q = q; a.kv = kv; a.out = o; a.lse = lse;
  hipLaunchKernelGGL(xattn_fwd_kernel, dim3((unsigned)p.walks, (unsigned)g.H, (unsigned)g.B),
                     dim3(AT_THREADS), 0, s, a);
  MPA_CHECK_LAUNCH();
}

int64_t xattn_ws_floats(const XattnGeom& g) { return xattn_plan(g).ws_floats; }

void xattn_bwd(const bf16_raw* d_o, const bf16_raw* q, const bf16_raw* kv, const bf16_raw* o,
               const float* lse, const XattnGeom& g, bf16_raw* dq, bf16_raw* dkv, float* ws,
               hipStream_t s) {
  const XattnPlan p = xattn_plan(g);
  XattnArgs a = xattn_args(g, p);
  a.q = q; a.kv = kv; a.o = o; a.d_o = d_o; a.lse_in = lse; a.out = dq; a.slab = ws;
  hipLaunchKernelGGL(xattn_bwd_kernel, dim3((unsigned)p.walks, (unsigned)g.H, (unsigned)g.B),
                     dim3(AT_THREADS), 0, s, a);
  const int64_t nvec = (int64_t)g.B * g.Sk * 2 * g.H * (AT_D / 8);
  hipLaunchKernelGGL(xattn_dkv_sum_kernel, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, s, ws,
                     dkv, g.Sk, g.H, p.walks, nvec);
  MPA_CHECK_LAUNCH();
}

}  // namespace mpa
