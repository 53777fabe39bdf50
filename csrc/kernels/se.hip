// Squeeze-excite and activation-gate kernels for gfx950 (MobileNetV3's hardswish layers and
// SE segments).  NHWC bf16, C % 8 == 0, fp32 arithmetic, one rounding at each bf16 store.
//
// With t = aff[0] z + aff[1] (a train- or eval-mode BN as its [2, C] affine), act in {0
// identity, 1 ReLU, 2 hardswish} and a per-(image, channel) gate from two tiny fully connected
// layers on the H x W mean of act(t), the segment is u = act(t) gate.  act(t) is never stored:
// every kernel recomputes t from z in fp32, so forward and backward see the same t.
//
// These are VALU streaming kernels.  Pool, scale and activation have no reduction over
// channels and the gate is a matrix-vector product per image (960 x 240 at the largest, 0.2
// MFLOP): MFMA has nothing to work on.  What matters is the number of passes over the expanded
// tensor and that every pass is coalesced (plan: se_plan.h):
//
//  * a lane owns one 16-B vector (8 channels) of a pixel, adjacent lanes adjacent vectors and
//    then the next pixel: with one channel chunk a block's accesses are one contiguous range;
//  * a block owns (image, pixel slab, channel chunk), so a thread's channels and image are
//    fixed: affine, gate, dpool, mean, rstd and the BN sums are loaded once into registers and
//    the pixel loop is loads, FMAs and (forward / dx) one store;
//  * reductions go thread -> LDS, summed in slot order -> one partial row per (image, slab)
//    -> rows summed in row order.  No float atomics in any mode: results are bitwise
//    repeatable;
//  * the gate kernels run one block per image with the image's vectors in LDS; weights are
//    read as 16-B words, forward rows reduce across a power-of-two lane group by shuffles in
//    a fixed order, the transposed products of the backward keep columns in lanes and split
//    the rows over slots that are summed through LDS in slot order.
//
// Forward: z is read by act_pool and act_gate_fwd, u written once (3 passes).  Backward: du
// and z are read by act_gate_bwd_pool and act_gate_bwd_sums and act_gate_bwd_dx (du 3 reads,
// z 3 reads, dz 1 write; without SE the pool pass is not run).
#include "api.h"
#include "common.h"
#include "se_plan.h"

namespace mpa {
namespace {

struct SeArgs {
  const bf16_t* z;      // [N][HW][C]
  const bf16_t* du;     // [N][HW][C] (backward)
  bf16_t* out;          // u (fwd) / dz (dx)
  const float* aff;     // [2][C]
  const float* gate;    // [N][C] or null (ones)
  const float* dpool;   // [N][C] or null (zeros)
  const float* mean;    // [C] or null (with rstd: dx returns g)
  const float* rstd;    // [C]
  const float* gamma;   // [C] or null (ones)
  const float* sums;    // [2][C] (dx)
  float* part;          // partial rows [N * slabs][C or 2 C]
  int N, HW, C, CV, act;
  int cvb, chunks, nslots, pps, slabs;
  float inv_m;          // 1 / (N HW)
};

enum { SE_POOL = 0, SE_FWD = 1, SE_BWD_POOL = 2, SE_BWD_SUMS = 3, SE_BWD_DX = 4 };

__device__ __forceinline__ float act_val(float t, int act) {
  if (act == 1) return fmaxf(t, 0.f);
  if (act == 2) return t * fminf(fmaxf(t + 3.f, 0.f), 6.f) * (1.f / 6.f);
  return t;
}

// torch's derivatives: ReLU 1 for t > 0; hardswish 0 for t <= -3, 1 for t >= 3, t / 3 + 0.5
// between (torch's hardswish_backward takes the open interval)
__device__ __forceinline__ float act_der(float t, int act) {
  if (act == 1) return t > 0.f ? 1.f : 0.f;
  if (act == 2) return t <= -3.f ? 0.f : (t >= 3.f ? 1.f : fmaf(t, 1.f / 3.f, 0.5f));
  return 1.f;
}

__device__ __forceinline__ void load8(const float* p, float* f) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
  f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

template <int MODE>
__global__ __launch_bounds__(SE_THREADS) void se_stream_kernel(SeArgs a) {
  constexpr bool RED = MODE == SE_POOL || MODE == SE_BWD_POOL || MODE == SE_BWD_SUMS;
  constexpr bool BWD = MODE >= SE_BWD_POOL;
  constexpr bool GRAD = MODE == SE_BWD_SUMS || MODE == SE_BWD_DX;  // forms g
  constexpr int NACC = MODE == SE_BWD_SUMS ? 16 : 8;
  __shared__ float red[RED ? SE_THREADS * NACC : 1];
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int chunk = b % a.chunks;
  b /= a.chunks;
  const int slab = b % a.slabs, n = b / a.slabs;
  const int cvb = a.cvb, c0v = chunk * cvb;
  const int cv = tid % cvb, slot = tid / cvb;
  const bool on = slot < a.nslots && c0v + cv < a.CV;
  const int p0 = slab * a.pps, p1 = min(a.HW, p0 + a.pps);
  const int act = a.act;
  const size_t cofs = (size_t)(c0v + cv) * 8;

  float sc[8], sh[8], gt[8], dp[8], mu[8], rs[8], k1[8], m1[8], m2[8], acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j) acc[j] = 0.f;
  const bool bn = GRAD && a.mean != nullptr;
  if (on) {
    load8(a.aff + cofs, sc);
    load8(a.aff + a.C + cofs, sh);
    if (MODE == SE_FWD || GRAD) {
#pragma unroll
      for (int j = 0; j < 8; ++j) gt[j] = 1.f;
      if (a.gate) load8(a.gate + (size_t)n * a.C + cofs, gt);
    }
    if (GRAD) {
#pragma unroll
      for (int j = 0; j < 8; ++j) dp[j] = 0.f;
      if (a.dpool) load8(a.dpool + (size_t)n * a.C + cofs, dp);
      if (bn) {
        load8(a.mean + cofs, mu);
        load8(a.rstd + cofs, rs);
      }
    }
    if (MODE == SE_BWD_DX && bn) {
      load8(a.sums + cofs, m1);
      load8(a.sums + a.C + cofs, m2);
      if (a.gamma) load8(a.gamma + cofs, k1);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        k1[j] = (a.gamma ? k1[j] : 1.f) * rs[j];
        m1[j] *= a.inv_m;
        m2[j] *= a.inv_m;
      }
    }

    const size_t step = (size_t)a.nslots * a.C;
    size_t o = ((size_t)n * a.HW + p0 + slot) * a.C + cofs;
#pragma unroll 2
    for (int p = p0 + slot; p < p1; p += a.nslots, o += step) {
      float zf[8], df[8], r[8];
      unpack8(*(const uint4*)(a.z + o), zf);
      if (BWD) unpack8(*(const uint4*)(a.du + o), df);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float t = fmaf(sc[j], zf[j], sh[j]);
        if (MODE == SE_POOL) acc[j] += act_val(t, act);
        if (MODE == SE_FWD) r[j] = act_val(t, act) * gt[j];
        if (MODE == SE_BWD_POOL) acc[j] = fmaf(df[j], act_val(t, act), acc[j]);
        if (GRAD) {
          const float g = fmaf(df[j], gt[j], dp[j]) * act_der(t, act);
          const float xh = bn ? (zf[j] - mu[j]) * rs[j] : 0.f;
          if (MODE == SE_BWD_SUMS) {
            acc[j] += g;
            acc[8 + j] = fmaf(g, xh, acc[8 + j]);
          } else {
            r[j] = bn ? k1[j] * ((g - m1[j]) - xh * m2[j]) : g;
          }
        }
      }
      if (MODE == SE_FWD || MODE == SE_BWD_DX) *(uint4*)(a.out + o) = pack8(r);
    }
  }

  if (RED) {
    // slots summed in slot order; one partial row per (image, slab): [C], or [sum g | sum g xh]
#pragma unroll
    for (int j = 0; j < NACC; ++j) red[tid * NACC + j] = acc[j];
    __syncthreads();
    for (int e = tid; e < cvb * NACC; e += SE_THREADS) {
      const int v = e / NACC, j = e % NACC;
      float s = 0.f;
      for (int q = 0; q < a.nslots; ++q) s += red[(q * cvb + v) * NACC + j];
      if (c0v + v < a.CV) {
        const int c = (c0v + v) * 8 + (j & 7);
        const size_t row = (size_t)n * a.slabs + slab;
        if (NACC == 8) a.part[row * a.C + c] = s;
        else a.part[row * 2 * a.C + (j < 8 ? c : a.C + c)] = s;
      }
    }
  }
}

// out[n][c] = scale * (the image's slab rows summed in slab order)
__global__ __launch_bounds__(256) void se_finish_kernel(const float* __restrict__ part, int N,
                                                        int slabs, int C, float scale,
                                                        float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * C) return;
  const int n = i / C, c = i - n * C;
  float s = 0.f;
  for (int q = 0; q < slabs; ++q) s += part[((size_t)n * slabs + q) * C + c];
  out[i] = s * scale;
}

// slab [S][W]: rows [r0, r0 + chunk) summed in row order into row r0
__global__ __launch_bounds__(256) void se_fold_kernel(float* __restrict__ slab, int S, int W,
                                                      int chunk) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= W) return;
  const int r0 = blockIdx.y * chunk, r1 = min(S, r0 + chunk);
  float s = 0.f;
  for (int r = r0; r < r1; ++r) s += slab[(size_t)r * W + w];
  slab[(size_t)r0 * W + w] = s;
}

// out[w] = the heads' sum in row order
__global__ __launch_bounds__(256) void se_heads_kernel(const float* __restrict__ slab, int heads,
                                                       int rstep, int W, float* __restrict__ out) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= W) return;
  float s = 0.f;
  for (int h = 0; h < heads; ++h) s += slab[(size_t)h * rstep * W + w];
  out[w] = s;
}

__device__ __forceinline__ float dot8(const uint4& w, const float* x) {
  float wf[8];
  unpack8(w, wf);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s = fmaf(wf[j], x[j], s);
  return s;
}

// y[r] = sum_i w[r][i] x[i] for r < R: a group of G lanes (power of two) owns a row, strides
// the row's I / 8 16-B words and reduces by shuffles in a fixed order; SE_THREADS / G rows per
// trip, every lane takes every trip.  Lane 0 of a group calls emit(r, sum).
template <typename Emit>
__device__ __forceinline__ void rows_matvec(const bf16_t* __restrict__ w, const float* x, int R,
                                            int I, int G, Emit emit) {
  const int tid = threadIdx.x, gl = tid & (G - 1), per = SE_THREADS / G, iv = I / 8;
  for (int r0 = 0; r0 < R; r0 += per) {
    const int r = r0 + tid / G;
    float s = 0.f;
    if (r < R)
      for (int v = gl; v < iv; v += G) s += dot8(*(const uint4*)(w + (size_t)r * I + v * 8), x + v * 8);
    for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (r < R && gl == 0) emit(r, s);
  }
}

// y[i] = sum_r w[r][i] x[r] for i < I (the transposed product): thread (word v of I / 8, slot
// q) sums rows q, q + nslots, ...; the slots are summed through red[] in slot order.  Thread
// e < I calls emit(e, sum).  I / 8 <= SE_THREADS.
template <typename Emit>
__device__ __forceinline__ void cols_matvec(const bf16_t* __restrict__ w, const float* x, int R,
                                            int I, float* red, Emit emit) {
  const int tid = threadIdx.x, iv = I / 8, nslots = SE_THREADS / iv;
  const int v = tid % iv, q = tid / iv;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (q < nslots)
    for (int r = q; r < R; r += nslots) {
      float wf[8];
      unpack8(*(const uint4*)(w + (size_t)r * I + v * 8), wf);
      const float xr = x[r];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(wf[j], xr, acc[j]);
    }
  __syncthreads();  // red[]'s previous readers are done
#pragma unroll
  for (int j = 0; j < 8; ++j) red[tid * 8 + j] = acc[j];
  __syncthreads();
  for (int e = tid; e < I; e += SE_THREADS) {
    float s = 0.f;
    for (int k = 0; k < nslots; ++k) s += red[(k * iv + (e >> 3)) * 8 + (e & 7)];
    emit(e, s);
  }
}

// h = relu(W1 s + b1), gate = hardsigmoid(W2 h + b2); one block per image
__global__ __launch_bounds__(SE_THREADS) void se_gate_kernel(
    const float* __restrict__ pooled, const bf16_t* __restrict__ w1, const float* __restrict__ b1,
    const bf16_t* __restrict__ w2, const float* __restrict__ b2, int C, int Cs, int G1, int G2,
    float* __restrict__ h, float* __restrict__ gate) {
  extern __shared__ float sm[];
  float* sl = sm;       // [C]
  float* hl = sm + C;   // [Cs]
  const int n = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += SE_THREADS) sl[c] = pooled[(size_t)n * C + c];
  __syncthreads();
  rows_matvec(w1, sl, Cs, C, G1, [&](int r, float s) {
    const float v = fmaxf(s + b1[r], 0.f);
    hl[r] = v;
    h[(size_t)n * Cs + r] = v;
  });
  __syncthreads();
  rows_matvec(w2, hl, C, Cs, G2, [&](int r, float s) {
    gate[(size_t)n * C + r] = fminf(fmaxf(s + b2[r] + 3.f, 0.f), 6.f) * (1.f / 6.f);
  });
}

// dpre2 = dgate / 6 where 0 < gate < 1; dpre1 = W2^T dpre2 where h > 0; dpool = W1^T dpre1 / HW
__global__ __launch_bounds__(SE_THREADS) void se_gate_bwd_kernel(
    const float* __restrict__ dgate, const float* __restrict__ h, const float* __restrict__ gate,
    const bf16_t* __restrict__ w1, const bf16_t* __restrict__ w2, int C, int Cs, float inv_hw,
    float* __restrict__ dpre2, float* __restrict__ dpre1, float* __restrict__ dpool) {
  extern __shared__ float sm[];
  float* d2 = sm;             // [C]
  float* d1 = sm + C;         // [Cs]
  float* red = sm + C + Cs;   // [SE_THREADS][8]
  const int n = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += SE_THREADS) {
    const float gv = gate[(size_t)n * C + c];
    const float v = (gv > 0.f && gv < 1.f) ? dgate[(size_t)n * C + c] * (1.f / 6.f) : 0.f;
    d2[c] = v;
    dpre2[(size_t)n * C + c] = v;
  }
  __syncthreads();
  cols_matvec(w2, d2, C, Cs, red, [&](int e, float s) {
    const float v = h[(size_t)n * Cs + e] > 0.f ? s : 0.f;
    d1[e] = v;
    dpre1[(size_t)n * Cs + e] = v;
  });
  __syncthreads();
  cols_matvec(w1, d1, Cs, C, red, [&](int e, float s) { dpool[(size_t)n * C + e] = s * inv_hw; });
}

// dw[o][i] (+)= sum_n dpre[n][o] inp[n][i] for e = o I + i < O I, db[o] (+)= sum_n dpre[n][o]
// for e = O I + o: one thread per element, images summed in image order
__global__ __launch_bounds__(256) void se_fc_wgrad_kernel(const float* __restrict__ dpre,
                                                          const float* __restrict__ inp, int N,
                                                          int O, int I, float* __restrict__ dw,
                                                          float* __restrict__ db, int overwrite) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= O * I + O) return;
  const bool bias = e >= O * I;
  const int o = bias ? e - O * I : e / I, i = bias ? 0 : e - o * I;
  float s = 0.f;
  if (bias) {
    for (int n = 0; n < N; ++n) s += dpre[(size_t)n * O + o];
  } else {
#pragma unroll 4
    for (int n = 0; n < N; ++n) s = fmaf(dpre[(size_t)n * O + o], inp[(size_t)n * I + i], s);
  }
  if (bias && !db) return;
  float* dst = bias ? db + o : dw + e;
  *dst = overwrite ? s : *dst + s;
}

SeArgs se_args(const SeGeom& g, const SePlan& p, const bf16_raw* z, const float* aff, int act) {
  SeArgs a{};
  a.z = z;
  a.aff = aff;
  a.act = act;
  a.N = g.N; a.HW = g.HW; a.C = g.C; a.CV = g.C / 8;
  a.cvb = p.cvb; a.chunks = p.chunks; a.nslots = p.nslots; a.pps = p.pps; a.slabs = p.slabs;
  a.inv_m = 1.f / ((float)g.N * (float)g.HW);
  return a;
}

template <int MODE>
void se_launch(const SeArgs& a, const SePlan& p, hipStream_t s) {
  hipLaunchKernelGGL(se_stream_kernel<MODE>, dim3((unsigned)p.grid), dim3(SE_THREADS), 0, s, a);
  MPA_CHECK_LAUNCH();
}

void se_finish(const float* part, const SeGeom& g, const SePlan& p, float scale, float* out,
               hipStream_t s) {
  hipLaunchKernelGGL(se_finish_kernel, dim3((g.N * g.C + 255) / 256), dim3(256), 0, s, part, g.N,
                     p.slabs, g.C, scale, out);
  MPA_CHECK_LAUNCH();
}

}  // namespace

void act_pool(const bf16_raw* z, const float* aff, int act, const SeGeom& g, float* pooled,
              float* ws, hipStream_t s) {
  const SePlan p = se_plan(g);
  SeArgs a = se_args(g, p, z, aff, act);
  a.part = ws;
  se_launch<SE_POOL>(a, p, s);
  se_finish(ws, g, p, 1.f / (float)g.HW, pooled, s);
}

void se_gate(const float* pooled, const bf16_raw* w1, const float* b1, const bf16_raw* w2,
             const float* b2, int N, int C, int Cs, float* h, float* gate, hipStream_t s) {
  hipLaunchKernelGGL(se_gate_kernel, dim3(N), dim3(SE_THREADS), se_gate_lds_bytes(C, Cs, false), s,
                     pooled, (const bf16_t*)w1, b1, (const bf16_t*)w2, b2, C, Cs,
                     se_row_lanes(C / 8), se_row_lanes(Cs / 8), h, gate);
  MPA_CHECK_LAUNCH();
}

void act_gate_fwd(const bf16_raw* z, const float* aff, int act, const float* gate,
                  const SeGeom& g, bf16_raw* u, hipStream_t s) {
  const SePlan p = se_plan(g);
  SeArgs a = se_args(g, p, z, aff, act);
  a.gate = gate;
  a.out = u;
  se_launch<SE_FWD>(a, p, s);
}

void act_gate_bwd_pool(const bf16_raw* du, const bf16_raw* z, const float* aff, int act,
                       const SeGeom& g, float* dgate, float* ws, hipStream_t s) {
  const SePlan p = se_plan(g);
  SeArgs a = se_args(g, p, z, aff, act);
  a.du = du;
  a.part = ws;
  se_launch<SE_BWD_POOL>(a, p, s);
  se_finish(ws, g, p, 1.f, dgate, s);
}

void se_gate_bwd(const float* dgate, const float* h, const float* gate, const bf16_raw* w1,
                 const bf16_raw* w2, float inv_hw, int N, int C, int Cs, float* dpre2,
                 float* dpre1, float* dpool, hipStream_t s) {
  hipLaunchKernelGGL(se_gate_bwd_kernel, dim3(N), dim3(SE_THREADS), se_gate_lds_bytes(C, Cs, true),
                     s, dgate, h, gate, (const bf16_t*)w1, (const bf16_t*)w2, C, Cs, inv_hw, dpre2,
                     dpre1, dpool);
  MPA_CHECK_LAUNCH();
}

void se_fc_wgrad(const float* dpre, const float* inp, int N, int O, int I, float* dw, float* db,
                 bool overwrite, hipStream_t s) {
  hipLaunchKernelGGL(se_fc_wgrad_kernel, dim3((O * I + O + 255) / 256), dim3(256), 0, s, dpre, inp,
                     N, O, I, dw, db, overwrite ? 1 : 0);
  MPA_CHECK_LAUNCH();
}

void act_gate_bwd_sums(const bf16_raw* du, const bf16_raw* z, const float* aff, int act,
                       const float* gate, const float* dpool, const float* mean,
                       const float* rstd, const SeGeom& g, float* sums, float* ws, hipStream_t s) {
  const SePlan p = se_plan(g);
  SeArgs a = se_args(g, p, z, aff, act);
  a.du = du;
  a.gate = gate;
  a.dpool = dpool;
  a.mean = mean;
  a.rstd = rstd;
  a.part = ws;
  se_launch<SE_BWD_SUMS>(a, p, s);
  const int W = 2 * g.C, chunk = se_fold_chunk(p.rows), heads = (p.rows + chunk - 1) / chunk;
  if (chunk > 1)
    hipLaunchKernelGGL(se_fold_kernel, dim3((W + 255) / 256, heads), dim3(256), 0, s, ws, p.rows,
                       W, chunk);
  hipLaunchKernelGGL(se_heads_kernel, dim3((W + 255) / 256), dim3(256), 0, s, ws, heads, chunk, W,
                     sums);
  MPA_CHECK_LAUNCH();
}

void act_gate_bwd_dx(const bf16_raw* du, const bf16_raw* z, const float* aff, int act,
                     const float* gate, const float* dpool, const float* mean, const float* rstd,
                     const float* gamma, const float* sums, const SeGeom& g, bf16_raw* dz,
                     hipStream_t s) {
  const SePlan p = se_plan(g);
  SeArgs a = se_args(g, p, z, aff, act);
  a.du = du;
  a.gate = gate;
  a.dpool = dpool;
  a.mean = mean;
  a.rstd = rstd;
  a.gamma = gamma;
  a.sums = sums;
  a.out = dz;
  se_launch<SE_BWD_DX>(a, p, s);
}

}  // namespace mpa
