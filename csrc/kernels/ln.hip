// Channels-last LayerNorm, exact GELU and layer scale with residual add for gfx950: the
// ConvNeXt block's non-GEMM passes.  Rows [M][C] bf16 (M = N H W), C % 8 == 0, fp32
// parameters, statistics and accumulators.  Plan: ln_plan.h.
//
//  * LayerNorm reduces over the channels of one pixel (bn.hip reduces over pixels per
//    channel), so a row lives in registers: L adjacent lanes own one row, lane l holds the
//    16-B vectors l, l + L, ... (V of them, 8 V channels).  Adjacent lanes load adjacent
//    vectors and a wave covers 64 / L adjacent rows: every access is a coalesced 16-B access
//    over one contiguous span.  Mean and centred variance are two passes over the registers;
//    the L lanes meet with xor shuffles (all lanes end with the same bits).  One load and one
//    store per element, no LDS in the forward.
//  * the backward recomputes xhat from x and the saved (mean, rstd), needs two more row sums
//    for dx, and in the same pass keeps fp32 sums of dy, dy xhat and the stored dx for the
//    lane's channels.  A block walks a contiguous slab of rows, folds its row slots through LDS
//    in slot order and writes one slab row [dgamma | dbeta | dpre_bias].
//  * GELU and layer scale are 16-B streaming kernels; their backward keeps per-thread column
//    sums (fc1's bias gradient / the scale's gradient) that take the same slab route.
//  * slab rows are summed in row order by ln_fold_kernel / ln_final_kernel: no float atomics,
//    bitwise repeatable.
#include "api.h"
#include "common.h"
#include "ln_plan.h"

namespace mpa {
namespace {

struct LnArgs {
  const bf16_t* x;
  const bf16_t* dy;
  const float* pre_bias;  // [C] or null: t = x + pre_bias
  const float* gamma;
  const float* beta;
  const float* stat_in;   // bwd: [M][2] (mean, rstd)
  bf16_t* out;            // y / dx
  float* stat;            // fwd: [M][2]
  float* slab;            // bwd: [rows][width]
  int M, C, CV, L, slab_rows, width;
  float eps;
};

// sum over the L lanes of a row (L a power of two); every lane receives the same bits
__device__ __forceinline__ float row_sum(float v, int L) {
  for (int o = L >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int V>
__device__ __forceinline__ void load_params(const float* p, int l, int L, int CV, float (*r)[8]) {
#pragma unroll
  for (int v = 0; v < V; ++v)
#pragma unroll
    for (int j = 0; j < 8; ++j) r[v][j] = (p && l + v * L < CV) ? p[(l + v * L) * 8 + j] : 0.f;
}

template <int V>
__global__ __launch_bounds__(LN_THREADS) void ln_fwd_kernel(LnArgs a) {
  const int tid = threadIdx.x, L = a.L, l = tid & (L - 1), rs = tid / L, rpt = LN_THREADS / L;
  float gm[V][8], bt[V][8], pb[V][8];
  load_params<V>(a.gamma, l, L, a.CV, gm);
  load_params<V>(a.beta, l, L, a.CV, bt);
  load_params<V>(a.pre_bias, l, L, a.CV, pb);
  const float fc = (float)a.C;
  const int r0 = blockIdx.x * a.slab_rows;
  // (the trip loop is uniform over the block: the shuffles below need every lane of a row)
  for (int t0 = 0; t0 < a.slab_rows && r0 + t0 < a.M; t0 += rpt) {
    const int row = r0 + t0 + rs;
    const bool ok = row < a.M;
    const size_t base = (size_t)row * a.C;
    float t[V][8];
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const bool on = ok && l + v * L < a.CV;
      uint4 w = make_uint4(0, 0, 0, 0);
      if (on) w = ld_stream(a.x + base + (size_t)(l + v * L) * 8);
      unpack8(w, t[v]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        t[v][j] += pb[v][j];
        s += t[v][j];
      }
    }
    const float mean = row_sum(s, L) / fc;
    float q = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const bool in = l + v * L < a.CV;  // masked tail vectors take no part in the variance
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        t[v][j] = in ? t[v][j] - mean : 0.f;
        q = fmaf(t[v][j], t[v][j], q);
      }
    }
    const float rstd = 1.0f / sqrtf(row_sum(q, L) / fc + a.eps);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (!(ok && l + v * L < a.CV)) continue;
      float y[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] = fmaf(t[v][j] * rstd, gm[v][j], bt[v][j]);
      st_stream(a.out + base + (size_t)(l + v * L) * 8, pack8(y));
    }
    if (ok && l == 0) *(float2*)(a.stat + (size_t)row * 2) = make_float2(mean, rstd);
  }
}

// DP: also the column sums of the stored dx (the gradient of pre_bias)
template <int V, bool DP>
__global__ __launch_bounds__(LN_THREADS) void ln_bwd_kernel(LnArgs a) {
  __shared__ float red[8 * V * LN_THREADS];
  const int tid = threadIdx.x, L = a.L, l = tid & (L - 1), rs = tid / L, rpt = LN_THREADS / L;
  float gm[V][8], pb[V][8];
  load_params<V>(a.gamma, l, L, a.CV, gm);
  load_params<V>(a.pre_bias, l, L, a.CV, pb);
  float dg[V][8], db[V][8], dp[DP ? V : 1][8];
#pragma unroll
  for (int v = 0; v < V; ++v)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      dg[v][j] = 0.f;
      db[v][j] = 0.f;
      if constexpr (DP) dp[v][j] = 0.f;
    }
  const float fc = (float)a.C;
  const int r0 = blockIdx.x * a.slab_rows;
  for (int t0 = 0; t0 < a.slab_rows && r0 + t0 < a.M; t0 += rpt) {
    const int row = r0 + t0 + rs;
    const bool ok = row < a.M;
    const size_t base = (size_t)row * a.C;
    float2 mr = make_float2(0.f, 0.f);
    if (ok) mr = *(const float2*)(a.stat_in + (size_t)row * 2);
    float xh[V][8], g[V][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const bool on = ok && l + v * L < a.CV;
      uint4 wx = make_uint4(0, 0, 0, 0), wd = make_uint4(0, 0, 0, 0);
      if (on) {
        wx = ld_stream(a.x + base + (size_t)(l + v * L) * 8);
        wd = ld_stream(a.dy + base + (size_t)(l + v * L) * 8);
      }
      float dyf[8];
      unpack8(wx, xh[v]);
      unpack8(wd, dyf);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        xh[v][j] = on ? ((xh[v][j] + pb[v][j]) - mr.x) * mr.y : 0.f;
        g[v][j] = dyf[j] * gm[v][j];
        s1 += g[v][j];
        s2 = fmaf(g[v][j], xh[v][j], s2);
        db[v][j] += dyf[j];
        dg[v][j] = fmaf(dyf[j], xh[v][j], dg[v][j]);
      }
    }
    const float m1 = row_sum(s1, L) / fc, m2 = row_sum(s2, L) / fc;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (!(ok && l + v * L < a.CV)) continue;
      float dx[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) dx[j] = mr.y * ((g[v][j] - m1) - xh[v][j] * m2);
      const uint4 w = pack8(dx);
      st_stream(a.out + base + (size_t)(l + v * L) * 8, w);
      if constexpr (DP) {  // of the stored (rounded) dx: what the depthwise conv's dgrad reads
        unpack8(w, dx);
#pragma unroll
        for (int j = 0; j < 8; ++j) dp[v][j] += dx[j];
      }
    }
  }

  // block fold, one quantity at a time: red[k][thread], output (k, l) sums its rpt row slots
  // in slot order
  float* srow = a.slab + (size_t)blockIdx.x * a.width;
#pragma unroll
  for (int qn = 0; qn < (DP ? 3 : 2); ++qn) {
    __syncthreads();
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        red[(v * 8 + j) * LN_THREADS + tid] = qn == 0 ? dg[v][j] : (qn == 1 ? db[v][j] : dp[DP ? v : 0][j]);
    __syncthreads();
    for (int o = tid; o < L * 8 * V; o += LN_THREADS) {
      const int k = o / L, ll = o - k * L;
      float s = 0.f;
      for (int r = 0; r < rpt; ++r) s += red[k * LN_THREADS + r * L + ll];
      const int c = (ll + (k >> 3) * L) * 8 + (k & 7);
      if (c < a.C) srow[qn * a.C + c] = s;
    }
  }
}

// slab [S][W]: rows [r0, r0 + chunk) summed into row r0 (four interleaved chains, fixed order)
__global__ __launch_bounds__(256) void ln_fold_kernel(float* __restrict__ slab, int S, int W,
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

// slab column w = q C + c: out_q[c] (+)= the heads' sum in row order
struct LnOuts {
  float* p[3];
};
__global__ __launch_bounds__(256) void ln_final_kernel(const float* __restrict__ slab, int heads,
                                                       int rstep, int W, int C, LnOuts out,
                                                       int overwrite) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= W) return;
  float s = 0.f;
  for (int h = 0; h < heads; ++h) s += slab[(size_t)h * rstep * W + w];
  const int q = w / C;
  float* o = (q == 0 ? out.p[0] : (q == 1 ? out.p[1] : out.p[2])) + (w - q * C);
  *o = overwrite ? s : *o + s;
}

void reduce_slab(float* ws, int rows, int W, int C, LnOuts out, bool overwrite, hipStream_t s) {
  const int chunk = ln_fold_chunk(rows);
  const int heads = (rows + chunk - 1) / chunk;
  if (chunk > 1)
    hipLaunchKernelGGL(ln_fold_kernel, dim3((W + 255) / 256, heads), dim3(256), 0, s, ws, rows, W,
                       chunk);
  hipLaunchKernelGGL(ln_final_kernel, dim3((W + 255) / 256), dim3(256), 0, s, ws, heads, chunk, W,
                     C, out, overwrite ? 1 : 0);
  MPA_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ GELU and layer scale
// exact GELU in the operation order of ATen's kernel: h 0.5 (1 + erf(h / sqrt 2))
__device__ __forceinline__ float gelu_f(float h) {
  return (h * 0.5f) * (1.0f + erff(h * 0.70710678118654752440f));
}
// Phi(h) + h phi(h)
__device__ __forceinline__ float gelu_der(float h) {
  const float cdf = 0.5f * (1.0f + erff(h * 0.70710678118654752440f));
  const float pdf = expf(-0.5f * h * h) * 0.39894228040143267794f;
  return fmaf(h, pdf, cdf);
}

// PRE: a = gelu(h + pre_bias[c]), the sum in fp32 (no rounding between it and the GELU)
template <bool PRE>
__global__ __launch_bounds__(256) void gelu_fwd_kernel(const bf16_t* __restrict__ h,
                                                       const float* __restrict__ pre_bias,
                                                       bf16_t* __restrict__ out, int64_t nvec,
                                                       int CV) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  float f[8];
  unpack8(ld_stream(h + i * 8), f);
  if (PRE) {
    const int cv = (int)(i % CV);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] += pre_bias[cv * 8 + j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = gelu_f(f[j]);
  st_stream(out + i * 8, pack8(f));
}

// out = res + gamma[c] y, one fused multiply-add per element
__global__ __launch_bounds__(256) void scale_add_fwd_kernel(const bf16_t* __restrict__ y,
                                                            const float* __restrict__ gamma,
                                                            const bf16_t* __restrict__ res,
                                                            bf16_t* __restrict__ out, int64_t nvec,
                                                            int CV) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  const int cv = (int)(i % CV);
  float yf[8], rf[8];
  unpack8(ld_stream(y + i * 8), yf);
  unpack8(ld_stream(res + i * 8), rf);
#pragma unroll
  for (int j = 0; j < 8; ++j) rf[j] = fmaf(gamma[cv * 8 + j], yf[j], rf[j]);
  st_stream(out + i * 8, pack8(rf));
}

struct ColArgs {
  const bf16_t* g;      // da / dout
  const bf16_t* src;    // h / y
  const float* gamma;   // scale_add
  const float* pre;     // gelu: pre_bias (PRE)
  bf16_t* out;          // dh / dy
  float* slab;          // [rows][C] or null (no column sums wanted)
  int M, C, CV, cvb, chunks, nslots, slab_rows;
};

// SCALE false: dh = da gelu'(h), column sums of the stored dh; PRE: gelu'(h + pre[c]).
// SCALE true:  dy = gamma dout, column sums of dout y.
template <bool SCALE, bool PRE>
__global__ __launch_bounds__(LN_THREADS) void col_bwd_kernel(ColArgs a) {
  __shared__ float red[8 * LN_THREADS];
  const int tid = threadIdx.x;
  const int chunk = blockIdx.x % a.chunks, sr = blockIdx.x / a.chunks;
  const int cv = tid % a.cvb, slot = tid / a.cvb, c0v = chunk * a.cvb;
  const bool on = slot < a.nslots && c0v + cv < a.CV;
  float acc[8], gm[8], pb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    acc[j] = 0.f;
    gm[j] = (SCALE && on) ? a.gamma[(c0v + cv) * 8 + j] : 0.f;
    pb[j] = (PRE && on) ? a.pre[(c0v + cv) * 8 + j] : 0.f;
  }
  if (on) {
    const int r1 = min(a.M, (sr + 1) * a.slab_rows);
    for (int row = sr * a.slab_rows + slot; row < r1; row += a.nslots) {
      const size_t ofs = (size_t)row * a.C + (size_t)(c0v + cv) * 8;
      float gf[8], sf[8], o[8];
      unpack8(ld_stream(a.g + ofs), gf);
      unpack8(ld_stream(a.src + ofs), sf);
      if (PRE) {
#pragma unroll
        for (int j = 0; j < 8; ++j) sf[j] += pb[j];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = SCALE ? gm[j] * gf[j] : gf[j] * gelu_der(sf[j]);
      const uint4 w = pack8(o);
      st_stream(a.out + ofs, w);
      if (SCALE) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(gf[j], sf[j], acc[j]);
      } else {
        unpack8(w, o);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += o[j];
      }
    }
  }
  if (!a.slab) return;
#pragma unroll
  for (int j = 0; j < 8; ++j) red[j * LN_THREADS + tid] = acc[j];
  __syncthreads();
  for (int o = tid; o < a.cvb * 8; o += LN_THREADS) {
    const int j = o / a.cvb, v = o - j * a.cvb;
    float s = 0.f;
    for (int q = 0; q < a.nslots; ++q) s += red[j * LN_THREADS + q * a.cvb + v];
    if (c0v + v < a.CV) a.slab[(size_t)sr * a.C + (size_t)(c0v + v) * 8 + j] = s;
  }
}

template <bool SCALE, bool PRE = false>
void col_bwd(const bf16_raw* g, const bf16_raw* src, const float* gamma, const LnGeom& geom,
             bf16_raw* out, float* sums, bool overwrite, float* ws, hipStream_t s,
             const float* pre = nullptr) {
  const ColPlan p = ln_col_plan(geom);
  ColArgs a{};
  a.g = g; a.src = src; a.gamma = gamma; a.pre = pre; a.out = out;
  a.slab = sums ? ws : nullptr;
  a.M = geom.M; a.C = geom.C; a.CV = geom.C / 8;
  a.cvb = p.cvb; a.chunks = p.chunks; a.nslots = p.nslots; a.slab_rows = p.slab;
  hipLaunchKernelGGL((col_bwd_kernel<SCALE, PRE>), dim3((unsigned)p.grid), dim3(LN_THREADS), 0, s, a);
  MPA_CHECK_LAUNCH();
  if (sums) reduce_slab(ws, p.rows, geom.C, geom.C, LnOuts{{sums, nullptr, nullptr}}, overwrite, s);
}

LnArgs ln_args(const LnGeom& g, const LnPlan& p) {
  LnArgs a{};
  a.M = g.M; a.C = g.C; a.CV = g.C / 8; a.L = p.L; a.slab_rows = p.slab;
  return a;
}

}  // namespace

void ln_fwd(const bf16_raw* x, const float* pre_bias, const float* gamma, const float* beta,
            float eps, const LnGeom& g, bf16_raw* y, float* stat, hipStream_t s) {
  const LnPlan p = ln_plan(g);
  LnArgs a = ln_args(g, p);
  a.x = x; a.pre_bias = pre_bias; a.gamma = gamma; a.beta = beta; a.eps = eps;
  a.out = y; a.stat = stat;
  const dim3 grid((unsigned)p.grid), block(LN_THREADS);
  if (p.V == 1) hipLaunchKernelGGL(ln_fwd_kernel<1>, grid, block, 0, s, a);
  else if (p.V == 2) hipLaunchKernelGGL(ln_fwd_kernel<2>, grid, block, 0, s, a);
  else if (p.V == 3) hipLaunchKernelGGL(ln_fwd_kernel<3>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(ln_fwd_kernel<4>, grid, block, 0, s, a);
  MPA_CHECK_LAUNCH();
}

template <int V>
static void ln_bwd_launch(const LnArgs& a, const LnPlan& p, bool dp, hipStream_t s) {
  const dim3 grid((unsigned)p.grid), block(LN_THREADS);
  if (dp) hipLaunchKernelGGL((ln_bwd_kernel<V, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((ln_bwd_kernel<V, false>), grid, block, 0, s, a);
}

void ln_bwd(const bf16_raw* dy, const bf16_raw* x, const float* pre_bias, const float* gamma,
            const float* stat, const LnGeom& g, bf16_raw* dx, float* dgamma, float* dbeta,
            float* dpre_bias, bool overwrite, float* ws, hipStream_t s) {
  const LnPlan p = ln_plan(g);
  LnArgs a = ln_args(g, p);
  a.x = x; a.dy = dy; a.pre_bias = pre_bias; a.gamma = gamma; a.stat_in = stat;
  a.out = dx; a.slab = ws;
  const bool dp = dpre_bias != nullptr;
  a.width = (dp ? 3 : 2) * g.C;
  if (p.V == 1) ln_bwd_launch<1>(a, p, dp, s);
  else if (p.V == 2) ln_bwd_launch<2>(a, p, dp, s);
  else if (p.V == 3) ln_bwd_launch<3>(a, p, dp, s);
  else ln_bwd_launch<4>(a, p, dp, s);
  MPA_CHECK_LAUNCH();
  reduce_slab(ws, p.rows, a.width, g.C, LnOuts{{dgamma, dbeta, dpre_bias}}, overwrite, s);
}

void gelu_fwd(const bf16_raw* h, const LnGeom& g, bf16_raw* out, hipStream_t s,
              const float* pre_bias) {
  const int64_t nvec = (int64_t)g.M * (g.C / 8);
  const dim3 grid((unsigned)((nvec + 255) / 256)), block(256);
  if (pre_bias) hipLaunchKernelGGL(gelu_fwd_kernel<true>, grid, block, 0, s, h, pre_bias, out, nvec, g.C / 8);
  else hipLaunchKernelGGL(gelu_fwd_kernel<false>, grid, block, 0, s, h, pre_bias, out, nvec, g.C / 8);
  MPA_CHECK_LAUNCH();
}

void gelu_bwd(const bf16_raw* da, const bf16_raw* h, const LnGeom& g, bf16_raw* dh, float* dbias,
              float* ws, hipStream_t s, const float* pre_bias) {
  if (pre_bias) col_bwd<false, true>(da, h, nullptr, g, dh, dbias, false, ws, s, pre_bias);
  else col_bwd<false>(da, h, nullptr, g, dh, dbias, false, ws, s);
}

void scale_add_fwd(const bf16_raw* y, const float* gamma, const bf16_raw* res, const LnGeom& g,
                   bf16_raw* out, hipStream_t s) {
  const int64_t nvec = (int64_t)g.M * (g.C / 8);
  hipLaunchKernelGGL(scale_add_fwd_kernel, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, s, y,
                     gamma, res, out, nvec, g.C / 8);
  MPA_CHECK_LAUNCH();
}

void scale_add_bwd(const bf16_raw* dout, const bf16_raw* y, const float* gamma, const LnGeom& g,
                   bf16_raw* dy, float* dgamma, bool overwrite, float* ws, hipStream_t s) {
  col_bwd<true>(dout, y, gamma, g, dy, dgamma, overwrite, ws, s);
}

}  // namespace mpa
