// Fused flat-arena optimizers (K11): ONE streaming pass over the fp32 master weights,
// gradients and optimizer state of the whole model.  Applies the data-parallel 1/N
// gradient scale (the average of mpi_tools.py:36 folded in), L2 weight decay, the
// torch.optim.Adam / torch.optim.SGD update rule, and writes the bf16 weight shadow the
// MFMA kernels read (no separate cast pass).  The step counter lives on the device so the
// update is HIP-graph capturable.  Reference: Adam(lr=4e-4) at main.py:125,155.
#include "common.h"
#include "api.h"
#include <algorithm>

namespace mpa {

// The update loops are __device__ functions shared by the host-argument kernels
// (adam_kernel / sgd_kernel) and the device-argument kernels (adam_dev_kernel /
// sgd_dev_kernel, which take lr and the gradient scale from the hyper record), so the two
// forms cannot drift: with equal lr / scale they are bitwise equal.  The grid-stride
// start and stride are taken in the kernels (GRID_I0 / GRID_STRIDE) and passed in: read in
// a __device__ function, blockDim loses the kernel's uniform-workgroup-size fast path.
#define GRID_I0 (blockIdx.x * (int64_t)blockDim.x + threadIdx.x)
#define GRID_STRIDE ((int64_t)gridDim.x * blockDim.x)
__device__ __forceinline__ void adam_body(float* __restrict__ p, const float* __restrict__ g,
                                          float* __restrict__ m, float* __restrict__ v,
                                          bf16_t* __restrict__ shadow,
                                          const float* __restrict__ step, int64_t n4,
                                          float lr, float b1, float b2, float eps,
                                          float wd, float gs, int64_t i0, int64_t stride) {
  const float t = step[0] + 1.f;
  const float bc1 = 1.f - powf(b1, t);
  const float bc2s = sqrtf(1.f - powf(b2, t));
  const float step_size = lr / bc1;
  // streaming-bound: 1.33 GB per step at 44 M parameters in ~213 us (6.2 TB/s); the
  // correctly rounded sqrt / divide keep torch.optim.Adam's update bit-for-bit
  for (int64_t i = i0; i < n4; i += stride) {
    float4 pp = ((float4*)p)[i];
    const float4 gg = ((const float4*)g)[i];
    float4 mm = ((float4*)m)[i];
    float4 vv = ((float4*)v)[i];
    float* pf = (float*)&pp;
    const float* gf = (const float*)&gg;
    float* mf = (float*)&mm;
    float* vf = (float*)&vv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gr = gf[j] * gs;
      if (wd != 0.f) gr += wd * pf[j];
      mf[j] = b1 * mf[j] + (1.f - b1) * gr;
      vf[j] = b2 * vf[j] + (1.f - b2) * gr * gr;
      const float denom = sqrtf(vf[j]) / bc2s + eps;
      pf[j] -= step_size * mf[j] / denom;
    }
    ((float4*)p)[i] = pp;
    ((float4*)m)[i] = mm;
    ((float4*)v)[i] = vv;
    if (shadow) ((uint2*)shadow)[i] = make_uint2(pack2(pf[0], pf[1]), pack2(pf[2], pf[3]));
  }
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v,
                                                    bf16_t* __restrict__ shadow,
                                                    const float* __restrict__ step, int64_t n4,
                                                    float lr, float b1, float b2, float eps,
                                                    float wd, float gs) {
  adam_body(p, g, m, v, shadow, step, n4, lr, b1, b2, eps, wd, gs, GRID_I0, GRID_STRIDE);
}

// lr / gradient scale / skip flag from the hyper record hyper_kernel wrote (stream order);
// the skip branch is uniform over the whole grid
__global__ __launch_bounds__(256) void adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v,
                                                        bf16_t* __restrict__ shadow,
                                                        const float* __restrict__ step,
                                                        const float* __restrict__ hyper, int64_t n4,
                                                        float b1, float b2, float eps, float wd) {
  if (hyper[HYPER_SKIP] != 0.f) return;
  adam_body(p, g, m, v, shadow, step, n4, hyper[HYPER_LR], b1, b2, eps, wd, hyper[HYPER_SCALE],
            GRID_I0, GRID_STRIDE);
}

__device__ __forceinline__ void sgd_body(float* __restrict__ p, const float* __restrict__ g,
                                         float* __restrict__ buf, bf16_t* __restrict__ shadow,
                                         const float* __restrict__ step, int64_t n4,
                                         float lr, float momentum, float dampening,
                                         float wd, int nesterov, float gs, int64_t i0,
                                         int64_t stride) {
  const bool first = step[0] == 0.f;
  for (int64_t i = i0; i < n4; i += stride) {
    float4 pp = ((float4*)p)[i];
    const float4 gg = ((const float4*)g)[i];
    float4 bb = ((float4*)buf)[i];
    float* pf = (float*)&pp;
    const float* gf = (const float*)&gg;
    float* bf = (float*)&bb;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gr = gf[j] * gs;
      if (wd != 0.f) gr += wd * pf[j];
      if (momentum != 0.f) {
        bf[j] = first ? gr : momentum * bf[j] + (1.f - dampening) * gr;
        gr = nesterov ? gr + momentum * bf[j] : bf[j];
      }
      pf[j] -= lr * gr;
    }
    ((float4*)p)[i] = pp;
    if (momentum != 0.f) ((float4*)buf)[i] = bb;
    if (shadow) ((uint2*)shadow)[i] = make_uint2(pack2(pf[0], pf[1]), pack2(pf[2], pf[3]));
  }
}

__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ buf, bf16_t* __restrict__ shadow,
                                                   const float* __restrict__ step, int64_t n4,
                                                   float lr, float momentum, float dampening,
                                                   float wd, int nesterov, float gs) {
  sgd_body(p, g, buf, shadow, step, n4, lr, momentum, dampening, wd, nesterov, gs, GRID_I0,
           GRID_STRIDE);
}

__global__ __launch_bounds__(256) void sgd_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ buf, bf16_t* __restrict__ shadow,
                                                       const float* __restrict__ step,
                                                       const float* __restrict__ hyper, int64_t n4,
                                                       float momentum, float dampening, float wd,
                                                       int nesterov) {
  if (hyper[HYPER_SKIP] != 0.f) return;
  sgd_body(p, g, buf, shadow, step, n4, hyper[HYPER_LR], momentum, dampening, wd, nesterov,
           hyper[HYPER_SCALE], GRID_I0, GRID_STRIDE);
}

// ------------------------------------------------- global gradient norm + per-step recipe
// grad_sqnorm: sum of squares of the flat fp32 gradient arena, for global-norm clipping.
// A read-only stream: each thread issues SQ_LOADS 16-byte loads (a block covers a
// contiguous 32 KB per round, lanes adjacent) before it consumes any, squares into four
// accumulators in a fixed order, then wave64 shuffle -> LDS -> one float per block in the
// workspace slab.  No float atomics: hyper_kernel (one block) sums the slab in a fixed
// order, so the result depends only on (values, n) - bitwise reproducible in every mode
// and equal on every data-parallel rank after the all-reduce.
// The arena's alignment padding (parallel/arena.py ALIGN = 64) is part of the sum: it is
// zero after zero_grad and no kernel writes it, and it must stay zero
// (tests/test_recipe_gpu.py asserts it after a training step).
constexpr int SQ_LOADS = 8;       // 16-byte loads in flight per thread (the slab reductions' 8)
constexpr int SQ_GRID_CAP = 2048;  // 256 CUs x 8 blocks, a multiple of the 8 XCDs

__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const float4* __restrict__ g, int64_t n4,
                                                          float* __restrict__ part) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  const int64_t round = (int64_t)gridDim.x * (256 * SQ_LOADS);
  for (int64_t base = (int64_t)blockIdx.x * (256 * SQ_LOADS); base < n4; base += round) {
    float4 x[SQ_LOADS];
    if (base + 256 * SQ_LOADS <= n4) {  // (uniform per block)
#pragma unroll
      for (int u = 0; u < SQ_LOADS; ++u) x[u] = g[base + u * 256 + threadIdx.x];
    } else {
#pragma unroll
      for (int u = 0; u < SQ_LOADS; ++u) {
        const int64_t i = base + u * 256 + threadIdx.x;
        x[u] = i < n4 ? g[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
#pragma unroll
    for (int u = 0; u < SQ_LOADS; ++u) {
      a0 += x[u].x * x[u].x;
      a1 += x[u].y * x[u].y;
      a2 += x[u].z * x[u].z;
      a3 += x[u].w * x[u].w;
    }
  }
  __shared__ float ws[4];
  const float w = wave_sum((a0 + a1) + (a2 + a3));
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// fixed-order sum of the slab by ONE block of 256 threads; the result is valid in thread 0
__device__ __forceinline__ float slab_sum(const float* __restrict__ part, int nparts) {
  __shared__ float ws[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) a += part[i];
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = a;
  __syncthreads();
  return (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

__global__ __launch_bounds__(256) void sqnorm_sum_kernel(const float* __restrict__ part, int nparts,
                                                         float* __restrict__ out) {
  const float s = slab_sum(part, nparts);
  if (threadIdx.x == 0) out[0] = s;
}

// hyper_update: this step's learning rate (warm-up, then constant | cosine | step decay of
// the 0-based update index k = step[0]) and, with clipping (nparts > 0), the global norm of
// the averaged gradient, torch's clip coefficient and the non-finite skip flag.  One block;
// thread 0 writes the record with ordinary stores.
__global__ __launch_bounds__(256) void hyper_kernel(const float* __restrict__ step,
                                                    const float* __restrict__ part, int nparts,
                                                    float* __restrict__ hyper, HyperCfg c) {
  float sumsq = 0.f;
  if (nparts > 0) sumsq = slab_sum(part, nparts);
  if (threadIdx.x != 0) return;
  const float k = step[0];
  float lr = c.base_lr;
  if (k < c.warmup) {
    lr = c.base_lr * (k + 1.f) / c.warmup;
  } else if (c.kind == HYPER_COSINE) {
    if (k < c.total) {
      const float p = (k - c.warmup) / fmaxf(1.f, c.total - c.warmup);
      lr = c.base_lr * (c.min_ratio + (1.f - c.min_ratio) * 0.5f * (1.f + cospif(p)));
    } else {
      lr = c.base_lr * c.min_ratio;
    }
  } else if (c.kind == HYPER_STEP) {
    lr = c.base_lr * powf(c.gamma, floorf(k / c.decay_steps));
  }
  float norm = 0.f, coef = 1.f, skip = 0.f, bad = hyper[HYPER_NONFINITE];
  if (nparts > 0) {
    norm = c.grad_scale * sqrtf(sumsq);
    if (!isfinite(sumsq)) {  // inf / NaN gradients (or a sum past fp32): skip the update
      skip = 1.f;
      coef = 0.f;
      bad += 1.f;
    } else if (norm > c.max_norm) {
      coef = fminf(1.f, c.max_norm / (norm + 1e-6f));  // torch.nn.utils.clip_grad_norm_
    }
  }
  hyper[HYPER_LR] = lr;
  hyper[HYPER_SCALE] = c.grad_scale * coef;  // coef == 1: bitwise grad_scale
  hyper[HYPER_NORM] = norm;
  hyper[HYPER_COEF] = coef;
  hyper[HYPER_SKIP] = skip;
  hyper[HYPER_NONFINITE] = bad;
  hyper[HYPER_SUMSQ] = sumsq;
}

static int blocks_for(int64_t n4) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((n4 + 255) / 256, 4096));
}

void adam_step(float* p, const float* g, float* m, float* v, bf16_raw* shadow, const float* step,
               int64_t n, float lr, float b1, float b2, float eps, float wd, float gs,
               hipStream_t s) {
  const int64_t n4 = n / 4;
  hipLaunchKernelGGL(adam_kernel, dim3(blocks_for(n4)), dim3(256), 0, s, p, g, m, v, shadow, step,
                     n4, lr, b1, b2, eps, wd, gs);
}

void sgd_step(float* p, const float* g, float* buf, bf16_raw* shadow, const float* step,
              int64_t n, float lr, float momentum, float dampening, float wd, int nesterov,
              float gs, hipStream_t s) {
  const int64_t n4 = n / 4;
  hipLaunchKernelGGL(sgd_kernel, dim3(blocks_for(n4)), dim3(256), 0, s, p, g, buf, shadow, step,
                     n4, lr, momentum, dampening, wd, nesterov, gs);
}

void adam_step_dev(float* p, const float* g, float* m, float* v, bf16_raw* shadow,
                   const float* step, const float* hyper, int64_t n, float b1, float b2,
                   float eps, float wd, hipStream_t s) {
  const int64_t n4 = n / 4;
  hipLaunchKernelGGL(adam_dev_kernel, dim3(blocks_for(n4)), dim3(256), 0, s, p, g, m, v, shadow,
                     step, hyper, n4, b1, b2, eps, wd);
}

void sgd_step_dev(float* p, const float* g, float* buf, bf16_raw* shadow, const float* step,
                  const float* hyper, int64_t n, float momentum, float dampening, float wd,
                  int nesterov, hipStream_t s) {
  const int64_t n4 = n / 4;
  hipLaunchKernelGGL(sgd_dev_kernel, dim3(blocks_for(n4)), dim3(256), 0, s, p, g, buf, shadow,
                     step, hyper, n4, momentum, dampening, wd, nesterov);
}

int grad_sqnorm_grid_cap() { return SQ_GRID_CAP; }
int64_t grad_sqnorm_sweep() { return (int64_t)SQ_GRID_CAP * 256 * SQ_LOADS * 4; }

int grad_sqnorm(const float* g, int64_t n, float* part, hipStream_t s) {
  const int64_t n4 = n / 4, per = 256 * SQ_LOADS;
  int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((n4 + per - 1) / per, SQ_GRID_CAP));
  blocks = (blocks + 7) / 8 * 8;  // a multiple of the XCD count (<= SQ_GRID_CAP, itself one)
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((int)blocks), dim3(256), 0, s, (const float4*)g, n4,
                     part);
  return (int)blocks;
}

void grad_sqnorm_sum(const float* part, int nparts, float* out, hipStream_t s) {
  hipLaunchKernelGGL(sqnorm_sum_kernel, dim3(1), dim3(256), 0, s, part, nparts, out);
}

void hyper_update(const float* step, const float* part, int nparts, float* hyper,
                  const HyperCfg& cfg, hipStream_t s) {
  hipLaunchKernelGGL(hyper_kernel, dim3(1), dim3(256), 0, s, step, part, nparts, hyper, cfg);
}

// ------------------------------------------- layer-wise optimizers: AdamW / LAMB / LARS
// The segment plan tells the flat-arena kernels which parameter an element belongs to.
// seg: [nseg][SEG_COLS] int64 = (offset, aligned length, first chunk, chunk count, flags);
// segment s is parameter s's aligned arena slice, the segments tile [0, n) and start on
// 64-element boundaries, so a float4 never straddles two parameters.  Each segment is cut
// into chunks of at most SEG_CHUNK elements, consecutive in the chunk table; chunk_seg[c]
// is chunk c's segment.  One block per chunk: everything a block reads from the plan is
// uniform, and a chunk never crosses a segment.
// Norms: one float per chunk (wave64 shuffle -> LDS, fixed order), then trust_ratio_kernel
// sums a segment's partials with one block in a fixed order.  No float atomics: a
// parameter's norm depends only on (values, plan), so it is bitwise reproducible in every
// mode and equal on every data-parallel rank.
// Every kernel here takes lr / gradient scale / skip flag from the hyper record and writes
// nothing when hyper[HYPER_SKIP] != 0.
constexpr int SEG_CHUNK = 16384;  // elements: 256 threads x 8 float4 x 2 rounds

struct Chunk {
  int64_t off;  // first element
  int n4;       // float4s (0: a malformed plan entry - touch nothing)
  int seg;
  int flags;
};

__device__ __forceinline__ Chunk chunk_of(const int64_t* __restrict__ seg,
                                          const int* __restrict__ chunk_seg, int nseg, int c,
                                          int64_t n) {
  Chunk k;
  k.seg = chunk_seg[c];
  k.off = 0;
  k.n4 = 0;
  k.flags = 0;
  if (k.seg < 0 || k.seg >= nseg) {
    k.seg = 0;
    return k;
  }
  const int64_t* d = seg + (int64_t)k.seg * SEG_COLS;
  const int64_t rel = ((int64_t)c - d[SEG_FIRST]) * SEG_CHUNK;
  const int64_t left = d[SEG_LEN] - rel;
  const int64_t len = left < SEG_CHUNK ? left : (int64_t)SEG_CHUNK;
  k.off = d[SEG_OFF] + rel;
  k.flags = (int)d[SEG_FLAGS];
  // the plan is built on the host (optim.py); an entry outside the arena is not followed
  if (rel >= 0 && len > 0 && k.off >= 0 && (k.off & 3) == 0 && k.off + len <= n)
    k.n4 = (int)(len / 4);
  return k;
}

// block sums of two values; valid in thread 0
__device__ __forceinline__ void block_sum2(float& a, float& b) {
  __shared__ float ws[8];
  a = wave_sum(a);
  b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) {
    ws[threadIdx.x >> 6] = a;
    ws[4 + (threadIdx.x >> 6)] = b;
  }
  __syncthreads();
  a = (ws[0] + ws[1]) + (ws[2] + ws[3]);
  b = (ws[4] + ws[5]) + (ws[6] + ws[7]);
}

// part[c] = sum over chunk c of (x * scale)^2, scale = hyper[HYPER_SCALE] when scaled
__global__ __launch_bounds__(256) void seg_sqnorm_kernel(const float* __restrict__ x, int64_t n,
                                                         const int64_t* __restrict__ seg,
                                                         const int* __restrict__ chunk_seg,
                                                         int nseg,
                                                         const float* __restrict__ hyper,
                                                         int scaled, float* __restrict__ part) {
  if (hyper[HYPER_SKIP] != 0.f) return;
  const Chunk k = chunk_of(seg, chunk_seg, nseg, blockIdx.x, n);
  const float sc = scaled ? hyper[HYPER_SCALE] : 1.f;
  const float4* __restrict__ x4 = (const float4*)(x + k.off);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int base = 0; base < k.n4; base += 256 * SQ_LOADS) {
    float4 v[SQ_LOADS];
#pragma unroll
    for (int u = 0; u < SQ_LOADS; ++u) {
      const int i = base + u * 256 + threadIdx.x;
      v[u] = i < k.n4 ? x4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < SQ_LOADS; ++u) {
      const float e0 = v[u].x * sc, e1 = v[u].y * sc, e2 = v[u].z * sc, e3 = v[u].w * sc;
      a0 += e0 * e0;
      a1 += e1 * e1;
      a2 += e2 * e2;
      a3 += e3 * e3;
    }
  }
  float a = (a0 + a1) + (a2 + a3), b = 0.f;
  block_sum2(a, b);
  if (threadIdx.x == 0) part[blockIdx.x] = a;
}

// The element math of LAMB, shared by stage 1 (norms of the would-be update) and stage 2
// (the update), so the u that is normed is bitwise the u that is applied: new moments
// (adam_body's expressions with wd = 0) and u = m^ / (sqrt(v^) + eps) + wd_s * p.
struct AdamCoef {
  float b1, b2, eps, bc1, bc2s;
};

__device__ __forceinline__ AdamCoef adam_coef(const float* __restrict__ step, float b1, float b2,
                                              float eps) {
  const float t = step[0] + 1.f;
  AdamCoef c;
  c.b1 = b1;
  c.b2 = b2;
  c.eps = eps;
  // once per thread, in double: 1 - powf(b2, t) loses b2^t / (1 - b2^t) = 125 ulps at t = 8,
  // which the norm of u would carry as a relative error of 1e-5
  c.bc1 = (float)(1.0 - pow((double)b1, (double)t));
  c.bc2s = (float)sqrt(1.0 - pow((double)b2, (double)t));
  return c;
}

__device__ __forceinline__ void moments_elem(float g, float gs, float& m, float& v,
                                             const AdamCoef& c) {
  // the contractions the compiler picks for adam_body's `b1 * m + (1 - b1) * gr` and
  // `b2 * v + (1 - b2) * gr * gr`, spelled out: under -ffp-contract=fast the same source
  // text fused the other product here, and the moments must be bitwise Adam's
  // (test_updates_match_oracle compares them with adam_step_dev's)
  const float gr = g * gs;
  m = fmaf(1.f - c.b1, gr, c.b1 * m);
  v = fmaf(gr, (1.f - c.b2) * gr, c.b2 * v);
}

__device__ __forceinline__ float lamb_elem(float p, float g, float gs, float& m, float& v,
                                           float wd_s, const AdamCoef& c) {
  moments_elem(g, gs, m, v, c);
  const float denom = sqrtf(v) / c.bc2s + c.eps;
  return (m / c.bc1) / denom + wd_s * p;
}

constexpr int LN_LOADS = 2;  // float4s per stream in flight per thread (4 streams)

// LAMB stage 1: per chunk, sum p^2 and sum u^2 of the update direction the step would
// apply.  Reads p, g, m, v; writes only the two partials.
__global__ __launch_bounds__(256) void lamb_norms_kernel(
    const float* __restrict__ p, const float* __restrict__ g, const float* __restrict__ m,
    const float* __restrict__ v, int64_t n, const float* __restrict__ step,
    const float* __restrict__ hyper, const int64_t* __restrict__ seg,
    const int* __restrict__ chunk_seg, int nseg, float* __restrict__ part_p,
    float* __restrict__ part_u, float b1, float b2, float eps, float wd) {
  if (hyper[HYPER_SKIP] != 0.f) return;
  const Chunk k = chunk_of(seg, chunk_seg, nseg, blockIdx.x, n);
  const AdamCoef c = adam_coef(step, b1, b2, eps);
  const float gs = hyper[HYPER_SCALE];
  const float wd_s = (k.flags & SEG_DECAY) ? wd : 0.f;
  const float4* __restrict__ p4 = (const float4*)(p + k.off);
  const float4* __restrict__ g4 = (const float4*)(g + k.off);
  const float4* __restrict__ m4 = (const float4*)(m + k.off);
  const float4* __restrict__ v4 = (const float4*)(v + k.off);
  float sp[4] = {0.f, 0.f, 0.f, 0.f}, su[4] = {0.f, 0.f, 0.f, 0.f};
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int base = 0; base < k.n4; base += 256 * LN_LOADS) {
    float4 pp[LN_LOADS], gg[LN_LOADS], mm[LN_LOADS], vv[LN_LOADS];
#pragma unroll
    for (int u = 0; u < LN_LOADS; ++u) {
      const int i = base + u * 256 + threadIdx.x;
      const bool in = i < k.n4;  // past the chunk: p = g = m = v = 0 gives u = 0
      pp[u] = in ? p4[i] : z;
      gg[u] = in ? g4[i] : z;
      mm[u] = in ? m4[i] : z;
      vv[u] = in ? v4[i] : z;
    }
#pragma unroll
    for (int u = 0; u < LN_LOADS; ++u) {
      const float* pf = (const float*)&pp[u];
      const float* gf = (const float*)&gg[u];
      float* mf = (float*)&mm[u];
      float* vf = (float*)&vv[u];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float uu = lamb_elem(pf[j], gf[j], gs, mf[j], vf[j], wd_s, c);
        sp[j] += pf[j] * pf[j];
        su[j] += uu * uu;
      }
    }
  }
  float a = (sp[0] + sp[1]) + (sp[2] + sp[3]), b = (su[0] + su[1]) + (su[2] + su[3]);
  block_sum2(a, b);
  if (threadIdx.x == 0) {
    part_p[blockIdx.x] = a;
    part_u[blockIdx.x] = b;
  }
}

// One block per segment: fixed-order sums of its chunks' partials, the two norms and the
// trust ratio.  LAMB: |p| / |u|.  LARS: trust_coef * |p| / (|g^| + wd_s * |p| + 1e-8), g^ the
// scaled gradient.  1 when the segment is not adaptive or either norm is 0.
__global__ __launch_bounds__(256) void trust_ratio_kernel(
    const int64_t* __restrict__ seg, int nchunks, const float* __restrict__ part_p,
    const float* __restrict__ part_b, const float* __restrict__ hyper, int mode,
    float trust_coef, float wd, float* __restrict__ ratio, float* __restrict__ norms) {
  if (hyper[HYPER_SKIP] != 0.f) return;
  const int64_t* d = seg + (int64_t)blockIdx.x * SEG_COLS;
  const int64_t first = d[SEG_FIRST];
  int64_t cnt = d[SEG_NCHUNK];
  if (first < 0 || cnt < 0 || first + cnt > nchunks) cnt = 0;
  float a = 0.f, b = 0.f;
  for (int64_t i = threadIdx.x; i < cnt; i += 256) {
    a += part_p[first + i];
    b += part_b[first + i];
  }
  block_sum2(a, b);
  if (threadIdx.x != 0) return;
  const int flags = (int)d[SEG_FLAGS];
  const float pn = sqrtf(a), bn = sqrtf(b);
  float r = 1.f;
  if ((flags & SEG_ADAPT) && pn > 0.f && bn > 0.f) {
    if (mode == TRUST_LARS) {
      const float wd_s = (flags & SEG_DECAY) ? wd : 0.f;
      r = trust_coef * pn / (bn + wd_s * pn + 1e-8f);
    } else {
      r = pn / bn;
    }
  }
  ratio[blockIdx.x] = r;
  norms[2 * blockIdx.x] = pn;
  norms[2 * blockIdx.x + 1] = bn;
}

// LAMB stage 2 (p -= lr * ratio[s] * u, u from lamb_elem) and AdamW (ADAMW: torch's order,
// p *= 1 - lr * wd_s, then adam_body's step; no ratio).  Both update m, v and write the
// bf16 shadow.
template <bool ADAMW>
__global__ __launch_bounds__(256) void lamb_step_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, bf16_t* __restrict__ shadow, int64_t n,
    const float* __restrict__ step, const float* __restrict__ hyper,
    const int64_t* __restrict__ seg, const int* __restrict__ chunk_seg, int nseg,
    const float* __restrict__ ratio, float b1, float b2, float eps, float wd) {
  if (hyper[HYPER_SKIP] != 0.f) return;
  const Chunk k = chunk_of(seg, chunk_seg, nseg, blockIdx.x, n);
  const AdamCoef c = adam_coef(step, b1, b2, eps);
  const float lr = hyper[HYPER_LR], gs = hyper[HYPER_SCALE];
  const float wd_s = (k.flags & SEG_DECAY) ? wd : 0.f;
  const float step_size = lr / c.bc1;
  const float keep = 1.f - lr * wd_s;
  const float lr_r = ADAMW ? lr : lr * ratio[k.seg];
  float4* __restrict__ p4 = (float4*)(p + k.off);
  const float4* __restrict__ g4 = (const float4*)(g + k.off);
  float4* __restrict__ m4 = (float4*)(m + k.off);
  float4* __restrict__ v4 = (float4*)(v + k.off);
  uint2* __restrict__ s2 = shadow ? (uint2*)(shadow + k.off) : nullptr;
  for (int i = threadIdx.x; i < k.n4; i += 256) {
    float4 pp = p4[i];
    const float4 gg = g4[i];
    float4 mm = m4[i];
    float4 vv = v4[i];
    float* pf = (float*)&pp;
    const float* gf = (const float*)&gg;
    float* mf = (float*)&mm;
    float* vf = (float*)&vv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (ADAMW) {
        moments_elem(gf[j], gs, mf[j], vf[j], c);
        const float denom = sqrtf(vf[j]) / c.bc2s + c.eps;
        pf[j] *= keep;
        pf[j] -= step_size * mf[j] / denom;
      } else {
        const float uu = lamb_elem(pf[j], gf[j], gs, mf[j], vf[j], wd_s, c);
        pf[j] -= lr_r * uu;
      }
    }
    p4[i] = pp;
    m4[i] = mm;
    v4[i] = vv;
    if (s2) s2[i] = make_uint2(pack2(pf[0], pf[1]), pack2(pf[2], pf[3]));
  }
}

// LARS: g' = ratio[s] * (g^ + wd_s * p), then sgd_body's momentum rule with wd = 0 (first
// step seeds the buffer; dampening; nesterov); writes the bf16 shadow
__global__ __launch_bounds__(256) void lars_step_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
    bf16_t* __restrict__ shadow, int64_t n, const float* __restrict__ step,
    const float* __restrict__ hyper, const int64_t* __restrict__ seg,
    const int* __restrict__ chunk_seg, int nseg, const float* __restrict__ ratio,
    float momentum, float dampening, float wd, int nesterov) {
  if (hyper[HYPER_SKIP] != 0.f) return;
  const Chunk k = chunk_of(seg, chunk_seg, nseg, blockIdx.x, n);
  const bool first = step[0] == 0.f;
  const float lr = hyper[HYPER_LR], gs = hyper[HYPER_SCALE];
  const float wd_s = (k.flags & SEG_DECAY) ? wd : 0.f;
  const float r = ratio[k.seg];
  float4* __restrict__ p4 = (float4*)(p + k.off);
  const float4* __restrict__ g4 = (const float4*)(g + k.off);
  float4* __restrict__ b4 = (float4*)(buf + k.off);
  uint2* __restrict__ s2 = shadow ? (uint2*)(shadow + k.off) : nullptr;
  for (int i = threadIdx.x; i < k.n4; i += 256) {
    float4 pp = p4[i];
    const float4 gg = g4[i];
    float4 bb = b4[i];
    float* pf = (float*)&pp;
    const float* gf = (const float*)&gg;
    float* bf = (float*)&bb;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gr = r * (gf[j] * gs + wd_s * pf[j]);
      if (momentum != 0.f) {
        bf[j] = first ? gr : momentum * bf[j] + (1.f - dampening) * gr;
        gr = nesterov ? gr + momentum * bf[j] : bf[j];
      }
      pf[j] -= lr * gr;
    }
    p4[i] = pp;
    if (momentum != 0.f) b4[i] = bb;
    if (s2) s2[i] = make_uint2(pack2(pf[0], pf[1]), pack2(pf[2], pf[3]));
  }
}

int seg_chunk() { return SEG_CHUNK; }

void seg_sqnorm(const float* x, int64_t n, const int64_t* seg, const int* chunk_seg, int nseg,
                int nchunks, const float* hyper, int scaled, float* part, hipStream_t s) {
  if (nchunks <= 0) return;
  hipLaunchKernelGGL(seg_sqnorm_kernel, dim3(nchunks), dim3(256), 0, s, x, n, seg, chunk_seg,
                     nseg, hyper, scaled, part);
}

void lamb_norms(const float* p, const float* g, const float* m, const float* v, int64_t n,
                const float* step, const float* hyper, const int64_t* seg, const int* chunk_seg,
                int nseg, int nchunks, float* part_p, float* part_u, float b1, float b2,
                float eps, float wd, hipStream_t s) {
  if (nchunks <= 0) return;
  hipLaunchKernelGGL(lamb_norms_kernel, dim3(nchunks), dim3(256), 0, s, p, g, m, v, n, step,
                     hyper, seg, chunk_seg, nseg, part_p, part_u, b1, b2, eps, wd);
}

void trust_ratio(const int64_t* seg, int nseg, int nchunks, const float* part_p,
                 const float* part_b, const float* hyper, int mode, float trust_coef, float wd,
                 float* ratio, float* norms, hipStream_t s) {
  if (nseg <= 0) return;
  hipLaunchKernelGGL(trust_ratio_kernel, dim3(nseg), dim3(256), 0, s, seg, nchunks, part_p,
                     part_b, hyper, mode, trust_coef, wd, ratio, norms);
}

void lamb_step_dev(float* p, const float* g, float* m, float* v, bf16_raw* shadow, int64_t n,
                   const float* step, const float* hyper, const int64_t* seg,
                   const int* chunk_seg, int nseg, int nchunks, const float* ratio, float b1,
                   float b2, float eps, float wd, int adamw, hipStream_t s) {
  if (nchunks <= 0) return;
  if (adamw)
    hipLaunchKernelGGL(lamb_step_kernel<true>, dim3(nchunks), dim3(256), 0, s, p, g, m, v,
                       shadow, n, step, hyper, seg, chunk_seg, nseg, ratio, b1, b2, eps, wd);
  else
    hipLaunchKernelGGL(lamb_step_kernel<false>, dim3(nchunks), dim3(256), 0, s, p, g, m, v,
                       shadow, n, step, hyper, seg, chunk_seg, nseg, ratio, b1, b2, eps, wd);
}

void lars_step_dev(float* p, const float* g, float* buf, bf16_raw* shadow, int64_t n,
                   const float* step, const float* hyper, const int64_t* seg,
                   const int* chunk_seg, int nseg, int nchunks, const float* ratio,
                   float momentum, float dampening, float wd, int nesterov, hipStream_t s) {
  if (nchunks <= 0) return;
  hipLaunchKernelGGL(lars_step_kernel, dim3(nchunks), dim3(256), 0, s, p, g, buf, shadow, n,
                     step, hyper, seg, chunk_seg, nseg, ratio, momentum, dampening, wd,
                     nesterov);
}

// ------------------------------------------------------------------------- weight EMA
// ema += w * (p - ema) over the trainable fp32 arena, w = 1 - d_t with
// d_t = warmup ? min(decay, (1 + t) / (10 + t)) : decay and t = step[0], the optimizer's
// counter after this step's increment (the launch follows transpose_krsc / step_inc in
// stream order).  t comes from device memory, so a captured graph replays the warm-up.
// Every operation is rounded on its own (no contraction): p == ema gives p - ema = 0 and
// ema + 0 = ema, a fixed point (up to the sign of a zero: -0 + +0 = +0), and the fp32
// oracle (ops/ref.py ema_update) reproduces the kernel bit for bit.
__device__ __forceinline__ float ema_weight(const float* __restrict__ step, float decay,
                                            int warmup) {
#pragma clang fp contract(off)
  float d = decay;
  if (warmup) {
    const float t = step[0];
    const float num = 1.f + t;
    const float den = 10.f + t;
    d = fminf(decay, num / den);
  }
  return 1.f - d;
}

__device__ __forceinline__ float ema_elem(float e, float p, float w) {
#pragma clang fp contract(off)
  const float diff = p - e;
  float prod = w * diff;
  // the build's -ffp-contract=fast lets the backend fuse across the pragma; an empty asm
  // that takes the product through a register keeps it a rounded value of its own
  asm("" : "+v"(prod));
  return e + prod;
}

__device__ __forceinline__ float4 ema_elem4(float4 e, const float4 p, float w) {
  e.x = ema_elem(e.x, p.x, w);
  e.y = ema_elem(e.y, p.y, w);
  e.z = ema_elem(e.z, p.z, w);
  e.w = ema_elem(e.w, p.w, w);
  return e;
}

// 12 bytes per element (p read, ema read and written): 44.28 M elements in ~86 us warm
// (6.2 TB/s, the 354 MB partly cache resident) and ~130 us after a cache-evicting write
// (4.1 TB/s).  More float4 pairs in flight per thread (2, 4, 8; grid-strided or block
// contiguous) and grids of 2,048 to 8,192 blocks all measured within 5 % of this form.
__global__ __launch_bounds__(256) void ema_kernel(float4* __restrict__ ema,
                                                   const float4* __restrict__ p,
                                                   const float* __restrict__ step, int64_t n4,
                                                   float decay, int warmup) {
  const float w = ema_weight(step, decay, warmup);
  const int64_t stride = GRID_STRIDE;
  for (int64_t i = GRID_I0; i < n4; i += stride) ema[i] = ema_elem4(ema[i], p[i], w);
}

// The model's floating-point buffers (BN running statistics): small separate tensors.
// table [nbuf][EMA_COLS] int64 = (source address, offset into ema_buf, length), built once
// on the host; one block per row, scalar access (a source is only 4-byte aligned, lengths
// are arbitrary).  Same w and element formula as ema_kernel.  A row that does not lie
// inside ema_buf[0:n) is not followed.
__global__ __launch_bounds__(256) void ema_multi_kernel(float* __restrict__ ema_buf, int64_t n,
                                                         const int64_t* __restrict__ table,
                                                         const float* __restrict__ step,
                                                         float decay, int warmup) {
  const int64_t* r = table + (int64_t)blockIdx.x * EMA_COLS;
  const float* __restrict__ src = (const float*)(uintptr_t)r[EMA_SRC];
  const int64_t off = r[EMA_OFF], len = r[EMA_LEN];
  if (src == nullptr || off < 0 || len <= 0 || off > n || len > n - off) return;
  const float w = ema_weight(step, decay, warmup);
  float* __restrict__ e = ema_buf + off;
  for (int64_t i = threadIdx.x; i < len; i += 256) e[i] = ema_elem(e[i], src[i], w);
}

void ema_update(float* ema, const float* p, const float* step, int64_t n, float decay,
                int warmup, hipStream_t s) {
  const int64_t n4 = n / 4;
  if (n4 <= 0) return;
  hipLaunchKernelGGL(ema_kernel, dim3(blocks_for(n4)), dim3(256), 0, s, (float4*)ema,
                     (const float4*)p, step, n4, decay, warmup);
}

void ema_update_multi(float* ema_buf, int64_t n, const int64_t* table, int nbuf,
                      const float* step, float decay, int warmup, hipStream_t s) {
  if (nbuf <= 0) return;
  hipLaunchKernelGGL(ema_multi_kernel, dim3(nbuf), dim3(256), 0, s, ema_buf, n, table, step,
                     decay, warmup);
}

static void step_inc_launch(float* step, hipStream_t s);

// ------------------------------------------------------------ transposed weight shadow
// wt[c][t][k] = w[k][t][c] for every registered conv / linear weight, from the bf16 shadow
// the optimizer just wrote: dgrad then reads its B operand K-contiguous, exactly like the
// forward GEMM.  seg: [nseg][6] int64 = (src_off, dst_off, K, RS, C, first_tile); one
// 64x64 (k, c) tile of one tap per block, tiles of all weights in one flat grid.
__global__ __launch_bounds__(256) void transpose_krsc_kernel(const bf16_t* __restrict__ w,
                                                              bf16_t* __restrict__ wt,
                                                              const int64_t* __restrict__ seg,
                                                              int nseg, int total_tiles,
                                                              float* __restrict__ step_inc) {
  // the optimizer kernel that read the step counter has completed (stream order): count
  // the step here instead of in a launch of its own
  if (step_inc && blockIdx.x == 0 && threadIdx.x == 0) *step_inc += 1.f;
  // 64 (k) x 64 (c) tile, rows of eight 16-B chunks; chunk q of row r is stored at
  // position q ^ ((r >> 3) & 7), so the store phase's column gathers (8 lanes per k-row
  // group, one k-row from each of 8 row groups) hit 8 distinct chunk positions: no bank
  // conflicts (with a padded [64][72] tile they were 4-way)
  __shared__ __attribute__((aligned(16))) bf16_t tile[64][64];
  // one tile per block (a grid-stride loop over tiles with 2,048 blocks measured slower)
  for (int b = blockIdx.x; b < total_tiles; b += gridDim.x) {
    __syncthreads();  // previous tile's gathers done before the tile is overwritten
    int lo = 0, hi = nseg - 1;  // last segment whose first_tile <= b (uniform)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (seg[mid * 6 + 5] <= b) lo = mid; else hi = mid - 1;
    }
    const int64_t* d = seg + lo * 6;
    const int64_t so = d[0], dof = d[1];
    const int K = (int)d[2], RS = (int)d[3], C = (int)d[4];  // K % 8 == 0, C % 8 == 0
    const int tk = (K + 63) / 64, tc = (C + 63) / 64;
    int r = b - (int)d[5];
    const int t = r / (tk * tc);
    r -= t * tk * tc;
    const int k0 = (r / tc) * 64, c0 = (r % tc) * 64;
    // load: 512 16-B chunks (64 k-rows x 8 c-chunks), 2 per thread
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int q = threadIdx.x + 256 * h;
      const int row = q >> 3, ch = q & 7;
      const int k = k0 + row, c = c0 + ch * 8;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (k < K && c < C) v = *(const uint4*)(w + so + ((size_t)k * RS + t) * C + c);
      *(uint4*)&tile[row][(ch ^ ((row >> 3) & 7)) * 8] = v;
    }
    __syncthreads();
    // store: 512 16-B chunks (64 c-rows x 8 k-chunks), each gathered from a tile column
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int q = threadIdx.x + 256 * h;
      const int crow = q >> 3, kk = (q & 7) * 8;
      const int c = c0 + crow, k = k0 + kk;
      if (c < C && k < K) {
        const int cpos = crow & 7, cq = crow >> 3;
        const int col = ((cq ^ (q & 7)) << 3) + cpos;  // rows kk..kk+7 share (row >> 3) = q & 7
        uint32_t e[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          e[u] = (uint32_t)tile[kk + 2 * u][col] | ((uint32_t)tile[kk + 2 * u + 1][col] << 16);
        *(uint4*)(wt + dof + ((size_t)c * RS + t) * K + k) = make_uint4(e[0], e[1], e[2], e[3]);
      }
    }
  }
}

void transpose_krsc(const bf16_raw* w, bf16_raw* wt, const int64_t* seg, int nseg,
                    int total_tiles, hipStream_t s, float* step_inc) {
  if (nseg <= 0 || total_tiles <= 0) {
    if (step_inc) step_inc_launch(step_inc, s);
    return;
  }
  hipLaunchKernelGGL(transpose_krsc_kernel, dim3(total_tiles), dim3(256), 0, s, w, wt, seg, nseg,
                     total_tiles, step_inc);
}

// ------------------------------------------------------------------------ small helpers
__global__ __launch_bounds__(256) void zero_f32_kernel(float4* __restrict__ t, int64_t n4) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x)
    t[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ void step_inc_kernel(float* step) { *step += 1.f; }

// dst[i] += src[i] (fp32; small vectors: a bias gradient from a fused reduction)
__global__ __launch_bounds__(256) void add_f32_kernel(float* __restrict__ dst,
                                                     const float* __restrict__ src, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    dst[i] += src[i];
}

// t viewed as [rows][period] fp32: zero columns [first, first + count) of every row (the
// pixel-pair stem's weight-gradient column past the kernel, layers.Conv2d.fix_grad)
__global__ __launch_bounds__(256) void zero_cols_f32_kernel(float* __restrict__ t, int64_t rows,
                                                            int period, int first, int count) {
  const int64_t n = rows * count;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / count;
    t[r * period + first + (int)(i - r * count)] = 0.f;
  }
}

// a += b over bf16 vectors (fp32 add, one rounding): two computed gradient contributions
// of one activation (GradJoin) summed without an ATen elementwise kernel
__global__ __launch_bounds__(256) void add_bf16_kernel(uint4* __restrict__ a,
                                                       const uint4* __restrict__ b, int64_t n8) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n8;
       i += (int64_t)gridDim.x * blockDim.x) {
    float x[8], y[8];
    unpack8(a[i], x);
    unpack8(b[i], y);
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] += y[j];
    a[i] = pack8(x);
  }
}

void zero_cols_f32(float* t, int64_t rows, int period, int first, int count, hipStream_t s) {
  const int64_t n = rows * count;
  if (n > 0)
    hipLaunchKernelGGL(zero_cols_f32_kernel, dim3(blocks_for((n + 3) / 4)), dim3(256), 0, s, t,
                       rows, period, first, count);
}

void add_bf16(bf16_raw* a, const bf16_raw* b, int64_t n, hipStream_t s) {
  const int64_t n8 = n / 8;
  if (n8 > 0)
    hipLaunchKernelGGL(add_bf16_kernel, dim3(blocks_for((n8 + 1) / 2)), dim3(256), 0, s,
                       (uint4*)a, (const uint4*)b, n8);
}

void zero_f32(float* t, int64_t n, hipStream_t s) {
  const int64_t n4 = n / 4;
  if (n4 > 0)
    hipLaunchKernelGGL(zero_f32_kernel, dim3(blocks_for(n4)), dim3(256), 0, s, (float4*)t, n4);
}

void add_f32(float* dst, const float* src, int64_t n, hipStream_t s) {
  if (n > 0)
    hipLaunchKernelGGL(add_f32_kernel, dim3(std::min<int64_t>((n + 255) / 256, 1024)), dim3(256),
                       0, s, dst, src, n);
}

static void step_inc_launch(float* step, hipStream_t s) {
  hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, s, step);
}
void step_inc(float* step, hipStream_t s) { step_inc_launch(step, s); }

}  // namespace mpa
