// Fused softmax cross-entropy (K10) and argmax accuracy (K12).
//
// Forward: one workgroup per row makes ONE pass over the logits with an online
// (running max, rescaled sum) log-sum-exp - no max pass, no materialised softmax - and
// adds (lse - logit[label]) / B into the scalar loss.  Backward recomputes
// softmax = exp(logit - lse) from the saved per-row LSE and writes
// (softmax - onehot) * grad_out / B in bf16: logits are read twice in total, the
// gradient written once.  Reference: nn.CrossEntropyLoss at main.py:134,150 over a
// 64,500-wide head (utils.py:39); argmax accuracy at main.py:182-183.
//
// Rows may be padded (row stride ld >= NC): classifier heads store their output dim
// rounded up to a multiple of 32 so every GEMM of the head stays 16-B granular; the
// backward writes zeros into the padding columns of dlogits.
//
// SMOOTH (label smoothing, torch's cross_entropy(label_smoothing=eps)): the row loss is
// lse - (1-eps) * logit[label] - (eps/NC) * sum_c logit[c] and the gradient subtracts
// (1-eps) * onehot + eps/NC instead of onehot.  The forward's only new quantity is the
// per-row sum of the logits, accumulated in the same pass and reduced in the same fixed
// order as (m, s); the backward needs only the two constants.  Everything smoothing adds
// sits under "if constexpr (SMOOTH)", and eps == 0 launches the SMOOTH = false
// instantiations: the plain loss runs the code it ran before smoothing existed.
//
// MIX (Mixup / CutMix, two labels per row): the target is lam * onehot(y) + (1 - lam) *
// onehot(y2) before smoothing, with lam read per row from device memory (a captured graph
// replays with new values).  The forward looks up a second logit, row loss = lse - (1-eps) *
// (lam * x[y] + (1-lam) * x[y2]) - (eps/NC) * sum_c x[c]; the backward subtracts (1-eps) *
// (lam * [c == y] + (1-lam) * [c == y2]), the two weights added first, so y == y2 and a
// swap of (y, lam) with (y2, 1-lam) come out right.  Everything it adds sits under "if
// constexpr (MIX)" - the kernel arguments too (CeMix) - and null labels2 launches the
// MIX = false instantiations: the one-label loss runs the code it ran before.
//
// ADJ (logit adjustment, Menon et al. 2021): the loss is CE of z = float(x) + bias with bias
// fp32 [NC] (tau * log prior), added in registers - the bf16 logits in memory stay as they
// are.  z takes x's place everywhere: the online LSE (the saved lse is lse(z)), the smoothed
// sum, the picked logits and the backward's softmax.  bias is read with 16-B loads beside the
// logit loads (two per 8 logits) and only in [0, NC): a vector that straddles NC reads its
// valid columns one by one.  258 KB at NC = 64,500, so it stays in L2 and HBM still streams
// only logits.  Everything it adds sits under "if constexpr (ADJ)" - the kernel argument too
// (CeAdj, ahead of CeMix: empty, it sits in the padding in front of the mixed kernels'
// pointers, so no existing argument moves) - and a null bias launches the ADJ = false
// instantiations.
//
// Top-k accuracy (topk_correct): no selection or sort - a row is correct iff fewer than k
// columns outrank its label's logit, ties going to the lower index (argmax_kernel's rule).
#include "common.h"
#include "api.h"
#include <cstdlib>
#include <algorithm>

namespace mpa {

template <int V>
__device__ __forceinline__ void load_v(const bf16_t* p, float* f) {
  if constexpr (V == 8) {
    unpack8(*(const uint4*)p, f);
  } else if constexpr (V == 4) {
    const uint2 u = *(const uint2*)p;
    f[0] = __uint_as_float(u.x << 16); f[1] = __uint_as_float(u.x & 0xffff0000u);
    f[2] = __uint_as_float(u.y << 16); f[3] = __uint_as_float(u.y & 0xffff0000u);
  } else {
    f[0] = bf2f(p[0]);
  }
}

__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  if (mn == -INFINITY) return;
  s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
  m = mn;
}

// lam * a + (1 - lam) * b with every operation rounded on its own: exactly a at lam == 1
// and b at lam == 0, and symmetric under (a, lam) <-> (b, 1 - lam) for dyadic lam
__device__ __forceinline__ float ce_mix2(float lam, float a, float b) {
#pragma clang fp contract(off)
  const float om = 1.f - lam;
  const float pa = lam * a;
  const float pb = om * b;
  return pa + pb;
}

// the MIX instantiations' extra kernel arguments (an empty argument otherwise)
template <bool MIX>
struct CeMix {};
template <>
struct CeMix<true> {
  const int64_t* labels2;  // [B]
  const float* lam;        // [B]
};

// the ADJ instantiations' extra kernel argument (an empty argument otherwise)
template <bool ADJ>
struct CeAdj {};
template <>
struct CeAdj<true> {
  const float* bias;  // [NC] fp32, 16-B aligned
};

// b[j] = bias[c0 + j] for the columns c0 + j < NC, 0 for the rest (never read); c0 % V == 0,
// so a whole vector is V/4 aligned 16-B loads
template <int V>
__device__ __forceinline__ void load_bias(const float* __restrict__ bias, int c0, int NC,
                                          float* b) {
  if (c0 + V <= NC) {
    if constexpr (V == 1) {
      b[0] = bias[c0];
    } else {
#pragma unroll
      for (int q = 0; q < V / 4; ++q) {
        const float4 u = *(const float4*)(bias + c0 + 4 * q);
        b[4 * q] = u.x; b[4 * q + 1] = u.y; b[4 * q + 2] = u.z; b[4 * q + 3] = u.w;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) b[j] = c0 + j < NC ? bias[c0 + j] : 0.f;
  }
}

// the (adjusted) logit of column c, 0 <= c < NC
template <bool ADJ>
__device__ __forceinline__ float ce_pick(const bf16_t* x, int64_t c, const CeAdj<ADJ>& aj) {
  if constexpr (ADJ) return bf2f(x[c]) + aj.bias[c];
  else return bf2f(x[c]);
}

// Block-reduce the per-thread (m, s) - and, SMOOTH, the logit sum t - in a fixed order
// (wave shuffle, then 4 LDS entries) and have thread 0 write the row's lse and loss term.
template <bool SMOOTH, bool MIX, bool ADJ>
__device__ __forceinline__ void ce_row_finish(float m, float s, float t, const bf16_t* x, int row,
                                              const int64_t* __restrict__ labels, int B, int NC,
                                              float* __restrict__ row_loss,
                                              float* __restrict__ lse_out, float eps,
                                              const CeMix<MIX>& mx, const CeAdj<ADJ>& aj) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    lse_merge(m, s, m2, s2);
    if constexpr (SMOOTH) t += __shfl_xor(t, o, 64);
  }
  __shared__ float sm[4], ss[4], st[SMOOTH ? 4 : 1];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sm[w] = m; ss[w] = s;
    if constexpr (SMOOTH) st[w] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = sm[0], S = ss[0];
    for (int i = 1; i < 4; ++i) lse_merge(M, S, sm[i], ss[i]);
    const float lse = M + __logf(S);
    lse_out[row] = lse;
    const int64_t lab = labels[row];
    if constexpr (MIX) {  // both labels valid (the callers' contract)
      const int64_t lab2 = mx.labels2[row];
      const bool ok = lab >= 0 && lab < NC && lab2 >= 0 && lab2 < NC;
      const float picked = ce_mix2(mx.lam[row], ce_pick<ADJ>(x, ok ? lab : 0, aj),
                                   ce_pick<ADJ>(x, ok ? lab2 : 0, aj));
      if constexpr (SMOOTH) {
        const float T = (st[0] + st[1]) + (st[2] + st[3]);
        const float l = lse - (1.f - eps) * picked - (eps / (float)NC) * T;
        row_loss[row] = ok ? l / (float)B : 0.f;
      } else {
        row_loss[row] = (lse - (ok ? picked : lse)) / (float)B;
      }
    } else if constexpr (SMOOTH) {
      const float T = (st[0] + st[1]) + (st[2] + st[3]);
      const float l = lse - (1.f - eps) * ce_pick<ADJ>(x, lab >= 0 && lab < NC ? lab : 0, aj) -
                      (eps / (float)NC) * T;
      row_loss[row] = (lab >= 0 && lab < NC) ? l / (float)B : 0.f;
    } else {
      const float picked = (lab >= 0 && lab < NC) ? ce_pick<ADJ>(x, lab, aj) : lse;
      row_loss[row] = (lse - picked) / (float)B;
    }
  }
}

template <int V, bool SMOOTH = false, bool MIX = false, bool ADJ = false>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const bf16_t* __restrict__ logits,
                                                      const int64_t* __restrict__ labels, int B,
                                                      int NC, int ld, float* __restrict__ row_loss,
                                                      float* __restrict__ lse_out, float eps,
                                                      CeAdj<ADJ> aj, CeMix<MIX> mx) {
  const int row = blockIdx.x;
  const bf16_t* x = logits + (size_t)row * ld;
  float m = -INFINITY, s = 0.f, t = 0.f;
  const int nv = NC / V;
  for (int i = threadIdx.x; i < nv; i += 256) {
    float f[V];
    load_v<V>(x + (size_t)i * V, f);
    if constexpr (ADJ) {
      float b[V];
      load_bias<V>(aj.bias, i * V, NC, b);
#pragma unroll
      for (int j = 0; j < V; ++j) f[j] += b[j];
    }
    float lm = f[0];
#pragma unroll
    for (int j = 1; j < V; ++j) lm = fmaxf(lm, f[j]);
    const float mn = fmaxf(m, lm);
    float acc = s * __expf(m - mn);
#pragma unroll
    for (int j = 0; j < V; ++j) acc += __expf(f[j] - mn);
    m = mn;
    s = acc;
    if constexpr (SMOOTH) {
#pragma unroll
      for (int j = 0; j < V; ++j) t += f[j];
    }
  }
  ce_row_finish<SMOOTH, MIX, ADJ>(m, s, t, x, row, labels, B, NC, row_loss, lse_out, eps, mx,
                                  aj);
}

// Padded rows (ld % 8 == 0, 16-B aligned; the 64,500-class head has ld = 64,512): 16-B
// loads over the whole padded row with columns >= NC masked to -inf, U loads issued before
// any is consumed.  The unpadded kernel above walked 64,500 columns in 8-B loads, one load
// per online-LSE step, and streamed ~2.2 TB/s (30 us per 66 MB of logits).
template <int U, bool SMOOTH = false, bool MIX = false, bool ADJ = false>
__global__ __launch_bounds__(256) void ce_fwd_padded_kernel(const bf16_t* __restrict__ logits,
                                                             const int64_t* __restrict__ labels,
                                                             int B, int NC, int ld,
                                                             float* __restrict__ row_loss,
                                                             float* __restrict__ lse_out,
                                                             float eps, CeAdj<ADJ> aj,
                                                             CeMix<MIX> mx) {
  const int row = blockIdx.x;
  const bf16_t* x = logits + (size_t)row * ld;
  float m = -INFINITY, s = 0.f, t = 0.f;
  const int nv = ld / 8;
  for (int i0 = threadIdx.x; i0 < nv; i0 += 256 * U) {
    uint4 v[U];
    float b[ADJ ? U : 1][8];  // ADJ: the bias of the same columns, in flight with the logits
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * 256;
      v[u] = i < nv ? *(const uint4*)(x + (size_t)i * 8) : make_uint4(0u, 0u, 0u, 0u);
      if constexpr (ADJ) load_bias<8>(aj.bias, i * 8, NC, b[u]);  // (reads nothing at >= NC)
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c0 = (i0 + u * 256) * 8;
      if (c0 >= NC) continue;
      float f[8];
      unpack8(v[u], f);
      if constexpr (ADJ) {
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] += b[u][j];
      }
      float lm = -INFINITY;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (c0 + j >= NC) f[j] = -INFINITY;
        else if constexpr (SMOOTH) t += f[j];  // pad columns add 0, not the -inf mask
        lm = fmaxf(lm, f[j]);
      }
      const float mn = fmaxf(m, lm);
      float acc = s * __expf(m - mn);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += __expf(f[j] - mn);
      m = mn;
      s = acc;
    }
  }
  ce_row_finish<SMOOTH, MIX, ADJ>(m, s, t, x, row, labels, B, NC, row_loss, lse_out, eps, mx,
                                  aj);
}

// SMOOTH: onw = 1 - eps is the label's weight, unif = eps / NC every class's share.
// MIX: column c loses onw * (lam * [c == y] + (1 - lam) * [c == y2]).
template <int V, bool SMOOTH = false, bool MIX = false, bool ADJ = false>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const bf16_t* __restrict__ logits,
                                                      const int64_t* __restrict__ labels,
                                                      const float* __restrict__ lse,
                                                      const float* __restrict__ grad_out, int B,
                                                      int NC, int ld, bf16_t* __restrict__ dlogits,
                                                      float weight, float onw, float unif,
                                                      CeAdj<ADJ> aj, CeMix<MIX> mx) {
  const float scale = grad_out[0] * weight / (float)B;
  const int nv = ld / V;  // whole padded row: columns >= NC get zero gradient
  const int64_t total = (int64_t)B * nv;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int row = (int)(t / nv);
    const int c0 = (int)(t - (int64_t)row * nv) * V;
    const float l = lse[row];
    const int64_t lab = labels[row];
    int64_t lab2 = 0;
    float lam = 1.f;
    if constexpr (MIX) lab2 = mx.labels2[row], lam = mx.lam[row];
    float f[V];
    const size_t off = (size_t)row * ld + c0;
    load_v<V>(logits + off, f);
    if constexpr (ADJ) {
      float b[V];
      load_bias<V>(aj.bias, c0, NC, b);
#pragma unroll
      for (int j = 0; j < V; ++j) f[j] += b[j];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float p = __expf(f[j] - l);
      if constexpr (MIX) {
        if constexpr (SMOOTH) p -= unif;
        if (c0 + j == lab || c0 + j == lab2) {  // the two weights first: their sum is exact
                                                // for lam = 1, 0 and dyadic values
          const float w = (c0 + j == lab ? lam : 0.f) + (c0 + j == lab2 ? 1.f - lam : 0.f);
          if constexpr (SMOOTH) p -= onw * w;
          else p -= w;
        }
      } else if constexpr (SMOOTH) {
        p -= unif;
        if (c0 + j == lab) p -= onw;
      } else {
        if (c0 + j == lab) p -= 1.f;
      }
      f[j] = (c0 + j < NC) ? p * scale : 0.f;
    }
    if constexpr (V == 8) {
      *(uint4*)(dlogits + off) = pack8(f);
    } else if constexpr (V == 4) {
      *(uint2*)(dlogits + off) = make_uint2(pack2(f[0], f[1]), pack2(f[2], f[3]));
    } else {
      dlogits[off] = f2bf(f[0]);
    }
  }
}

__global__ __launch_bounds__(256) void argmax_kernel(const bf16_t* __restrict__ logits,
                                                      const int64_t* __restrict__ labels, int NC,
                                                      int ld, unsigned long long* __restrict__ count) {
  const int row = blockIdx.x;
  const bf16_t* x = logits + (size_t)row * ld;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = threadIdx.x; i < NC; i += 256) {
    const float v = bf2f(x[i]);
    if (v > best) { best = v; bi = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(best, o, 64);
    const int i2 = __shfl_xor(bi, o, 64);
    if (v2 > best || (v2 == best && i2 < bi)) { best = v2; bi = i2; }
  }
  __shared__ float sv[4];
  __shared__ int si[4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sv[w] = best; si[w] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i)
      if (sv[i] > best || (sv[i] == best && si[i] < bi)) { best = sv[i]; bi = si[i]; }
    if ((int64_t)bi == labels[row]) atomicAdd(count, 1ull);
  }
}

// argmax_kernel's row argmax (duplicated, so that kernel stays as it was) feeding per-class
// counters as well: stats int64 [3][NC] = support, predicted, true positives.  count gets what
// argmax_kernel adds.  A row whose label is outside [0, NC) touches no counter; an all-NaN
// (or all -inf) row has no prediction (bi stays 0x7fffffff).  Integer atomics: exact under
// contention and independent of their order.
__global__ __launch_bounds__(256) void argmax_stats_kernel(const bf16_t* __restrict__ logits,
                                                            const int64_t* __restrict__ labels,
                                                            int NC, int ld,
                                                            unsigned long long* __restrict__ count,
                                                            unsigned long long* __restrict__ stats) {
  const int row = blockIdx.x;
  const bf16_t* x = logits + (size_t)row * ld;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = threadIdx.x; i < NC; i += 256) {
    const float v = bf2f(x[i]);
    if (v > best) { best = v; bi = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(best, o, 64);
    const int i2 = __shfl_xor(bi, o, 64);
    if (v2 > best || (v2 == best && i2 < bi)) { best = v2; bi = i2; }
  }
  __shared__ float sv[4];
  __shared__ int si[4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sv[w] = best; si[w] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i)
      if (sv[i] > best || (sv[i] == best && si[i] < bi)) { best = sv[i]; bi = si[i]; }
    const int64_t lab = labels[row];
    if ((int64_t)bi == lab) atomicAdd(count, 1ull);
    if (lab >= 0 && lab < NC) {
      atomicAdd(stats + lab, 1ull);
      if (bi < NC) atomicAdd(stats + (size_t)NC + bi, 1ull);
      if ((int64_t)bi == lab) atomicAdd(stats + 2 * (size_t)NC + lab, 1ull);
    }
  }
}

// Top-k accuracy: the row is correct iff fewer than k columns outrank its label, where
// column c outranks the label when x[c] > x[label], or x[c] == x[label] and c < label
// (argmax_kernel's tie rule, so k = 1 counts what argmax_correct counts).  Rows whose label
// is outside [0, NC) or whose label logit is NaN are not counted (x[label] is not read for
// the former); NaNs elsewhere compare false.  VEC: 16-B loads over the padded row
// (ld % 8 == 0, 16-B aligned), U in flight as in ce_fwd_padded_kernel, columns >= NC
// excluded.  Integer counts all the way, so the result does not depend on any order.
template <bool VEC, int U>
__global__ __launch_bounds__(256) void topk_kernel(const bf16_t* __restrict__ logits,
                                                    const int64_t* __restrict__ labels, int NC,
                                                    int ld, int k,
                                                    unsigned long long* __restrict__ count) {
  const int row = blockIdx.x;
  const bf16_t* x = logits + (size_t)row * ld;
  const int64_t lab64 = labels[row];
  if (lab64 < 0 || lab64 >= NC) return;  // block-uniform
  const int lab = (int)lab64;
  const float xl = bf2f(x[lab]);
  if (xl != xl) return;  // block-uniform
  int n = 0;
  if constexpr (VEC) {
    const int nv = ld / 8;
    for (int i0 = threadIdx.x; i0 < nv; i0 += 256 * U) {
      uint4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * 256;
        v[u] = i < nv ? *(const uint4*)(x + (size_t)i * 8) : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c0 = (i0 + u * 256) * 8;
        if (c0 >= NC) continue;
        float f[8];
        unpack8(v[u], f);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = c0 + j;
          n += (c < NC && (f[j] > xl || (f[j] == xl && c < lab))) ? 1 : 0;
        }
      }
    }
  } else {
    for (int c = threadIdx.x; c < NC; c += 256) {
      const float v = bf2f(x[c]);
      n += (v > xl || (v == xl && c < lab)) ? 1 : 0;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  __shared__ int sn[4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sn[w] = n;
  __syncthreads();
  if (threadIdx.x == 0 && sn[0] + sn[1] + sn[2] + sn[3] < k) atomicAdd(count, 1ull);
}

// ---- topk_predict: which classes won, and their softmax probabilities, in one pass.
//
// Candidates are the columns c < NC whose logit is neither NaN nor -inf; c outranks d when
// x[c] > x[d], or x[c] == x[d] and c < d (argmax_kernel's rule).  idx[row][j] is the candidate
// that exactly j candidates outrank, prob[row][j] = exp(x[idx] - lse) with lse the fp32
// log-sum-exp of the row's NC columns (ce_fwd's quantity); slots past the last candidate get
// idx = -1, prob = 0.
//
// Each lane walks its columns in rising order with an online (max, sum) pair and a sorted list
// of its K best (value, index) pairs: arrays indexed only by unrolled constants, so they live in
// registers.  A new value enters the list only when it is greater than the list's last entry,
// and inside the list it passes only smaller entries: equal values keep their column order.
// The row's k best are among the lanes' lists, so the block then runs k rounds: the lanes' list
// heads are reduced (wave shuffles, then four LDS entries; each round has its own entries, so
// one barrier per round is enough), thread 0 writes the winner and the lane that held it pops
// its head.  No atomics and a fixed reduction order: a row's outputs depend on that row alone.

constexpr int TOP_NONE = 0x7fffffff;  // the index of an empty list slot (argmax_kernel's "none")

// (v, c) outranks (v2, c2)
__device__ __forceinline__ bool top_outranks(float v, int c, float v2, int c2) {
  return v > v2 || (v == v2 && c < c2);
}

// insert (v, c) into the descending list; the caller has checked v > lv[K - 1]
template <int K>
__device__ __forceinline__ void top_insert(float (&lv)[K], int (&li)[K], float v, int c) {
#pragma unroll
  for (int j = K - 1; j > 0; --j) {
    const bool up = v > lv[j - 1];  // v goes above slot j-1, whose entry moves down to j
    const bool here = v > lv[j];
    li[j] = up ? li[j - 1] : (here ? c : li[j]);
    lv[j] = up ? lv[j - 1] : (here ? v : lv[j]);
  }
  if (v > lv[0]) { lv[0] = v; li[0] = c; }
}

// VEC: 16-B loads over the vectors that hold a column < NC (ld % 8 == 0, 16-B aligned), U in
// flight as in topk_kernel, columns >= NC masked to -inf (no candidate, exp() = 0).
template <int K, bool VEC, int U>
__global__ __launch_bounds__(256) void topk_predict_kernel(const bf16_t* __restrict__ logits,
                                                            int NC, int ld, int k,
                                                            int* __restrict__ idx,
                                                            float* __restrict__ prob) {
  const int row = blockIdx.x;
  const bf16_t* x = logits + (size_t)row * ld;
  float m = -INFINITY, s = 0.f;
  float lv[K];
  int li[K];
#pragma unroll
  for (int j = 0; j < K; ++j) { lv[j] = -INFINITY; li[j] = TOP_NONE; }
  if constexpr (VEC) {
    const int nv = (NC + 7) / 8;
    for (int i0 = threadIdx.x; i0 < nv; i0 += 256 * U) {
      uint4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * 256;
        v[u] = i < nv ? *(const uint4*)(x + (size_t)i * 8) : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c0 = (i0 + u * 256) * 8;
        if (c0 >= NC) continue;
        float f[8];
        unpack8(v[u], f);
        float lm = -INFINITY;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (c0 + j >= NC) f[j] = -INFINITY;
          lm = fmaxf(lm, f[j]);  // (skips NaN)
        }
        if (lm == -INFINITY) continue;  // no candidate here, and nothing for the sum
        const float mn = fmaxf(m, lm);
        float acc = s * __expf(m - mn);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += __expf(f[j] - mn);
        m = mn;
        s = acc;
        if (lm > lv[K - 1]) {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (f[j] > lv[K - 1]) top_insert<K>(lv, li, f[j], c0 + j);
        }
      }
    }
  } else {
    for (int c = threadIdx.x; c < NC; c += 256) {
      const float v = bf2f(x[c]);
      lse_merge(m, s, v, 1.f);
      if (v > lv[K - 1]) top_insert<K>(lv, li, v, c);  // (false for a NaN)
    }
  }
  // the row's log-sum-exp, in ce_row_finish's order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    lse_merge(m, s, m2, s2);
  }
  __shared__ float sm[4], ss[4];
  __shared__ float sv[K][4];
  __shared__ int si[K][4];
  const int w = threadIdx.x >> 6;
  const bool lead = (threadIdx.x & 63) == 0;
  if (lead) { sm[w] = m; ss[w] = s; }
  // sm / ss are published by round 0's barrier and read by thread 0 alone, which keeps the
  // row's lse for every round
  float lse = 0.f;
  for (int r = 0; r < k; ++r) {
    float bv = lv[0];
    int bi = li[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float v2 = __shfl_xor(bv, o, 64);
      const int i2 = __shfl_xor(bi, o, 64);
      if (top_outranks(v2, i2, bv, bi)) { bv = v2; bi = i2; }
    }
    if (lead) { sv[r][w] = bv; si[r][w] = bi; }
    __syncthreads();
    bv = sv[r][0]; bi = si[r][0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
      if (top_outranks(sv[r][i], si[r][i], bv, bi)) { bv = sv[r][i]; bi = si[r][i]; }
    if (li[0] == bi) {  // column indices are unique: one lane (or, with none left, any empty one)
#pragma unroll
      for (int j = 0; j + 1 < K; ++j) { lv[j] = lv[j + 1]; li[j] = li[j + 1]; }
      lv[K - 1] = -INFINITY; li[K - 1] = TOP_NONE;
    }
    if (threadIdx.x == 0) {
      if (r == 0) {
        float M = sm[0], S = ss[0];
        for (int i = 1; i < 4; ++i) lse_merge(M, S, sm[i], ss[i]);
        lse = M + __logf(S);
      }
      const bool some = bi != TOP_NONE;
      idx[(size_t)row * k + r] = some ? bi : -1;
      // (the sum's rounding can leave lse a few ulps under the largest logit)
      prob[(size_t)row * k + r] = some ? fminf(__expf(bv - lse), 1.f) : 0.f;
    }
  }
}

// loss = sum of the per-row terms in a FIXED order (strided per-thread partial sums, then a
// fixed tree): bitwise reproducible, unlike one float atomic per row (whose order varies
// between launches), and one launch like the memset it replaces.
__global__ __launch_bounds__(256) void ce_loss_sum_kernel(const float* __restrict__ row_loss, int B,
                                                          float* __restrict__ loss, int accumulate,
                                                          float weight, float* __restrict__ acc) {
  __shared__ float red[256];
  float a = 0.f;
  for (int i = threadIdx.x; i < B; i += 256) a += row_loss[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float v = weight * red[0];
    if (accumulate) *loss += v;
    else *loss = v;
    if (acc) *acc += v;  // the trainer's running loss sum (one host sync per epoch)
  }
}

// loss: [1 + B] floats - the mean loss at [0], the per-row terms after it
void ce_fwd(const bf16_raw* logits, const int64_t* labels, int B, int NC, int ld, float* loss,
            float* lse, hipStream_t s, float smoothing, const int64_t* labels2,
            const float* lam, const float* bias) {
  float* rows = loss + 1;
  ce_fwd_rows(logits, labels, B, NC, ld, rows, lse, s, smoothing, labels2, lam, bias);
  hipLaunchKernelGGL(ce_loss_sum_kernel, dim3(1), dim3(256), 0, s, rows, B, loss,
                     0, 1.f, (float*)nullptr);
}

// out[0] = (or +=) weight * mean CE; acc[0] += the same (when acc is set).  rows: B floats of
// scratch.  Several heads (Inception's main + 0.4 * aux) sum into one loss this way.
void ce_fwd_weighted(const bf16_raw* logits, const int64_t* labels, int B, int NC, int ld,
                     float* out, float* acc, float weight, bool accumulate, float* rows,
                     float* lse, hipStream_t s, float smoothing, const int64_t* labels2,
                     const float* lam, const float* bias) {
  ce_fwd_rows(logits, labels, B, NC, ld, rows, lse, s, smoothing, labels2, lam, bias);
  hipLaunchKernelGGL(ce_loss_sum_kernel, dim3(1), dim3(256), 0, s, rows, B, out,
                     accumulate ? 1 : 0, weight, acc);
}

// the forward's choice of kernel, for one flavour
template <bool SMOOTH, bool MIX, bool ADJ>
static void ce_fwd_rows_t(const bf16_raw* logits, const int64_t* labels, int B, int NC, int ld,
                          float* loss, float* lse, hipStream_t s, float eps, CeMix<MIX> mx,
                          CeAdj<ADJ> aj) {
  if (ld % 8 == 0 && ld >= NC && reinterpret_cast<uintptr_t>(logits) % 16 == 0) {
    hipLaunchKernelGGL((ce_fwd_padded_kernel<4, SMOOTH, MIX, ADJ>), dim3(B), dim3(256), 0, s,
                       logits, labels, B, NC, ld, loss, lse, eps, aj, mx);
    return;
  }
  const int g = NC % 8 == 0 && ld % 8 == 0 ? 8 : (NC % 4 == 0 && ld % 4 == 0 ? 4 : 1);
  if (g == 8)
    hipLaunchKernelGGL((ce_fwd_kernel<8, SMOOTH, MIX, ADJ>), dim3(B), dim3(256), 0, s, logits,
                       labels, B, NC, ld, loss, lse, eps, aj, mx);
  else if (g == 4)
    hipLaunchKernelGGL((ce_fwd_kernel<4, SMOOTH, MIX, ADJ>), dim3(B), dim3(256), 0, s, logits,
                       labels, B, NC, ld, loss, lse, eps, aj, mx);
  else
    hipLaunchKernelGGL((ce_fwd_kernel<1, SMOOTH, MIX, ADJ>), dim3(B), dim3(256), 0, s, logits,
                       labels, B, NC, ld, loss, lse, eps, aj, mx);
}

template <bool SMOOTH, bool MIX>
static void ce_fwd_rows_a(const bf16_raw* logits, const int64_t* labels, int B, int NC, int ld,
                          float* loss, float* lse, hipStream_t s, float eps, CeMix<MIX> mx,
                          const float* bias) {
  if (bias)
    ce_fwd_rows_t<SMOOTH, MIX, true>(logits, labels, B, NC, ld, loss, lse, s, eps, mx,
                                     CeAdj<true>{bias});
  else
    ce_fwd_rows_t<SMOOTH, MIX, false>(logits, labels, B, NC, ld, loss, lse, s, eps, mx,
                                      CeAdj<false>{});
}

// smoothing == 0 launches the SMOOTH = false instantiations, null labels2 the one-label
// ones, null bias the unadjusted ones (the plain loss, unchanged)
void ce_fwd_rows(const bf16_raw* logits, const int64_t* labels, int B, int NC, int ld, float* loss,
                 float* lse, hipStream_t s, float smoothing, const int64_t* labels2,
                 const float* lam, const float* bias) {
  if (labels2) {
    const CeMix<true> mx{labels2, lam};
    if (smoothing != 0.f)
      ce_fwd_rows_a<true, true>(logits, labels, B, NC, ld, loss, lse, s, smoothing, mx, bias);
    else
      ce_fwd_rows_a<false, true>(logits, labels, B, NC, ld, loss, lse, s, 0.f, mx, bias);
    return;
  }
  if (smoothing != 0.f)
    ce_fwd_rows_a<true, false>(logits, labels, B, NC, ld, loss, lse, s, smoothing,
                               CeMix<false>{}, bias);
  else
    ce_fwd_rows_a<false, false>(logits, labels, B, NC, ld, loss, lse, s, 0.f, CeMix<false>{},
                                bias);
}

template <bool SMOOTH, bool MIX, bool ADJ>
static void ce_bwd_t(const bf16_raw* logits, const int64_t* labels, const float* lse,
                     const float* grad_out, int B, int NC, int ld, bf16_raw* dlogits,
                     hipStream_t s, float weight, float eps, CeMix<MIX> mx, CeAdj<ADJ> aj) {
  const int V = (ld % 8 == 0) ? 8 : (ld % 4 == 0 ? 4 : 1);
  const int64_t total = (int64_t)B * (ld / V);
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 8192));
  const float onw = 1.f - eps, unif = eps / (float)NC;
#define CE_BWD(VV)                                                                               \
  hipLaunchKernelGGL((ce_bwd_kernel<VV, SMOOTH, MIX, ADJ>), dim3(blocks), dim3(256), 0, s,       \
                     logits, labels, lse, grad_out, B, NC, ld, dlogits, weight, onw, unif, aj, mx)
  if (V == 8) CE_BWD(8);
  else if (V == 4) CE_BWD(4);
  else CE_BWD(1);
#undef CE_BWD
}

template <bool SMOOTH, bool MIX>
static void ce_bwd_a(const bf16_raw* logits, const int64_t* labels, const float* lse,
                     const float* grad_out, int B, int NC, int ld, bf16_raw* dlogits,
                     hipStream_t s, float weight, float eps, CeMix<MIX> mx, const float* bias) {
  if (bias)
    ce_bwd_t<SMOOTH, MIX, true>(logits, labels, lse, grad_out, B, NC, ld, dlogits, s, weight,
                                eps, mx, CeAdj<true>{bias});
  else
    ce_bwd_t<SMOOTH, MIX, false>(logits, labels, lse, grad_out, B, NC, ld, dlogits, s, weight,
                                 eps, mx, CeAdj<false>{});
}

void ce_bwd(const bf16_raw* logits, const int64_t* labels, const float* lse,
            const float* grad_out, int B, int NC, int ld, bf16_raw* dlogits, hipStream_t s,
            float weight, float smoothing, const int64_t* labels2, const float* lam,
            const float* bias) {
  if (labels2) {
    const CeMix<true> mx{labels2, lam};
    if (smoothing != 0.f)
      ce_bwd_a<true, true>(logits, labels, lse, grad_out, B, NC, ld, dlogits, s, weight,
                           smoothing, mx, bias);
    else
      ce_bwd_a<false, true>(logits, labels, lse, grad_out, B, NC, ld, dlogits, s, weight, 0.f,
                            mx, bias);
    return;
  }
  if (smoothing != 0.f)
    ce_bwd_a<true, false>(logits, labels, lse, grad_out, B, NC, ld, dlogits, s, weight,
                          smoothing, CeMix<false>{}, bias);
  else
    ce_bwd_a<false, false>(logits, labels, lse, grad_out, B, NC, ld, dlogits, s, weight, 0.f,
                           CeMix<false>{}, bias);
}

void argmax_correct(const bf16_raw* logits, const int64_t* labels, int B, int NC, int ld,
                    int64_t* count, hipStream_t s) {
  hipLaunchKernelGGL(argmax_kernel, dim3(B), dim3(256), 0, s, logits, labels, NC, ld,
                     (unsigned long long*)count);
}

void argmax_stats(const bf16_raw* logits, const int64_t* labels, int B, int NC, int ld,
                  int64_t* count, int64_t* stats, hipStream_t s) {
  hipLaunchKernelGGL(argmax_stats_kernel, dim3(B), dim3(256), 0, s, logits, labels, NC, ld,
                     (unsigned long long*)count, (unsigned long long*)stats);
}

// count += #{rows whose label is among the k largest logits} (ties to the lower index)
void topk_correct(const bf16_raw* logits, const int64_t* labels, int B, int NC, int ld, int k,
                  int64_t* count, hipStream_t s) {
  if (ld % 8 == 0 && ld >= NC && reinterpret_cast<uintptr_t>(logits) % 16 == 0)
    hipLaunchKernelGGL((topk_kernel<true, 4>), dim3(B), dim3(256), 0, s, logits, labels, NC, ld,
                       k, (unsigned long long*)count);
  else
    hipLaunchKernelGGL((topk_kernel<false, 1>), dim3(B), dim3(256), 0, s, logits, labels, NC, ld,
                       k, (unsigned long long*)count);
}

template <int K>
static void topk_predict_k(const bf16_raw* logits, int B, int NC, int ld, int k, int* idx,
                           float* prob, hipStream_t s) {
  if (ld % 8 == 0 && ld >= NC && reinterpret_cast<uintptr_t>(logits) % 16 == 0)
    hipLaunchKernelGGL((topk_predict_kernel<K, true, 4>), dim3(B), dim3(256), 0, s, logits, NC,
                       ld, k, idx, prob);
  else
    hipLaunchKernelGGL((topk_predict_kernel<K, false, 1>), dim3(B), dim3(256), 0, s, logits, NC,
                       ld, k, idx, prob);
}

// idx int32 [B][k], prob fp32 [B][k], 1 <= k <= 16: the lanes' lists hold the next
// instantiated size (1, 5, 8 or 16)
void topk_predict(const bf16_raw* logits, int B, int NC, int ld, int k, int* idx, float* prob,
                  hipStream_t s) {
  if (B <= 0) return;
  if (k <= 1) topk_predict_k<1>(logits, B, NC, ld, k, idx, prob, s);
  else if (k <= 5) topk_predict_k<5>(logits, B, NC, ld, k, idx, prob, s);
  else if (k <= 8) topk_predict_k<8>(logits, B, NC, ld, k, idx, prob, s);
  else topk_predict_k<16>(logits, B, NC, ld, k, idx, prob, s);
}

}  // namespace mpa
