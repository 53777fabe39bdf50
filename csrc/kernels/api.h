// Host-side launcher API of the gfx950 kernel library.  Plain pointers + POD argument
// structs, no torch headers: the .hip translation units compile in seconds and the
// torch-facing binding layer (csrc/bindings.cpp) validates shapes and allocates.
#pragma once
#include <algorithm>
#include <string>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "igemm_args.h"

namespace mpa {

struct HaloLaunch;   // halo_plan.h (included by the two files that plan: conv_halo.hip, igemm.hip)
struct HaloWLaunch;

// igemm.hip
int64_t igemm_slab_floats(int M, int N);
void igemm_rows(IGemmArgs a, int vw, float* ws, float* slab, hipStream_t s);  // B K-contig
// dgrad GEMMs: B N-contiguous (the forward weight, read with transposing LDS loads) or,
// with bkc, K-contiguous (the transposed weight copy; set a.b_tapmap)
void igemm_rows_dgrad(IGemmArgs a, int vw, float* ws, hipStream_t s, bool bkc = false);
// all stride phases of a strided-conv dgrad (a.nphase, a.ph[], shared a.taps) in one launch
// on the LDS-DMA engine when eligible, else one igemm_rows_dgrad per phase
void igemm_rows_dgrad_phases(IGemmArgs a, int vw, hipStream_t s, bool bkc = false);
// whether a merged-phase dgrad with a second source (a.A2) runs on the kernel that reads it
bool igemm_dgrad_src2_ok(const IGemmArgs& a, int vw, bool bkc);
// dgrad with the fused BN-backward reduction (a.ep_* set): sums[2][N] receives
// (sum g, sum g * xhat); slab holds igemm_bnred_slab_floats(a) floats
int64_t igemm_bnred_slab_floats(int M, int N, int nphase);
void igemm_rows_dgrad_bnred(IGemmArgs a, int vw, bool bkc, float* slab, float* sums,
                            hipStream_t s);
void igemm_wgrad(WGradArgs a, int vwa, int vwb, hipStream_t s);
int64_t igemm_ws_floats(int M, int N, int Ktot);          // split-K partials (0: no split)
int64_t igemm_wgrad_ws_floats(int Kout, int Ncols, int Mpix);  // wgrad split slab (0: none)
int igemm_engine();  // 0 register staging, 1 LDS-DMA rows GEMMs (default), 2 LDS-DMA all
void igemm_set_engine(int engine);
void igemm_force_tile(int bm, int bn, int splits);  // measurement override (0: auto)
// tile autotuner (igemm.hip): on by default (MPA_TUNE=0 off); the cached choices as text
void igemm_set_tune(int on);
void igemm_set_tune_drain(int on);  // tuner drains the device (1) or its stream (0)
std::string igemm_tuned_table();
// adopt a table in igemm_tuned_table()'s format (replace: drop the current entries first)
int igemm_tuned_load(const std::string& table, bool replace);
void igemm_set_dma_uni(int on);  // LDS-DMA uniform-tap fast path (default on)
bool igemm_stap_ok();  // super-tap forward available (engine >= 1 and fast path on)
// conv_halo.hip: halo-staged direct 3x3 / stride-1 conv (forward and stride-1 dgrad with
// a K-contiguous B).  conv3_halo_plan is plan_halo (halo_plan.h) under the process's
// switches and active_cus(); run_rows / the fused-reduction dgrad plan once and, unless the
// plan's kind is None, launch it: conv3_halo returns the statistics-slab rows written
// (<= HALO_MAX_ROWS).  conv3_halo_ok: the plan's kind is not None.
HaloLaunch conv3_halo_plan(const IGemmArgs& a);
bool conv3_halo_ok(const IGemmArgs& a);
int conv3_halo(IGemmArgs a, const HaloLaunch& plan, hipStream_t s);
void igemm_set_halo(int on);                 // MPA_HALO=0 disables (A/B, bitwise tests)
void igemm_set_halo_mi7(int on);     // MPA_HALO_MI7 (448-pixel resident-weight tiles)
void igemm_set_halo_strip(int mode);  // MPA_HALO_STRIP (0 off, 1 wide images, 2 + layer1 3-stage)
// halo-staged pixel-pair stem weight gradient (conv_stem.hip): partials into a.slab
// ([Z][64][224], <= stem_wgrad_ws_floats()); returns Z
bool stem_wgrad_ok(const WGradArgs& a);
int stem_wgrad(WGradArgs a, hipStream_t s);
int64_t stem_wgrad_ws_floats();
// the same weight gradient with the stem's BN + ReLU + 3x3/s2/p1 max-pool backward formed in
// its operand staging (a.dy = the conv output z; dz is never written): partials into a.slab
struct StemPoolArgs {
  const bf16_raw* dp;    // pooled gradient [N][PP][PQ][64]
  const uint8_t* idx;    // window argmax tap (3 i + k) [N][PP][PQ][64]
  const float *mean, *rstd, *gamma, *beta;
  const float* sums;     // [2][64]: sum g, sum g xhat over the batch (maxpool_bn_bwd_sums)
  int PP, PQ;            // pooled extent (P / 2, Q / 2)
  float invM;            // set by stem_pool_wgrad
};
bool stem_pool_wgrad_ok(const WGradArgs& a, const StemPoolArgs& q);
int stem_pool_wgrad(WGradArgs a, StemPoolArgs q, hipStream_t s);
// stem_pool_wgrad + the slab reduction into a.dw
void igemm_stem_pool_wgrad(WGradArgs a, StemPoolArgs q, hipStream_t s);
// halo-staged 3x3/s1 weight gradient (plan_halo_wgrad; None without a.slab): partials into
// a.slab ([Z][Kout][9C]); returns Z
HaloWLaunch conv3_halo_wgrad_plan(const WGradArgs& a);
bool conv3_halo_wgrad_ok(const WGradArgs& a);
int conv3_halo_wgrad(const WGradArgs& a, const HaloWLaunch& plan, hipStream_t s);
void igemm_set_halo_wxmap(int on);  // XCD-grouped halo weight-gradient blocks (MPA_HALO_WXMAP)
void igemm_set_halo_wprod(int on);  // producer-wave halo weight gradients (MPA_HALO_WPROD)
// Geometry-sized halo fetch of the linear-tile 3x3 kernels (default on; A/B and tests), and
// the planned halo DMA instructions per wave for H x W images: 256-pixel forward / dgrad
// tiles (of 9), 4-wave 128-pixel weight-gradient tiles (per chunk, of 7)
void igemm_set_halo_trim(int on);
int conv3_halo_dma_count(int H, int W);
int conv3_halo_wgrad_dma_count(int H, int W);
int64_t conv3_halo_wgrad_ws_floats(int Kout, int Ncols);
bool igemm_halo_enabled();
// Comm-aware persistent grids (conv_halo.hip).  While a data-parallel collective overlaps
// backward, its CTAs hold CUs that a persistent conv block (146-150 KB of LDS) cannot
// share; a block whose static tile share is queued behind one starts late and stretches
// the whole kernel.  The bucketer reserves the collective's CTA count while a bucket is in
// flight, and the persistent launches (halo fwd/dgrad and wgrad, stem fwd and wgrad) size
// their grids to the CUs left: active_cus() = CU count - reserve, a multiple of 8 (XCDs).
void set_comm_reserve(int cus);
int comm_reserve();
int active_cus();
// conv_stem.hip: direct row-staged forward of the 7x7 pixel-pair stem (super-tap layout,
// 64 output channels); run_rows takes it when conv_stem_ok.  Returns the slab rows written.
bool conv_stem_ok(const IGemmArgs& a);
int conv_stem(IGemmArgs a, hipStream_t s);
void igemm_set_stem(int on);  // MPA_STEM_DIRECT=0 disables (A/B, tests)

// bn.hip  (x/y/res/dy/dx: [M][C] bf16 rows; per-channel fp32 vectors)
// ws: float workspace of bn_ws_floats(M, C) elements (per-block partial-sum slab)
int64_t bn_ws_floats(int M, int C);
void slab_reduce(const float* slab, int S, int W, float* out, bool zero_out, hipStream_t s);
// deferred BN-backward corrections of a dense block (bn.hip, bn_defer_step_kernel); the host
// guarantees (Ci - s0) % 8 == 0 and 256 % ((Ci - s0) / 8) == 0
// DenseNet norm1 -> conv1 dgrad hand-off kernel (dense_gacc.hip)
bool dense_gacc_ok(const IGemmArgs& a);
void dense_gacc(IGemmArgs a, float* slab, float* sums, hipStream_t s);
void bn_defer_step(const float* sums, const float* gamma, const float* mean, const float* rstd,
                   int Ci, int s0, int M, float* k12, int ldk, float* dgamma, float* dbeta,
                   void* G, bool g_f32, int ldg, const bf16_raw* x, int ldx, bf16_raw* out,
                   hipStream_t s);
// MPA_DETERMINISTIC: fixed-order cross-block reductions, no timing-based tile autotuning
void set_deterministic(int on);
bool deterministic();
// sums [2][C] of (x - shift) and (x - shift)^2 over M rows -> out [mean(C), var(C)]
// slab [S][2C] of shifted (sum, sumsq) rows -> sums [2C] and out [mean(C), var(C)] (the
// slab may be folded in place); replaces slab_reduce + stats_finalize
void slab_stats(float* slab, int S, int C, const float* shift, int M, float* sums, float* out,
                hipStream_t s, int out_ld = 0);
void stats_finalize(const float* sums, const float* shift, int M, int C, float* out,
                    hipStream_t s);
void bn_stats(const bf16_raw* x, int M, int C, const float* shift, float* stats, float* ws,
              hipStream_t s);
void bn_fwd_train(const bf16_raw* x, const float* stats, const float* gamma, const float* beta,
                  float* rmean, float* rvar, float momentum, float eps, const bf16_raw* res,
                  int relu, int M, int C, bf16_raw* y, float* mean, float* rstd,
                  int64_t* counter, hipStream_t s,  // counter (num_batches_tracked) += 1
                  uint8_t* ymask = nullptr,  // optional ReLU bit mask of y ([M*C/8] bytes)
                  int ldx = 0,   // x row stride (0: C) - a channel prefix of a wider buffer
                  int lds = 0,   // stats = [mean | var] rows lds apart (0: C)
                  const float* res_aff = nullptr,  // [2][C]: res enters as res * aff0 + aff1
                  int ldy = 0);  // y row stride (0: C) - a channel window of a wider buffer
// mean / rstd / running stats / num_batches_tracked of a train-mode BN whose apply pass is
// deferred to its consumer; aff [2][C] = [gamma rstd | beta - mean gamma rstd]
void bn_stats_affine(const float* stats, const float* gamma, const float* beta, float* rmean,
                     float* rvar, float momentum, float eps, int M, int C, float* mean,
                     float* rstd, float* aff, int64_t* counter, hipStream_t s);
// avgpool2x2/s2(relu(z * aff0 + aff1)) without writing the BN output (H, W even, C % 8 == 0)
void bn_relu_avgpool2_fwd(const bf16_raw* z, const float* aff, int N, int H, int W, int C,
                          bf16_raw* y, hipStream_t s);
// y = relu?(x * aff[c] + aff[C + c]) (aff [2][C]: bn_stats_affine's scale | shift)
void affine_act(const bf16_raw* x, const float* aff, int relu, int M, int C, bf16_raw* y,
                hipStream_t s);
void bn_fwd_eval(const bf16_raw* x, const float* gamma, const float* beta, const float* rmean,
                 const float* rvar, float eps, const bf16_raw* res, int relu, int M, int C,
                 bf16_raw* y, hipStream_t s, int ldx = 0);
// zmask_beta (y == null): the ReLU mask of y = relu(bn(x)) is recomputed from x with this
// beta (no residual in the forward), so y is never read
void bn_bwd(const bf16_raw* dy, const bf16_raw* x, const bf16_raw* y, const float* mean,
            const float* rstd, const float* gamma, float* dgamma, float* dbeta, int M, int C,
            bf16_raw* dx, bf16_raw* g, float* ws, hipStream_t s,
            const float* zmask_beta = nullptr,
            const uint8_t* ymask = nullptr,  // bit mask from bn_fwd_train, used instead of y
            int ldx = 0,             // x row stride (0: C)
            float* gacc = nullptr,   // non-null: dx ADDED in fp32 into gacc [M][ldg] (dx unused)
            int ldg = 0,
            int lddx = 0,            // dx row stride (0: C) - a channel window of a wider buffer
            bool gacc_bf16 = false,  // gacc holds bf16 (cast the pointer) instead of fp32
            int lddy = 0);           // dy row stride (0: C) - a channel window of a wider buffer
// backward of relu(bn(x) + bn2(x2)), both train-mode BNs (bn2: a deferred downsample BN
// applied on read): dx and dx2 from one reduce and one apply pass, mask = the forward's bit
// mask; ws holds bn_pair_ws_floats(M, C) floats
// 2x2 / stride-2 / pad-0 max pool over an even image (VGG): one pooled pixel x 8 channels
// per thread; backward with yp + sums: the pooled tensor is a ReLU output whose producer's
// mask and bias-gradient sum are applied / reduced here (sums [C]; ws maxpool2_ws_floats)
bool maxpool2_ok(int N, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw);
void maxpool2_fwd(const bf16_raw* x, int N, int H, int W, int C, bf16_raw* y, uint8_t* idx,
                  hipStream_t s);
int64_t maxpool2_ws_floats(int N, int H, int W, int C);
void maxpool2_bwd(const bf16_raw* dy, const uint8_t* idx, const bf16_raw* yp, int N, int H, int W,
                  int C, bf16_raw* dx, float* sums, float* ws, hipStream_t s);
int64_t bn_pair_ws_floats(int M, int C);
void bn_bwd_pair(const bf16_raw* dy, const bf16_raw* x, const bf16_raw* x2, const uint8_t* ymask,
                 const float* mean, const float* rstd, const float* gamma, const float* mean2,
                 const float* rstd2, const float* gamma2, float* dgamma, float* dbeta,
                 float* dgamma2, float* dbeta2, int M, int C, bf16_raw* dx, bf16_raw* dx2,
                 float* ws, hipStream_t s);
void bn_bwd_apply(const bf16_raw* dy, const bf16_raw* x, const bf16_raw* y, const float* mean,
                  const float* rstd, const float* gamma, float* dgamma, float* dbeta, int M,
                  int C, bf16_raw* dx, bf16_raw* g, const float* sums, hipStream_t s,
                  int lddy = 0);
void act_bwd(const bf16_raw* dy, const bf16_raw* y, float* dbias, int M, int C, bf16_raw* g,
             float* ws, hipStream_t s);
void relu_fwd(const bf16_raw* x, int64_t n, bf16_raw* y, hipStream_t s);
// fused BN(train) + ReLU + max-pool (stems): z [N][H][W][C] -> y [N][P][Q][C] + argmax idx;
// backward: dp, idx, z -> dz (BN backward of the ReLU(BN) through the pool), ws of
// maxpool_bn_ws_floats(N*H*W, C) floats; C % 8 == 0.  zsel (optional, [N][P][Q][C]): the raw
// z at each window's argmax, written by the forward; with it the backward's reduction pass
// reads only pooled-size tensors
void bn_relu_maxpool_fwd(const bf16_raw* z, const float* stats, const float* gamma,
                         const float* beta, float* rmean, float* rvar, float momentum, float eps,
                         int N, int H, int W, int C, int P, int Q, int kh, int kw, int sh, int sw,
                         int ph, int pw, bf16_raw* y, uint8_t* idx, float* mean, float* rstd,
                         int64_t* counter, hipStream_t s, bf16_raw* zsel = nullptr);
int64_t maxpool_bn_ws_floats(int M, int C);
// pooled-only backward reduction of the fused stem: sums (ws[0 .. 2C)) and dgamma / dbeta
void maxpool_bn_bwd_sums(const bf16_raw* dp, const bf16_raw* zsel, const float* mean,
                         const float* rstd, const float* gamma, const float* beta, float* dgamma,
                         float* dbeta, int MP, int C, float* ws, hipStream_t s);
void maxpool_bn_bwd(const bf16_raw* dp, const uint8_t* idx, const bf16_raw* z, const float* mean,
                    const float* rstd, const float* gamma, const float* beta, float* dgamma,
                    float* dbeta, int N, int H, int W, int C, int P, int Q, int kh, int kw, int sh,
                    int sw, int ph, int pw, bf16_raw* dz, float* ws, hipStream_t s,
                    const bf16_raw* zsel = nullptr);

// pool.hip  (NHWC)
void maxpool_fwd(const bf16_raw* x, int N, int H, int W, int C, int P, int Q, int kh, int kw,
                 int sh, int sw, int ph, int pw, bf16_raw* y, uint8_t* idx, hipStream_t s);
void maxpool_bwd(const bf16_raw* dy, const uint8_t* idx, int N, int H, int W, int C, int P,
                 int Q, int kh, int kw, int sh, int sw, int ph, int pw, bf16_raw* dx,
                 hipStream_t s);
// ldx / ldo: pixel stride of x / dx (0: C) - a channel window of a wider NHWC buffer
void avgpool_fwd(const bf16_raw* x, int N, int H, int W, int C, int P, int Q, int kh, int kw,
                 int sh, int sw, int ph, int pw, int count_include_pad, bf16_raw* y,
                 hipStream_t s, int ldx = 0);
void avgpool_bwd(const bf16_raw* dy, int N, int H, int W, int C, int P, int Q, int kh, int kw,
                 int sh, int sw, int ph, int pw, int count_include_pad, bf16_raw* dx,
                 hipStream_t s, int ldo = 0);
void adaptive_avgpool_fwd(const bf16_raw* x, int N, int H, int W, int C, int P, int Q,
                          bf16_raw* y, hipStream_t s);
void adaptive_avgpool_bwd(const bf16_raw* dy, int N, int H, int W, int C, int P, int Q,
                          bf16_raw* dx, hipStream_t s);

// concat.hip (NHWC channel concat / split; every segment's channels % 8 == 0)
constexpr int CAT_MAXSEG = 32;
// fp32 gradient buffer G [pixels][ldg]: G[:, off:off+cs] (+)= src (bf16 [pixels][cs]) /
// dst = bf16(G[:, off:off+cs]); ldg, off, cs multiples of 8
void chan_accum(float* g, int ldg, int off, const bf16_raw* src, int cs, int pixels, bool assign,
                hipStream_t s);
void chan_extract(const float* g, int ldg, int off, bf16_raw* dst, int cs, int pixels,
                  hipStream_t s);
void concat_channels(const bf16_raw* const* xs, const int* chans, int nseg, int pixels,
                     int ctotal, bf16_raw* y, hipStream_t s);
// dst [rows][ld] (16-bit units) at unit offset off <- src [rows][cs]; ld, off, cs % 8 == 0
// (bf16 activations, or fp32 rows as pairs of units)
void chan_insert(bf16_raw* dst, int ld, int off, const bf16_raw* src, int cs, int rows,
                 hipStream_t s);
// dst [rows][cs] <- src [rows][ld] at unit offset off (the inverse of chan_insert)
void chan_slice(const bf16_raw* src, int ld, int off, bf16_raw* dst, int cs, int rows,
                hipStream_t s);
void split_channels(const bf16_raw* dy, const int* chans, int nseg, int pixels, int ctotal,
                    bf16_raw* const* dxs, hipStream_t s);

// loss.hip
// logits rows have stride ld >= NC (padded heads); ce_bwd writes dlogits with stride ld and
// zeros in columns NC..ld-1.  smoothing: torch's label_smoothing in [0, 1]; 0 runs the plain
// kernels.  labels2 + lam (optional device arrays [B], both or neither): row r's target is
// lam[r] * onehot(labels[r]) + (1 - lam[r]) * onehot(labels2[r]) before smoothing (Mixup /
// CutMix); null runs the one-label kernels.  bias (optional device array, fp32 [NC], 16-B
// aligned): logit adjustment - the loss is CE of float(logits) + bias, the saved lse is that
// sum's; only bias[0:NC) is read; null runs the unadjusted kernels.
void ce_fwd_rows(const bf16_raw* logits, const int64_t* labels, int B, int NC, int ld, float* row_loss,
                 float* lse, hipStream_t s, float smoothing = 0.f,
                 const int64_t* labels2 = nullptr, const float* lam = nullptr,
                 const float* bias = nullptr);
// loss: [1 + B] floats (mean at [0], per-row terms after it; fixed-order sum)
void ce_fwd(const bf16_raw* logits, const int64_t* labels, int B, int NC, int ld, float* loss,
            float* lse, hipStream_t s, float smoothing = 0.f, const int64_t* labels2 = nullptr,
            const float* lam = nullptr, const float* bias = nullptr);
void ce_bwd(const bf16_raw* logits, const int64_t* labels, const float* lse,
            const float* grad_out, int B, int NC, int ld, bf16_raw* dlogits, hipStream_t s,
            float weight = 1.f, float smoothing = 0.f, const int64_t* labels2 = nullptr,
            const float* lam = nullptr, const float* bias = nullptr);
void ce_fwd_weighted(const bf16_raw* logits, const int64_t* labels, int B, int NC, int ld,
                     float* out, float* acc, float weight, bool accumulate, float* rows,
                     float* lse, hipStream_t s, float smoothing = 0.f,
                     const int64_t* labels2 = nullptr, const float* lam = nullptr,
                     const float* bias = nullptr);
// fp32 t[0:n) = 0 (n % 4 == 0, 16-B aligned); step[0] += 1
void zero_f32(float* t, int64_t n, hipStream_t s);
void add_f32(float* dst, const float* src, int64_t n, hipStream_t s);  // dst += src
// t as [rows][period] fp32: zero columns [first, first + count)
void zero_cols_f32(float* t, int64_t rows, int period, int first, int count, hipStream_t s);
// a += b, bf16 [n] (n % 8 == 0, 16-B aligned)
void add_bf16(bf16_raw* a, const bf16_raw* b, int64_t n, hipStream_t s);
void step_inc(float* step, hipStream_t s);
void argmax_correct(const bf16_raw* logits, const int64_t* labels, int B, int NC, int ld,
                    int64_t* count, hipStream_t s);
// argmax_correct's count, and per-class counters stats int64 [3][NC]: for every row with a
// label in [0, NC), stats[0][label] += 1 (support), stats[1][pred] += 1 (predicted; an all-NaN
// row predicts nothing) and stats[2][label] += 1 when pred == label (true positives)
void argmax_stats(const bf16_raw* logits, const int64_t* labels, int B, int NC, int ld,
                  int64_t* count, int64_t* stats, hipStream_t s);
// count += #{rows whose label is among the k largest logits}; ties go to the lower index
// (k = 1 is argmax_correct); out-of-range labels and NaN label logits are not counted
void topk_correct(const bf16_raw* logits, const int64_t* labels, int B, int NC, int ld, int k,
                  int64_t* count, hipStream_t s);
// idx int32 [B][k] / prob fp32 [B][k], 1 <= k <= 16: the row's k best classes in topk_correct's
// order (x[c] > x[d], or equal and c < d) and their softmax probabilities; NaN and -inf logits
// are no candidates, and slots past the last candidate get idx = -1, prob = 0.  No atomics: a
// row's outputs depend on that row alone
void topk_predict(const bf16_raw* logits, int B, int NC, int ld, int k, int* idx, float* prob,
                  hipStream_t s);

// optim.hip (flat fp32 arenas)
void adam_step(float* p, const float* g, float* m, float* v, bf16_raw* shadow,
               const float* step, int64_t n, float lr, float b1, float b2, float eps, float wd,
               float grad_scale, hipStream_t s);
void sgd_step(float* p, const float* g, float* buf, bf16_raw* shadow, const float* step,
              int64_t n, float lr, float momentum, float dampening, float wd, int nesterov,
              float grad_scale, hipStream_t s);
// Per-step training recipe on the device (LR schedule + global-norm gradient clipping).
// hyper[HYPER_N] fp32: the record hyper_update writes and the *_step_dev kernels read.
enum { HYPER_LR = 0, HYPER_SCALE = 1, HYPER_NORM = 2, HYPER_COEF = 3, HYPER_SKIP = 4,
       HYPER_NONFINITE = 5, HYPER_SUMSQ = 6, HYPER_N = 8 };
enum { HYPER_CONSTANT = 0, HYPER_COSINE = 1, HYPER_STEP = 2 };
struct HyperCfg {
  int kind;           // HYPER_CONSTANT | HYPER_COSINE | HYPER_STEP
  float base_lr;
  float warmup;       // W: lr = base * (k + 1) / W while k < W
  float total;        // T (cosine)
  float min_ratio;    // r (cosine floor)
  float gamma;        // step: base * gamma ^ floor(k / decay_steps)
  float decay_steps;  // > 0 when kind == HYPER_STEP
  float max_norm;     // clipping threshold (used when nparts > 0)
  float grad_scale;   // the data-parallel 1/N
};
// sum of squares of g[0:n) (n % 4 == 0, 16-B aligned), stage 1: one partial per block into
// part[0:returned count) (count <= grad_sqnorm_grid_cap()); fixed order, no atomics
int grad_sqnorm(const float* g, int64_t n, float* part, hipStream_t s);
int grad_sqnorm_grid_cap();
int64_t grad_sqnorm_sweep();  // elements one full-grid round of stage 1 covers
// stage 2 on its own: out[0] = fixed-order sum of part[0:nparts) (one block)
void grad_sqnorm_sum(const float* part, int nparts, float* out, hipStream_t s);
// stage 2 fused with the schedule / clip arithmetic: k = step[0]; nparts == 0: no clipping
void hyper_update(const float* step, const float* part, int nparts, float* hyper,
                  const HyperCfg& cfg, hipStream_t s);
// adam_step / sgd_step with lr and the gradient scale read from hyper (no-op when
// hyper[HYPER_SKIP] != 0)
void adam_step_dev(float* p, const float* g, float* m, float* v, bf16_raw* shadow,
                   const float* step, const float* hyper, int64_t n, float b1, float b2,
                   float eps, float wd, hipStream_t s);
void sgd_step_dev(float* p, const float* g, float* buf, bf16_raw* shadow, const float* step,
                  const float* hyper, int64_t n, float momentum, float dampening, float wd,
                  int nesterov, hipStream_t s);
// Layer-wise optimizers (AdamW / LAMB / LARS) on a segment plan over the arena.
// seg [nseg][SEG_COLS] int64: parameter s's aligned slice, its chunks and its flags;
// chunk_seg [nchunks] int32: the segment of each chunk (a segment's chunks are consecutive,
// each at most seg_chunk() elements).  n: elements of the arena-shaped buffers; a plan
// entry outside [0, n) is not followed.  All read lr / gradient scale / skip flag from
// hyper and write nothing when hyper[HYPER_SKIP] != 0; no float atomics.
enum { SEG_OFF = 0, SEG_LEN = 1, SEG_FIRST = 2, SEG_NCHUNK = 3, SEG_FLAGS = 4, SEG_COLS = 5 };
enum { SEG_DECAY = 1, SEG_ADAPT = 2 };     // flag bits
enum { TRUST_LAMB = 0, TRUST_LARS = 1 };  // trust_ratio modes
int seg_chunk();
// part[c] = sum over chunk c of (x * (scaled ? hyper[HYPER_SCALE] : 1))^2
void seg_sqnorm(const float* x, int64_t n, const int64_t* seg, const int* chunk_seg, int nseg,
                int nchunks, const float* hyper, int scaled, float* part, hipStream_t s);
// LAMB stage 1: per chunk sum p^2 and sum u^2, u = m^ / (sqrt(v^) + eps) + wd_s * p from the
// moments the step would produce; p, g, m, v are only read
void lamb_norms(const float* p, const float* g, const float* m, const float* v, int64_t n,
                const float* step, const float* hyper, const int64_t* seg, const int* chunk_seg,
                int nseg, int nchunks, float* part_p, float* part_u, float b1, float b2,
                float eps, float wd, hipStream_t s);
// per segment: fixed-order sums of its partials -> norms[s] = (|p|, |b|) and ratio[s]
// (TRUST_LAMB: |p| / |b|; TRUST_LARS: trust_coef * |p| / (|b| + wd_s * |p| + 1e-8); 1 when
// the segment is not SEG_ADAPT or a norm is 0)
void trust_ratio(const int64_t* seg, int nseg, int nchunks, const float* part_p,
                 const float* part_b, const float* hyper, int mode, float trust_coef, float wd,
                 float* ratio, float* norms, hipStream_t s);
// LAMB stage 2: p -= lr * ratio[s] * u; adamw != 0: torch.optim.AdamW (p *= 1 - lr * wd_s,
// then the Adam step; ratio is not read).  wd_s = wd on SEG_DECAY segments, else 0.
void lamb_step_dev(float* p, const float* g, float* m, float* v, bf16_raw* shadow, int64_t n,
                   const float* step, const float* hyper, const int64_t* seg,
                   const int* chunk_seg, int nseg, int nchunks, const float* ratio, float b1,
                   float b2, float eps, float wd, int adamw, hipStream_t s);
// LARS: g' = ratio[s] * (g^ + wd_s * p), then sgd_step's momentum rule with wd = 0
void lars_step_dev(float* p, const float* g, float* buf, bf16_raw* shadow, int64_t n,
                   const float* step, const float* hyper, const int64_t* seg,
                   const int* chunk_seg, int nseg, int nchunks, const float* ratio,
                   float momentum, float dampening, float wd, int nesterov, hipStream_t s);
// Weight EMA: ema[i] += w * (p[i] - ema[i]) for i in [0, n) (n % 4 == 0, 16-B aligned),
// w = 1 - d_t, d_t = warmup ? min(decay, (1 + t) / (10 + t)) : decay, t = step[0]; every
// operation rounded on its own in fp32.  Reads p, writes only ema[0:n).
void ema_update(float* ema, const float* p, const float* step, int64_t n, float decay,
                int warmup, hipStream_t s);
// The same update for nbuf small fp32 tensors in one launch.  table [nbuf][EMA_COLS] int64
// on the device = (source address, offset into ema_buf, length); sources need 4-byte
// alignment only; n: elements of ema_buf (a row outside it is not followed).
enum { EMA_SRC = 0, EMA_OFF = 1, EMA_LEN = 2, EMA_COLS = 3 };
void ema_update_multi(float* ema_buf, int64_t n, const int64_t* table, int nbuf,
                      const float* step, float decay, int warmup, hipStream_t s);
// wt[c][t][k] = w[k][t][c] per segment (src_off, dst_off, K, RS, C, first_tile) of seg
// step_inc (optional): the optimizer's step counter, incremented by the same launch
void transpose_krsc(const bf16_raw* w, bf16_raw* wt, const int64_t* seg, int nseg,
                    int total_tiles, hipStream_t s, float* step_inc = nullptr);

// preprocess.hip
struct Norm3 {
  float mean[3];
  float std[3];
};
// zero border around the resized image (pre-padded pixel-pair stem input); all 0 = none
struct OutPad {
  int top, bottom, left, right;
};
void preprocess_set_copy(int on);  // identity-size fast path on/off (tests, A/B)
// ext (optional): per-image source extents [B][2] = (h, w) inside the [H][W] pitch (mode 0)
// box (optional, mode 0 only): per-image crop boxes [B][5] = (y0, x0, h, w, flip) in source
// pixels of image b's slot; image b is resized from its box (which must lie inside its
// extent - the caller checks, the kernel does not) and mirrored along W when flip != 0
// mix + lam (optional, mode 0 only, both or neither, and then box is required - full-extent
// boxes when there is no crop): Mixup / CutMix.  mix [B][5] = (partner, y0, x0, h, w) - an
// image of the same batch and a rectangle in output pixels (inside [0, OH] x [0, OW]; h or
// w == 0: none) - and lam [B] in [0, 1]: the output is the partner's inside the rectangle
// and bf16(lam * own + (1 - lam) * partner's) outside it (trusted like the boxes)
void preprocess(const uint8_t* img, int B, int H, int W, int OH, int OW, Norm3 nrm, int mode,
                int cpad, OutPad pad, bf16_raw* out, hipStream_t s, const int* ext = nullptr,
                const int* box = nullptr, const int* mix = nullptr, const float* lam = nullptr);
// PIL-exact bicubic (eval transform): per-image extents ext [B][2] (h, w) inside the
// [Hp][Wp] pitch (nullptr: all full), per-image table selectors sel [B][2]; tmp holds
// B * Hp * OW RGBx words
void preprocess_pil(const uint8_t* img, int B, int Hp, int Wp, const int* ext, const int* sel,
                    const int* hb, const int* hk, int kh, const int* vb, const int* vk, int kv,
                    int OH, int OW, Norm3 nrm, int cpad, OutPad pd, uint32_t* tmp, bf16_raw* out,
                    hipStream_t s);
// counter (optional, device uint32): added to offset and incremented after the launch
void dropout_fwd(const bf16_raw* x, int64_t n, float p, uint64_t seed, uint64_t offset,
                 uint32_t* counter, bf16_raw* y, uint8_t* mask, hipStream_t s);
void dropout_bwd(const bf16_raw* dy, const uint8_t* mask, int64_t n, float p, bf16_raw* dx,
                 hipStream_t s);

// diag.hip: stand-in for a concurrent RCCL collective (bench.py --emulate-comm)
void comm_emulator(int blocks, int threads, int lds_bytes, double us, float* sink, hipStream_t s);
void atomic_latency(int blocks, int iters, int mode, int* q, hipStream_t s);  // diag.hip

}  // namespace mpa
