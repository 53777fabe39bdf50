// CPU check of the launch geometry conv_args.h derives from a layer's shape (conv_args.h and
// igemm_args.h are the only project headers included; any host C++17 compiler, no GPU
// toolchain).  Run by tests/test_conv_args_cpu.py, plain and under AddressSanitizer +
// UndefinedBehaviorSanitizer.
//
//   conv_args_check sweep        interprets the arguments of a grid of shapes (see for_cases)
//                                and compares with textbook convolutions, exactly
//   conv_args_check wgrad        the WGradArgs fields of the same shapes against their
//                                definitions
//   conv_args_check dump SHAPE.. one line per shape: every geometry field, taps and phases
//   conv_args_check exec SHAPE.. interprets and compares the given shapes
//
//   SHAPE  fwd:N,H,W,C,K,R,S,sh,sw,ph,pw,STAP         STAP 1: the 8-channel super-tap form
//          dgrad:N,H,W,C,K,R,S,sh,sw,ph,pw,WT         WT 1: from the transposed weight
//          pair:N,H,W,C,K,R,S,sh,sw,ph,pw,R2,S2,ph2,pw2   dgrad plus a second conv's, WT 1
//          pointwise:NIMG,H,W,Cin,Cout,ldb,TAPMAP     (dump only)
//          wgrad:N,H,W,C,K,R,S,sh,sw,ph,pw            (dump only)
//   x is [N, H, W, C], w [K, R, S, C]; dy's extent is the forward conv's.
//
// `exec` below is the meaning of IGemmArgs: what igemm_rows_kernel (igemm.hip) and the
// LDS-DMA kernels (igemm_dma.hip) compute, as nested loops with no tiling.  One point where
// the kernels read the arguments differently: with a K-contiguous B the uniform-tap LDS-DMA
// kernel addresses B by taps.bt[t] whether or not b_tapmap is set, the other kernels by t
// unless it is set.  Every builder emits bt[t] == t where b_tapmap is 0 and B is
// K-contiguous, so the readings agree on all launches; run_case requires just that.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "conv_args.h"

using namespace mpa;

#define REQUIRE(cond)          \
  do {                         \
    if (!(cond)) return #cond; \
  } while (0)

typedef std::vector<double> Vec;  // small integers: every sum is exact

// ------------------------------------------------------------------------ interpreter
struct Operands {
  const Vec* A;
  const Vec* B;
  const Vec* A2;  // second source (taps tagged TAP_SRC2 of a stride-phase launch), or null
  const Vec* B2;
  Vec* C;
  std::vector<int>* writes;  // per output pixel: how many launches / phases stored it
};

// bkc: B is K-contiguous (the launchers' argument of that name; always true forward).
// Null, or the first thing that is not as the kernels need it.
static const char* exec(const IGemmArgs& a, bool bkc, const Operands& o) {
  const int nlaunch = a.nphase > 0 ? a.nphase : 1;
  REQUIRE(a.nphase >= 0 && a.nphase <= MAXPH && !(a.stap && a.nphase));
  for (int l = 0; l < nlaunch; ++l) {
    const PhaseDesc d = a.nphase > 0 ? a.ph[l]
                                     : PhaseDesc{a.M, a.oH, a.oW, a.Ktot, 0, a.T, a.Poh, a.Pow, 0,
                                                 FastDiv{}, FastDiv{}};
    if (a.nphase == 0 && d.M == 0) continue;  // (a strided dgrad whose phases all lack taps)
    REQUIRE(d.tap0 >= 0 && d.T > 0 && d.tap0 + d.T <= MAXT);
    REQUIRE(d.Ktot == d.T * (a.stap ? 32 : a.aC));
    REQUIRE(d.oH > 0 && d.oW > 0 && d.M % (d.oH * d.oW) == 0);
    for (int m = 0; m < d.M; ++m) {
      const int img = m / (d.oH * d.oW), oh = m % (d.oH * d.oW) / d.oW, ow = m % d.oW;
      const int dh_ = d.Poh + a.Uoh * oh, dw_ = d.Pow + a.Uow * ow;
      REQUIRE(dh_ >= 0 && dh_ < a.dH && dw_ >= 0 && dw_ < a.dW);
      const size_t pix = ((size_t)img * a.dH + dh_) * a.dW + dw_;
      REQUIRE(pix < o.writes->size() && (pix + 1) * a.ldc <= o.C->size() && a.N <= a.ldc);
      ++(*o.writes)[pix];
      for (int n = 0; n < a.N; ++n) {
        double acc = 0;
        for (int t = 0; t < d.T; ++t) {
          const int e = d.tap0 + t, bt = a.taps.bt[e], wtap = bt & 0xfff;
          // bits 12..: the super-tap's column count (single launches), the source tag (phases)
          const bool src2 = a.nphase > 0 && (bt & TAP_SRC2);
          const int cols = a.stap ? bt >> 12 : 1;
          REQUIRE(bkc || !(a.stap || src2 || a.b_tapmap));
          REQUIRE(!src2 || (o.A2 && o.B2));
          const Vec& A = src2 ? *o.A2 : *o.A;
          const Vec& B = src2 ? *o.B2 : *o.B;
          for (int j = 0; j < cols; ++j) {
            const int ih = oh * a.Uh + a.Oh + a.taps.dh[e], iw = ow * a.Uw + a.Ow + a.taps.dw[e] + j;
            if (ih < 0 || ih >= a.aH || iw < 0 || iw >= a.aW) continue;  // reads zero
            for (int c = 0; c < a.aC; ++c) {
              const size_t ai = (((size_t)img * a.aH + ih) * a.aW + iw) * a.aC + c;
              const size_t bi = a.stap  ? (size_t)n * a.ldb + (size_t)(wtap + j) * a.aC + c
                                : src2  ? (size_t)n * a.ldb2 + (size_t)wtap * a.aC + c
                                : !bkc  ? ((size_t)c * a.RS + wtap) * a.ldb + n
                                : a.b_tapmap ? (size_t)n * a.ldb + (size_t)wtap * a.aC + c
                                             : (size_t)n * a.ldb + (size_t)t * a.aC + c;
              REQUIRE(ai < A.size() && bi < B.size());
              acc += A[ai] * B[bi];
            }
          }
        }
        double& out = (*o.C)[pix * a.ldc + n];
        out = a.beta ? out + acc : acc;
      }
    }
  }
  return nullptr;
}

// ------------------------------------------------------------------------ references
// y[n][p][q][k] = sum x[n][p * sh - ph + r][q * sw - pw + s][c] * w[k][r][s][c], zero padding
static Vec conv_ref(const ConvShape& q, int P, int Q, const Vec& x, const Vec& w) {
  Vec y((size_t)q.N * P * Q * q.K, 0.0);
  for (int n = 0; n < q.N; ++n)
    for (int p = 0; p < P; ++p)
      for (int qq = 0; qq < Q; ++qq)
        for (int k = 0; k < q.K; ++k)
          for (int r = 0; r < q.R; ++r)
            for (int s = 0; s < q.S; ++s) {
              const int h = p * q.sh - q.ph + r, v = qq * q.sw - q.pw + s;
              if (h < 0 || h >= q.H || v < 0 || v >= q.W) continue;
              for (int c = 0; c < q.C; ++c)
                y[(((size_t)n * P + p) * Q + qq) * q.K + k] +=
                    x[(((size_t)n * q.H + h) * q.W + v) * q.C + c] *
                    w[(((size_t)k * q.R + r) * q.S + s) * q.C + c];
            }
  return y;
}

// the transposed conv: dx += every dy element scattered through the taps it was made from
static void dgrad_ref(const ConvShape& q, int P, int Q, const Vec& dy, const Vec& w, Vec& dx) {
  for (int n = 0; n < q.N; ++n)
    for (int p = 0; p < P; ++p)
      for (int qq = 0; qq < Q; ++qq)
        for (int k = 0; k < q.K; ++k)
          for (int r = 0; r < q.R; ++r)
            for (int s = 0; s < q.S; ++s) {
              const int h = p * q.sh - q.ph + r, v = qq * q.sw - q.pw + s;
              if (h < 0 || h >= q.H || v < 0 || v >= q.W) continue;
              for (int c = 0; c < q.C; ++c)
                dx[(((size_t)n * q.H + h) * q.W + v) * q.C + c] +=
                    dy[(((size_t)n * P + p) * Q + qq) * q.K + k] *
                    w[(((size_t)k * q.R + r) * q.S + s) * q.C + c];
            }
}

// wt[c][r * S + s][k] = w[k][r][s][c]
static Vec transposed(const ConvShape& q, const Vec& w) {
  Vec wt(w.size());
  const int RS = q.R * q.S;
  for (int k = 0; k < q.K; ++k)
    for (int t = 0; t < RS; ++t)
      for (int c = 0; c < q.C; ++c) wt[((size_t)c * RS + t) * q.K + k] = w[((size_t)k * RS + t) * q.C + c];
  return wt;
}

// ------------------------------------------------------------------------ cases
// A fixed pseudo-random stream (an LCG): a case's batch, channel counts and data are drawn
// from it, so none is tied to a position in the loops.
struct Rng {
  uint32_t r = 12345u;
  int next(int n) { return (int)(((r = r * 1664525u + 1013904223u) >> 16) % (uint32_t)n); }
};

static Vec values(size_t n, Rng& g) {
  Vec v(n);
  for (double& x : v) x = g.next(7) - 3;
  return v;
}

enum Kind { FWD, DGRAD, PAIR, POINTWISE, WGRAD };
static const char* const KINDS[] = {"fwd", "dgrad", "pair", "pointwise", "wgrad"};

struct Case {
  Kind kind;
  ConvShape q;        // (POINTWISE: N, H, W, C = Cin, K = Cout; R = ldb, S = tapmap)
  bool flag;          // FWD: super-tap form; DGRAD / PAIR: from the transposed weight
  DgradSrc2Shape s2;  // PAIR
};

static int out_h(const ConvShape& q) { return conv_out_extent(q.H, q.R, q.sh, q.ph); }
static int out_w(const ConvShape& q) { return conv_out_extent(q.W, q.S, q.sw, q.pw); }

static const char* build(const Case& c, IGemmArgs& a, bool& any_empty) {
  any_empty = false;
  switch (c.kind) {
    case FWD: return conv_fwd_args(c.q, c.flag, a);
    case DGRAD: return conv_dgrad_args(c.q, out_h(c.q), out_w(c.q), c.flag, nullptr, a, any_empty);
    case PAIR: return conv_dgrad_args(c.q, out_h(c.q), out_w(c.q), c.flag, &c.s2, a, any_empty);
    default: a = pointwise_args(c.q.N, c.q.H, c.q.W, c.q.C, c.q.K, c.q.R, c.q.S != 0); return nullptr;
  }
}

static const int KERNELS[] = {1, 2, 3, 5, 7};

// f(case) over: H, W in 1..9 x R, S in KERNELS x strides 1..3, each per axis (stride >
// kernel: phases without taps) x row pad 0..3; the column pad 0..3, batch 1..2 and C, K in
// 1..3 drawn per geometry (the two axes' taps are built independently of each other).
// Per geometry: the forward conv (and, for one S > 1 geometry in four, the C == 8 forward in
// its plain and super-tap forms), the dgrad from w and from the transposed weight, and - for
// one strided geometry in four - the pair with every second conv of kernel 1..3, pad 0..1
// per axis whose output grid coincides (3x3/s2/p1 with 1x1/s2/p0 among them).  Geometries
// with an empty output are passed with kind FWD only: the callers count them as skipped.
template <class F>
static void for_cases(F&& f) {
  Rng g;
  for (int H = 1; H <= 9; ++H)
  for (int W = 1; W <= 9; ++W)
  for (int R : KERNELS)
  for (int S : KERNELS)
  for (int sh = 1; sh <= 3; ++sh)
  for (int sw = 1; sw <= 3; ++sw)
  for (int ph = 0; ph <= 3; ++ph) {
    const int pw = g.next(4);
    const ConvShape q{1 + g.next(2), H, W, 1 + g.next(3), 1 + g.next(3), R, S, sh, sw, ph, pw};
    const bool stem = g.next(4) == 0, pair = g.next(4) == 0;
    f(Case{FWD, q, false, {}});
    if (out_h(q) <= 0 || out_w(q) <= 0) continue;
    if (stem && S > 1) {
      ConvShape q8 = q;
      q8.C = 8;
      f(Case{FWD, q8, false, {}});
      f(Case{FWD, q8, true, {}});
    }
    f(Case{DGRAD, q, false, {}});
    f(Case{DGRAD, q, true, {}});
    if (!pair || (sh == 1 && sw == 1)) continue;
    for (int R2 = 1; R2 <= 3; ++R2)
    for (int S2 = 1; S2 <= 3; ++S2)
    for (int ph2 = 0; ph2 <= 1; ++ph2)
    for (int pw2 = 0; pw2 <= 1; ++pw2)
      if (conv_out_extent(H, R2, sh, ph2) == out_h(q) && conv_out_extent(W, S2, sw, pw2) == out_w(q))
        f(Case{PAIR, q, true, {R2, S2, ph2, pw2}});
  }
  // one tap: a linear layer's forward, its dgrad from [Cout][Cin] (N-contiguous B) and from
  // the transpose, and the image-grid form with the tap map set
  for (int n = 1; n <= 3; ++n)
  for (int ci = 1; ci <= 3; ++ci)
  for (int co = 1; co <= 3; ++co) {
    f(Case{POINTWISE, {n, 1, 1, ci, co, ci, 0, 1, 1, 0, 0}, true, {}});
    f(Case{POINTWISE, {n, 1, 1, co, ci, ci, 0, 1, 1, 0, 0}, false, {}});
    f(Case{POINTWISE, {n, 1, 1, co, ci, co, 0, 1, 1, 0, 0}, true, {}});
    f(Case{POINTWISE, {n, 2, 3, co, ci, co, 1, 1, 1, 0, 0}, true, {}});
  }
}

static std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
static std::string fmt(const char* f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

static std::string describe(const Case& c) {
  const ConvShape& q = c.q;
  if (c.kind == POINTWISE)
    return fmt("pointwise n%d %dx%d c%d k%d ldb%d tapmap%d", q.N, q.H, q.W, q.C, q.K, q.R, q.S);
  std::string s = fmt("%s n%d %dx%d c%d k%d %dx%d s%d,%d p%d,%d", KINDS[c.kind], q.N, q.H, q.W, q.C,
                      q.K, q.R, q.S, q.sh, q.sw, q.ph, q.pw);
  if (c.kind == FWD) s += fmt(" stap%d", c.flag);
  if (c.kind == DGRAD || c.kind == PAIR) s += fmt(" wt%d", c.flag);
  if (c.kind == PAIR) s += fmt(" + %dx%d p%d,%d", c.s2.R, c.s2.S, c.s2.ph, c.s2.pw);
  return s;
}

// ------------------------------------------------------------------------ one case
// does the stride phase of dx row / column y have a tap of an R-tap kernel with pad p?
static bool axis_has_tap(int y, int R, int stride, int p) {
  for (int r = 0; r < R; ++r)
    if ((y % stride + p - r) % stride == 0) return true;
  return false;
}

// builds the case's arguments, interprets them on drawn data and compares with the
// reference; accumulating (beta) or into a wider row stride by coin flip
static const char* run_case(const Case& c, Rng& g) {
  const ConvShape& q = c.q;
  IGemmArgs a;
  bool any_empty;
  REQUIRE(!build(c, a, any_empty));
  for (int i = 0; i < std::max(a.nphase, 1); ++i) {  // no index in taps reaches MAXT
    const int end = a.nphase ? a.ph[i].tap0 + a.ph[i].T : a.T;
    REQUIRE(end <= MAXT && (a.nphase == 0 || (a.ph[i].tap0 >= 0 && a.ph[i].T > 0)));
  }
  a.ldc = a.N + 3 * g.next(2);
  std::vector<int> writes;
  Vec C, want;
  if (c.kind == FWD || c.kind == POINTWISE) {
    const bool pt = c.kind == POINTWISE;
    const int P = pt ? q.H : out_h(q), Q = pt ? q.W : out_w(q);
    const ConvShape q1{q.N, q.H, q.W, q.C, q.K, 1, 1, 1, 1, 0, 0};
    const Vec x = values((size_t)q.N * q.H * q.W * q.C, g);
    const Vec w = values((size_t)q.K * (pt ? 1 : q.R * q.S) * q.C, g);
    // (POINTWISE, flag 0: B is the N-contiguous [Cin][Cout], w transposed)
    const Vec B = pt && !c.flag ? transposed(q1, w) : w;
    for (int t = 0; t < a.T && !a.stap && !a.b_tapmap; ++t) REQUIRE(a.taps.bt[t] == t);
    REQUIRE(a.M == q.N * P * Q && a.N == q.K && a.dH == P && a.dW == Q);
    want = conv_ref(pt ? q1 : q, P, Q, x, w);
    writes.assign((size_t)a.M, 0);
    C.assign((size_t)a.M * a.ldc, 777.0);
    const Operands o{&x, &B, nullptr, nullptr, &C, &writes};
    if (const char* bad = exec(a, pt ? c.flag : true, o)) return bad;
    for (int w_ : writes) REQUIRE(w_ == 1);
  } else {
    const int P = out_h(q), Q = out_w(q);
    const ConvShape q2{q.N, q.H, q.W, q.C, q.K, c.s2.R, c.s2.S, q.sh, q.sw, c.s2.ph, c.s2.pw};
    const bool two = c.kind == PAIR;
    const Vec dy = values((size_t)q.N * P * Q * q.K, g), w = values((size_t)q.K * q.R * q.S * q.C, g);
    const Vec dy2 = values(two ? dy.size() : 0, g);
    const Vec w2 = values(two ? (size_t)q.K * q2.R * q2.S * q.C : 0, g);
    const Vec B = c.flag ? transposed(q, w) : w, B2 = two ? transposed(q2, w2) : Vec();
    const size_t npix = (size_t)q.N * q.H * q.W;
    a.beta = g.next(2);
    REQUIRE(a.N == q.C && a.dH == q.H && a.dW == q.W);
    const Vec old = values(npix * q.C, g);
    want = a.beta ? old : Vec(npix * q.C, 0.0);
    dgrad_ref(q, P, Q, dy, w, want);
    if (two) dgrad_ref(q2, P, Q, dy2, w2, want);
    // dx as the binding hands it over: the accumulated-into tensor, or fresh memory that is
    // zeroed when a phase has no taps
    C.assign(npix * a.ldc, 777.0);
    for (size_t i = 0; i < npix; ++i)
      for (int n = 0; n < a.N; ++n)
        if (a.beta || any_empty) C[i * a.ldc + n] = a.beta ? old[i * q.C + n] : 0.0;
    writes.assign(npix, 0);
    const Operands o{&dy, &B, two ? &dy2 : nullptr, two ? &B2 : nullptr, &C, &writes};
    if (const char* bad = exec(a, c.flag, o)) return bad;
    // every dx pixel is stored by exactly one phase, or by none where its phase has no taps
    long covered = 0, rows = 0;
    bool saw_empty = false;
    for (size_t i = 0; i < npix; ++i) {
      const int y = (int)(i / q.W % q.H), x = (int)(i % q.W);
      const bool has = (axis_has_tap(y, q.R, q.sh, q.ph) && axis_has_tap(x, q.S, q.sw, q.pw)) ||
                       (two && axis_has_tap(y, q2.R, q.sh, q2.ph) && axis_has_tap(x, q2.S, q.sw, q2.pw));
      REQUIRE(writes[i] == (has ? 1 : 0));
      covered += has;
      saw_empty |= !has;
    }
    REQUIRE(saw_empty == any_empty);
    for (int i = 0; i < a.nphase; ++i) rows += a.ph[i].M;
    REQUIRE((a.nphase ? rows : a.M) == covered);
  }
  for (size_t i = 0; i < want.size() / a.N; ++i)
    for (int n = 0; n < a.ldc; ++n)
      REQUIRE(C[i * a.ldc + n] == (n < a.N ? want[i * a.N + n] : 777.0));
  return nullptr;
}

static int run_sweep() {
  long executed = 0, skipped = 0, by_kind[4] = {0, 0, 0, 0};
  const char* bad = nullptr;
  std::string where;
  Rng data;
  data.r = 2463534242u;
  for_cases([&](const Case& c) {
    if (bad) return;
    if (c.kind != POINTWISE && (out_h(c.q) <= 0 || out_w(c.q) <= 0)) { ++skipped; return; }
    ++executed;
    ++by_kind[c.kind];
    if ((bad = run_case(c, data))) where = describe(c);
  });
  if (bad) {
    printf("conv_args_check FAILED: %s\n  at %s\n", bad, where.c_str());
    return 1;
  }
  printf("conv_args_check sweep ok: %ld shapes executed (%ld fwd, %ld dgrad, %ld pair, %ld "
         "pointwise), %ld skipped (empty output)\n",
         executed, by_kind[FWD], by_kind[DGRAD], by_kind[PAIR], by_kind[POINTWISE], skipped);
  return 0;
}

// ------------------------------------------------------------------------ wgrad fields
static const char* check_wgrad(const ConvShape& q, int P, int Q) {
  for (int ow = 0; ow < 2; ++ow) {
    const WGradArgs a = conv_wgrad_args(q, P, Q, ow != 0);
    REQUIRE(!a.dy && !a.x && !a.dw && !a.slab);
    REQUIRE(a.Kout == q.K && a.C == q.C && a.H == q.H && a.W == q.W && a.P == P && a.Q == Q);
    REQUIRE(a.R == q.R && a.S == q.S && a.sh == q.sh && a.sw == q.sw && a.ph == q.ph && a.pw == q.pw);
    REQUIRE(a.Mpix == q.N * P * Q && a.Ncols == q.R * q.S * q.C && a.overwrite == ow);
    REQUIRE(a.ktiles_per_split == 0 && a.tiles_n == 0 && a.tiles_total == 0);
  }
  return nullptr;
}

static int run_wgrad() {
  long shapes = 0;
  const char* bad = nullptr;
  std::string where;
  for_cases([&](const Case& c) {
    if (bad || c.kind != FWD || c.flag || out_h(c.q) <= 0 || out_w(c.q) <= 0) return;
    ++shapes;
    if ((bad = check_wgrad(c.q, out_h(c.q), out_w(c.q)))) where = describe(c);
  });
  // a linear layer [B, Cin] -> [B, Cout]: the 1x1 conv of B one-pixel images
  for (int B = 1; B <= 3 && !bad; ++B)
    for (int ci = 1; ci <= 9 && !bad; ++ci)
      for (int co = 1; co <= 9 && !bad; ++co) {
        const ConvShape q{B, 1, 1, ci, co, 1, 1, 1, 1, 0, 0};
        const WGradArgs a = conv_wgrad_args(q, out_h(q), out_w(q), false);
        ++shapes;
        bad = check_wgrad(q, 1, 1);
        if (!bad && !(a.Mpix == B && a.Ncols == ci && a.Kout == co && a.P == 1 && a.Q == 1))
          bad = "linear: Mpix == B, Ncols == Cin, Kout == Cout";
        if (bad) where = fmt("linear b%d cin%d cout%d", B, ci, co);
      }
  if (bad) {
    printf("conv_args_check FAILED: %s\n  at %s\n", bad, where.c_str());
    return 1;
  }
  printf("conv_args_check wgrad ok: %ld shapes\n", shapes);
  return 0;
}

// ------------------------------------------------------------------------ dump
static std::string line(const IGemmArgs& a) {
  std::string s = fmt("a %dx%dx%d o %dx%d M %d U %d,%d O %d,%d T %d Ktot %d N %d RS %d ldb %d "
                      "d %dx%d Uo %d,%d Po %d,%d nphase %d tapmap %d stap %d ldb2 %d | taps",
                      a.aH, a.aW, a.aC, a.oH, a.oW, a.M, a.Uh, a.Uw, a.Oh, a.Ow, a.T, a.Ktot, a.N,
                      a.RS, a.ldb, a.dH, a.dW, a.Uoh, a.Uow, a.Poh, a.Pow, a.nphase, a.b_tapmap,
                      a.stap, a.ldb2);
  int ntaps = a.T;
  for (int i = 0; i < a.nphase; ++i) ntaps = std::max(ntaps, a.ph[i].tap0 + a.ph[i].T);
  for (int t = 0; t < ntaps; ++t) s += fmt(" %d,%d,%#x", a.taps.dh[t], a.taps.dw[t], a.taps.bt[t]);
  s += " | ph";
  for (int i = 0; i < a.nphase; ++i) {
    const PhaseDesc& d = a.ph[i];
    s += fmt(" [M %d o %dx%d Ktot %d taps %d+%d Po %d,%d]", d.M, d.oH, d.oW, d.Ktot, d.tap0, d.T,
             d.Poh, d.Pow);
  }
  return s;
}

static std::string line(const WGradArgs& a) {
  return fmt("Kout %d C %d x %dx%d dy %dx%d w %dx%d s %d,%d p %d,%d Mpix %d Ncols %d overwrite %d",
             a.Kout, a.C, a.H, a.W, a.P, a.Q, a.R, a.S, a.sh, a.sw, a.ph, a.pw, a.Mpix, a.Ncols,
             a.overwrite);
}

static bool parse(const char* s, Case& c) {
  int v[15] = {0};
  int n = 0;
  const char* colon = strchr(s, ':');
  if (!colon) return false;
  for (const char* p = colon; p && n < 15; p = strchr(p + 1, ','))
    if (sscanf(p + 1, "%d", &v[n++]) != 1) return false;
  int kind = -1;
  for (int i = 0; i < 5; ++i)
    if (!strncmp(s, KINDS[i], colon - s) && strlen(KINDS[i]) == (size_t)(colon - s)) kind = i;
  static const int COUNT[] = {12, 12, 15, 7, 11};
  if (kind < 0 || n != COUNT[kind]) return false;
  c = Case{(Kind)kind, {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10]}, false, {}};
  if (kind == POINTWISE) c.q = ConvShape{v[0], v[1], v[2], v[3], v[4], v[5], v[6], 1, 1, 0, 0};
  if (kind == FWD || kind == DGRAD) c.flag = v[11] != 0;
  if (kind == PAIR) { c.flag = true; c.s2 = DgradSrc2Shape{v[11], v[12], v[13], v[14]}; }
  return true;
}

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!strcmp(mode, "sweep") && argc == 2) return run_sweep();
  if (!strcmp(mode, "wgrad") && argc == 2) return run_wgrad();
  const bool dump = !strcmp(mode, "dump");
  if ((!dump && strcmp(mode, "exec")) || argc < 3) {
    fprintf(stderr, "usage: conv_args_check sweep | wgrad | dump SHAPE... | exec SHAPE...\n");
    return 2;
  }
  Rng data;
  for (int i = 2; i < argc; ++i) {
    Case c;
    if (!parse(argv[i], c) || (!dump && c.kind > PAIR)) {
      fprintf(stderr, "conv_args_check: cannot read '%s'\n", argv[i]);
      return 2;
    }
    const std::string name = describe(c);
    if (c.kind == WGRAD) {
      printf("%s : %s\n", name.c_str(), line(conv_wgrad_args(c.q, out_h(c.q), out_w(c.q), false)).c_str());
      continue;
    }
    IGemmArgs a;
    bool any_empty;
    const char* bad = build(c, a, any_empty);
    if (!bad && dump) {
      printf("%s : %s | empty %d\n", name.c_str(), line(a).c_str(), any_empty);
      continue;
    }
    if (!bad && (out_h(c.q) <= 0 || out_w(c.q) <= 0)) bad = "empty output";
    if (!bad) bad = run_case(c, data);
    printf("%s : %s\n", name.c_str(), bad ? bad : "exec ok");
    if (bad) return 1;
  }
  return 0;
}
