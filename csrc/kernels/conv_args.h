// From a layer's shape to the geometry of its GEMM launch: pure functions that fill the
// shape-dependent fields of IGemmArgs / WGradArgs (extents, strides, tap table, stride
// phases) and leave every pointer and epilogue field zero for the binding layer.  Only the
// C++ standard library and igemm_args.h: no HIP, no torch, so conv_args_check.cpp runs these
// on the CPU against textbook convolutions (tests/test_conv_args_cpu.py).
//
// Limits of the tables (MAXT taps, MAXPH stride phases) are reported as a message, null when
// the launch fits; each is tested before the write that would overrun.
#pragma once
#include "igemm_args.h"

namespace mpa {

// x [N, H, W, C] (NHWC), w [K, R, S, C], stride (sh, sw), zero padding (ph, pw)
struct ConvShape {
  int N, H, W, C, K, R, S, sh, sw, ph, pw;
};

// output extent along one axis (an empty output is <= 0; the callers reject or skip it)
inline int conv_out_extent(int in, int kernel, int stride, int pad) {
  return (in + 2 * pad - kernel) / stride + 1;
}

// Forward conv: row m = (img, p, q) of y gathers x at (p * sh - ph + r, q * sw - pw + s); B
// is w itself, K-contiguous.  stap (the caller's decision: C == 8, S > 1 and the engine has
// the form): 4 adjacent kernel columns per tap entry - their input pixels are 64 contiguous
// bytes in NHWC - so the 8-channel image stem takes the uniform-tap fast path; columns past
// S get zero weights.  K grows from R*S*8 to R*ceil(S/4)*32.
inline const char* conv_fwd_args(const ConvShape& q, bool stap, IGemmArgs& a) {
  a = IGemmArgs{};
  if (q.R * q.S > MAXT) return "too many taps";
  const int P = conv_out_extent(q.H, q.R, q.sh, q.ph), Q = conv_out_extent(q.W, q.S, q.sw, q.pw);
  a.aH = q.H; a.aW = q.W; a.aC = q.C;
  a.oH = P; a.oW = Q; a.M = q.N * P * Q;
  a.Uh = q.sh; a.Uw = q.sw; a.Oh = -q.ph; a.Ow = -q.pw;
  a.N = q.K; a.RS = q.R * q.S; a.ldb = a.RS * q.C;
  a.dH = P; a.dW = Q; a.Uoh = 1; a.Uow = 1;
  int t = 0;
  for (int r = 0; r < q.R; ++r)
    for (int s = 0; s < q.S; s += stap ? 4 : 1, ++t) {
      a.taps.dh[t] = (short)r; a.taps.dw[t] = (short)s;
      a.taps.bt[t] = (short)(stap ? (r * q.S + s) | (std::min(4, q.S - s) << 12) : t);
    }
  a.T = t;
  a.Ktot = stap ? t * 32 : t * q.C;
  a.stap = stap;
  return nullptr;
}

// the taps of a second conv that read the same input with the same stride (kernel R x S,
// pad ph / pw): see conv_dgrad_args
struct DgradSrc2Shape {
  int R, S, ph, pw;
};

// appends the taps (r, s) of an R x S kernel that land on dx rows / columns congruent to
// (a_, b_) modulo the stride; false: the table is full
inline bool dgrad_phase_taps(Taps& taps, int& T, int a_, int b_, int R, int S, int sh, int sw,
                             int ph, int pw, short tag) {
  for (int r = 0; r < R; ++r) {
    if (((a_ + ph - r) % sh) != 0) continue;
    for (int s = 0; s < S; ++s) {
      if (((b_ + pw - s) % sw) != 0) continue;
      if (T >= MAXT) return false;
      taps.dh[T] = (short)((a_ + ph - r) / sh);
      taps.dw[T] = (short)((b_ + pw - s) / sw);
      taps.bt[T] = (short)((r * S + s) | tag);
      ++T;
    }
  }
  return true;
}

// Data gradient of the conv q for any stride; dy is [N, P, Q, K].  Sub-pixel decomposition:
// output phase (a_, b_) of dx - its pixels (a_ + sh * i, b_ + sw * j) - is a stride-1 conv of
// dy with the taps (r, s) congruent to it.  wt: B is the transposed weight [C][R*S][K]
// (K-contiguous, rows indexed by weight tap) instead of w.  src2 (optional): the taps of a
// second conv join the phases they hit, tagged TAP_SRC2 (IGemmArgs::A2).
//
// Phases without taps (stride > kernel) are removed - their dx pixels are written by no
// one - and any_empty says that there were some.  Stride 1 has one phase and is described by
// the single-launch fields (nphase == 0); any other stride by ph[0 .. nphase).
inline const char* conv_dgrad_args(const ConvShape& q, int P, int Q, bool wt,
                                   const DgradSrc2Shape* src2, IGemmArgs& a, bool& any_empty) {
  a = IGemmArgs{};
  any_empty = false;
  if (q.R * q.S > MAXT) return "too many taps";
  a.aH = P; a.aW = Q; a.aC = q.K;
  a.Uh = 1; a.Uw = 1;
  a.N = q.C; a.RS = q.R * q.S;
  a.ldb = wt ? a.RS * q.K : q.C;
  a.b_tapmap = wt;
  if (src2) a.ldb2 = src2->R * src2->S * q.K;
  a.dH = q.H; a.dW = q.W; a.Uoh = q.sh; a.Uow = q.sw;
  int T = 0, nph = 0;
  for (int a_ = 0; a_ < q.sh; ++a_)
    for (int b_ = 0; b_ < q.sw; ++b_) {
      const int Hp = (q.H - a_ + q.sh - 1) / q.sh, Wp = (q.W - b_ + q.sw - 1) / q.sw;
      if (Hp <= 0 || Wp <= 0) continue;
      const int t0 = T;
      if (!dgrad_phase_taps(a.taps, T, a_, b_, q.R, q.S, q.sh, q.sw, q.ph, q.pw, 0) ||
          (src2 && !dgrad_phase_taps(a.taps, T, a_, b_, src2->R, src2->S, q.sh, q.sw, src2->ph,
                                     src2->pw, TAP_SRC2)))
        return "too many taps";
      if (nph >= MAXPH) return "too many stride phases";
      a.ph[nph++] = PhaseDesc{q.N * Hp * Wp, Hp, Wp, (T - t0) * q.K, t0, T - t0, a_, b_, 0,
                              FastDiv{}, FastDiv{}};
    }
  int k = 0;
  for (int i = 0; i < nph; ++i) {
    if (a.ph[i].T > 0) a.ph[k++] = a.ph[i];
    else any_empty = true;
  }
  if (q.sh == 1 && q.sw == 1) {
    const PhaseDesc& d = a.ph[0];
    a.M = d.M; a.oH = d.oH; a.oW = d.oW; a.T = d.T; a.Ktot = d.Ktot;
  } else {
    a.nphase = k;
  }
  return nullptr;
}

// One tap, no gather: rows are the pixels of nimg H x W images (H = W = 1: a linear layer's
// samples), y[m][0 .. Cout) = x[m][0 .. Cin) . B.  ldb is B's row stride - Cin for a
// K-contiguous [Cout][Cin], Cout for an N-contiguous [Cin][Cout]; tapmap sets b_tapmap (the
// map of the one tap is the identity).
inline IGemmArgs pointwise_args(int nimg, int H, int W, int Cin, int Cout, int ldb,
                                bool tapmap = false) {
  IGemmArgs a{};
  a.aH = H; a.aW = W; a.aC = Cin;
  a.oH = H; a.oW = W; a.M = nimg * H * W;
  a.Uh = 1; a.Uw = 1;
  a.T = 1;
  a.Ktot = Cin;
  a.N = Cout; a.RS = 1; a.ldb = ldb;
  a.b_tapmap = tapmap;
  a.dH = H; a.dW = W; a.Uoh = 1; a.Uow = 1;
  return a;
}

// Weight gradient dw [K][R*S*C] = dy^T [K][N*P*Q] . im2col(x); dy is [N, P, Q, K].  A linear
// layer is the 1x1 conv of B one-pixel images.
inline WGradArgs conv_wgrad_args(const ConvShape& q, int P, int Q, bool overwrite) {
  WGradArgs a{};
  a.Kout = q.K; a.C = q.C; a.H = q.H; a.W = q.W; a.P = P; a.Q = Q; a.R = q.R; a.S = q.S;
  a.sh = q.sh; a.sw = q.sw; a.ph = q.ph; a.pw = q.pw;
  a.Mpix = q.N * P * Q;
  a.Ncols = q.R * q.S * q.C;
  a.overwrite = overwrite ? 1 : 0;
  return a;
}

}  // namespace mpa
