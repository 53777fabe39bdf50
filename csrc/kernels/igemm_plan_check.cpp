// CPU check of the implicit-GEMM launch planner (igemm_plan.h with conv_args.h and
// halo_plan.h: no HIP; any host C++17 compiler).  Run by tests/test_igemm_plan_cpu.py, plain
// and under AddressSanitizer + UndefinedBehaviorSanitizer.
//
//   igemm_plan_check                 the dispatch of the model zoo's layers (ZOO below) at
//                                    batch 32 and 3 under engine 0, 1 and 2
//   igemm_plan_check ARG...          the dispatch of the given shapes under the switches set
//                                    before them
//   igemm_plan_check sweep           every plan of a grid of shapes, switches and tuner
//                                    candidates against the limits the kernels and the
//                                    callers state (check_rows / check_phases / check_wgrad)
//
//   ARG    engine=0|1|2  dma_uni=0|1  kpad=0|1  force=BM,BN,SPLITS  tile=BM,BN (a tuned tile)
//          fwd:N,H,W,C,K,R,S,sh,sw,ph,pw,STAP         STAP 1: super-tap form where available
//          dgrad:N,H,W,C,K,R,S,sh,sw,ph,pw,WT         WT 1: the transposed weight exists
//          bnred:N,H,W,C,K,R,S,sh,sw,ph,pw,WT         dgrad with the fused BN-backward reduction
//          pair:N,H,W,C,K,R,S,sh,sw,ph,pw,R2,S2,ph2,pw2   dgrad plus a second conv's, WT 1
//          pointwise:NIMG,H,W,Cin,Cout,ldb,TAPMAP     ldb == Cin, TAPMAP 0: a forward (linear)
//                                                      launch, else a dgrad launch
//          wgrad:N,H,W,C,K,R,S,sh,sw,ph,pw
//
// Each shape becomes the launch the binding layer makes of it (operand widths, K-contiguous
// B, workspace from the sizing functions: `call_*` below) and prints one line per launch:
// kernel and template arguments, grid, block, the planned argument fields, the finalize /
// reduce launch, the statistics-slab rows where statistics are asked for, the workspace
// floats and the tuner key.  Launches the 3x3 halo path takes first are printed as such.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "conv_args.h"
#include "halo_plan.h"
#include "igemm_plan.h"

using namespace mpa;

static std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
static std::string fmt(const char* f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

template <class T>
static T* some() {  // a 16-B aligned non-null address that is never read
  return reinterpret_cast<T*>(uintptr_t(4096));
}

static int vec_width(int c) { return c % 8 == 0 ? 8 : (c % 4 == 0 ? 4 : 1); }
static const char* tf(bool b) { return b ? "true" : "false"; }
constexpr int CUS = 256;

// ------------------------------------------------------------------------ launch lines
static std::string line(const RowsLaunch& p, bool stats, int64_t ws) {
  std::string s;
  if (p.family == RowsFamily::Reg)
    s = fmt("igemm_rows_kernel<%d, %d, %d, %d, %d, %s, %s>", p.BM, p.BN, p.WM, p.WN, p.VW, tf(p.BKC),
            tf(p.SPLIT));
  else
    s = fmt("igemm_rows_dma%s_kernel<%d, %d, %d, %d, %s, %s, %s>",
            p.family == RowsFamily::DmaUni ? "_uni" : "", p.BM, p.BN, p.WM, p.WN, tf(p.BKC),
            tf(p.SPLIT), tf(p.PH));
  s += fmt(" grid %d,1,%d block %d kps %d tiles_n %d tiles_total %d Ktot %d kpad %d", p.grid_x,
           p.splits, p.block, p.ktiles_per_split, p.tiles_n, p.tiles_total, p.Ktot, p.kpad);
  if (p.PH) {
    s += " ph";
    for (int i = 0; i < p.nphase; ++i) s += fmt(" %d", p.ph_tiles[i]);
  }
  s += p.fin_cw ? fmt(" | splitk_finalize_kernel<%d> grid %d,%d", p.fin_cw, p.fin_gx, p.fin_gy)
                : std::string(" | none");
  s += stats ? fmt(" | slab_rows %d", p.slab_rows) : std::string(" | slab_rows -");
  return s + fmt(" | ws %lld", (long long)ws);
}

static std::string line(const WGradLaunch& p, int64_t ws) {
  std::string s;
  if (p.family == WGradFamily::Reg)
    s = fmt("igemm_wgrad_kernel<%d, %d, %d, %d, %d, %d>", p.BM, p.BN, p.WM, p.WN, p.VWA, p.VWB);
  else
    s = fmt("igemm_wgrad_dma%s_kernel<%d, %d, %d, %d>", p.family == WGradFamily::DmaInc ? "_inc" : "",
            p.BM, p.BN, p.WM, p.WN);
  s += fmt(" grid %d,1,%d block %d kps %d tiles_n %d tiles_total %d", p.grid_x, p.splits, p.block,
           p.ktiles_per_split, p.tiles_n, p.tiles_total);
  if (p.family == WGradFamily::DmaInc)
    s += fmt(" inc %d,%d,%d,%d,%d,%d,%d", p.inc.dq_s, p.inc.dp_s, p.inc.qwrap, p.inc.pwrap,
             p.inc.step_off, p.inc.qwrap_off, p.inc.pwrap_off);
  s += p.reduce == WGradReduce::None ? std::string(" | none")
       : fmt(" | wgrad_reduce%s_kernel grid %d", p.reduce == WGradReduce::Scalar ? "_scalar" : "",
             p.reduce_blocks);
  return s + fmt(" | ws %lld", (long long)ws);
}

// ------------------------------------------------------------------------ the callers
// What takes a launch before the GEMM engine is asked: the 3x3 halo plan.  (The pixel-pair
// 7x7 stem's tests, conv_stem_ok / stem_wgrad_ok, live in conv_stem.hip and are not repeated
// here: give this program no pixel-pair stem shape, 7x4 taps on 8 channels - it would print
// the GEMM plan the stem path pre-empts.)
static bool halo_fwd(const IGemmArgs& a) {
  return plan_halo(a, HaloSwitches{}, CUS).kind != HaloKind::None;
}

struct Config {
  GemmSwitches sw;
  TileSize tuned{0, 0};
};

// igemm_rows / igemm_rows_dgrad: halo, else one planned GEMM
static std::string call_rows(IGemmArgs a, bool bkc, int vw, bool stats, bool have_ws, const Config& c) {
  a.A = some<const bf16_raw>();
  a.B = some<const bf16_raw>();
  a.C = some<void>();
  if (stats) a.stats = some<float>();
  const bool dma = rows_dma(vw, c.sw);
  if (dma && bkc && halo_fwd(a)) return "halo";
  // (the binding allocates the split workspace the sizing function asks for, if any)
  const int64_t ws = have_ws ? rows_ws_floats(a.M, a.N, a.Ktot, c.sw) : 0;
  const int kp = rows_kpad_ktot(a, bkc, vw, c.sw);
  const RowsLaunch p = plan_rows(a, bkc, vw, ws > 0, c.sw, c.tuned);
  // the key under which the tuner files the shape (the LDS-DMA engine's launches only)
  const std::string key = dma && a.M > 0 ? rows_key(a, kp ? kp : a.Ktot, bkc, ws > 0 && !kp) : "-";
  return line(p, stats, ws) + " | " + key;
}

// igemm_rows_dgrad_phases: one merged launch on the LDS-DMA engine, else one per phase
static std::vector<std::string> call_phases(IGemmArgs a, bool bkc, int vw, const Config& c) {
  std::vector<std::string> out;
  if (rows_dma(vw, c.sw) && a.nphase <= MAXPH) {
    const RowsLaunch p = plan_rows_phases(a, bkc, c.sw, c.tuned);
    if (p.tiles_total > 0) {
      out.push_back(line(p, false, 0) + " | " + rows_key(a, a.Ktot, bkc, false));
      return out;
    }
  }
  for (int i = 0; i < a.nphase; ++i) {
    const PhaseDesc& d = a.ph[i];
    IGemmArgs b = a;
    b.nphase = 0;
    b.M = d.M; b.oH = d.oH; b.oW = d.oW; b.Ktot = d.Ktot; b.T = d.T;
    out.push_back(fmt("phase %d: ", i) + call_rows(b, bkc, vw, false, false, Config{c.sw, {0, 0}}));
  }
  return out;
}

// igemm_rows_dgrad_bnred: halo, else one launch on the LDS-DMA engine
static std::string call_bnred(IGemmArgs a, bool bkc, const Config& c) {
  a.ep_bnred = 1;
  a.stats = a.stats_sums = some<float>();
  a.ep_z = a.ep_y = some<const bf16_raw>();
  a.ep_mean = a.ep_rstd = some<const float>();
  if (a.nphase == 0 && bkc && halo_fwd(a)) return "halo";
  const RowsLaunch p = a.nphase > 0 ? plan_rows_phases(a, bkc, c.sw, TileSize{})
                                    : plan_rows_on(a, bkc, 8, false, true, false, c.sw, TileSize{});
  return line(p, true, 0);
}

static std::string call_wgrad(WGradArgs a, int vwa, int vwb, const Config& c) {
  const int64_t ws = wgrad_gemm_ws_floats(a.Kout, a.Ncols, a.Mpix, c.sw);
  a.dy = a.x = some<const bf16_raw>();
  a.dw = a.slab = some<float>();
  if (c.sw.engine >= 1 && plan_halo_wgrad(a, HaloSwitches{}, CUS).kind != HaloWKind::None) return "halo";
  const bool tuner = vwa == 8 && vwb == 8 && c.sw.engine >= 1 && a.Mpix > 0;
  return line(plan_wgrad(a, vwa, vwb, c.sw, c.tuned), ws) + " | " + (tuner ? wgrad_key(a) : "-");
}

// ------------------------------------------------------------------------ shapes
enum Kind { FWD, DGRAD, BNRED, PAIR, POINTWISE, WGRAD };
static const char* const KINDS[] = {"fwd", "dgrad", "bnred", "pair", "pointwise", "wgrad"};

struct Shape {
  Kind kind;
  ConvShape q;  // (POINTWISE: N, H, W, C = Cin, K = Cout; R = ldb, S = tapmap)
  bool flag;
  DgradSrc2Shape s2;
};

static bool parse(const char* s, Shape& c) {
  int v[15] = {0};
  int n = 0;
  const char* colon = strchr(s, ':');
  if (!colon) return false;
  for (const char* p = colon; p && n < 15; p = strchr(p + 1, ','))
    if (sscanf(p + 1, "%d", &v[n++]) != 1) return false;
  int kind = -1;
  for (int i = 0; i < 6; ++i)
    if (!strncmp(s, KINDS[i], colon - s) && strlen(KINDS[i]) == (size_t)(colon - s)) kind = i;
  static const int COUNT[] = {12, 12, 12, 15, 7, 11};
  if (kind < 0 || n != COUNT[kind]) return false;
  c = Shape{(Kind)kind, {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10]}, false, {}};
  if (kind == POINTWISE) c.q = ConvShape{v[0], v[1], v[2], v[3], v[4], v[5], v[6], 1, 1, 0, 0};
  if (kind == FWD || kind == DGRAD || kind == BNRED) c.flag = v[11] != 0;
  if (kind == PAIR) { c.flag = true; c.s2 = DgradSrc2Shape{v[11], v[12], v[13], v[14]}; }
  return true;
}

static std::string describe(const Shape& c) {
  const ConvShape& q = c.q;
  if (c.kind == POINTWISE)
    return fmt("pointwise n%d %dx%d c%d k%d ldb%d tapmap%d", q.N, q.H, q.W, q.C, q.K, q.R, q.S);
  std::string s = fmt("%s n%d %dx%d c%d k%d %dx%d s%d,%d p%d,%d", KINDS[c.kind], q.N, q.H, q.W, q.C,
                      q.K, q.R, q.S, q.sh, q.sw, q.ph, q.pw);
  if (c.kind == FWD) s += fmt(" stap%d", c.flag);
  if (c.kind == DGRAD || c.kind == BNRED || c.kind == PAIR) s += fmt(" wt%d", c.flag);
  if (c.kind == PAIR) s += fmt(" + %dx%d p%d,%d", c.s2.R, c.s2.S, c.s2.ph, c.s2.pw);
  return s;
}

// the launches the binding layer makes of a shape (csrc/bindings.cpp), one line each
static std::vector<std::string> dispatch(const Shape& c, const Config& cfg) {
  const ConvShape& q = c.q;
  const int P = conv_out_extent(q.H, q.R, q.sh, q.ph), Q = conv_out_extent(q.W, q.S, q.sw, q.pw);
  IGemmArgs a;
  bool empty = false;
  switch (c.kind) {
    case FWD: {  // conv + BatchNorm statistics into a dense output
      const bool stap = c.flag && q.C == 8 && q.S > 1 && cfg.sw.dma_uni && cfg.sw.engine >= 1;
      if (conv_fwd_args(q, stap, a)) return {"too many taps"};
      a.ldc = q.K;
      return {call_rows(a, true, vec_width(q.C), true, true, cfg)};
    }
    case POINTWISE: {
      const bool bkc = q.R == q.C;
      a = pointwise_args(q.N, q.H, q.W, q.C, q.K, q.R, q.S != 0);
      a.ldc = q.K;
      if (bkc && !q.S) return {call_rows(a, true, vec_width(q.C), false, true, cfg)};
      return {call_rows(a, bkc, std::min(vec_width(q.C), vec_width(q.K)), false, true, cfg)};
    }
    case WGRAD:
      return {call_wgrad(conv_wgrad_args(q, P, Q, false), vec_width(q.K), q.C % 8 == 0 ? 8 : 1, cfg)};
    default: break;
  }
  const int vw = std::min(vec_width(q.K), vec_width(q.C));
  const bool bkc = c.flag && vw == 8;
  if (conv_dgrad_args(q, P, Q, bkc, c.kind == PAIR ? &c.s2 : nullptr, a, empty)) return {"too many taps"};
  a.ldc = q.C;
  if (c.kind == BNRED) {
    if (!(cfg.sw.engine >= 1 && vw == 8 && bkc) || empty) return {"not available"};
    return {call_bnred(a, bkc, cfg)};
  }
  if (q.sh == 1 && q.sw == 1) return {call_rows(a, bkc, vw, false, true, cfg)};
  if (c.kind == PAIR) {
    a.A2 = a.B2 = some<const bf16_raw>();
    if (!dgrad_src2_ok(a, vw, bkc, cfg.sw)) return {"apart"};
  }
  return call_phases(a, bkc, vw, cfg);
}

// The model zoo: the 26 launches pinned in tests/test_conv_args_cpu.py (ResNet stem in both
// forms with its dgrad and weight gradient, a 3x3/s1, a 3x3/s2 alone and with its 1x1/s2
// shortcut, the 1x1/s2, Inception's 1x7 / 7x1 / 3x3/s2 valid / 5x5/p2, DenseNet's 1x1 and
// its one-tap dgrad, a linear layer), then the classifier heads of ResNet-50 / DenseNet /
// the 64,500-class flagship, the deeper stages' stride-2 dgrads alone and with their
// shortcut, their fused-reduction form, and the non-halo weight gradients of those layers.
static const char* const ZOO[] = {
    "fwd:%d,224,224,8,64,7,7,2,2,3,3,1", "fwd:%d,224,224,8,64,7,7,2,2,3,3,0",
    "dgrad:%d,224,224,8,64,7,7,2,2,3,3,0", "wgrad:%d,224,224,8,64,7,7,2,2,3,3",
    "fwd:%d,56,56,64,64,3,3,1,1,1,1,0", "dgrad:%d,56,56,64,64,3,3,1,1,1,1,1",
    "dgrad:%d,56,56,64,64,3,3,1,1,1,1,0", "wgrad:%d,56,56,64,64,3,3,1,1,1,1",
    "fwd:%d,56,56,64,128,3,3,2,2,1,1,0", "dgrad:%d,56,56,64,128,3,3,2,2,1,1,1",
    "pair:%d,56,56,64,128,3,3,2,2,1,1,1,1,0,0",
    "fwd:%d,56,56,64,128,1,1,2,2,0,0,0", "dgrad:%d,56,56,64,128,1,1,2,2,0,0,1",
    "fwd:%d,17,17,128,128,1,7,1,1,0,3,0", "dgrad:%d,17,17,128,128,1,7,1,1,0,3,1",
    "fwd:%d,17,17,128,192,7,1,1,1,3,0,0", "dgrad:%d,17,17,128,192,7,1,1,1,3,0,1",
    "fwd:%d,35,35,288,384,3,3,2,2,0,0,0", "dgrad:%d,35,35,288,384,3,3,2,2,0,0,1",
    "fwd:%d,35,35,48,64,5,5,1,1,2,2,0", "dgrad:%d,35,35,48,64,5,5,1,1,2,2,1",
    "fwd:%d,56,56,128,128,1,1,1,1,0,0,0", "pointwise:%d,56,56,128,64,128,1",
    "pointwise:%d,1,1,512,1000,512,0", "pointwise:%d,1,1,1000,512,512,0",
    "wgrad:%d,1,1,512,1000,1,1,1,1,0,0",
    // linear heads: forward, dgrad from w and from the transposed weight, weight gradient
    "pointwise:%d,1,1,2048,1000,2048,0", "pointwise:%d,1,1,1000,2048,2048,0",
    "pointwise:%d,1,1,1000,2048,1000,1", "wgrad:%d,1,1,2048,1000,1,1,1,1,0,0",
    "pointwise:%d,1,1,512,64500,512,0", "pointwise:%d,1,1,64500,512,64500,1",
    "wgrad:%d,1,1,512,64500,1,1,1,1,0,0",
    // stride-2 dgrads of the deeper stages, alone, with the shortcut, with the BN reduction
    "dgrad:%d,28,28,128,256,3,3,2,2,1,1,1", "pair:%d,28,28,128,256,3,3,2,2,1,1,1,1,0,0",
    "dgrad:%d,14,14,256,512,3,3,2,2,1,1,1", "pair:%d,14,14,256,512,3,3,2,2,1,1,1,1,0,0",
    "dgrad:%d,28,28,128,256,3,3,2,2,1,1,0", "bnred:%d,28,28,128,256,3,3,2,2,1,1,1",
    "bnred:%d,56,56,64,64,1,1,1,1,0,0,1", "bnred:%d,35,35,48,64,5,5,1,1,2,2,1",
    // weight gradients that stay on the GEMM engine
    "wgrad:%d,56,56,64,128,3,3,2,2,1,1", "wgrad:%d,56,56,64,128,1,1,2,2,0,0",
    "wgrad:%d,14,14,256,512,3,3,2,2,1,1", "wgrad:%d,14,14,256,512,1,1,2,2,0,0",
    "wgrad:%d,17,17,128,192,7,1,1,1,3,0", "wgrad:%d,35,35,48,64,5,5,1,1,2,2",
    "wgrad:%d,56,56,256,64,1,1,1,1,0,0",
};

static int print_shape(const char* arg, const Config& cfg) {
  Shape c;
  if (!parse(arg, c)) {
    fprintf(stderr, "igemm_plan_check: cannot read '%s'\n", arg);
    return 2;
  }
  for (const std::string& ln : dispatch(c, cfg))
    printf("%s e%d : %s\n", describe(c).c_str(), cfg.sw.engine, ln.c_str());
  return 0;
}

static int print_zoo() {
  for (int engine = 0; engine <= 2; ++engine)
    for (int batch : {32, 3})
      for (const char* z : ZOO) {
        Config cfg;
        cfg.sw.engine = engine;
        if (int r = print_shape(fmt(z, batch).c_str(), cfg)) return r;
      }
  return 0;
}

// ------------------------------------------------------------------------ sweep
#define REQUIRE(cond)          \
  do {                         \
    if (!(cond)) return #cond; \
  } while (0)

static const char* check_splits(int ktiles, int splits, int kps) {
  REQUIRE(splits >= 1 && splits <= 65535 && kps >= 1);
  REQUIRE((int64_t)splits * kps >= ktiles);
  REQUIRE(splits == 1 || (int64_t)(splits - 1) * kps < ktiles);  // no split is empty
  return nullptr;
}

// The uniform-tap kernel's 32-bit offsets, from the operands' definitions and not through
// the header: A holds the launch's images (its rows' pixels / pixels per image, of the first
// phase in a merged launch) of aH x aW x aC bf16; B has N rows (K-contiguous) or aC * RS rows
// (N-contiguous) of ldb; a second source's B2 has N rows of ldb2.
static bool operands_below_2g(const IGemmArgs& a, bool bkc) {
  const int64_t limit = int64_t(1) << 31;
  const int64_t rows = a.nphase > 0 ? a.ph[0].M : a.M;
  const int64_t per_image = a.nphase > 0 ? (int64_t)a.ph[0].oH * a.ph[0].oW : (int64_t)a.oH * a.oW;
  int64_t images = 0;
  while (images * per_image < rows) ++images;  // (per_image >= 1 in every swept launch)
  const int64_t b_rows = bkc ? a.N : (int64_t)a.aC * a.RS;
  return images * a.aH * a.aW * a.aC * 2 < limit && b_rows * a.ldb * 2 < limit &&
         (int64_t)a.N * a.ldb2 * 2 < limit;
}

static const char* check_family(const RowsLaunch& p, const IGemmArgs& a, bool bkc, int vw,
                                const GemmSwitches& sw) {
  const Tile* t = p.family == RowsFamily::Reg ? find_tile(kRowsRegTiles, p.BM, p.BN)
                                              : find_tile(kRowsDmaTiles, p.BM, p.BN);
  REQUIRE(t && t->wm == p.WM && t->wn == p.WN && p.block == p.WM * p.WN * 64);
  REQUIRE(p.family != RowsFamily::Reg || (p.block == 256 && !p.kpad && !p.PH));
  REQUIRE(p.family == RowsFamily::Reg || (vw == 8 && p.VW == 8));
  REQUIRE(p.VW == 8 || p.VW == 4 || p.VW == 1);
  REQUIRE(p.VW <= vw && p.BKC == bkc);
  REQUIRE(p.grid_x == p.tiles_total && p.tiles_total >= 1 && p.SPLIT == (p.splits > 1));
  if (p.family == RowsFamily::DmaUni) {
    REQUIRE(sw.dma_uni && operands_below_2g(a, bkc));
    REQUIRE(a.aC % 32 == 0 || a.stap || (p.kpad && bkc));
  }
  REQUIRE(rows_uni_fits(a, bkc) == operands_below_2g(a, bkc));
  return nullptr;
}

// one rows GEMM as igemm_rows / igemm_rows_dgrad launch it
static const char* check_rows(const IGemmArgs& a, bool bkc, int vw, bool allow_split,
                              const GemmSwitches& sw, TileSize tuned) {
  const RowsLaunch p = plan_rows(a, bkc, vw, allow_split, sw, tuned);
  if (const char* bad = check_family(p, a, bkc, vw, sw)) return bad;
  REQUIRE(!p.PH && p.nphase == 0);
  REQUIRE(p.tiles_n == (a.N + p.BN - 1) / p.BN);
  REQUIRE(p.tiles_total == (a.M + p.BM - 1) / p.BM * p.tiles_n);
  if (const char* bad = check_splits((p.Ktot + BK - 1) / BK, p.splits, p.ktiles_per_split)) return bad;
  REQUIRE(p.splits == 1 || allow_split);
  REQUIRE(p.to_ws == (p.splits > 1) && (p.fin_cw != 0) == (p.splits > 1));
  if (p.splits > 1)
    REQUIRE((int64_t)p.splits * a.M * a.N <= rows_ws_floats(a.M, a.N, a.Ktot, sw));
  // statistics slab: igemm_slab_floats(M, N) = slab_rows_max(M) rows and the sums
  REQUIRE(p.slab_rows >= 1 && p.slab_rows <= slab_rows_max(a.M));
  if (p.fin_cw) {
    REQUIRE(p.fin_cw == 32 || p.fin_cw == 64);
    REQUIRE(p.fin_gx >= 1 && p.fin_gx * p.fin_cw >= a.N && (p.fin_gx - 1) * p.fin_cw < a.N);
    REQUIRE(p.fin_gy >= 1 && p.fin_gy <= slab_rows_max(a.M) && p.slab_rows == p.fin_gy);
  }
  // K padding: exactly on the LDS-DMA engine's K-contiguous launches of 16-B but not
  // 32-granular channel counts that the uniform-tap kernel can address, and the public
  // predicate says the same
  const bool pads = vw == 8 && sw.engine >= 1 && sw.kpad && sw.dma_uni && bkc && !a.stap &&
                    a.nphase == 0 && a.aC % 8 == 0 && a.aC % 32 != 0 && operands_below_2g(a, bkc);
  REQUIRE((p.kpad != 0) == pads && rows_kpad_ok(a, bkc, vw, sw) == pads);
  if (p.kpad) {
    REQUIRE(p.family == RowsFamily::DmaUni && bkc && p.splits == 1);
    REQUIRE(p.Ktot == a.T * ((a.aC + 31) / 32 * 32) && p.Ktot == rows_kpad_ktot(a, bkc, vw, sw));
  } else {
    REQUIRE(p.Ktot == a.Ktot);
  }
  IGemmArgs b = a;
  p.apply(b);
  REQUIRE(b.Ktot == p.Ktot && b.kpad == p.kpad && b.tiles_n == p.tiles_n &&
          b.tiles_total == p.tiles_total && b.ktiles_per_split == p.ktiles_per_split);
  return nullptr;
}

// the fused BN-backward dgrad without phases: the LDS-DMA engine, unsplit, unpadded
static const char* check_bnred(const IGemmArgs& a, bool bkc, const GemmSwitches& sw) {
  const RowsLaunch p = plan_rows_on(a, bkc, 8, false, true, false, sw, TileSize{});
  if (const char* bad = check_family(p, a, bkc, 8, sw)) return bad;
  REQUIRE(p.family != RowsFamily::Reg && p.splits == 1 && !p.kpad && p.Ktot == a.Ktot);
  REQUIRE(p.slab_rows == (a.M + p.BM - 1) / p.BM);
  REQUIRE((int64_t)p.slab_rows * 2 * a.N <= bnred_slab_floats(a.M, a.N, 1));
  return nullptr;
}

// a merged stride-phase launch; dx_pixels: what the binding sizes the bnred slab with
static const char* check_phases(const IGemmArgs& a, bool bkc, int64_t dx_pixels,
                                const GemmSwitches& sw, TileSize tuned) {
  const RowsLaunch p = plan_rows_phases(a, bkc, sw, tuned);
  if (const char* bad = check_family(p, a, bkc, 8, sw)) return bad;
  REQUIRE(p.PH && p.family != RowsFamily::Reg && p.splits == 1 && !p.fin_cw && !p.to_ws);
  REQUIRE(p.nphase == a.nphase && a.nphase >= 1 && a.nphase <= MAXPH);
  REQUIRE(p.tiles_n == (a.N + p.BN - 1) / p.BN);
  int most = 0;
  int64_t rows = 0;
  for (int i = 0; i < a.nphase; ++i) {
    REQUIRE(p.ph_tiles[i] == (a.ph[i].M + p.BM - 1) / p.BM * p.tiles_n);
    most = std::max(most, p.ph_tiles[i]);
    rows += (a.ph[i].M + p.BM - 1) / p.BM;
  }
  REQUIRE(p.tiles_total == a.nphase * most && p.slab_rows == rows);
  REQUIRE(rows * 2 * a.N <= bnred_slab_floats((int)dx_pixels, a.N, a.nphase));
  // every phase's K loop runs in one piece
  for (int i = 0; i < a.nphase; ++i) REQUIRE(p.ktiles_per_split >= (a.ph[i].Ktot + BK - 1) / BK);
  // a second source is accepted exactly when this launch reads it
  REQUIRE(dgrad_src2_ok(a, 8, bkc, sw) ==
          (sw.engine >= 1 && bkc && p.family == RowsFamily::DmaUni && p.PH));
  REQUIRE(rows_uni_src2_ok(a, bkc, sw) == (bkc && p.family == RowsFamily::DmaUni));
  IGemmArgs b = a;
  p.apply(b);
  for (int i = 0; i < a.nphase; ++i) REQUIRE(b.ph[i].tiles == p.ph_tiles[i]);
  return nullptr;
}

static const char* check_wgrad(const WGradArgs& a, int vwa, int vwb, const GemmSwitches& sw,
                               TileSize tuned) {
  const WGradLaunch p = plan_wgrad(a, vwa, vwb, sw, tuned);
  const Tile* t = p.family == WGradFamily::Reg   ? find_tile(kWgradRegTiles, p.BM, p.BN)
                  : p.family == WGradFamily::Dma ? find_tile(kWgradDmaTiles, p.BM, p.BN)
                                                 : find_tile(kWgradIncTiles, p.BM, p.BN);
  REQUIRE(t && t->wm == p.WM && t->wn == p.WN && p.block == p.WM * p.WN * 64);
  REQUIRE(p.family == WGradFamily::Reg || (vwa == 8 && vwb == 8 && sw.engine >= 1));
  REQUIRE(p.family != WGradFamily::Reg || p.block == 256);
  REQUIRE((p.VWA == 8 || p.VWA == 4 || p.VWA == 1) && p.VWA <= vwa && (p.VWB == 8 || p.VWB == 1) &&
          p.VWB <= vwb);
  REQUIRE(p.tiles_n == (a.Ncols + p.BN - 1) / p.BN);
  REQUIRE(p.tiles_total == (a.Kout + p.BM - 1) / p.BM * p.tiles_n && p.tiles_total >= 1);
  REQUIRE(p.grid_x == p.tiles_total);
  if (const char* bad = check_splits((a.Mpix + BK - 1) / BK, p.splits, p.ktiles_per_split)) return bad;
  const int64_t n = (int64_t)a.Kout * a.Ncols;
  if (p.splits > 1) {
    REQUIRE(p.splits * n <= (16ll << 20));
    REQUIRE(p.splits * n <= wgrad_gemm_ws_floats(a.Kout, a.Ncols, a.Mpix, sw));
  }
  REQUIRE((p.reduce != WGradReduce::None) == (p.splits > 1));
  if (p.reduce == WGradReduce::Vector) REQUIRE(n % 4 == 0 && p.reduce_blocks == (n / 4 + 63) / 64);
  if (p.reduce == WGradReduce::Scalar) REQUIRE(p.reduce_blocks >= 1 && p.reduce_blocks <= 4096);
  if (p.family == WGradFamily::DmaInc) {
    REQUIRE(sw.dma_uni && p.block == 256 && a.Kout >= 8 && a.Ncols >= 8);
    REQUIRE(BK / a.Q + 1 <= a.P);  // one wrap per step
    REQUIRE((int64_t)a.Mpix / (a.P * a.Q) * a.H * a.W * a.C < (1ll << 31));
    REQUIRE(p.inc.dq_s == a.sw * (BK % a.Q) && p.inc.dp_s == a.sh * (BK / a.Q));
    REQUIRE(p.inc.qwrap == a.Q * a.sw && p.inc.pwrap == a.P * a.sh);
  }
  return nullptr;
}

// ---- the grid.  Rows GEMMs: M x N x channels x taps (K = taps * channels; the 8-channel
// super-tap form among them) x operand width x B layout x allow_split x switches x (no tuned
// tile + every candidate the tuner would accept).  A launch's pixels are one image row
// (aH = oH = 1), plus a few image stacks whose operands pass 2^31 bytes.
static const int SIZES[] = {1, 7, 8, 31, 32, 33, 48, 80, 96, 128, 129, 256, 1000, 25088};
static const int COLS[] = {1, 7, 8, 31, 32, 33, 48, 64, 80, 96, 128, 192, 256, 1000};
static const int CHANNELS[] = {1, 4, 8, 24, 32, 48, 64, 80, 96};
static const int TAPS[] = {1, 2, 9, 25, 49};

static std::vector<GemmSwitches> switch_configs() {
  std::vector<GemmSwitches> v;
  // (64 x 64 is no tile of any family; a split count alone may be forced too)
  static const int FORCE[][3] = {{0, 0, 0}, {256, 256, 0}, {128, 64, 3}, {0, 0, 5}, {64, 64, 0}, {256, 128, 1000}};
  for (int engine = 0; engine <= 2; ++engine)
    for (int uni = 0; uni < 2; ++uni)
      for (int kpad = 0; kpad < 2; ++kpad)
        for (const auto& f : FORCE) {
          if (engine == 0 && !(uni && kpad)) continue;  // (the register engine reads neither)
          GemmSwitches sw;
          sw.engine = engine; sw.dma_uni = uni != 0; sw.kpad = kpad != 0;
          sw.force_bm = f[0]; sw.force_bn = f[1]; sw.force_splits = f[2];
          v.push_back(sw);
        }
  return v;
}

struct Sweep {
  long plans = 0;
  const char* bad = nullptr;
  std::string where;
  std::map<std::string, std::string> keys;  // tuner key -> the fields it was made from
  bool fail(const char* b, const std::string& w) {
    if (b && !bad) { bad = b; where = w; }
    return bad != nullptr;
  }
  // Two argument sets that differ in a field the key prints never share a key: the text
  // separates its fields.  This is less than "any field a plan reads": the choice between
  // the uniform-tap and the generic kernel also reads ldb, ldb2, RS, the operand width and
  // the dma_uni / kpad switches, none of which the key carries (the launch code before this
  // header had the same keys, and their text is an interface between ranks, so they stay).
  // Every caller derives ldb / ldb2 / RS and the width from fields the key does carry; the
  // switches are process-wide.  A sweep over them would report shared keys, so it is left out.
  void key(const std::string& k, const std::string& fields) {
    auto it = keys.emplace(k, fields).first;
    if (it->second != fields) fail("one tuner key for two shapes", k + " <- " + fields + " / " + it->second);
  }
};

static std::string sw_name(const GemmSwitches& sw) {
  return fmt("engine=%d dma_uni=%d kpad=%d force=%d,%d,%d", sw.engine, sw.dma_uni, sw.kpad, sw.force_bm,
             sw.force_bn, sw.force_splits);
}

static std::string rows_fields(const IGemmArgs& a, int Ktot, bool bkc, bool split) {
  std::string s = fmt("%d|%d|%d|%d|%d|%d|%d|%d|%d|%d|%d|%d|%d|%d|%d|%d|%d|%d|%d", bkc, split, a.M, a.N,
                      Ktot, a.aH, a.aW, a.aC, a.oH, a.oW, a.Uh, a.Uw, a.Oh, a.Ow, a.T, a.stap, a.beta,
                      a.relu, a.nphase);
  for (int i = 0; i < a.nphase; ++i) s += fmt("|%d|%d", a.ph[i].M, a.ph[i].Ktot);
  return s;
}

// the tuner's candidates for a rows launch as tuned_tile filters them: the candidate rule,
// the tile honoured, the split slab inside the caller's workspace (that last filter is the
// limit itself, so for candidates check_rows' workspace test holds by construction; it is a
// real test for the untuned, forced-tile and forced-split plans)
static void sweep_rows_case(Sweep& S, const IGemmArgs& a, bool bkc, int vw, bool want_split,
                            const GemmSwitches& sw) {
  const bool allow = want_split && rows_ws_floats(a.M, a.N, a.Ktot, sw) > 0;
  const std::string where = fmt("rows M%d N%d aC%d T%d Ktot%d stap%d bkc%d vw%d split%d ", a.M, a.N, a.aC,
                                a.T, a.Ktot, a.stap, bkc, vw, allow) + sw_name(sw);
  ++S.plans;
  if (S.fail(check_rows(a, bkc, vw, allow, sw, TileSize{0, 0}), where)) return;
  const int kp = rows_kpad_ktot(a, bkc, vw, sw);
  S.key(rows_key(a, kp ? kp : a.Ktot, bkc, allow && !kp), rows_fields(a, kp ? kp : a.Ktot, bkc, allow && !kp));
  if (!rows_dma(vw, sw) || (sw.force_bm && sw.force_bn)) return;  // (the tuner does not run)
  const int64_t cap = allow && !kp ? rows_ws_floats(a.M, a.N, kp ? kp : a.Ktot, sw) : 0;
  for (const TileSize& c : kRowsCands) {
    if (!rows_cand_ok(c, a.N)) continue;
    const RowsLaunch p = plan_rows(a, bkc, vw, allow, sw, c);
    if (p.BM != c.bm || p.BN != c.bn) continue;
    if (p.splits > 1 && (int64_t)p.splits * a.M * a.N > cap) continue;
    ++S.plans;
    if (S.fail(check_rows(a, bkc, vw, allow, sw, c), where + fmt(" tile=%d,%d", c.bm, c.bn))) return;
  }
}

static IGemmArgs rows_args(int M, int N, int aC, int T, bool stap, bool bkc) {
  IGemmArgs a{};
  a.aH = 1; a.aW = M; a.aC = aC; a.oH = 1; a.oW = M; a.M = M;
  a.Uh = a.Uw = 1; a.T = T; a.Ktot = stap ? 32 * T : T * aC; a.N = N; a.RS = T;
  a.ldb = bkc ? a.Ktot : N; a.ldc = N; a.dH = 1; a.dW = M; a.Uoh = a.Uow = 1;
  a.stap = stap;
  return a;
}

static void sweep_rows(Sweep& S, const std::vector<GemmSwitches>& sws) {
  for (int M : SIZES)
  for (int N : COLS)
  for (int aC : CHANNELS)
  for (int T : TAPS)
  for (int bkc = 0; bkc < 2; ++bkc)
  for (int vw : {1, 4, 8}) {
    if (aC % vw != 0 || (vw > 1 && !bkc && N % vw != 0)) continue;
    for (int split = 0; split < 2; ++split)
      for (const GemmSwitches& sw : sws) {
        if (S.bad) return;
        sweep_rows_case(S, rows_args(M, N, aC, T, false, bkc != 0), bkc != 0, vw, split != 0, sw);
        if (aC == 8 && bkc && vw == 8 && sw.dma_uni && sw.engine >= 1)  // (igemm_stap_ok)
          sweep_rows_case(S, rows_args(M, N, aC, T, true, true), true, 8, split != 0, sw);
        if (vw == 8 && bkc && !split) {
          ++S.plans;
          if (S.fail(check_bnred(rows_args(M, N, aC, T, false, true), true, sw), "bnred " + sw_name(sw))) return;
        }
      }
  }
  // operands past 2^31 bytes (A: 4096 images of 512 x 512 x 64; B: 40000 x 40000): never
  // the uniform-tap kernel, so no padded K and no second source either
  for (const GemmSwitches& sw : sws) {
    IGemmArgs a = rows_args(512 * 512, 64, 64, 9, false, true);
    a.aH = a.oH = 512; a.aW = a.oW = 512; a.M = 4096 * 512 * 512;
    sweep_rows_case(S, a, true, 8, true, sw);
    a.aC = 48; a.Ktot = 9 * 48;
    sweep_rows_case(S, a, true, 8, true, sw);
    IGemmArgs b = rows_args(32, 40000, 40000, 1, false, true);
    sweep_rows_case(S, b, true, 8, true, sw);
    if (rows_dma(8, sw))
      S.fail(plan_rows(a, true, 8, false, sw, {0, 0}).family == RowsFamily::Dma ? nullptr : "2^31-byte A: generic kernel", sw_name(sw));
  }
}

// merged stride-phase launches: nphase 1, 4 and MAXPH phases of unequal size, K of one to
// four taps per phase
static void sweep_phases(Sweep& S, const std::vector<GemmSwitches>& sws) {
  for (int nphase : {1, 4, MAXPH})
  for (int M : SIZES)
  for (int N : COLS)
  for (int aC : {8, 32, 48, 64})
  for (int bkc = 0; bkc < 2; ++bkc) {
    IGemmArgs a = rows_args(M, N, aC, 0, false, bkc != 0);
    a.M = 0; a.oH = a.oW = 0; a.Ktot = 0; a.RS = 9; a.ldb = bkc ? 9 * aC : N; a.ldb2 = aC;
    a.nphase = nphase;
    int64_t pixels = 0;
    int tap0 = 0;
    for (int i = 0; i < nphase; ++i) {
      const int m = std::max(1, M - 37 * i), t = 1 + i % 4;
      a.ph[i] = PhaseDesc{m, 1, m, t * aC, tap0, t, 0, i, 0, FastDiv{}, FastDiv{}};
      tap0 = (tap0 + t) % 64;
      pixels += m;
    }
    for (const GemmSwitches& sw : sws) {
      if (S.bad) return;
      const std::string where = fmt("phases %d M%d N%d aC%d bkc%d ", nphase, M, N, aC, bkc) + sw_name(sw);
      ++S.plans;
      if (S.fail(check_phases(a, bkc != 0, pixels, sw, TileSize{0, 0}), where)) return;
      S.key(rows_key(a, a.Ktot, bkc != 0, false), rows_fields(a, a.Ktot, bkc != 0, false));
      if (!rows_dma(8, sw) || (sw.force_bm && sw.force_bn)) continue;
      for (const TileSize& c : kRowsCands) {
        if (!rows_cand_ok(c, a.N)) continue;
        const RowsLaunch p = plan_rows_phases(a, bkc != 0, sw, c);
        if (p.BM != c.bm || p.BN != c.bn || p.tiles_total <= 0) continue;
        ++S.plans;
        if (S.fail(check_phases(a, bkc != 0, pixels, sw, c), where + fmt(" tile=%d,%d", c.bm, c.bn))) return;
      }
    }
  }
}

// weight gradients: Kout x C x kernel x output grid x batch (Mpix below BK among them); the
// 1x1 kernel makes Ncols = C, so Ncols too takes 1, 7, 8, 31, 32, 33, 48, 80 and 96
static void sweep_wgrad(Sweep& S, const std::vector<GemmSwitches>& sws) {
  static const int KOUT[] = {1, 7, 8, 31, 32, 33, 48, 64, 80, 96, 128, 256, 512, 1000};
  static const int RS[][2] = {{1, 1}, {3, 3}, {7, 7}, {1, 7}, {7, 4}};
  static const int PQ[][2] = {{1, 1}, {1, 7}, {7, 7}, {17, 17}, {2, 40}, {56, 56}, {112, 112}, {512, 512}};
  for (int Kout : KOUT)
  for (int C : {1, 7, 8, 31, 32, 33, 48, 64, 80, 96})
  for (const auto& rs : RS)
  for (const auto& pq : PQ)
  for (int batch : {1, 3, 32, 512, 4096})
  for (int stride : {1, 2}) {
    const int64_t mpix = (int64_t)batch * pq[0] * pq[1];
    if (mpix >= (1ll << 31)) continue;
    const ConvShape q{batch, (pq[0] - 1) * stride + rs[0], (pq[1] - 1) * stride + rs[1], C, Kout, rs[0],
                      rs[1], stride, stride, 0, 0};
    const WGradArgs a = conv_wgrad_args(q, pq[0], pq[1], false);
    for (int vwa : {vec_width(Kout), 1})
      for (const GemmSwitches& sw : sws) {
        if (S.bad) return;
        const int vwb = C % 8 == 0 ? 8 : 1;
        const std::string where = fmt("wgrad K%d C%d %dx%d o%dx%d b%d s%d vwa%d ", Kout, C, rs[0], rs[1],
                                      pq[0], pq[1], batch, stride, vwa) + sw_name(sw);
        ++S.plans;
        if (S.fail(check_wgrad(a, vwa, vwb, sw, TileSize{0, 0}), where)) return;
        S.key(wgrad_key(a), fmt("%d|%d|%d|%d|%d|%d|%d|%d|%d|%d|%d|%d|%d|%d", a.Kout, a.Ncols, a.Mpix, a.H,
                                a.W, a.C, a.P, a.Q, a.R, a.S, a.sh, a.sw, a.ph, a.pw));
        if (!(vwa == 8 && vwb == 8 && sw.engine >= 1) || (sw.force_bm && sw.force_bn)) continue;
        const int64_t cap = wgrad_gemm_ws_floats(a.Kout, a.Ncols, a.Mpix, sw);
        for (const TileSize& c : kWgradCands) {
          if (!wgrad_cand_ok(c, a)) continue;
          const WGradLaunch p = plan_wgrad(a, vwa, vwb, sw, c);
          if (p.BM != c.bm || p.BN != c.bn) continue;
          if (p.splits > 1 && (int64_t)p.splits * a.Kout * a.Ncols > cap) continue;
          ++S.plans;
          if (S.fail(check_wgrad(a, vwa, vwb, sw, c), where + fmt(" tile=%d,%d", c.bm, c.bn))) return;
        }
      }
  }
}

// the tile tables: distinct rows, a wave grid that divides the tile into 16 x 16 fragments,
// the register tiles a subset of the LDS-DMA tiles, every candidate a tile
static const char* check_tables() {
  auto ok = [](const Tile* t, int n) {
    for (int i = 0; i < n; ++i) {
      if (t[i].bm % (16 * t[i].wm) || t[i].bn % (16 * t[i].wn) || t[i].block() > 512) return false;
      for (int j = 0; j < i; ++j)
        if (t[j].bm == t[i].bm && t[j].bn == t[i].bn) return false;
    }
    return true;
  };
  REQUIRE(ok(kRowsRegTiles, 3) && ok(kRowsDmaTiles, 6) && ok(kWgradRegTiles, 2) &&
          ok(kWgradDmaTiles, 5) && ok(kWgradIncTiles, 2));
  for (const Tile& t : kRowsRegTiles) REQUIRE(find_tile(kRowsDmaTiles, t.bm, t.bn) && t.block() == 256);
  for (const Tile& t : kWgradRegTiles) REQUIRE(find_tile(kWgradDmaTiles, t.bm, t.bn) && t.block() == 256);
  for (const Tile& t : kWgradIncTiles) REQUIRE(find_tile(kWgradDmaTiles, t.bm, t.bn) && t.block() == 256);
  for (const TileSize& c : kRowsCands) REQUIRE(find_tile(kRowsDmaTiles, c.bm, c.bn));
  for (const TileSize& c : kWgradCands) REQUIRE(find_tile(kWgradDmaTiles, c.bm, c.bn));
  for (const Tile& t : kRowsDmaTiles) REQUIRE(t.bm >= 128);  // slab_rows_max counts 128-row tiles
  return nullptr;
}

static int run_sweep() {
  Sweep S;
  const std::vector<GemmSwitches> sws = switch_configs();
  S.fail(check_tables(), "tile tables");
  if (!S.bad) sweep_rows(S, sws);
  if (!S.bad) sweep_phases(S, sws);
  if (!S.bad) sweep_wgrad(S, sws);
  if (S.bad) {
    printf("igemm_plan_check FAILED: %s\n  at %s\n", S.bad, S.where.c_str());
    return 1;
  }
  printf("igemm_plan_check sweep ok: %ld plans, %zu tuner keys\n", S.plans, S.keys.size());
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 1) return print_zoo();
  if (argc == 2 && !strcmp(argv[1], "sweep")) return run_sweep();
  Config cfg;
  for (int i = 1; i < argc; ++i) {
    int v[3] = {0, 0, 0};
    if (sscanf(argv[i], "engine=%d", &v[0]) == 1) cfg.sw.engine = std::min(2, std::max(0, v[0]));
    else if (sscanf(argv[i], "dma_uni=%d", &v[0]) == 1) cfg.sw.dma_uni = v[0] != 0;
    else if (sscanf(argv[i], "kpad=%d", &v[0]) == 1) cfg.sw.kpad = v[0] != 0;
    else if (sscanf(argv[i], "force=%d,%d,%d", &v[0], &v[1], &v[2]) == 3) {
      cfg.sw.force_bm = v[0]; cfg.sw.force_bn = v[1]; cfg.sw.force_splits = v[2];
    } else if (sscanf(argv[i], "tile=%d,%d", &v[0], &v[1]) == 2) cfg.tuned = TileSize{v[0], v[1]};
    else if (int r = print_shape(argv[i], cfg)) return r;
  }
  return 0;
}
