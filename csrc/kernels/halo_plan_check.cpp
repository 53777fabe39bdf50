// CPU check of the halo launch planner (halo_plan.h, planning the launches conv_args.h
// describes - the only project headers included; any host C++17 compiler, no GPU toolchain).
// Run by tests/test_halo_plan_cpu.py, plain and under AddressSanitizer +
// UndefinedBehaviorSanitizer.
//
//   halo_plan_check [key=value | fwd:... | wgrad:...] ...
//
// prints one line per shape - the kernel instance with every template argument, grid, block
// and the plan's scalar fields - for the model zoo's 3x3 / stride-1 layers (no shape
// arguments) or for the given shapes:
//   fwd:B,H,W,C,N,MODE,FLAVOUR,WIDE   MODE same | valid | valid_dgrad | same_dgrad; H x W is
//                                     the conv's input image, C / N the GEMM's K and N
//                                     channels; FLAVOUR see FLAVOURS; WIDE 1: ldc = N + 64
//   wgrad:B,H,W,C,K,PAD
//   halo= trim= wres= mi7= wxmap= wprod= strip= cus=   switches / CU count for what follows
// and `sweep` walks a grid of shapes, switches and CU counts and checks every plan against
// the limits the kernels state (see check_fwd / check_wgrad); the first violation is printed
// with its shape and the exit status is 1.  `geometry`: see print_geometry.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "conv_args.h"
#include "halo_plan.h"

using namespace mpa;

static const char* const MODES[] = {"same", "valid", "valid_dgrad", "same_dgrad"};
// the six flavours halo_epi accepts, then three it rejects
static const char* const FLAVOURS[] = {"plain", "acc", "stats", "bias_relu", "bias_stats",
                                       "bnred", "relu", "bias", "bnred_y"};
constexpr int NMODE = 4, NFLAVOUR = 9;

struct FwdCase {
  int batch, H, W, c, n, mode, flavour, wide;
};
struct WCase {
  int batch, H, W, c, k, pad;
};

template <class T>
static T* some() {  // a non-null operand (the planner only tests presence)
  return reinterpret_cast<T*>(16);
}

// the launch the binding layer builds for the case; false: no such conv (valid, image < 3)
static bool make_fwd(const FwdCase& q, IGemmArgs& a) {
  const bool valid = q.mode == 1 || q.mode == 2, dgrad = q.mode >= 2;
  const int pad = valid ? 0 : 1;
  const int P = conv_out_extent(q.H, 3, 1, pad), Q = conv_out_extent(q.W, 3, 1, pad);
  a = IGemmArgs{};
  if (P <= 0 || Q <= 0) return false;
  // (the GEMM's K channels c are the conv's input channels, or dy's for the dgrad from the
  // transposed weight)
  bool empty;
  if (dgrad) conv_dgrad_args({q.batch, q.H, q.W, q.n, q.c, 3, 3, 1, 1, pad, pad}, P, Q, true,
                             nullptr, a, empty);
  else conv_fwd_args({q.batch, q.H, q.W, q.c, q.n, 3, 3, 1, 1, pad, pad}, false, a);
  a.A = some<const bf16_raw>();
  a.B = some<const bf16_raw>();
  a.C = some<void>();
  a.ldc = q.n + (q.wide ? 64 : 0);
  switch (q.flavour) {
    case 1: a.beta = 1; break;
    case 2: a.stats = some<float>(); break;
    case 3: a.bias = some<const float>(); a.relu = 1; break;
    case 4: a.bias = some<const float>(); a.stats = some<float>(); break;
    case 5: case 8:
      a.ep_bnred = 1;
      a.stats = a.stats_sums = some<float>();
      a.ep_z = some<const bf16_raw>();
      a.ep_mean = a.ep_rstd = a.ep_gamma = a.ep_beta = some<const float>();
      if (q.flavour == 8) a.ep_y = some<const bf16_raw>();
      break;
    case 6: a.relu = 1; break;
    case 7: a.bias = some<const float>(); break;
    default: break;
  }
  return true;
}

static bool make_wgrad(const WCase& q, WGradArgs& a) {
  a = conv_wgrad_args({q.batch, q.H, q.W, q.c, q.k, 3, 3, 1, 1, q.pad, q.pad},
                      conv_out_extent(q.H, 3, 1, q.pad), conv_out_extent(q.W, 3, 1, q.pad), false);
  a.dy = a.x = some<const bf16_raw>();
  a.dw = a.slab = some<float>();
  return a.P > 0 && a.Q > 0;
}

// ------------------------------------------------------------------------ printing
static const char* tf(bool b) { return b ? "true" : "false"; }

static std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
static std::string fmt(const char* f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

static std::string kernel_name(const HaloLaunch& L) {
  switch (L.kind) {
    case HaloKind::None: return "none";
    case HaloKind::Strip:
      return fmt("conv3_strip_kernel<%s, %d, %d, %d>", tf(L.wres), L.epi, L.ns, L.nj);
    default:
      return fmt("conv3_halo_kernel<%s, %d, %s, %d, %d>", tf(L.wres), L.epi, tf(L.full), L.nj,
                 L.kind == HaloKind::Linear448 ? 7 : 4);
  }
}

static std::string kernel_name(const HaloWLaunch& L) {
  if (L.kind == HaloWKind::None) return "none";
  return fmt("conv3_halo_wgrad_kernel<%d, %s, %s, %s, %d, %d>", L.w2t,
             tf(L.kind == HaloWKind::OneChunk), tf(L.kind == HaloWKind::Strip), tf(L.prod), L.km,
             L.ht);
}

static std::string describe(const FwdCase& q) {
  return fmt("fwd b%d %dx%d c%d n%d %s %s ldc%d", q.batch, q.H, q.W, q.c, q.n, MODES[q.mode],
             FLAVOURS[q.flavour], q.n + (q.wide ? 64 : 0));
}
static std::string describe(const WCase& q) {
  return fmt("wgrad b%d %dx%d c%d k%d pad%d", q.batch, q.H, q.W, q.c, q.k, q.pad);
}

// kernel, grid, block and the plan's scalar fields (name: the instance, however obtained)
static std::string line(const std::string& name, const HaloLaunch& L) {
  if (L.kind == HaloKind::None) return name;
  std::string s = fmt("%s grid %d block %d tiles_n %d tiles_total %d |", name.c_str(), L.grid,
                      L.threads, L.tiles_n, L.tiles_total);
  if (L.kind == HaloKind::Strip) {
    const StripPlan& h = L.strip;
    return s + fmt(" tr %d tw %d p %d hiw %d tiles_c %d tiles_img %d tiles_total %d cc %d "
                   "ch %d cw %d a_bytes %u b_bytes %u",
                   h.tr, h.tw, h.p, h.hiw, h.tiles_c, h.tiles_img, h.tiles_total, h.cc, h.ch,
                   h.cw, h.a_bytes, h.b_bytes);
  }
  const HaloPlan& h = L.lin;
  return s + fmt(" w2 %d hiw %d tiles_m %d tiles_total %d cc %d a_bytes %u b_bytes %u", h.w2,
                 h.hiw, h.tiles_m, h.tiles_total, h.cc, h.a_bytes, h.b_bytes);
}

static std::string line(const std::string& name, const HaloWLaunch& L) {
  if (L.kind == HaloWKind::None) return name;
  const HaloWPlan& h = L.plan;
  return fmt("%s grid %d block %d | w2 %d tiles_m %d parts %d kparts %d Z %d xmap %d tr %d "
             "tw %d tiles_c %d tiles_img %d dy_bytes %u x_bytes %u",
             name.c_str(), L.grid, L.threads, h.w2, h.tiles_m, h.parts, h.kparts, h.Z, h.xmap,
             h.tr, h.tw, h.tiles_c, h.tiles_img, h.dy_bytes, h.x_bytes);
}

// ------------------------------------------------------------------------ limits
constexpr int LDS_CU = 160 * 1024;  // LDS of a gfx950 CU (conv3_halo_kernel's budget assert)

#define REQUIRE(cond)          \
  do {                         \
    if (!(cond)) return #cond; \
  } while (0)

// what conv3_halo_kernel / conv3_strip_kernel state about their launch (comments and
// static_asserts of conv_halo.hip); null: all hold
static const char* check_fwd(const IGemmArgs& a, const HaloSwitches& sw, const HaloLaunch& L) {
  const int epi = halo_epi(a);
  if (L.kind == HaloKind::None) return nullptr;
  REQUIRE(sw.halo && epi >= 0 && L.epi == epi);
  const bool strip = L.kind == HaloKind::Strip, mi7 = L.kind == HaloKind::Linear448;
  // instantiated combinations
  REQUIRE(a.N == 32 ? L.nj == 2 : (L.nj == 4 && a.N % 64 == 0));
  REQUIRE(L.nj == 4 || epi == 0 || epi == EP_STATS || (strip && (epi == EP_BETA || epi == EP_BNRED)));
  REQUIRE(!mi7 || (L.wres && L.full && L.nj == 4 && (epi == 0 || epi == EP_STATS)));
  REQUIRE(strip ? (L.ns == 2 || (L.ns == 3 && L.wres)) && !L.full : L.ns == 0);
  REQUIRE(!L.wres || (sw.wres && a.N <= 64 && a.aC <= 64));  // one resident 64 x 9 x C tile
  REQUIRE(L.threads == (mi7 ? 256 : 512));
  // persistent grid: one statistics-slab row per block, whole XCDs, a fixed column tile
  REQUIRE(L.grid > 0 && L.grid <= HALO_MAX_ROWS && L.grid % 8 == 0);
  REQUIRE(L.tiles_n == (a.N + 63) / 64 && L.grid % L.tiles_n == 0);
  // 32-bit offsets
  const int64_t nimg = a.M / ((int64_t)a.oH * a.oW);
  const int64_t a_bytes = nimg * a.aH * a.aW * a.aC * 2, b_bytes = (int64_t)a.N * a.ldb * 2;
  REQUIRE(a_bytes < (1ll << 31) && b_bytes < (1ll << 31) && (int64_t)a.M * a.ldc < (1ll << 31));
  if (strip) {
    const StripPlan& h = L.strip;
    REQUIRE(h.a_bytes == a_bytes && h.b_bytes == b_bytes && h.cc == a.aC / 32);
    REQUIRE(h.hiw >= 1 && h.hiw <= HB_HIW && (h.tr + 2) * h.p <= 64 * h.hiw && h.tw + 2 <= h.p);
    REQUIRE(h.p % 8 == 0 && h.tr >= 1 && h.tr * h.tw <= HB_BM && 2 * h.tr * h.tw >= HB_BM);
    REQUIRE(L.ns * h.hiw * 4096 + (L.wres ? h.cc : L.ns) * HB_WBYTES <= 2 * HB_HBYTES + 2 * HB_WBYTES);
    REQUIRE(h.tiles_c * h.tw >= a.oW && (h.tiles_c - 1) * h.tw < a.oW);
    REQUIRE(h.tiles_img == (a.oH + h.tr - 1) / h.tr * h.tiles_c);
    REQUIRE(h.tiles_total == nimg * h.tiles_img * L.tiles_n && L.tiles_total == h.tiles_total);
    REQUIRE(a.oH == a.aH - 2 * h.ch && a.oW == a.aW - 2 * h.cw);
    return nullptr;
  }
  const HaloPlan& h = L.lin;
  const int BM = mi7 ? HB_BM7 : HB_BM;
  const int64_t HW = (int64_t)a.aH * a.aW, need = halo_need(HB_BM, a.aH, a.aW, h.w2);
  REQUIRE(h.a_bytes == a_bytes && h.b_bytes == b_bytes && h.cc == a.aC / 32);
  REQUIRE(a.oH == a.aH && a.oW == a.aW && h.w2 == halo_pitch(a.aW) && h.w2 % 8 == 0);
  REQUIRE(HW + HB_BM < 65536 && a.aW + 2 <= 255);
  REQUIRE(need <= HB_HPX && h.hiw >= 1 && h.hiw <= HB_HIW);  // the stage holds the halo ...
  REQUIRE(h.hiw == HB_HIW || (sw.trim && 64 * h.hiw >= need));  // ... and the fetch covers it
  REQUIRE(!mi7 || (HW % HB_BM7 == 0 && HB_BM7 % a.aW == 0 && a.M % HB_BM7 == 0 &&
                   (HB_BM7 / a.aW + 2) * h.w2 <= HB_HPX7));
  // LDS: two halo stages of what the plan fetches (448-pixel tiles: their whole-row halo,
  // inside a CU's LDS), two weight stages that also hold the resident tile, the epilogue
  const int halo_bytes = mi7 ? (HB_BM7 / a.aW + 2) * h.w2 * 64 : h.hiw * 4 * 16 * 64;
  REQUIRE(2 * halo_bytes + 2 * HB_WBYTES + HB_RED + HB_COLS <= (mi7 ? LDS_CU : HB_LDS));
  REQUIRE(!L.wres || h.cc * HB_WBYTES <= 2 * HB_WBYTES);
  REQUIRE(h.tiles_m == (a.M + BM - 1) / BM && (!L.full || a.M % BM == 0));
  REQUIRE(h.tiles_total == h.tiles_m * L.tiles_n && L.tiles_total == h.tiles_total);
  return nullptr;
}

// what conv3_halo_wgrad_kernel states about its launch.  Its grid is Z blocks for each of
// `parts` partitions - any count up to HALO_MAX_ROWS; a multiple of 8 only where the plan
// asks for the XCD-grouped block order.
static const char* check_wgrad(const WGradArgs& a, const HaloSwitches& sw, const HaloWLaunch& L) {
  if (L.kind == HaloWKind::None) return nullptr;
  const HaloWPlan& h = L.plan;
  const bool strip = L.kind == HaloWKind::Strip, rr = L.kind == HaloWKind::Linear && !L.prod;
  REQUIRE(sw.halo && a.C % 32 == 0 && a.Kout % 32 == 0);
  // instantiated combinations
  REQUIRE(L.prod ? sw.wprod && !strip && L.w2t == 0 : (L.w2t == 0 || (rr && L.w2t == h.w2)));
  REQUIRE(L.w2t == 0 || L.w2t == 16 || L.w2t == 32 || L.w2t == 48 || L.w2t == 64);
  REQUIRE(L.km == 4 || (L.km == 2 && L.prod && a.Kout == 32));
  REQUIRE(L.ht == HW_HIW || (rr && sw.trim && ((L.w2t == 16 && L.ht == 4) || (L.w2t == 32 && L.ht == 5))));
  REQUIRE(L.threads == (L.prod ? 512 : 256));
  REQUIRE(h.kparts == (a.Kout + 63) / 64 && h.parts == h.kparts * ((a.C + 63) / 64));
  REQUIRE(h.Z >= 1 && h.Z <= h.tiles_m && L.grid == h.parts * h.Z && L.grid <= HALO_MAX_ROWS);
  REQUIRE(!h.xmap || (sw.wxmap && L.grid % 8 == 0));
  const int64_t nimg = a.Mpix / ((int64_t)a.P * a.Q);
  const int64_t dy_bytes = (int64_t)a.Mpix * a.Kout * 2, x_bytes = nimg * a.H * a.W * a.C * 2;
  REQUIRE(dy_bytes < (1ll << 31) && x_bytes < (1ll << 31));
  REQUIRE(h.dy_bytes == dy_bytes && h.x_bytes == x_bytes && h.w2 % 16 == 0);
  // LDS: two stages of a dy tile and the halo pixels the plan stages for the two chunks
  const int64_t halo_px = strip ? (int64_t)(h.tr + 2) * h.w2
                          : L.kind == HaloWKind::OneChunk ? (halo_need(HW_BM, a.H, a.W, h.w2) + 1) / 2
                                                          : L.ht * 4 * 16;
  REQUIRE(2 * (HW_DBYTES + 2 * halo_px * 64) <= HW_LDS);
  if (strip) {
    REQUIRE(sw.strip >= 1 && h.tr >= 1 && h.tw >= 8 && h.tr * h.tw <= HW_BM && h.tw + 2 <= h.w2);
    REQUIRE((h.tr + 2) * h.w2 <= HW_HPX);  // the strip's halo fits one chunk's stage
    REQUIRE(h.tiles_c * h.tw >= a.Q && (h.tiles_c - 1) * h.tw < a.Q);
    REQUIRE(h.tiles_img == (a.P + h.tr - 1) / h.tr * h.tiles_c && h.tiles_m == nimg * h.tiles_img);
    return nullptr;
  }
  const int64_t need = halo_need(HW_BM, a.H, a.W, h.w2);
  REQUIRE(a.ph == 1 && a.pw == 1 && h.w2 == halo_wgrad_pitch(a.W));
  REQUIRE((int64_t)a.H * a.W + HW_BM < 65536 && a.W + 2 <= 255);
  REQUIRE(h.tiles_m == (a.Mpix + HW_BM - 1) / HW_BM);
  if (L.kind == HaloWKind::OneChunk)  // both chunk areas hold one chunk's wider halo
    REQUIRE(a.C == 32 && need > HW_HPX && need <= 2 * HW_HPX);
  else
    REQUIRE(need <= HW_HPX && 64 * L.ht >= need);  // HT DMAs x 4 waves x 16 slots
  return nullptr;
}

// ------------------------------------------------------------------------ sweep
// default switches, then each switch flipped alone (the strip mode to both other values)
constexpr int NSWITCH = 9;
static HaloSwitches switch_config(int i) {
  HaloSwitches sw;
  switch (i) {
    case 1: sw.halo = false; break;
    case 2: sw.trim = false; break;
    case 3: sw.wres = false; break;
    case 4: sw.mi7 = false; break;
    case 5: sw.wxmap = false; break;
    case 6: sw.wprod = false; break;
    case 7: sw.strip = 0; break;
    case 8: sw.strip = 2; break;
    default: break;
  }
  return sw;
}

// image sizes: every square 1..64 and the zoo's larger ones, and a few non-square pairs
template <class F>
static void for_sizes(F&& f) {
  static const int big[] = {71, 73, 112, 147, 149, 224, 255, 256, 300};
  static const int pairs[][2] = {{56, 28}, {28, 56}, {7, 64}, {64, 7},  {224, 112}, {35, 17},
                                 {147, 73}, {8, 300}, {300, 8}, {3, 255}, {13, 9}};
  for (int s = 1; s <= 64; ++s) f(s, s);
  for (int s : big) f(s, s);
  for (const auto& p : pairs) f(p[0], p[1]);
}

static const int BATCHES[] = {1, 2, 3, 32}, NS[] = {32, 64, 96, 128, 192, 512};

// A fixed pseudo-random bit stream (an LCG): the CU count and the channel window of a case
// are drawn from it, so neither is tied to a position in the loops.
struct Bits {
  uint32_t r = 12345u;
  int next() { return (int)((r = r * 1664525u + 1013904223u) >> 31); }
};

// f(case, switch config index, switches, cus): the full product of sizes, batches, N, tap
// sets, flavours, the sixteen channel counts and the switch configs; CU count and channel
// window by coin flip (each size x batch repeats every other combination, 332 times)
template <class F>
static void sweep_fwd(F&& f) {
  Bits bits;
  for_sizes([&](int H, int W) {
    for (int b : BATCHES)
      for (int n : NS)
        for (int mode = 0; mode < 3; ++mode)  // (same_dgrad is `same` with the taps reversed)
          for (int fl = 0; fl < NFLAVOUR; ++fl)
            for (int c = 32; c <= 512; c += 32)
              for (int i = 0; i < NSWITCH; ++i) {
                const int wide = bits.next(), cus = bits.next() ? 224 : 256;
                f(FwdCase{b, H, W, c, n, mode, fl, wide}, i, switch_config(i), cus);
              }
  });
}

template <class F>
static void sweep_wgrad(F&& f) {
  Bits bits;
  for_sizes([&](int H, int W) {
    for (int b : BATCHES)
      for (int kout : NS)
        for (int c = 32; c <= 512; c += 32)
          for (int pad = 0; pad < 2; ++pad)
            for (int i = 0; i < NSWITCH; ++i)
              f(WCase{b, H, W, c, kout, pad}, i, switch_config(i), bits.next() ? 224 : 256);
  });
}

static int run_sweep() {
  long plans = 0, taken = 0;
  const char* bad = nullptr;
  std::string where;
  sweep_fwd([&](const FwdCase& q, int, const HaloSwitches& sw, int cus) {
    IGemmArgs a;
    if (bad || !make_fwd(q, a)) return;
    const HaloLaunch L = plan_halo(a, sw, cus);
    ++plans;
    taken += L.kind != HaloKind::None;
    if ((bad = check_fwd(a, sw, L))) where = describe(q) + " cus " + std::to_string(cus);
  });
  sweep_wgrad([&](const WCase& q, int, const HaloSwitches& sw, int cus) {
    WGradArgs a;
    if (bad || !make_wgrad(q, a)) return;
    const HaloWLaunch L = plan_halo_wgrad(a, sw, cus);
    ++plans;
    taken += L.kind != HaloWKind::None;
    if ((bad = check_wgrad(a, sw, L))) where = describe(q) + " cus " + std::to_string(cus);
  });
  if (bad) {
    printf("halo_plan_check FAILED: %s\n  at %s\n", bad, where.c_str());
    return 1;
  }
  printf("halo_plan_check sweep ok: %ld plans, %ld on the halo engine\n", plans, taken);
  return 0;
}

// ------------------------------------------------------------------------ the model zoo
static void print_fwd(const FwdCase& q, const HaloSwitches& sw, int cus) {
  IGemmArgs a;
  if (!make_fwd(q, a)) { printf("%s : no such conv\n", describe(q).c_str()); return; }
  const HaloLaunch L = plan_halo(a, sw, cus);
  printf("%s : %s\n", describe(q).c_str(), line(kernel_name(L), L).c_str());
}
static void print_wgrad(const WCase& q, const HaloSwitches& sw, int cus) {
  WGradArgs a;
  if (!make_wgrad(q, a)) { printf("%s : no such conv\n", describe(q).c_str()); return; }
  const HaloWLaunch L = plan_halo_wgrad(a, sw, cus);
  printf("%s : %s\n", describe(q).c_str(), line(kernel_name(L), L).c_str());
}

// f(fwd case) / g(wgrad case) over the zoo's 3x3 / stride-1 layers
template <class F, class G>
static void zoo(F&& f, G&& g) {
  // ResNet: forward with statistics, plain / accumulate / BN-link dgrad, weight gradient;
  // batch 32 and a batch whose last 256-pixel tile is a tail
  static const int resnet[][2] = {{56, 64}, {28, 128}, {14, 256}, {7, 512}};
  for (const auto& l : resnet)
    for (int b : {32, 3}) {
      f(FwdCase{b, l[0], l[0], l[1], l[1], 0, 2, 0});
      for (int fl : {0, 1, 5}) f(FwdCase{b, l[0], l[0], l[1], l[1], 3, fl, 0});
      g(WCase{b, l[0], l[0], l[1], l[1], 1});
    }
  // VGG: forward with bias + ReLU, weight gradient
  f(FwdCase{32, 224, 224, 64, 64, 0, 3, 0});
  g(WCase{32, 224, 224, 64, 64, 1});
  f(FwdCase{32, 112, 112, 128, 128, 0, 3, 0});
  g(WCase{32, 112, 112, 128, 128, 1});
  // DenseNet: growth-rate convs (128 -> 32 into a channel window), Kout == 32 weight gradient
  for (int s : {56, 7}) {
    f(FwdCase{32, s, s, 128, 32, 0, 0, 1});
    g(WCase{32, s, s, 128, 32, 1});
  }
  // Inception: the valid 149 -> 147 conv, the 147 x 147 same conv with C == 32, one 35 x 35
  f(FwdCase{32, 149, 149, 32, 32, 1, 2, 0});
  f(FwdCase{32, 149, 149, 32, 32, 2, 0, 0});
  g(WCase{32, 149, 149, 32, 32, 0});
  f(FwdCase{32, 147, 147, 32, 64, 0, 2, 0});
  f(FwdCase{32, 147, 147, 64, 32, 3, 0, 0});
  g(WCase{32, 147, 147, 32, 64, 1});
  f(FwdCase{32, 35, 35, 96, 96, 0, 2, 0});
  f(FwdCase{32, 35, 35, 96, 96, 3, 0, 0});
  g(WCase{32, 35, 35, 96, 96, 1});
}

// the linear tiles' geometry for H, W in 1..64, one line each (tools/halo_index_check.py
// emulates these; the test compares): pitch, halo_need and DMA count of the 256-pixel
// forward / dgrad tiles, then of the 128-pixel weight-gradient tiles, then the
// weight gradient's instantiated count
static void print_geometry() {
  for (int H = 1; H <= 64; ++H)
    for (int W = 1; W <= 64; ++W) {
      const int pf = halo_pitch(W), pw = halo_wgrad_pitch(W);
      const int64_t nf = halo_need(HB_BM, H, W, pf), nw = halo_need(HW_BM, H, W, pw);
      printf("%d %d %d %lld %d %d %lld %d %d\n", H, W, pf, (long long)nf,
             halo_dma_count(nf, HB_HIW, true), pw, (long long)nw,
             halo_dma_count(nw, HW_HIW, true), halo_wgrad_dma_count(H, W, true));
    }
}

static int find(const char* const* names, int n, const char* s) {
  for (int i = 0; i < n; ++i)
    if (!strcmp(names[i], s)) return i;
  return -1;
}

int main(int argc, char** argv) {
  HaloSwitches sw;
  int cus = 256, shapes = 0;
  for (int i = 1; i < argc; ++i) {
    const char* s = argv[i];
    int v[6];
    char m[32], fl[32];
    if (!strcmp(s, "sweep")) return run_sweep();
    if (!strcmp(s, "geometry")) return print_geometry(), 0;
    if (sscanf(s, "fwd:%d,%d,%d,%d,%d,%31[^,],%31[^,],%d", v, v + 1, v + 2, v + 3, v + 4, m, fl,
               v + 5) == 8 &&
        find(MODES, NMODE, m) >= 0 && find(FLAVOURS, NFLAVOUR, fl) >= 0) {
      print_fwd(FwdCase{v[0], v[1], v[2], v[3], v[4], find(MODES, NMODE, m),
                        find(FLAVOURS, NFLAVOUR, fl), v[5]}, sw, cus);
      ++shapes;
    } else if (sscanf(s, "wgrad:%d,%d,%d,%d,%d,%d", v, v + 1, v + 2, v + 3, v + 4, v + 5) == 6) {
      print_wgrad(WCase{v[0], v[1], v[2], v[3], v[4], v[5]}, sw, cus);
      ++shapes;
    } else if (sscanf(s, "halo=%d", v) == 1) sw.halo = v[0] != 0;
    else if (sscanf(s, "trim=%d", v) == 1) sw.trim = v[0] != 0;
    else if (sscanf(s, "wres=%d", v) == 1) sw.wres = v[0] != 0;
    else if (sscanf(s, "mi7=%d", v) == 1) sw.mi7 = v[0] != 0;
    else if (sscanf(s, "wxmap=%d", v) == 1) sw.wxmap = v[0] != 0;
    else if (sscanf(s, "wprod=%d", v) == 1) sw.wprod = v[0] != 0;
    else if (sscanf(s, "strip=%d", v) == 1) sw.strip = v[0];
    else if (sscanf(s, "cus=%d", v) == 1) cus = v[0];
    else {
      fprintf(stderr, "halo_plan_check: cannot read '%s'\n", s);
      return 2;
    }
  }
  if (!shapes)
    zoo([&](const FwdCase& q) { print_fwd(q, sw, cus); },
        [&](const WCase& q) { print_wgrad(q, sw, cus); });
  return 0;
}
