// CPU check of nattn_plan.h: sweeps maps and asserts what nattn.hip relies on.
//   g++ -std=c++17 -I csrc/kernels csrc/kernels/nattn_plan_check.cpp -o nattn_plan_check && ./nattn_plan_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nattn_plan.h"

using namespace mpa;

#define REQUIRE(c)                                                                             \
  do {                                                                                         \
    if (!(c)) {                                                                                \
      std::printf("FAILED %s (line %d): B %d H %d Hf %d Wf %d\n", #c, __LINE__, g.B, g.H, g.Hf, g.Wf); \
      std::exit(1);                                                                            \
    }                                                                                          \
  } while (0)

static int imin(int a, int b) { return a < b ? a : b; }

// one axis of length L: the ranges are separable, so every (query, key) pair of the definition
// is checked per axis.  `rows` selects the row roles (sub-tiles) or the column roles (slots).
static void check_axis(const NattnGeom& g, int L, bool rows) {
  const int tiles = (L + NA_TILE - 1) / NA_TILE;
  for (int i = 0; i < L; ++i) {  // the definition, and qlo / qhi against brute force
    const int s = nattn_ni(i, L);
    REQUIRE(s == (i - 3 < 0 ? 0 : (i - 3 > L - 7 ? L - 7 : i - 3)) && s >= 0 && s + NA_K <= L);
    int lo = L, hi = -1;
    for (int q = 0; q < L; ++q)
      if (nattn_in(q, i, L)) {
        lo = q < lo ? q : lo;
        hi = q > hi ? q : hi;
      }
    REQUIRE(lo == nattn_qlo(i, L) && hi == nattn_qhi(i, L));
    for (int q = lo; q <= hi; ++q) REQUIRE(nattn_in(q, i, L));  // the attending set is a range
  }
  REQUIRE(nattn_ni(L, L) == L - NA_K && nattn_ni(L + NA_TILE, L) == L - NA_K);  // past the map
  for (int t = 0; t < tiles; ++t) {
    // forward / dq: keys of the queries of a wave (rows: 2 of them; columns: the tile's 8)
    for (int w = 0; w < (rows ? 4 : 1); ++w) {
      const int q0 = NA_TILE * t + (rows ? 2 * w : 0), nq = rows ? 2 : NA_TILE;
      const int k0 = nattn_ni(q0, L), span = rows ? NA_SUB : NA_SLOTS;
      for (int q = q0; q < q0 + nq; ++q) {  // (queries past the map are computed too, clamped)
        const int qc = imin(q, L - 1), s = nattn_ni(qc, L);
        for (int k = s; k < s + NA_K; ++k) {
          REQUIRE(k - k0 >= 0 && k - k0 < span && k < L);
          const int rel = k - qc + NA_K - 1;
          REQUIRE(rel >= 0 && rel < NA_RPB);
        }
      }
    }
    // dkv: queries of the keys of a 4-wide patch; rows walk pairs whose count the block takes
    // from the longer of the tile's two patches
    int pairs = 0;
    for (int p = 0; p < 2; ++p) {
      const int ya = imin(NA_TILE * t + 4 * p, L - 1), yb = imin(NA_TILE * t + 4 * p + 3, L - 1);
      const int n = (nattn_qhi(yb, L) - nattn_qlo(ya, L) + 2) / 2;
      pairs = n > pairs ? n : pairs;
    }
    REQUIRE(2 * pairs <= NA_QROWS);
    for (int p = 0; p < 2; ++p) {
      const int K0 = NA_TILE * t + 4 * p, q0 = nattn_qlo(imin(K0, L - 1), L);
      for (int k = K0; k < K0 + 4 && k < L; ++k)
        for (int q = 0; q < L; ++q)
          if (nattn_in(q, k, L)) REQUIRE(q - q0 >= 0 && q - q0 < (rows ? 2 * pairs : NA_SLOTS));
    }
  }
}

static void check_geom(const NattnGeom& g) {
  REQUIRE(nattn_geom_error(g) == nullptr);
  const NattnPlan p = nattn_plan(g);
  REQUIRE(p.ty * NA_TILE >= g.Hf && (p.ty - 1) * NA_TILE < g.Hf && p.tx * NA_TILE >= g.Wf &&
          (p.tx - 1) * NA_TILE < g.Wf && p.tiles == p.ty * p.tx);
  // the walks cover every image once, none is empty; CUs first, then walks
  REQUIRE(p.bpw >= 1 && p.walks >= 1 && p.walks <= NA_MAX_WALKS && p.rows == p.walks * p.tiles);
  REQUIRE((p.walks - 1) * p.bpw < g.B && p.walks * p.bpw >= g.B);
  REQUIRE(p.bpw == 1 || p.walks == NA_MAX_WALKS || (int64_t)(p.walks - 1) * p.tiles * g.H < NA_FILL_BLOCKS);
  REQUIRE(p.delta_floats == (int64_t)g.B * g.H * g.Hf * g.Wf);
  REQUIRE(p.ws_floats == p.delta_floats + (int64_t)p.rows * g.H * NA_NB);
  REQUIRE(p.lds_fwd <= AT_LDS_LIMIT && p.lds_dq <= AT_LDS_LIMIT && p.lds_dkv <= AT_LDS_LIMIT);
  // both tilings (query rows 2 w + i / 8, key patches 4 x 4) cover every token exactly once
  std::vector<int> hq(g.Hf * g.Wf, 0), hk(g.Hf * g.Wf, 0);
  for (int t = 0; t < p.tiles; ++t)
    for (int w = 0; w < 4; ++w)
      for (int i = 0; i < 16; ++i) {
        const int ty = t / p.tx, tx = t - ty * p.tx;
        const int yq = NA_TILE * ty + 2 * w + (i >> 3), xq = NA_TILE * tx + (i & 7);
        if (yq < g.Hf && xq < g.Wf) ++hq[yq * g.Wf + xq];
        const int yk = NA_TILE * ty + 4 * (w >> 1) + (i >> 2), xk = NA_TILE * tx + 4 * (w & 1) + (i & 3);
        if (yk < g.Hf && xk < g.Wf) ++hk[yk * g.Wf + xk];
      }
  for (int n = 0; n < g.Hf * g.Wf; ++n) REQUIRE(hq[n] == 1 && hk[n] == 1);
  // every bias index of the definition, and the fold's slot of it, are in range
  for (int y = 0; y < g.Hf; ++y)
    for (int x = 0; x < g.Wf; ++x)
      for (int Y = nattn_ni(y, g.Hf); Y < nattn_ni(y, g.Hf) + NA_K; ++Y)
        for (int X = nattn_ni(x, g.Wf); X < nattn_ni(x, g.Wf) + NA_K; ++X) {
          const int rel = nattn_rel(y, x, Y, X);
          REQUIRE(rel >= 0 && rel < NA_NB);
          const int n = 16 * ((y % NA_TILE) / 2) + 8 * (y % 2) + x % NA_TILE;  // 16 wave + i
          REQUIRE(n == 8 * (y % NA_TILE) + x % NA_TILE);
          const int t = Y - nattn_ni(y / NA_TILE * NA_TILE + 2 * (n >> 4), g.Hf);
          const int c = X - nattn_ni(x / NA_TILE * NA_TILE, g.Wf);
          REQUIRE(t >= 0 && t < NA_SUB && c >= 0 && c < NA_SLOTS);
          REQUIRE((n * NA_FOLD_PITCH + 16 * t + c) * 4 + 4 <= NA_FOLD_BYTES);
        }
}

int main() {
  NattnGeom g{1, 1, 7, 7};
  // layout constants: a pair tile holds 32 rows of 32 positions, nattn_pos is a bijection onto
  // them and a 16-B fragment read stays inside a row; the fold tile lies below the bias floats
  std::vector<int> seen(32, 0);
  for (int a = 0; a < 2; ++a)
    for (int c = 0; c < NA_SLOTS; ++c) {
      REQUIRE(nattn_pos(a, c) >= 0 && nattn_pos(a, c) < 32);
      ++seen[nattn_pos(a, c)];
    }
  for (int v : seen) REQUIRE(v == 1);
  for (int lane = 0; lane < 64; ++lane)
    for (int dt = 0; dt < 2; ++dt) {
      const int row = 16 * dt + (lane & 15), col = 8 * (lane >> 4);
      REQUIRE(row < NA_D && col + 8 <= 32 && ((row * NA_PITCH + col) * 2) % 16 == 0);
      REQUIRE((row * NA_PITCH + col + 8) * 2 <= NA_PAIR_BYTES);
      REQUIRE(((lane & 15) * NA_PPITCH + 16 * dt + 4 * (lane >> 4) + 4) * 2 <= NA_PATCH_BYTES);
    }
  REQUIRE(NA_FWD_WAVE % 16 == 0 && NA_DQ_WAVE % 16 == 0 && NA_DKV_WAVE % 16 == 0);
  REQUIRE(NA_DQ_BYTES >= NA_FOLD_BYTES + NA_NB * 4 && NA_DQ_BYTES >= 4 * NA_DQ_WAVE + NA_NB * 4);
  REQUIRE(NA_RPB == 2 * NA_K - 1 && NA_NB == NA_RPB * NA_RPB && NA_HPB == 1);

  long n = 0;
  std::vector<int> sides;
  for (int L = 7; L <= 40; ++L) sides.push_back(L);
  sides.push_back(56);
  for (int L : sides) {
    g = NattnGeom{1, 1, L, L};
    check_axis(g, L, true);
    check_axis(g, L, false);
  }
  for (int Hf : sides)
    for (int Wf : sides) {
      g = NattnGeom{1 + (Hf + Wf) % 3, 1 + Hf % 4, Hf, Wf};
      check_geom(g);
      ++n;
    }
  // NAT-Mini's four levels at batch 256, and the test geometry with a 3-image walk
  const int st[5][6] = {{256, 2, 56, 49, 43, 6}, {256, 4, 28, 16, 32, 8}, {256, 8, 14, 4, 16, 16},
                        {256, 16, 7, 1, 16, 16}, {33, 2, 8, 1, 3, 11}};
  for (const auto& s : st) {
    g = NattnGeom{s[0], s[1], s[2], s[2]};
    check_geom(g);
    const NattnPlan p = nattn_plan(g);
    std::printf("B %d H %d map %d: tiles %d bpw %d walks %d\n", s[0], s[1], s[2], p.tiles, p.bpw, p.walks);
    REQUIRE(p.tiles == s[3] && p.bpw == s[4] && p.walks == s[5]);
  }
  const NattnGeom bad[] = {{1, 1, 6, 7}, {1, 1, 7, 6}, {0, 1, 7, 7}, {1, 0, 7, 7}, {65536, 1, 7, 7},
                           {1, 65536, 7, 7}, {4096, 16, 56, 56}};
  for (const NattnGeom& b : bad)
    if (!nattn_geom_error(b)) return std::printf("accepted a refused geometry\n"), 1;
  g = NattnGeom{1, 1, 7, 7};
  if (!nattn_geom_error(g, 64)) return std::printf("accepted head dim 64\n"), 1;
  std::printf("nattn_plan_check sweep ok: %ld plans\n", n);
  return 0;
}
