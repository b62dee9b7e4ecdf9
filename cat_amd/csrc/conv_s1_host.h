// Host side of the one-launch stage-1 entries (conv_pk.hip, conv_s1ws.hip, conv_s1w7.hip, conv_s1ws7.hip, conv_s1n7.hip; the table of
// entries: docs/CONV_VARIANTS.md, "Stage 1 in one launch"): the argument checks, the common kernel-argument fields, the grid and the FLOP
// count, templated on the kernel-argument struct A and the geometry struct G.  Every helper returns 0 or -22 with the error set; `what`
// is the entry's message prefix.  Slot k of NS convolves with kernel size slot_ks(NS, k): 5 3 1 or 7 5 3 1.
#pragma once
#include "common.h"
#include "conv_pk_tile.h"

namespace cat_s1 {

constexpr int TW = 16;      // output tile = cat_pk::TH x TW pixels
constexpr int slot_ks(int ns, int k) { return 2 * (ns - 1 - k) + 1; }

// ---- width domains of the wide kernels (one instantiation each)
inline bool tiles3(int w) { return w > 32 && w <= 48; }      // 3 N tiles: a wide slot at m = 42
inline bool wide_531(int w5, int w3, int w1) { return tiles3(w5) && tiles3(w3) && w1 > 160 && w1 <= 176; }      // 3 + 3 + 11 tiles
inline bool wide_7531(int w7, int w5, int w3, int w1) {      // 3 + 3 + 3 + 9 tiles (three depthwise branches)
  return tiles3(w7) && tiles3(w5) && tiles3(w3) && w1 > 128 && w1 <= 144;
}

// 2 * pixels * cin * sum_k nvalid[k] * ks^2
template <int NS, class G>
double flops(const G* g) {
  double kflops = 0.0;
  for (int k = 0; k < NS; ++k) kflops += (double)g->nvalid[k] * slot_ks(NS, k) * slot_ks(NS, k);
  return 2.0 * (double)g->N * g->H * g->W * g->cin * kflops;
}

// Input checks (geometry, 32-bit element offsets, a mirrored kmax x kmax window inside the plane) and the fields every kernel reads:
// x, xcs, c4, N, H, W, reflect, tiles_x, tiles.  *grid = workgroups.
template <class A, class G>
int input(A& a, const G* g, const float* x, int kmax, const char* what, int* grid) {
  CAT_REQUIRE(g->N > 0 && g->H > 0 && g->W > 0 && g->cin > 0 && (g->xcs & 3) == 0 && g->xcs >= g->cin, "%s: bad input geometry", what);
  CAT_REQUIRE((int64_t)g->N * g->H * g->W * g->xcs < (int64_t)4294967295LL, "%s: source larger than 2^32 elements", what);
  CAT_REQUIRE(!g->reflect || (kmax <= g->H && kmax <= g->W), "%s: reflect padding wider than the plane", what);
  a.x = x; a.xcs = g->xcs; a.c4 = (g->cin + 3) & ~3; a.N = g->N; a.H = g->H; a.W = g->W; a.reflect = g->reflect;
  a.tiles_x = cat::cdiv(g->W, TW);
  a.tiles = a.tiles_x * cat::cdiv(g->H, cat_pk::TH);
  const int64_t n = (int64_t)g->N * a.tiles;
  CAT_REQUIRE(n < (int64_t)2147483647, "%s: grid too large", what);      // implied by the element check: xcs >= 4, so N * H * W < 2^30 >= n
  *grid = (int)n;
  return 0;
}

// The (8 + 2 hl) x (16 + 2 hl) patch of the 5 3 1 kernels, whose arguments carry it; returns the LDS bytes of two tiles + the A-offset tables.
template <class A>
size_t patch(A& a, int hl) {
  a.hl = hl; a.tr = cat_pk::TH + 2 * hl; a.tc = TW + 2 * hl;
  return (size_t)2 * a.tr * a.tc * cat_pk::PITCH * sizeof(float) + 6 * cat_pk::TABN * sizeof(int);
}

// Column-slice contract: slot k writes columns [col0, col0 + width) of ys[k] (pixel stride ycs[k]; the same buffer for every slot in a
// forward) and, with `stats`, of the statistics table.  Fills pack, col0, width.
template <int NS, class A, class G>
int slices(A& a, const G* g, const float* const* packs, float* const* ys, const int* ycs, const float* stats, const char* what) {
  for (int k = 0; k < NS; ++k) {
    CAT_REQUIRE(packs[k] && ys[k] && (ycs[k] & 3) == 0 && g->col0[k] >= 0 && g->col0[k] + g->width[k] <= ycs[k] &&
                    (!stats || g->col0[k] + g->width[k] <= g->scs) && g->nvalid[k] <= g->width[k],
                "%s: slice %d", what, k);
    a.pack[k] = packs[k]; a.col0[k] = g->col0[k]; a.width[k] = g->width[k];
  }
  return 0;
}

// Buffer-per-slot contract: y_k = act(conv_k(x) + bias_k) into ys[k] with pixel stride g->ycs[k] (at most ycs_max[k] where given).  Fills
// pack, bias, y, ycs, nvalid, act, slope.
template <int NS, class A, class G>
int buffers(A& a, const G* g, const float* x, const float* const* packs, const float* const* biases, float* const* ys, const int* ycs_max,
            const char* what) {
  CAT_REQUIRE(x && packs && ys, "%s: null argument", what);
  for (int k = 0; k < NS; ++k) {
    CAT_REQUIRE(packs[k] && ys[k] && (g->ycs[k] & 3) == 0 && g->ycs[k] >= g->nvalid[k] && (!ycs_max || g->ycs[k] <= ycs_max[k]), "%s: slot %d",
                what, k);
    a.pack[k] = packs[k]; a.bias[k] = biases ? biases[k] : nullptr; a.y[k] = ys[k]; a.ycs[k] = g->ycs[k]; a.nvalid[k] = g->nvalid[k];
  }
  a.act = g->act; a.slope = g->slope;
  return 0;
}

}  // namespace cat_s1
