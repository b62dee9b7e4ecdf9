// cat_tstage1ws_fwd: the wide 5 3 1 stage 1 with statistics (the entries side by side: docs/CONV_VARIANTS.md, "Stage 1 in one launch").
// The main loop of tstage1w_kernel<3, 3, 11> (conv_pk_s1w_main.h) with the output contract of cat_tstage1_fwd.
//
// Statistics (conv_s1ws_epilogue.h, one text for this kernel and tstage1ws7_kernel, conv_s1ws7.hip; the formula and the reduction scheme of
// s1_epilogue<NT, true>, conv_s1_epilogue.h): per 8 x 16 tile and channel the sum over the tile's valid pixels and the sum of squared
// deviations from the TILE mean, two passes over the accumulators -- pixel columns rg and rows i in registers, the lane quarters lq by two
// xor shuffles, the four waves through LDS.  Deterministic, no atomics.  The six accumulator sets (5 x 5, 3 x 3, four passes of the 1 x 1
// slot) take the epilogue one after the other, three N tiles each.
//
// A translation unit of its own: the code generation of conv_pk.hip is pinned (tests/test_codegen.py) and stays as it is.
#include "common.h"
#include "conv_pk_tile.h"
#include "conv_s1_host.h"
#include "conv_s1ws_epilogue.h"

namespace cat_s1ws {

using namespace cat_pk;      // TH, PITCH, TABN, mma_groups, wload, wmma (conv_pk_tile.h)

__device__ __attribute__((aligned(16))) float g_zero[4] = {0.f, 0.f, 0.f, 0.f};

struct Args {
  const float* x; const float* pack[3]; const float* bias; float* y; float* stats;
  int xcs, c4, N, H, W, reflect, ycs, scs;
  int col0[3], width[3];
  int hl, tr, tc, tiles_x, tiles;
};

using cat_s1ws_epi::NT;      // N tiles per accumulator set
using cat_s1ws_epi::epilogue;      // conv_s1ws_epilogue.h, shared with tstage1ws7_kernel (conv_s1ws7.hip)

template <int N5, int N3, int N1>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void tstage1ws_kernel(const Args p) {
  static_assert(N5 == NT && N3 == NT, "the epilogue takes three N tiles per accumulator set");
#include "conv_pk_s1w_main.h"      // the main loop, shared with tstage1w_kernel (conv_pk.hip)
  float* red = smem + 2 * tile_floats + 6 * TABN;      // behind the tiles and the A-offset tables, which slower waves still read
  epilogue(acc5, p, 0, 0, n, tt, oy0, ox0, wave, lr, lq, red);
  epilogue(acc3, p, 1, 0, n, tt, oy0, ox0, wave, lr, lq, red);
  epilogue(accA, p, 2, 0, n, tt, oy0, ox0, wave, lr, lq, red);
  if constexpr (P1 > 1) epilogue(accB, p, 2, 3, n, tt, oy0, ox0, wave, lr, lq, red);
  if constexpr (P1 > 2) epilogue(accC, p, 2, 6, n, tt, oy0, ox0, wave, lr, lq, red);
  if constexpr (P1 > 3) epilogue(accD, p, 2, 9, n, tt, oy0, ox0, wave, lr, lq, red);
}

}  // namespace cat_s1ws

extern "C" {

int cat_tstage1ws_supported(int w5, int w3, int w1) { return cat_s1::wide_531(w5, w3, w1); }

int cat_tstage1ws_fwd(const cat_tstage1_t* g, const float* x, const float* const* packs, const float* bias, float* y, float* stats,
                      cat_stream_t stream) {
  cat_s1ws::Args a{};
  int grid;
  if (int rc = cat_s1::input(a, g, x, 5, "tstage1ws", &grid)) return rc;
  CAT_REQUIRE(cat_tstage1ws_supported(g->width[0], g->width[1], g->width[2]), "tstage1ws: no kernel for slot widths %d / %d / %d", g->width[0],
              g->width[1], g->width[2]);
  CAT_REQUIRE(x && packs && y && stats && (g->ycs & 3) == 0 && (g->scs & 3) == 0, "tstage1ws: output / statistics buffers");
  float* const ys[3] = {y, y, y};
  const int ycs[3] = {g->ycs, g->ycs, g->ycs};
  if (int rc = cat_s1::slices<3>(a, g, packs, ys, ycs, stats, "tstage1ws")) return rc;
  a.bias = bias; a.y = y; a.stats = stats; a.ycs = g->ycs; a.scs = g->scs;
  const size_t lds = cat_s1::patch(a, 2) + (size_t)8 * cat_s1ws::NT * 16 * sizeof(float);
  cat::ProfScope prof("conv_tstage1ws", cat_s1::flops<3>(g), 0.0, stream);
  cat_s1ws::tstage1ws_kernel<3, 3, 11><<<grid, 256, lds, (hipStream_t)stream>>>(a);
  return cat::check_launch("tstage1ws_fwd");
}

}  // extern "C"
