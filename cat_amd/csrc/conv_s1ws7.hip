// cat_tstage1ws7_fwd: the wide 7 5 3 1 stage 1 with statistics (the entries side by side: docs/CONV_VARIANTS.md, "Stage 1 in one launch").
// The main loop of tstage1w7_kernel<3, 3> (conv_s1w7_main.h) with the epilogue of tstage1ws_kernel (conv_s1ws_epilogue.h).
//
// The six accumulator sets (7 x 7, 5 x 5, 3 x 3, three passes of the 1 x 1 slot) take the epilogue one after the other, three N tiles each.
// LDS: the 56 KB of tstage1w7_kernel (tiles + tables) + 8 x 3 x 16 floats of reduction space behind them, two workgroups per CU.
//
// A translation unit of its own: the code generation of conv_s1w7.hip and conv_s1ws.hip is pinned and stays as it is; both headers are
// included textually / as a forced-inline template, and either file compiles to the instructions it had before the text moved.  This file's
// table is tests/golden/codegen_conv_s1ws7.json.
#include "common.h"
#include "conv_pk_tile.h"
#include "conv_s1_host.h"
#include "conv_s1ws_epilogue.h"

namespace cat_s1ws7 {

using namespace cat_pk;      // TH, PITCH, mma_groups, wload, wmma (conv_pk_tile.h)
using cat_s1ws_epi::NT;
using cat_s1ws_epi::epilogue;

__device__ __attribute__((aligned(16))) float g_zero[4] = {0.f, 0.f, 0.f, 0.f};

#define CAT_S1W7_DECLS
#include "conv_s1w7_main.h"      // the patch geometry and the LDS layout of the main loop
#undef CAT_S1W7_DECLS
constexpr size_t LDS_BYTES = MAIN_LDS_BYTES + (size_t)cat_s1ws_epi::RED_FLOATS * sizeof(float);
static_assert(LDS_BYTES <= 64 * 1024, "dynamic LDS without the opt-in");

struct Args {
  const float* x; const float* pack[NSLOT]; const float* bias; float* y; float* stats;
  int xcs, c4, N, H, W, reflect, ycs, scs;
  int col0[NSLOT], width[NSLOT];
  int tiles_x, tiles;
};

// NW N tiles per wide slot, 3 * P1 for the 1 x 1 slot
template <int NW, int P1>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void tstage1ws7_kernel(const Args p) {
  static_assert(NW == NT, "the epilogue takes three N tiles per accumulator set");
#include "conv_s1w7_main.h"      // the main loop, shared with tstage1w7_kernel (conv_s1w7.hip)
  float* red = smem + MAIN_LDS_BYTES / sizeof(float);      // behind the tiles and the A-offset tables, which slower waves still read
  epilogue(acc7, p, 0, 0, n, tt, oy0, ox0, wave, lr, lq, red);
  epilogue(acc5, p, 1, 0, n, tt, oy0, ox0, wave, lr, lq, red);
  epilogue(acc3, p, 2, 0, n, tt, oy0, ox0, wave, lr, lq, red);
  epilogue(accA, p, 3, 0, n, tt, oy0, ox0, wave, lr, lq, red);
  epilogue(accB, p, 3, 3, n, tt, oy0, ox0, wave, lr, lq, red);
  epilogue(accC, p, 3, 6, n, tt, oy0, ox0, wave, lr, lq, red);
}

}  // namespace cat_s1ws7

extern "C" {

int cat_tstage1ws7_supported(int w7, int w5, int w3, int w1) { return cat_s1::wide_7531(w7, w5, w3, w1); }

int cat_tstage1ws7_fwd(const cat_tstage1s7_t* g, const float* x, const float* const* packs, const float* bias, float* y, float* stats,
                       cat_stream_t stream) {
  using namespace cat_s1ws7;
  Args a{};
  int grid;
  if (int rc = cat_s1::input(a, g, x, 7, "tstage1ws7", &grid)) return rc;
  CAT_REQUIRE(cat_tstage1ws7_supported(g->width[0], g->width[1], g->width[2], g->width[3]), "tstage1ws7: no kernel for slot widths %d / %d / %d / %d",
              g->width[0], g->width[1], g->width[2], g->width[3]);
  CAT_REQUIRE(x && packs && y && stats && (g->ycs & 3) == 0 && (g->scs & 3) == 0, "tstage1ws7: output / statistics buffers");
  float* const ys[NSLOT] = {y, y, y, y};
  const int ycs[NSLOT] = {g->ycs, g->ycs, g->ycs, g->ycs};
  if (int rc = cat_s1::slices<NSLOT>(a, g, packs, ys, ycs, stats, "tstage1ws7")) return rc;
  a.bias = bias; a.y = y; a.stats = stats; a.ycs = g->ycs; a.scs = g->scs;
  cat::ProfScope prof("conv_tstage1ws7", cat_s1::flops<NSLOT>(g), 0.0, stream);
  tstage1ws7_kernel<3, 3><<<grid, 256, LDS_BYTES, (hipStream_t)stream>>>(a);
  return cat::check_launch("tstage1ws7_fwd");
}

}  // extern "C"
