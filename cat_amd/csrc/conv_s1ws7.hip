// Stage 1 of a WIDE InvertedResidualChannels block with the reference's default kernel sizes 3 5 7 in one launch, with statistics
// (cat_tstage1ws7_fwd): the computation of tstage1w7_kernel<3, 3> (csrc/conv_s1w7.hip; the main loop of both is conv_s1w7_main.h) -- the
// 7 x 7, 5 x 5 and 3 x 3 first convs of the residual branches (256 -> 42 each) and the N-concatenated 1 x 1 first convs of the three depthwise
// branches (256 -> 3 x 44 = 132; inception_modules.py:135-165) from ONE staging of the input tile per 16-channel chunk on the
// (8 + 6) x (16 + 6) patch -- with the output contract of cat_tstage1ws_fwd (csrc/conv_s1ws.hip; the epilogue of both is
// conv_s1ws_epilogue.h): every slot writes its column slice [col0, col0 + width) of ONE pre-norm buffer (bias added, no activation) and the
// per-tile statistics of its columns into the table cat_tnorm_finalize reads.  It serves the training forward of the wide block
// (cat_amd/fused_block.py) and the frozen InstanceNorm teacher (cat_amd/frozen_in.py) at 3 5 7, which before issued four cat_tconv_fwd
// launches that each staged the same 256-channel input.
//
// The six accumulator sets (7 x 7, 5 x 5, 3 x 3, three passes of the 1 x 1 slot) take the epilogue one after the other, three N tiles each.
// LDS: the 56 KB of tstage1w7_kernel (tiles + tables) + 8 x 3 x 16 floats of reduction space behind them, two workgroups per CU.
//
// A translation unit of its own: the code generation of conv_s1w7.hip and conv_s1ws.hip is pinned and stays as it is; both headers are
// included textually / as a forced-inline template, and either file compiles to the instructions it had before the text moved.  This file's
// table is tests/golden/codegen_conv_s1ws7.json.
#include "common.h"
#include "conv_pk_tile.h"
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

int cat_tstage1ws7_supported(int w7, int w5, int w3, int w1) {
  const bool wide = w7 > 32 && w7 <= 48 && w5 > 32 && w5 <= 48 && w3 > 32 && w3 <= 48;
  return wide && w1 > 128 && w1 <= 144;      // the instantiation that exists: 3 + 3 + 3 + 9 tiles (m = 42, three depthwise branches)
}

int cat_tstage1ws7_fwd(const cat_tstage1s7_t* g, const float* x, const float* const* packs, const float* bias, float* y, float* stats,
                       cat_stream_t stream) {
  using namespace cat_s1ws7;
  CAT_REQUIRE(g->N > 0 && g->H > 0 && g->W > 0 && g->cin > 0 && (g->xcs & 3) == 0 && g->xcs >= g->cin, "tstage1ws7: bad input geometry");
  CAT_REQUIRE((int64_t)g->N * g->H * g->W * g->xcs < (int64_t)4294967295LL, "tstage1ws7: source larger than 2^32 elements");
  CAT_REQUIRE(cat_tstage1ws7_supported(g->width[0], g->width[1], g->width[2], g->width[3]), "tstage1ws7: no kernel for slot widths %d / %d / %d / %d",
              g->width[0], g->width[1], g->width[2], g->width[3]);
  CAT_REQUIRE(!g->reflect || (7 <= g->H && 7 <= g->W), "tstage1ws7: reflect padding wider than the plane");
  CAT_REQUIRE(x && packs && y && stats && (g->ycs & 3) == 0 && (g->scs & 3) == 0, "tstage1ws7: output / statistics buffers");
  Args a{};
  a.x = x; a.bias = bias; a.y = y; a.stats = stats;
  a.xcs = g->xcs; a.c4 = (g->cin + 3) & ~3; a.N = g->N; a.H = g->H; a.W = g->W; a.reflect = g->reflect; a.ycs = g->ycs; a.scs = g->scs;
  double kflops = 0.0;
  for (int k = 0; k < NSLOT; ++k) {
    CAT_REQUIRE(packs[k] && g->col0[k] >= 0 && g->col0[k] + g->width[k] <= g->ycs && g->col0[k] + g->width[k] <= g->scs &&
                    g->nvalid[k] <= g->width[k],
                "tstage1ws7: slice %d", k);
    a.pack[k] = packs[k]; a.col0[k] = g->col0[k]; a.width[k] = g->width[k];
    kflops += (double)g->nvalid[k] * slot_ks(k) * slot_ks(k);
  }
  a.tiles_x = cat::cdiv(g->W, TW);
  a.tiles = a.tiles_x * cat::cdiv(g->H, TH);
  const int64_t grid = (int64_t)g->N * a.tiles;
  CAT_REQUIRE(grid < (int64_t)2147483647, "tstage1ws7: grid too large");
  cat::ProfScope prof("conv_tstage1ws7", 2.0 * (double)g->N * g->H * g->W * g->cin * kflops, 0.0, stream);
  tstage1ws7_kernel<3, 3><<<(int)grid, 256, LDS_BYTES, (hipStream_t)stream>>>(a);
  return cat::check_launch("tstage1ws7_fwd");
}

}  // extern "C"
