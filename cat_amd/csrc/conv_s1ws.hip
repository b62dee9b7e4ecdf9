// Stage 1 of a WIDE InvertedResidualChannels block in one launch, with statistics (cat_tstage1ws_fwd): the computation of
// tstage1w_kernel<3, 3, 11> (csrc/conv_pk.hip; the main loop of both is conv_pk_s1w_main.h) -- the 5 x 5 conv, the 3 x 3 conv and the
// N-concatenated 1 x 1 convs of the full-width teacher block (256 -> 42 / 42 / 176; inception_modules.py:135-165) from ONE staging of the
// input tile per 16-channel chunk -- with the output contract of cat_tstage1_fwd: every slot writes its column slice [col0, col0 + width)
// of ONE pre-norm buffer (bias added, no activation) and the per-tile statistics of its columns into the table cat_tnorm_finalize reads.
// It serves the training forward of the wide block (cat_amd/fused_block.py) and the frozen InstanceNorm teacher (cat_amd/frozen_in.py),
// which before issued three cat_tconv_fwd launches that each staged the same 256-channel input.
//
// Statistics (conv_s1ws_epilogue.h, one text for this kernel and tstage1ws7_kernel, conv_s1ws7.hip; the formula and the reduction scheme of
// s1_epilogue<NT, true>, conv_pk.hip): per 8 x 16 tile and channel the sum over the
// tile's valid pixels and the sum of squared deviations from the TILE mean, two passes over the accumulators -- pixel columns rg and rows i in
// registers, the lane quarters lq by two xor shuffles, the four waves through LDS.  Deterministic, no atomics.  The six accumulator sets
// (5 x 5, 3 x 3, four passes of the 1 x 1 slot) take the epilogue one after the other, three N tiles each.
//
// A translation unit of its own: the code generation of conv_pk.hip is pinned (tests/test_codegen.py) and stays as it is.
#include "common.h"
#include "conv_pk_tile.h"
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

int cat_tstage1ws_supported(int w5, int w3, int w1) {
  return w5 > 32 && w5 <= 48 && w3 > 32 && w3 <= 48 && w1 > 160 && w1 <= 176;      // the instantiation that exists: 3 + 3 + 11 tiles (m = 42)
}

int cat_tstage1ws_fwd(const cat_tstage1_t* g, const float* x, const float* const* packs, const float* bias, float* y, float* stats,
                      cat_stream_t stream) {
  CAT_REQUIRE(g->N > 0 && g->H > 0 && g->W > 0 && g->cin > 0 && (g->xcs & 3) == 0 && g->xcs >= g->cin, "tstage1ws: bad input geometry");
  CAT_REQUIRE((int64_t)g->N * g->H * g->W * g->xcs < (int64_t)4294967295LL, "tstage1ws: source larger than 2^32 elements");
  CAT_REQUIRE(cat_tstage1ws_supported(g->width[0], g->width[1], g->width[2]), "tstage1ws: no kernel for slot widths %d / %d / %d", g->width[0],
              g->width[1], g->width[2]);
  CAT_REQUIRE(!g->reflect || (5 <= g->H && 5 <= g->W), "tstage1ws: reflect padding wider than the plane");
  CAT_REQUIRE(x && packs && y && stats && (g->ycs & 3) == 0 && (g->scs & 3) == 0, "tstage1ws: output / statistics buffers");
  cat_s1ws::Args a{};
  a.x = x; a.bias = bias; a.y = y; a.stats = stats;
  a.xcs = g->xcs; a.c4 = (g->cin + 3) & ~3; a.N = g->N; a.H = g->H; a.W = g->W; a.reflect = g->reflect; a.ycs = g->ycs; a.scs = g->scs;
  double kflops = 0.0;
  for (int k = 0; k < 3; ++k) {
    CAT_REQUIRE(packs[k] && g->col0[k] >= 0 && g->col0[k] + g->width[k] <= g->ycs && g->col0[k] + g->width[k] <= g->scs &&
                    g->nvalid[k] <= g->width[k],
                "tstage1ws: slice %d", k);
    a.pack[k] = packs[k]; a.col0[k] = g->col0[k]; a.width[k] = g->width[k];
    const int ks = k == 0 ? 5 : (k == 1 ? 3 : 1);
    kflops += (double)g->nvalid[k] * ks * ks;
  }
  a.hl = 2;
  a.tr = cat_pk::TH + 4;
  a.tc = 16 + 4;
  a.tiles_x = cat::cdiv(g->W, 16);
  a.tiles = a.tiles_x * cat::cdiv(g->H, cat_pk::TH);
  const int64_t grid = (int64_t)g->N * a.tiles;
  CAT_REQUIRE(grid < (int64_t)2147483647, "tstage1ws: grid too large");
  const size_t lds = (size_t)2 * a.tr * a.tc * cat_pk::PITCH * sizeof(float) + 6 * cat_pk::TABN * sizeof(int) +
                     (size_t)8 * cat_s1ws::NT * 16 * sizeof(float);
  cat::ProfScope prof("conv_tstage1ws", 2.0 * (double)g->N * g->H * g->W * g->cin * kflops, 0.0, stream);
  cat_s1ws::tstage1ws_kernel<3, 3, 11><<<(int)grid, 256, lds, (hipStream_t)stream>>>(a);
  return cat::check_launch("tstage1ws_fwd");
}

}  // extern "C"
