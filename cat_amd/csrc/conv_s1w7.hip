// Stage 1 of an EVAL-mode (frozen, BatchNorm-folded) InvertedResidualChannels block with the reference's default kernel sizes 3 5 7 in one
// launch (cat_tstage1w7_fwd; cat_amd/frozen.py): the 7 x 7, 5 x 5 and 3 x 3 first convs of the residual branches (256 -> 42 each) and the
// N-concatenated 1 x 1 first convs of the three depthwise branches (256 -> 3 x 44 = 132; inception_modules.py:135-165) from ONE staging of the
// input tile per 16-channel chunk, epilogue = folded bias + activation, four output buffers.  The contract of cat_tstage1w_fwd (conv_pk.hip)
// with one more slot; without it the block ran a 128 x 128-tile GEMM and three padded first convs that each staged the same 256 channels.
//
// What differs from tstage1w_kernel<3, 3, 11> (its main loop, conv_pk_s1w_main.h, is pinned and serves the 5 x 5 patch only):
//   * the patch is (8 + 6) x (16 + 6) pixels: 1232 staging slots, 5 per thread (conv_pk7.hip's patch);
//   * the A-offset table of a slot has 256 entries per buffer: a 7 x 7 chunk has 49 x 4 = 196 (tap, quad) pairs, one thread fills one entry;
//   * four accumulator sets and four filter streams: (3 + 3 + 3 + 9) x 2 tiles of 16 x 16 per wave, the 1 x 1 slot in three passes of three
//     N tiles over the centre tap's A fragments.
// LDS: 2 x 14 x 22 x 80 B of tiles + 2 x 4 x 1 KB of tables = 56 KB, two workgroups per CU.
//
// A translation unit of its own: the code generation of conv_pk.hip is pinned (tests/test_codegen.py) and stays as it is; this file's table
// is tests/golden/codegen_conv_s1w7.json.  The main loop and the patch geometry live in conv_s1w7_main.h, one text for this kernel and its
// statistics-writing twin (tstage1ws7_kernel, conv_s1ws7.hip).
#include "common.h"
#include "conv_pk_tile.h"

namespace cat_s1w7 {

using namespace cat_pk;      // TH, PITCH, mma_groups, wload, wmma (conv_pk_tile.h)

__device__ __attribute__((aligned(16))) float g_zero[4] = {0.f, 0.f, 0.f, 0.f};

#define CAT_S1W7_DECLS
#include "conv_s1w7_main.h"      // the patch geometry and the LDS layout of the main loop
#undef CAT_S1W7_DECLS
constexpr size_t LDS_BYTES = MAIN_LDS_BYTES;
static_assert(LDS_BYTES <= 64 * 1024, "dynamic LDS without the opt-in");

struct Args {
  const float* x; const float* pack[NSLOT]; const float* bias[NSLOT]; float* y[NSLOT];
  int ycs[NSLOT], nvalid[NSLOT];
  int xcs, c4, N, H, W, reflect, act;
  float slope;
  int tiles_x, tiles;
};

// N tiles [t0, t0 + NT) of slot k: bias + activation; columns [nvalid, ycs) inside the slot's tiles come out as 0, columns of a wider
// pixel stride beyond the tiles (48 / 144) are not touched
template <int NT>
__device__ __forceinline__ void store(const f4 (&acc)[2][NT], const Args& p, int k, int t0, int n, int oy0, int ox0, int wave, int lr, int lq) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int oy = oy0 + 2 * wave + i;
    if (oy >= p.H) continue;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const int ox = ox0 + lq * 4 + rg;
      if (ox >= p.W) continue;
      float* yo = p.y[k] + (((int64_t)n * p.H + oy) * p.W + ox) * p.ycs[k];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int co = (t0 + j) * 16 + lr;
        if (co < p.nvalid[k]) yo[co] = cat::apply_act(acc[i][j][rg] + (p.bias[k] ? p.bias[k][co] : 0.f), p.act, p.slope);
        else if (co < p.ycs[k]) yo[co] = 0.f;
      }
    }
  }
}

// NW N tiles per wide slot, 3 * P1 for the 1 x 1 slot
template <int NW, int P1>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void tstage1w7_kernel(const Args p) {
#include "conv_s1w7_main.h"      // the main loop, shared with tstage1ws7_kernel (conv_s1ws7.hip)
  store<NW>(acc7, p, 0, 0, n, oy0, ox0, wave, lr, lq);
  store<NW>(acc5, p, 1, 0, n, oy0, ox0, wave, lr, lq);
  store<NW>(acc3, p, 2, 0, n, oy0, ox0, wave, lr, lq);
  store<3>(accA, p, 3, 0, n, oy0, ox0, wave, lr, lq);
  store<3>(accB, p, 3, 3, n, oy0, ox0, wave, lr, lq);
  store<3>(accC, p, 3, 6, n, oy0, ox0, wave, lr, lq);
}

}  // namespace cat_s1w7

extern "C" {

int cat_tstage1w7_supported(int w7, int w5, int w3, int w1) {
  const bool wide = w7 > 32 && w7 <= 48 && w5 > 32 && w5 <= 48 && w3 > 32 && w3 <= 48;
  return wide && w1 > 128 && w1 <= 144;      // the instantiation that exists: 3 + 3 + 3 + 9 tiles (m = 42, three depthwise branches)
}

int cat_tstage1w7_fwd(const cat_tstage1w7_t* g, const float* x, const float* const* packs, const float* const* biases, float* const* ys,
                      cat_stream_t stream) {
  using namespace cat_s1w7;
  CAT_REQUIRE(g->N > 0 && g->H > 0 && g->W > 0 && g->cin > 0 && (g->xcs & 3) == 0 && g->xcs >= g->cin, "tstage1w7: bad input geometry");
  CAT_REQUIRE((int64_t)g->N * g->H * g->W * g->xcs < (int64_t)4294967295LL, "tstage1w7: source larger than 2^32 elements");
  CAT_REQUIRE(cat_tstage1w7_supported(g->nvalid[0], g->nvalid[1], g->nvalid[2], g->nvalid[3]), "tstage1w7: no kernel for %d / %d / %d / %d output channels",
              g->nvalid[0], g->nvalid[1], g->nvalid[2], g->nvalid[3]);
  CAT_REQUIRE(!g->reflect || (7 <= g->H && 7 <= g->W), "tstage1w7: reflect padding wider than the plane");
  CAT_REQUIRE(x && packs && ys, "tstage1w7: null argument");
  Args a{};
  a.x = x; a.xcs = g->xcs; a.c4 = (g->cin + 3) & ~3; a.N = g->N; a.H = g->H; a.W = g->W; a.reflect = g->reflect; a.act = g->act; a.slope = g->slope;
  double kflops = 0.0;
  for (int k = 0; k < NSLOT; ++k) {
    CAT_REQUIRE(packs[k] && ys[k] && (g->ycs[k] & 3) == 0 && g->ycs[k] >= g->nvalid[k], "tstage1w7: slot %d", k);
    a.pack[k] = packs[k]; a.bias[k] = biases ? biases[k] : nullptr; a.y[k] = ys[k]; a.ycs[k] = g->ycs[k]; a.nvalid[k] = g->nvalid[k];
    kflops += (double)g->nvalid[k] * slot_ks(k) * slot_ks(k);
  }
  a.tiles_x = cat::cdiv(g->W, TW);
  a.tiles = a.tiles_x * cat::cdiv(g->H, TH);
  const int64_t grid = (int64_t)g->N * a.tiles;
  CAT_REQUIRE(grid < (int64_t)2147483647, "tstage1w7: grid too large");
  cat::ProfScope prof("conv_tstage1w7", 2.0 * (double)g->N * g->H * g->W * g->cin * kflops, 0.0, stream);
  tstage1w7_kernel<3, 3><<<(int)grid, 256, LDS_BYTES, (hipStream_t)stream>>>(a);
  return cat::check_launch("tstage1w7_fwd");
}

}  // extern "C"
