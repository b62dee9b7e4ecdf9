// cat_tstage1w7_fwd: the wide 7 5 3 1 stage 1 of a frozen block (the entries side by side: docs/CONV_VARIANTS.md, "Stage 1 in one
// launch").  The contract of cat_tstage1w_fwd (conv_pk.hip) with one more slot.
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
#include "conv_s1_host.h"
#include "conv_s1w_store.h"

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

// s1w_store (bias + activation into the slot's buffer): conv_s1w_store.h, shared with tstage1w_kernel (conv_pk.hip)

// NW N tiles per wide slot, 3 * P1 for the 1 x 1 slot
template <int NW, int P1>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void tstage1w7_kernel(const Args p) {
#include "conv_s1w7_main.h"      // the main loop, shared with tstage1ws7_kernel (conv_s1ws7.hip)
  s1w_store<NW>(acc7, p, 0, 0, n, oy0, ox0, wave, lr, lq);
  s1w_store<NW>(acc5, p, 1, 0, n, oy0, ox0, wave, lr, lq);
  s1w_store<NW>(acc3, p, 2, 0, n, oy0, ox0, wave, lr, lq);
  s1w_store<3>(accA, p, 3, 0, n, oy0, ox0, wave, lr, lq);
  s1w_store<3>(accB, p, 3, 3, n, oy0, ox0, wave, lr, lq);
  s1w_store<3>(accC, p, 3, 6, n, oy0, ox0, wave, lr, lq);
}

}  // namespace cat_s1w7

extern "C" {

int cat_tstage1w7_supported(int w7, int w5, int w3, int w1) { return cat_s1::wide_7531(w7, w5, w3, w1); }

int cat_tstage1w7_fwd(const cat_tstage1w7_t* g, const float* x, const float* const* packs, const float* const* biases, float* const* ys,
                      cat_stream_t stream) {
  using namespace cat_s1w7;
  Args a{};
  int grid;
  if (int rc = cat_s1::input(a, g, x, 7, "tstage1w7", &grid)) return rc;
  CAT_REQUIRE(cat_tstage1w7_supported(g->nvalid[0], g->nvalid[1], g->nvalid[2], g->nvalid[3]), "tstage1w7: no kernel for %d / %d / %d / %d output channels",
              g->nvalid[0], g->nvalid[1], g->nvalid[2], g->nvalid[3]);
  if (int rc = cat_s1::buffers<NSLOT>(a, g, x, packs, biases, ys, nullptr, "tstage1w7")) return rc;
  cat::ProfScope prof("conv_tstage1w7", cat_s1::flops<NSLOT>(g), 0.0, stream);
  tstage1w7_kernel<3, 3><<<grid, 256, LDS_BYTES, (hipStream_t)stream>>>(a);
  return cat::check_launch("tstage1w7_fwd");
}

}  // extern "C"
