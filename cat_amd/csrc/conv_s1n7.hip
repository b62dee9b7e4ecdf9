// cat_tstage1n7_fwd / cat_tstage1n7_dgrad: the narrow 7 5 3 1 stage 1 and the input gradients of such a unit's second convs (the entries
// side by side: docs/CONV_VARIANTS.md, "Stage 1 in one launch"): tstage1_kernel (csrc/conv_pk.hip) with one more slot on the
// (8 + 6) x (16 + 6) patch of conv_pk7.hip / conv_s1w7_main.h: four A-offset tables, four accumulator sets walked one after the other per
// chunk (mma_groups, conv_pk_tile.h), four filter streams in cat_tconv_pack / cat_prep_run kind 0 order.
//
// Workgroup = 256 threads = 8 x 16 output pixels, wave w owns rows 2w, 2w + 1.  Epilogue = s1_epilogue (conv_s1_epilogue.h, shared with
// tstage1_kernel): slot k writes columns [col0[k], col0[k] + width[k]) of its output buffer, bias added, no activation, padding columns as
// 0; with STATS the per-tile sum and squared deviations from the tile mean go into the same columns of the table cat_tnorm_finalize reads
// (deterministic, no atomics).  The staging text is conv_s1w7_stage.h, shared with the wide kernels.
//
// Instantiations: N7, N5, N3 in {1, 2} N tiles (<= 32 columns per wide slot), N1 in {1 .. 4} (<= 64 columns), each with and without
// statistics: the domain of cat_tstage1_dgrad_supported with one more slot, all of it (cat_tstage1n7_supported).
// LDS: 2 x 14 x 22 x 20 floats of tiles (49 280 B) + 2 x 4 x 256 table entries (8 192 B) + 8 x 4 x 16 floats of reduction space (2 048 B)
// = 59 520 B, two workgroups per CU.  Accumulators: at most (2 + 2 + 2 + 4) x 2 tiles x 4 = 80 registers.  This file's register table is
// tests/golden/codegen_conv_s1n7.json.
#include "common.h"
#include "conv_pk_tile.h"
#include "conv_s1_epilogue.h"
#include "conv_s1_host.h"

namespace cat_s1n7 {

using namespace cat_pk;      // TH, PITCH, mma_groups (conv_pk_tile.h), s1_epilogue (conv_s1_epilogue.h)

__device__ __attribute__((aligned(16))) float g_zero[4] = {0.f, 0.f, 0.f, 0.f};

#define CAT_S1W7_DECLS
#include "conv_s1w7_main.h"      // the patch geometry and the LDS layout of tiles + tables (MAIN_LDS_BYTES)
#undef CAT_S1W7_DECLS
constexpr int NMAX = 4;      // N tiles of the widest accumulator set (the 1 x 1 slot)
constexpr size_t LDS_BYTES = MAIN_LDS_BYTES + (size_t)8 * NMAX * 16 * sizeof(float);
static_assert(LDS_BYTES == 59520 && LDS_BYTES <= 64 * 1024, "dynamic LDS without the opt-in");

struct Args {
  const float* x; const float* pack[NSLOT]; const float* bias; float* ys[NSLOT]; float* stats;   // ys / ycs3: output buffer and pixel stride per slot
  int xcs, c4, N, H, W, reflect, ycs3[NSLOT], scs;
  int col0[NSLOT], width[NSLOT];
  int tiles_x, tiles;
};

// N7 / N5 / N3 / N1: 16-wide N tiles of the 7 x 7, 5 x 5, 3 x 3 and 1 x 1 slot (the host passes exactly cdiv(width, 16) each)
template <int N7, int N5, int N3, int N1, bool STATS>
__global__ __launch_bounds__(256) void tstage1n7_kernel(const Args p) {
  constexpr int MT = 2;
  static_assert(N7 >= 1 && N7 <= 2 && N5 >= 1 && N5 <= 2 && N3 >= 1 && N3 <= 2 && N1 >= 1 && N1 <= NMAX, "tile counts");
#include "conv_s1w7_stage.h"      // tile origin, gload / sstore: the staging of conv_s1w7_main.h
  const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f4 acc7[MT][N7], acc5[MT][N5], acc3[MT][N3], acc1[MT][N1];
  unsigned jb7[N7], jb5[N5], jb3[N3], jb1[N1];
#pragma unroll
  for (int j = 0; j < N7; ++j) jb7[j] = (unsigned)(j * 64 + lane) * 16u;
#pragma unroll
  for (int j = 0; j < N5; ++j) jb5[j] = (unsigned)(j * 64 + lane) * 16u;
#pragma unroll
  for (int j = 0; j < N3; ++j) jb3[j] = (unsigned)(j * 64 + lane) * 16u;
#pragma unroll
  for (int j = 0; j < N1; ++j) jb1[j] = (unsigned)(j * 64 + lane) * 16u;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int j = 0; j < N7; ++j) acc7[i][j] = zero4;
#pragma unroll
    for (int j = 0; j < N5; ++j) acc5[i][j] = zero4;
#pragma unroll
    for (int j = 0; j < N3; ++j) acc3[i][j] = zero4;
#pragma unroll
    for (int j = 0; j < N1; ++j) acc1[i][j] = zero4;
  }
  int abase[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) abase[i] = ((2 * wave + i) * TC + lr) * PITCH;
  const __amdgpu_buffer_rsrc_t r7 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.pack[0]), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t r5 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.pack[1]), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t r3 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.pack[2]), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.pack[3]), 0, 0x7fffffff, 0x00020000);
  unsigned so7 = 0, so5 = 0, so3 = 0, so1 = 0;     // byte offsets of the current chunk in the four streams
  gload(0);
  sstore(0, 0);
  __syncthreads();
  int buf = 0;
  for (int c0 = 0; c0 < p.c4; c0 += 16) {
    const bool more = c0 + 16 < p.c4;
    if (more) gload(c0 + 16);
    const int nq = min(4, (p.c4 - c0) >> 2);
    const float* tile = tile0 + buf * TILE_FLOATS;
    const int* tab = tab0 + buf * NSLOT * KTAB + lq;
    {
      const int ngr = (49 * nq + 3) >> 2;
      mma_groups<MT, N7>(acc7, tile, tab, abase, r7, jb7, so7, (unsigned)N7 * 1024u, ngr);
      so7 += (unsigned)ngr * N7 * 1024u;
    }
    {
      const int ngr = (25 * nq + 3) >> 2;
      mma_groups<MT, N5>(acc5, tile, tab + KTAB, abase, r5, jb5, so5, (unsigned)N5 * 1024u, ngr);
      so5 += (unsigned)ngr * N5 * 1024u;
    }
    {
      const int ngr = (9 * nq + 3) >> 2;
      mma_groups<MT, N3>(acc3, tile, tab + 2 * KTAB, abase, r3, jb3, so3, (unsigned)N3 * 1024u, ngr);
      so3 += (unsigned)ngr * N3 * 1024u;
    }
    mma_groups<MT, N1>(acc1, tile, tab + 3 * KTAB, abase, r1, jb1, so1, (unsigned)N1 * 1024u, 1);      // the centre tap's quads: one group
    so1 += (unsigned)N1 * 1024u;
    if (more) {
      sstore(buf ^ 1, c0 + 16);
      __syncthreads();
      buf ^= 1;
    }
  }
  __syncthreads();
  float* red = smem + MAIN_LDS_BYTES / sizeof(float);      // behind the tiles and the A-offset tables
  s1_epilogue<N7, STATS>(acc7, p, 0, n, tt, oy0, ox0, wave, lr, lq, red);
  s1_epilogue<N5, STATS>(acc5, p, 1, n, tt, oy0, ox0, wave, lr, lq, red);
  s1_epilogue<N3, STATS>(acc3, p, 2, n, tt, oy0, ox0, wave, lr, lq, red);
  s1_epilogue<N1, STATS>(acc1, p, 3, n, tt, oy0, ox0, wave, lr, lq, red);
}

static int launch(const cat_tstage1s7_t* g, const float* x, const float* const* packs, const float* bias, float* const* ys, const int* ycs,
                  float* stats, const char* what, const char* family, cat_stream_t stream) {
  Args a{};
  int grid;
  if (int rc = cat_s1::input(a, g, x, 7, what, &grid)) return rc;
  CAT_REQUIRE(cat_tstage1n7_supported(g->width[0], g->width[1], g->width[2], g->width[3]), "%s: no kernel for slot widths %d / %d / %d / %d", what,
              g->width[0], g->width[1], g->width[2], g->width[3]);
  CAT_REQUIRE(x && packs && ys && ycs, "%s: null argument", what);
  if (int rc = cat_s1::slices<NSLOT>(a, g, packs, ys, ycs, stats, what)) return rc;
  a.bias = bias; a.stats = stats; a.scs = g->scs;
  int nt[NSLOT];
  for (int k = 0; k < NSLOT; ++k) {
    nt[k] = cat::cdiv(g->width[k], 16);
    a.ys[k] = ys[k]; a.ycs3[k] = ycs[k];
  }
  hipStream_t s = (hipStream_t)stream;
  cat::ProfScope prof(family, cat_s1::flops<NSLOT>(g), 0.0, stream);
#define CAT_N7(A, B, C, D)                                                                             \
  if (nt[0] == A && nt[1] == B && nt[2] == C && nt[3] == D) {                                          \
    if (stats) tstage1n7_kernel<A, B, C, D, true><<<grid, 256, LDS_BYTES, s>>>(a);                     \
    else tstage1n7_kernel<A, B, C, D, false><<<grid, 256, LDS_BYTES, s>>>(a);                          \
    return cat::check_launch(what);                                                                    \
  }
#define CAT_N7_1(A, B, C) CAT_N7(A, B, C, 1) CAT_N7(A, B, C, 2) CAT_N7(A, B, C, 3) CAT_N7(A, B, C, 4)
#define CAT_N7_W(A) CAT_N7_1(A, 1, 1) CAT_N7_1(A, 1, 2) CAT_N7_1(A, 2, 1) CAT_N7_1(A, 2, 2)
  CAT_N7_W(1) CAT_N7_W(2)
#undef CAT_N7_W
#undef CAT_N7_1
#undef CAT_N7
  cat::set_error("%s: no kernel for %d / %d / %d / %d N tiles (cat_tstage1n7_supported)", what, nt[0], nt[1], nt[2], nt[3]);
  return -22;
}

}  // namespace cat_s1n7

extern "C" {

int cat_tstage1n7_supported(int w7, int w5, int w3, int w1) {
  return w7 > 0 && w5 > 0 && w3 > 0 && w1 > 0 && w7 <= 32 && w5 <= 32 && w3 <= 32 && w1 <= 64;      // <= 2 / 2 / 2 / 4 N tiles: every combination exists
}

int cat_tstage1n7_fwd(const cat_tstage1s7_t* g, const float* x, const float* const* packs, const float* bias, float* y, float* stats,
                      cat_stream_t stream) {
  CAT_REQUIRE(y && stats && (g->ycs & 3) == 0 && (g->scs & 3) == 0, "tstage1n7: output / statistics buffers");
  float* const ys[4] = {y, y, y, y};
  const int ycs[4] = {g->ycs, g->ycs, g->ycs, g->ycs};
  return cat_s1n7::launch(g, x, packs, bias, ys, ycs, stats, "tstage1n7", "conv_tstage1n7", stream);
}

int cat_tstage1n7_dgrad(const cat_tstage1s7_t* g, const float* dy, const float* const* packs, float* const* dxs, const int* dxcs,
                        cat_stream_t stream) {
  CAT_REQUIRE(dxs && dxcs && !g->reflect, "tstage1n7 dgrad: zero-padded convolutions only, one output buffer per slot");
  return cat_s1n7::launch(g, dy, packs, nullptr, dxs, dxcs, nullptr, "tstage1n7 dgrad", "conv_tstage1n7_dgrad", stream);
}

}  // extern "C"
