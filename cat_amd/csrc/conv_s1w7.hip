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
// is tests/golden/codegen_conv_s1w7.json.
#include "common.h"
#include "conv_pk_tile.h"

namespace cat_s1w7 {

using namespace cat_pk;      // TH, PITCH, mma_groups, wload, wmma (conv_pk_tile.h)

__device__ __attribute__((aligned(16))) float g_zero[4] = {0.f, 0.f, 0.f, 0.f};

constexpr int TW = 16, HL = 3, TR = TH + 2 * HL, TC = TW + 2 * HL, KTAB = 256, NSLOT = 4;
constexpr int SLOTS = TR * TC * 4, MAXIT = (SLOTS + 255) / 256, TILE_FLOATS = TR * TC * PITCH;
constexpr size_t LDS_BYTES = (size_t)2 * TILE_FLOATS * sizeof(float) + (size_t)2 * NSLOT * KTAB * sizeof(int);
static_assert(49 * 4 <= KTAB && KTAB <= 256, "one table entry per (tap, quad) pair of a chunk, filled by one thread each");
static_assert(LDS_BYTES <= 64 * 1024, "dynamic LDS without the opt-in");

__host__ __device__ constexpr int slot_ks(int k) { return 7 - 2 * k; }      // slot 0..3 = 7 x 7, 5 x 5, 3 x 3, 1 x 1

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
  constexpr int MT = 2, N1 = 3 * P1;
  static_assert(NW >= 1 && NW <= 3 && P1 == 3, "tile counts");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* tile0 = smem;
  int* tab0 = reinterpret_cast<int*>(smem + 2 * TILE_FLOATS);      // [buf][slot][KTAB]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lq = lane >> 4;
  const int tt = cat::xcd_remap(blockIdx.x, gridDim.x);
  const int n = tt / p.tiles, t = tt - n * p.tiles;
  const int oy0 = (t / p.tiles_x) * TH, ox0 = (t % p.tiles_x) * TW;
  const int quad = tid & 3;
  unsigned soff[MAXIT], smask = 0;
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int pix = (tid + it * 256) >> 2;
    const int r = pix / TC;
    int iy = oy0 - HL + r, ix = ox0 - HL + (pix - r * TC);
    bool v = tid + it * 256 < SLOTS;
    if (p.reflect) {
      v = v && iy > -p.H && iy < 2 * p.H - 1 && ix > -p.W && ix < 2 * p.W - 1;      // beyond a ragged tile's mirror range: never read
      iy = cat::reflect_idx(iy, p.H);
      ix = cat::reflect_idx(ix, p.W);
    } else {
      v = v && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
    }
    smask |= v ? (1u << it) : 0u;
    soff[it] = v ? ((unsigned)(n * p.H + iy) * (unsigned)p.W + (unsigned)ix) * (unsigned)p.xcs + quad * 4 : 0u;
  }
  f4 sreg[MAXIT];
  auto gload = [&](int c0) {
    const bool qv = c0 + quad * 4 < p.c4;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) sreg[it] = *reinterpret_cast<const f4*>((((smask >> it) & 1u) && qv) ? p.x + soff[it] + c0 : g_zero);
  };
  auto sstore = [&](int buf, int c0) {
    float* tile = tile0 + buf * TILE_FLOATS;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int idx = tid + it * 256;
      if (idx < SLOTS) *reinterpret_cast<f4*>(tile + (idx >> 2) * PITCH + quad * 4) = sreg[it];
    }
    const int nq = min(4, (p.c4 - c0) >> 2);
    const int tap = tid / nq, qd = tid - tap * nq;      // 256 threads, KTAB entries: one each
#pragma unroll
    for (int k = 0; k < NSLOT; ++k) {
      const int ks = slot_ks(k), taps = ks * ks;
      int off = 0;
      if (tid < ((taps * nq + 3) >> 2) * 4 && tap < taps) {
        const int ky = tap / ks, kx = tap - ky * ks, d = HL - (ks >> 1);
        off = ((d + ky) * TC + d + kx) * PITCH + qd * 4;
      }
      tab0[(buf * NSLOT + k) * KTAB + tid] = off;
    }
  };
  const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f4 acc7[MT][NW], acc5[MT][NW], acc3[MT][NW], accA[MT][3], accB[MT][3], accC[MT][3];      // the 1 x 1 slot: passes A..C of 3 tiles
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int j = 0; j < NW; ++j) acc7[i][j] = acc5[i][j] = acc3[i][j] = zero4;
#pragma unroll
    for (int j = 0; j < 3; ++j) accA[i][j] = accB[i][j] = accC[i][j] = zero4;
  }
  int abase[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) abase[i] = ((2 * wave + i) * TC + lr) * PITCH;
  const __amdgpu_buffer_rsrc_t r7 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.pack[0]), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t r5 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.pack[1]), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t r3 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.pack[2]), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.pack[3]), 0, 0x7fffffff, 0x00020000);
  unsigned jbw[NW], jb1[P1][3];
#pragma unroll
  for (int j = 0; j < NW; ++j) jbw[j] = (unsigned)(j * 64 + lane) * 16u;
#pragma unroll
  for (int q = 0; q < P1; ++q)
#pragma unroll
    for (int j = 0; j < 3; ++j) jb1[q][j] = (unsigned)((3 * q + j) * 64 + lane) * 16u;
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
      mma_groups<MT, NW>(acc7, tile, tab, abase, r7, jbw, so7, (unsigned)NW * 1024u, ngr);
      so7 += (unsigned)ngr * NW * 1024u;
    }
    {
      const int ngr = (25 * nq + 3) >> 2;
      mma_groups<MT, NW>(acc5, tile, tab + KTAB, abase, r5, jbw, so5, (unsigned)NW * 1024u, ngr);
      so5 += (unsigned)ngr * NW * 1024u;
    }
    f4 bw[3];
    wload<3>(bw, r1, jb1[0], so1);      // the first filter blocks of the 1 x 1 slot travel behind the 3 x 3 stream
    {
      const int ngr = (9 * nq + 3) >> 2;
      mma_groups<MT, NW>(acc3, tile, tab + 2 * KTAB, abase, r3, jbw, so3, (unsigned)NW * 1024u, ngr);
      so3 += (unsigned)ngr * NW * 1024u;
    }
    {
      // the 1 x 1 slot: ONE group per chunk (the centre tap's four quads), N1 tiles wide -- the A fragments are read once, the filter
      // blocks of pass q + 1 are in flight behind the MFMAs of pass q
      f4 aw[MT], bx[3];
      const int off = tab[3 * KTAB];
#pragma unroll
      for (int i = 0; i < MT; ++i) aw[i] = *reinterpret_cast<const f4*>(tile + abase[i] + off);
      wload<3>(bx, r1, jb1[1], so1);
      __builtin_amdgcn_sched_barrier(0);
      wmma<MT, 3>(accA, aw, bw);
      __builtin_amdgcn_sched_barrier(0);
      wload<3>(bw, r1, jb1[2], so1);
      __builtin_amdgcn_sched_barrier(0);
      wmma<MT, 3>(accB, aw, bx);
      __builtin_amdgcn_sched_barrier(0);
      wmma<MT, 3>(accC, aw, bw);
    }
    so1 += (unsigned)N1 * 1024u;
    if (more) {
      sstore(buf ^ 1, c0 + 16);
      __syncthreads();
      buf ^= 1;
    }
  }
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
