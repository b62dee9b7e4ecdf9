// The wide stage 1 for the kernel sizes 3 5 7 (3 + 3 + 3 + 9 N tiles on an (8 + 6) x (16 + 6) patch), shared by tstage1w7_kernel
// (csrc/conv_s1w7.hip: bias + activation into four buffers) and tstage1ws7_kernel (csrc/conv_s1ws7.hip: pre-norm slices of one buffer +
// per-tile statistics).  Included TWICE by either file:
//
//   * at namespace scope with CAT_S1W7_DECLS defined: the patch geometry and the LDS layout of the main loop (MAIN_LDS_BYTES: two tiles and
//     the A-offset tables; a kernel may append to it);
//   * inside the kernel, without it: the main loop, A FUNCTION-BODY FRAGMENT moved here verbatim from tstage1w7_kernel -- every line up to its
//     store calls -- so that either kernel compiles to exactly what it would with the text in place (the precedent and the reason:
//     conv_pk_s1w_main.h; the code generation of conv_s1w7.hip is pinned, tests/golden/codegen_conv_s1w7.json).  Its first half, the tile
//     origin and the staging of a chunk, is conv_s1w7_stage.h (included below where the text stood), which the narrow four-slot kernel
//     (tstage1n7_kernel, csrc/conv_s1n7.hip) includes on its own.
//
// The fragment expects, in scope: template parameters NW, P1; the kernel argument `p` with x, pack[4], xcs, c4, N, H, W, reflect, tiles_x,
// tiles; g_zero (four zero floats in global memory); cat_pk's TH, PITCH, mma_groups, wload, wmma; the declarations below.  It leaves the
// accumulators acc7, acc5, acc3, accA .. accC (the 1 x 1 slot in three passes of three N tiles) and n, tt, oy0, ox0, wave, lr, lq for the
// epilogue, and smem, the dynamic LDS.
#ifdef CAT_S1W7_DECLS

constexpr int TW = 16, HL = 3, TR = TH + 2 * HL, TC = TW + 2 * HL, KTAB = 256, NSLOT = 4;
constexpr int SLOTS = TR * TC * 4, MAXIT = (SLOTS + 255) / 256, TILE_FLOATS = TR * TC * PITCH;
constexpr size_t MAIN_LDS_BYTES = (size_t)2 * TILE_FLOATS * sizeof(float) + (size_t)2 * NSLOT * KTAB * sizeof(int);
static_assert(49 * 4 <= KTAB && KTAB <= 256, "one table entry per (tap, quad) pair of a chunk, filled by one thread each");

__host__ __device__ constexpr int slot_ks(int k) { return 7 - 2 * k; }      // slot 0..3 = 7 x 7, 5 x 5, 3 x 3, 1 x 1

#else

  constexpr int MT = 2, N1 = 3 * P1;
  static_assert(NW >= 1 && NW <= 3 && P1 == 3, "tile counts");
#include "conv_s1w7_stage.h"      // the tile origin and the staging of a chunk, shared with tstage1n7_kernel (conv_s1n7.hip)
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

#endif
