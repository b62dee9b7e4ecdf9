// Device code shared by the LDS-tile convolution kernels (csrc/conv_pk.hip) and the statistics-writing wide stage 1 (csrc/conv_s1ws.hip):
// the tile constants, the packed-filter buffer load, the MFMA stream of one staged chunk and the filter loads / MFMAs of the wide 1 x 1 slot.
// Moved here verbatim from conv_pk.hip.  The main loop the two wide stage-1 kernels share is conv_pk_s1w_main.h.
#pragma once
#include "common.h"

namespace cat_pk {

constexpr int TH = 8, PITCH = 20, TABN = 128;

// launch geometry of tconv_kernel (conv_pk.hip) and tconv7_kernel (conv_pk7.hip); their shared body is conv_pk_tconv_main.h
struct Launch {
  int hl, tr, tc;          // halo (left / top), staged rows / columns
  int tiles_x, tiles;      // output tiles per row / per image
  int nt_total, nblk;      // 16-wide N tiles of the output, N blocks (gridDim.x = N * tiles * nblk)
  int ablate;              // DIAGNOSTIC BUILD ONLY (cat::kDiag; CAT_PK_ABLATE, results become wrong): 1 every group reads the SAME filter block
                           // (L1 hits), 2 every A fragment reads LDS offset 0, 4 staging loads hit one cached line, 8 no staging / barrier after
                           // the first chunk.  The production kernels read `abl`, a compile-time 0
};

// cat_tconv_fwd launches that need the wider patch (a 7 x 7 segment, or hl + hr > 4): conv_pk7.hip
int tconv7_launch(const cat_tconv_t* g, const float* pack, const float* bias, float* y, cat_stream_t stream);

__device__ __forceinline__ f4 bload(const __amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff_) {
  const auto r = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff_, 0);
  static_assert(sizeof(r) == sizeof(f4), "buffer load width");
  return __builtin_bit_cast(f4, r);
}

// MFMA stream of one staged chunk: ngr groups of 4 (tap, quad) pairs, MT x NT accumulator tiles.  Two operand register sets in
// ping-pong (no copies); the operands of group g+1 and the A offset of group g+2 are requested BEFORE the 4*MT*NT MFMAs of group g are
// issued, so no load is waited for in the group that issued it.  tab = this lane quarter's A-offset table, so = byte offset of the
// chunk's first group in the packed filter stream, gbytes = bytes per group.
template <int MT, int NT>
__device__ __forceinline__ void mma_groups(f4 (&acc)[MT][NT], const float* tile, const int* tab, const int (&abase)[MT],
                                           const __amdgpu_buffer_rsrc_t rsrc, const unsigned (&jb)[NT], unsigned so, unsigned gbytes, int ngr) {
  const int last = ngr - 1;
  f4 a0[MT], a1[MT], b0[NT], b1[NT];
  int off = tab[0];
  int offn = tab[4 * min(1, last)];
#pragma unroll
  for (int i = 0; i < MT; ++i) a0[i] = *reinterpret_cast<const f4*>(tile + abase[i] + off);
#pragma unroll
  for (int j = 0; j < NT; ++j) b0[j] = bload(rsrc, jb[j], so);
  int gi = 0;
  while (true) {
    {
      const int g1 = min(gi + 1, last), g2 = min(gi + 2, last);
#pragma unroll
      for (int i = 0; i < MT; ++i) a1[i] = *reinterpret_cast<const f4*>(tile + abase[i] + offn);
#pragma unroll
      for (int j = 0; j < NT; ++j) b1[j] = bload(rsrc, jb[j], so + (unsigned)g1 * gbytes);
      offn = tab[4 * g2];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int tq = 0; tq < 4; ++tq)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[i][tq], b0[j][tq], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (++gi >= ngr) break;
    {
      const int g1 = min(gi + 1, last), g2 = min(gi + 2, last);
#pragma unroll
      for (int i = 0; i < MT; ++i) a0[i] = *reinterpret_cast<const f4*>(tile + abase[i] + offn);
#pragma unroll
      for (int j = 0; j < NT; ++j) b0[j] = bload(rsrc, jb[j], so + (unsigned)g1 * gbytes);
      offn = tab[4 * g2];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int tq = 0; tq < 4; ++tq)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[i][tq], b1[j][tq], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (++gi >= ngr) break;
  }
}

template <int NT>
__device__ __forceinline__ void wload(f4 (&b)[3], const __amdgpu_buffer_rsrc_t rsrc, const unsigned (&jb)[3], unsigned so) {
#pragma unroll
  for (int j = 0; j < NT; ++j) b[j] = bload(rsrc, jb[j], so);
}

template <int MT, int NT>
__device__ __forceinline__ void wmma(f4 (&acc)[MT][3], const f4 (&a)[MT], const f4 (&b)[3]) {
#pragma unroll
  for (int tq = 0; tq < 4; ++tq)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][tq], b[j][tq], acc[i][j], 0, 0, 0);
}

}  // namespace cat_pk
