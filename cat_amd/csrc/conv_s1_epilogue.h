// The epilogue of the narrow one-launch stage 1, shared by tstage1_kernel (csrc/conv_pk.hip: kernel sizes 5 3 1, three slots) and
// tstage1n7_kernel (csrc/conv_s1n7.hip: kernel sizes 7 5 3 1, four slots).  Moved here verbatim from conv_pk.hip; the kernel argument is a
// template parameter because the two kernels' argument structs differ in their slot count.  It reads p.bias, p.ys[], p.ycs3[], p.stats,
// p.H, p.W, p.scs, p.col0[], p.width[].
#pragma once
#include "conv_pk_tile.h"

namespace cat_pk {

// Slot k = NT N tiles: columns [col0[k], col0[k] + width[k]) of the slot's output buffer, bias added, no activation.  STATS: the per-tile
// sum and squared deviations from the tile mean into the same columns of p.stats (deterministic: registers, two xor shuffles, the four
// waves through LDS).  red: 8 * NT * 16 floats of LDS.
template <int NT, bool STATS, class A>
__device__ __forceinline__ void s1_epilogue(f4 (&acc)[2][NT], const A& p, int k, int n, int tt, int oy0, int ox0, int wave, int lr, int lq,
                                            float* red) {
  const int col0 = p.col0[k], width = p.width[k], nv = width;   // padding columns inside the slice carry zero filters: plain zeros come out
  const int cnt = min(TH, p.H - oy0) * min(16, p.W - ox0);
  float s[NT], mean[NT], bv[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int co = j * 16 + lr;
    bv[j] = (p.bias && co < nv) ? p.bias[col0 + co] : 0.f;
  }
  if constexpr (STATS) {     // per-tile statistics; the input-gradient use of the kernel has none
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bool rowv = oy0 + 2 * wave + i < p.H;
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) a += (rowv && ox0 + lq * 4 + rg < p.W) ? acc[i][j][rg] + bv[j] : 0.f;
      }
      a += __shfl_xor(a, 16, 64);
      a += __shfl_xor(a, 32, 64);
      if (lq == 0) red[wave * NT * 16 + j * 16 + lr] = a;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int c = j * 16 + lr;
      s[j] = (red[c] + red[NT * 16 + c]) + (red[2 * NT * 16 + c] + red[3 * NT * 16 + c]);
      mean[j] = s[j] / (float)cnt;
    }
    float* red2 = red + 4 * NT * 16;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bool rowv = oy0 + 2 * wave + i < p.H;
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const float d = acc[i][j][rg] + bv[j] - mean[j];
          a += (rowv && ox0 + lq * 4 + rg < p.W) ? d * d : 0.f;
        }
      }
      a += __shfl_xor(a, 16, 64);
      a += __shfl_xor(a, 32, 64);
      if (lq == 0) red2[wave * NT * 16 + j * 16 + lr] = a;
    }
    __syncthreads();
    if (wave == 0 && lq == 0) {
      float* dst = p.stats + (int64_t)tt * 2 * p.scs + col0;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int c = j * 16 + lr;
        if (c < width) {
          const bool cv = c < nv;
          dst[c] = cv ? s[j] : 0.f;
          dst[p.scs + c] = cv ? (red2[c] + red2[NT * 16 + c]) + (red2[2 * NT * 16 + c] + red2[3 * NT * 16 + c]) : 0.f;
        }
      }
    }
    __syncthreads();   // red is reused by the next sub-convolution
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int oy = oy0 + 2 * wave + i;
    if (oy >= p.H) continue;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const int ox = ox0 + lq * 4 + rg;
      if (ox >= p.W) continue;
      float* yo = p.ys[k] + (((int64_t)n * p.H + oy) * p.W + ox) * p.ycs3[k] + col0;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int co = j * 16 + lr;
        if (co < nv) yo[co] = acc[i][j][rg] + bv[j];
        else if (co < width) yo[co] = 0.f;
      }
    }
  }
}

}  // namespace cat_pk
