// The statistics epilogue of the one-launch wide stage 1, shared by tstage1ws_kernel (csrc/conv_s1ws.hip: kernel sizes 1 3 5, three slots)
// and tstage1ws7_kernel (csrc/conv_s1ws7.hip: kernel sizes 3 5 7, four slots).  Moved here verbatim from conv_s1ws.hip; the kernel argument
// is a template parameter because the two kernels' argument structs differ in their slot count.  It reads p.bias, p.y, p.stats, p.H, p.W,
// p.ycs, p.scs, p.col0[], p.width[].
//
// Statistics (the formula and the reduction scheme of s1_epilogue<NT, true>, conv_pk.hip): per 8 x 16 tile and channel the sum over the
// tile's valid pixels and the sum of squared deviations from the TILE mean, two passes over the accumulators -- pixel columns rg and rows i in
// registers, the lane quarters lq by two xor shuffles, the four waves through LDS.  Deterministic, no atomics.
#pragma once
#include "conv_pk_tile.h"

namespace cat_s1ws_epi {

using namespace cat_pk;      // TH, f4

constexpr int NT = 3;      // N tiles per accumulator set
constexpr int RED_FLOATS = 8 * NT * 16;      // the LDS an epilogue reduces through: [2][4][NT * 16] floats

// One accumulator set = N tiles [t0, t0 + 3) of slot k: columns col0[k] + t0 * 16 + [0, 48) as far as they lie inside the slot's width.
// Padding columns inside the slice carry zero filters and a zero bias: plain zeros come out, in y and in the table.
// red: RED_FLOATS floats of LDS.
template <class A>
__device__ __forceinline__ void epilogue(const f4 (&acc)[2][NT], const A& p, int k, int t0, int n, int tt, int oy0, int ox0, int wave, int lr,
                                         int lq, float* red) {
  const int col0 = p.col0[k] + t0 * 16, width = p.width[k] - t0 * 16;      // this set's first column; columns left in the slot (may be <= 0)
  const int cnt = min(TH, p.H - oy0) * min(16, p.W - ox0);
  float s[NT], mean[NT], bv[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int co = j * 16 + lr;
    bv[j] = (p.bias && co < width) ? p.bias[col0 + co] : 0.f;
  }
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
        dst[c] = s[j];
        dst[p.scs + c] = (red2[c] + red2[NT * 16 + c]) + (red2[2 * NT * 16 + c] + red2[3 * NT * 16 + c]);
      }
    }
  }
  __syncthreads();   // red is reused by the next accumulator set
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int oy = oy0 + 2 * wave + i;
    if (oy >= p.H) continue;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const int ox = ox0 + lq * 4 + rg;
      if (ox >= p.W) continue;
      float* yo = p.y + (((int64_t)n * p.H + oy) * p.W + ox) * p.ycs + col0;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int co = j * 16 + lr;
        if (co < width) yo[co] = acc[i][j][rg] + bv[j];
      }
    }
  }
}

}  // namespace cat_s1ws_epi
