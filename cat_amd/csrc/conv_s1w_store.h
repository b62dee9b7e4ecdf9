// The store of the buffer-per-slot stage-1 kernels (tstage1w_kernel, conv_pk.hip; tstage1w7_kernel, conv_s1w7.hip), one text for both,
// a forced-inline template on the argument struct (fields y[], ycs[], nvalid[], bias[], act, slope, H, W).
#pragma once
#include "conv_pk_tile.h"

namespace cat_pk {

// N tiles [t0, t0 + NT) of slot k: bias + activation; columns [nvalid, ycs) inside the slot's tiles come out as 0, columns of a wider
// pixel stride beyond the tiles are not touched
template <int NT, class A>
__device__ __forceinline__ void s1w_store(const f4 (&acc)[2][NT], const A& p, int k, int t0, int n, int oy0, int ox0, int wave, int lr, int lq) {
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

}  // namespace cat_pk
