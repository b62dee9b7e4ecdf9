// The staging half of the 3 5 7 stage-1 kernels on the (8 + 6) x (16 + 6) patch: A FUNCTION-BODY FRAGMENT, moved here verbatim from
// conv_s1w7_main.h, which includes it at the place the text stood (so the kernels of conv_s1w7.hip and conv_s1ws7.hip compile to exactly what
// they did), and included by tstage1n7_kernel (csrc/conv_s1n7.hip), whose K walk differs.
//
// It expects, in scope: the kernel argument `p` with x, xcs, c4, H, W, reflect, tiles_x, tiles; g_zero (four zero floats in global memory);
// cat_pk's TH, PITCH; the declarations of conv_s1w7_main.h (CAT_S1W7_DECLS).  It leaves smem (the dynamic LDS), tile0 / tab0 (the two tiles and
// the [buf][slot][KTAB] A-offset tables), tid, lane, wave, lr, lq, tt, n, oy0, ox0 and the lambdas gload(c0) (global -> registers) and
// sstore(buf, c0) (registers -> LDS tile + the chunk's A-offset tables of all four slots).
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
