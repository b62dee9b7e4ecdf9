// The main loop of the wide stage 1 (the teacher's 3 + 3 + 11 N tiles), shared by tstage1w_kernel (csrc/conv_pk.hip: bias + activation into three
// buffers) and tstage1ws_kernel (csrc/conv_s1ws.hip: pre-norm slices of one buffer + per-tile statistics).  A FUNCTION-BODY FRAGMENT, moved
// here verbatim from tstage1w_kernel and included textually inside both kernels, so that either compiles to exactly what it would with the
// text in place (the code generation of conv_pk.hip is pinned, tests/test_codegen.py; a function template around this loop changed the
// register allocation of tstage1w_kernel).  Expects, in scope: template parameters N5, N3, N1; the kernel argument `p` with x, pack[3], xcs,
// c4, N, H, W, reflect, hl, tr, tc, tiles_x, tiles; g_zero (four zero floats in global memory); cat_pk's TH, PITCH, TABN, mma_groups, wload,
// wmma.  Leaves: the accumulators acc5, acc3, accA .. accD (the 1 x 1 slot in passes of three N tiles; P1 passes, R1 tiles in the last)
// and n, tt, oy0, ox0, wave, lr, lq for the epilogue.  Dynamic LDS: two tiles of tr x tc x PITCH floats, then 6 x TABN A offsets.
  constexpr int MT = 2, TW = 16, MAXIT = ((TH + 4) * (TW + 4) * 4 + 255) / 256;
  constexpr int P1 = (N1 + 2) / 3, R1 = N1 - 3 * (P1 - 1);      // passes over the 1 x 1 slot, tiles of the last one (1..3)
  static_assert(N1 >= 1 && N1 <= 12 && N5 >= 1 && N5 <= 3 && N3 >= 1 && N3 <= 3, "tile counts");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tile_floats = p.tr * p.tc * PITCH;
  float* tile0 = smem;
  int* tab0 = reinterpret_cast<int*>(smem + 2 * tile_floats);      // [buf][3][TABN]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lq = lane >> 4;
  const int tt = cat::xcd_remap(blockIdx.x, gridDim.x);
  const int n = tt / p.tiles, t = tt - n * p.tiles;
  const int oy0 = (t / p.tiles_x) * TH, ox0 = (t % p.tiles_x) * TW;
  const int slots = p.tr * p.tc * 4, quad = tid & 3;
  unsigned soff[MAXIT], smask = 0;
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int pix = (tid + it * 256) >> 2;
    const int r = pix / p.tc;
    int iy = oy0 - p.hl + r, ix = ox0 - p.hl + (pix - r * p.tc);
    bool v = tid + it * 256 < slots;
    if (p.reflect) {
      v = v && iy > -p.H && iy < 2 * p.H - 1 && ix > -p.W && ix < 2 * p.W - 1;
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
    float* tile = tile0 + buf * tile_floats;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int idx = tid + it * 256;
      if (idx < slots) *reinterpret_cast<f4*>(tile + (idx >> 2) * PITCH + quad * 4) = sreg[it];
    }
    const int nq = min(4, (p.c4 - c0) >> 2);
    if (tid < TABN) {
      const int tap = tid / nq, qd = tid - tap * nq;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int ks = k == 0 ? 5 : (k == 1 ? 3 : 1), taps = ks * ks;
        int off = 0;
        if (tid < ((taps * nq + 3) >> 2) * 4 && tap < taps) {
          const int ky = tap / ks, kx = tap - ky * ks, d = p.hl - (ks >> 1);
          off = ((d + ky) * p.tc + d + kx) * PITCH + qd * 4;
        }
        tab0[(buf * 3 + k) * TABN + tid] = off;
      }
    }
  };
  const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f4 acc5[MT][N5], acc3[MT][N3], accA[MT][3], accB[MT][3], accC[MT][3], accD[MT][3];      // the 1 x 1 slot: passes A..D of up to 3 tiles
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int j = 0; j < N5; ++j) acc5[i][j] = zero4;
#pragma unroll
    for (int j = 0; j < N3; ++j) acc3[i][j] = zero4;
#pragma unroll
    for (int j = 0; j < 3; ++j) accA[i][j] = accB[i][j] = accC[i][j] = accD[i][j] = zero4;
  }
  int abase[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) abase[i] = ((2 * wave + i) * p.tc + lr) * PITCH;
  const __amdgpu_buffer_rsrc_t r5 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.pack[0]), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t r3 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.pack[1]), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.pack[2]), 0, 0x7fffffff, 0x00020000);
  unsigned jb5[N5], jb3[N3], jb1[4][3];
#pragma unroll
  for (int j = 0; j < N5; ++j) jb5[j] = (unsigned)(j * 64 + lane) * 16u;
#pragma unroll
  for (int j = 0; j < N3; ++j) jb3[j] = (unsigned)(j * 64 + lane) * 16u;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int j = 0; j < 3; ++j) jb1[q][j] = (unsigned)(min(3 * q + j, N1 - 1) * 64 + lane) * 16u;
  unsigned so5 = 0, so3 = 0, so1 = 0;     // byte offsets of the current chunk in the three streams
  gload(0);
  sstore(0, 0);
  __syncthreads();
  int buf = 0;
  for (int c0 = 0; c0 < p.c4; c0 += 16) {
    const bool more = c0 + 16 < p.c4;
    if (more) gload(c0 + 16);
    const int nq = min(4, (p.c4 - c0) >> 2);
    const float* tile = tile0 + buf * tile_floats;
    const int* tab = tab0 + buf * 3 * TABN + lq;
    f4 bw[3];
    wload<(P1 == 1 ? R1 : 3)>(bw, r1, jb1[0], so1);
    {
      const int ngr = (25 * nq + 3) >> 2;
      mma_groups<MT, N5>(acc5, tile, tab, abase, r5, jb5, so5, (unsigned)N5 * 1024u, ngr);
      so5 += (unsigned)ngr * N5 * 1024u;
    }
    {
      const int ngr = (9 * nq + 3) >> 2;
      mma_groups<MT, N3>(acc3, tile, tab + TABN, abase, r3, jb3, so3, (unsigned)N3 * 1024u, ngr);
      so3 += (unsigned)ngr * N3 * 1024u;
    }
    {
      // the 1 x 1 slot: ONE group per chunk (the centre tap's four quads), N1 tiles wide -- the A fragments are read once, the filter
      // blocks of pass q + 1 are in flight behind the MFMAs of pass q, those of pass 0 were requested at the top of the chunk
      f4 aw[MT], bx[3];
      const int off = tab[2 * TABN];
#pragma unroll
      for (int i = 0; i < MT; ++i) aw[i] = *reinterpret_cast<const f4*>(tile + abase[i] + off);
      if constexpr (P1 > 1) wload<(P1 == 2 ? R1 : 3)>(bx, r1, jb1[1], so1);
      __builtin_amdgcn_sched_barrier(0);
      wmma<MT, (P1 == 1 ? R1 : 3)>(accA, aw, bw);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (P1 > 1) {
        if constexpr (P1 > 2) wload<(P1 == 3 ? R1 : 3)>(bw, r1, jb1[2], so1);
        __builtin_amdgcn_sched_barrier(0);
        wmma<MT, (P1 == 2 ? R1 : 3)>(accB, aw, bx);
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (P1 > 2) {
        if constexpr (P1 > 3) wload<R1>(bx, r1, jb1[3], so1);
        __builtin_amdgcn_sched_barrier(0);
        wmma<MT, (P1 == 3 ? R1 : 3)>(accC, aw, bw);
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (P1 > 3) wmma<MT, R1>(accD, aw, bx);
    }
    so1 += (unsigned)N1 * 1024u;
    if (more) {
      sstore(buf ^ 1, c0 + 16);
      __syncthreads();
      buf ^= 1;
    }
  }
