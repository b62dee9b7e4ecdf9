// The body of the LDS-tile convolution kernel, shared by tconv_kernel<NT, TW> (csrc/conv_pk.hip: patch (8 + 4) x (TW + 4), 128 table entries)
// and tconv7_kernel<NT> (csrc/conv_pk7.hip: patch (8 + 6) x (16 + 6), 256 table entries for the 196 (tap, quad) pairs of a 7 x 7 chunk).
// Moved here verbatim from conv_pk.hip.  The including kernel provides, in scope: the template parameters NT and TW, its arguments
// (g, pack, bias, y, L), `constexpr int HALO` (hl + hr the staged patch is sized for) and `constexpr int KTAB` (entries of one A-offset table),
// and a __device__ float g_zero[4] of its translation unit.
  constexpr int MT = TW / 8;
  constexpr int MAXIT = ((TH + HALO) * (TW + HALO) * 4 + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tile_floats = L.tr * L.tc * PITCH;
  float* tile0 = smem;
  int* tab0 = reinterpret_cast<int*>(smem + 2 * tile_floats);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lq = lane >> 4;
  // block -> (image, tile, N block): N blocks of one tile are adjacent (they stage the same patch), tiles of one image adjacent
  const int bid = cat::xcd_remap(blockIdx.x, gridDim.x);
  const int nb = bid % L.nblk, tt = bid / L.nblk;
  const int n = tt / L.tiles, t = tt - n * L.tiles;
  const int oy0 = (t / L.tiles_x) * TH, ox0 = (t % L.tiles_x) * TW;
  const int j0 = nb * NT;
  const int slots = L.tr * L.tc * 4;
  const int quad = tid & 3;
  const int abl = cat::kDiag ? L.ablate : 0;

  // staging map: this thread's patch pixels (independent of the segment)
  int sy[MAXIT], sx[MAXIT];
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int pix = (tid + it * 256) >> 2;
    const int r = pix / L.tc;
    sy[it] = oy0 - L.hl + r;
    sx[it] = ox0 - L.hl + (pix - r * L.tc);
  }

  // cursor over (segment, 16-channel chunk)
  int cs_ = 0, cc0 = 0;                 // segment, first channel of the chunk
  int64_t cpack = g.seg[0].pack_off;    // float offset of the chunk's packed filters
  unsigned soff[MAXIT];
  unsigned smask = 0;
  auto locate = [&](int s) {   // source offsets of the patch pixels for segment s
    const int refl = g.seg[s].reflect, xcs = g.seg[s].xcs;
    smask = 0;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      int iy = sy[it], ix = sx[it];
      bool v = tid + it * 256 < slots;
      if (refl) {
        v = v && iy > -g.H && iy < 2 * g.H - 1 && ix > -g.W && ix < 2 * g.W - 1;
        iy = cat::reflect_idx(iy, g.H);
        ix = cat::reflect_idx(ix, g.W);
      } else {
        v = v && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
      }
      smask |= v ? (1u << it) : 0u;
      soff[it] = v ? ((unsigned)(n * g.H + iy) * (unsigned)g.W + (unsigned)ix) * (unsigned)xcs + quad * 4 : 0u;   // < 2^32 elements (host-checked)
    }
    if (abl & 4) smask = 0;
  };
  f4 sreg[MAXIT], ssc, ssh;
  int s_act = 0;
  float s_neg = 1.f;
  bool s_aff = false, s_qv = false;
  auto gload = [&](int s, int c0) {
    const float* src = g.seg[s].src;
    s_qv = c0 + quad * 4 < g.seg[s].c4;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const bool v = ((smask >> it) & 1u) && s_qv;
      sreg[it] = *reinterpret_cast<const f4*>(v ? src + soff[it] + c0 : g_zero);
    }
    s_aff = g.seg[s].scale != nullptr;
    s_act = g.seg[s].act;
    s_neg = s_act == CAT_ACT_RELU ? 0.f : (s_act == CAT_ACT_LRELU ? g.seg[s].slope : 1.f);
    if (s_aff) {
      const int so = n * g.seg[s].sstride + c0 + quad * 4;
      ssc = *reinterpret_cast<const f4*>(s_qv ? g.seg[s].scale + so : g_zero);
      ssh = *reinterpret_cast<const f4*>(s_qv ? g.seg[s].shift + so : g_zero);
    }
  };
  auto sstore = [&](int buf, int s, int c0) {
    float* tile = tile0 + buf * tile_floats;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int idx = tid + it * 256;
      f4 v = sreg[it];
      if (s_aff || s_act) {   // wave-uniform
        const bool ok = ((smask >> it) & 1u) && s_qv;   // padding pixels / channels stay exactly 0
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float a = s_aff ? fmaf(v[e], ssc[e], ssh[e]) : v[e];
          a = a > 0.f ? a : a * s_neg;      // s_neg: 0 (ReLU), slope (LeakyReLU), 1 (none)
          v[e] = ok ? a : 0.f;
        }
      }
      if (idx < slots) *reinterpret_cast<f4*>(tile + (idx >> 2) * PITCH + quad * 4) = v;
    }
    // per-lane-quarter A offsets of every MFMA group of this chunk: pair p = 4 g + lq -> (tap, channel quad)
    const int ks = g.seg[s].ks, taps = ks * ks;
    const int nq = min(4, (g.seg[s].c4 - c0) >> 2);
    const int ngr = (taps * nq + 3) >> 2;
    if (tid < KTAB) {
      int off = 0;
      if (tid < ngr * 4) {
        const int tap = tid / nq, qd = tid - tap * nq;
        if (tap < taps) {
          const int ky = tap / ks, kx = tap - ky * ks;
          const int d = L.hl - g.seg[s].padv;
          off = ((d + ky) * L.tc + d + kx) * PITCH + qd * 4;
        }
      }
      tab0[buf * KTAB + tid] = (abl & 2) ? 0 : off;
    }
  };

  f4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

  int abase[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int row = 2 * wave + (MT == 2 ? i : (i >> 1)), col = (MT == 2 ? 0 : (i & 1) * 16) + lr;
    abase[i] = (row * L.tc + col) * PITCH;
  }
  // B stream of this lane: [group][N tile][lane][4]; tiles beyond the output's last one re-read the last valid tile (masked at the store)
  // packed filters through a buffer resource: per-lane byte offset in voffset, the group's offset in soffset (scalar) -- no vector
  // ALU address arithmetic in the MFMA stream
  const __amdgpu_buffer_rsrc_t prsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pack), 0, 0x7fffffff, 0x00020000);
  unsigned jb[NT];   // byte offsets inside one group
#pragma unroll
  for (int j = 0; j < NT; ++j) jb[j] = (unsigned)(min(j0 + j, L.nt_total - 1) * 64 + lane) * 16u;
  const int gstride = L.nt_total * 256;

  locate(0);
  gload(0, 0);
  sstore(0, 0, 0);
  __syncthreads();
  int buf = 0;
  while (true) {
    // next chunk
    int ns = cs_, nc0 = cc0 + 16;
    const int ks = g.seg[cs_].ks, taps = ks * ks;
    const int nq = min(4, (g.seg[cs_].c4 - cc0) >> 2);
    const int ngr = (taps * nq + 3) >> 2;
    int64_t npack = cpack + (int64_t)ngr * gstride;
    if (nc0 >= g.seg[cs_].c4) {
      ++ns;
      nc0 = 0;
      if (ns < g.nseg) {
        npack = g.seg[ns].pack_off;
        locate(ns);
      }
    }
    const bool more = ns < g.nseg;
    const bool stage = !(abl & 8);
    if (more && stage) gload(ns, nc0);   // in flight behind this chunk's MFMA stream

    mma_groups<MT, NT>(acc, tile0 + buf * tile_floats, tab0 + buf * KTAB + lq, abase, prsrc, jb, (abl & 1) ? 0u : (unsigned)cpack * 4u,
                       (abl & 1) ? 0u : (unsigned)gstride * 4u, ngr);
    if (!more) break;
    if (stage) {
      sstore(buf ^ 1, ns, nc0);
      __syncthreads();
      buf ^= 1;
    }
    cs_ = ns;
    cc0 = nc0;
    cpack = npack;
  }

  if (g.stats) {
    // per-tile sum and sum of squared deviations from the TILE mean of the pre-activation output (two passes over the accumulators:
    // no E[x^2] - E[x]^2 cancellation); cat_tnorm_finalize merges the tiles with the exact pairwise formula
    float* red = smem + 2 * tile_floats + 2 * KTAB;   // [2][4 waves][NT * 16]
    const int cnt = min(TH, g.Ho - oy0) * min(TW, g.Wo - ox0);
    float s[NT], mean[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int co = (j0 + j) * 16 + lr;
      const float b = (bias && co < g.Nn) ? bias[co] : 0.f;
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const bool rowv = oy0 + 2 * wave + (MT == 2 ? i : (i >> 1)) < g.Ho;
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const bool v = rowv && ox0 + (MT == 2 ? 0 : (i & 1) * 16) + lq * 4 + rg < g.Wo;
          a += v ? acc[i][j][rg] + b : 0.f;
        }
      }
      a += __shfl_xor(a, 16, 64);
      a += __shfl_xor(a, 32, 64);
      s[j] = a;
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
      const int co = (j0 + j) * 16 + lr;
      const float b = (bias && co < g.Nn) ? bias[co] : 0.f;
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const bool rowv = oy0 + 2 * wave + (MT == 2 ? i : (i >> 1)) < g.Ho;
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const bool v = rowv && ox0 + (MT == 2 ? 0 : (i & 1) * 16) + lq * 4 + rg < g.Wo;
          const float d = acc[i][j][rg] + b - mean[j];
          a += v ? d * d : 0.f;
        }
      }
      a += __shfl_xor(a, 16, 64);
      a += __shfl_xor(a, 32, 64);
      if (lq == 0) red2[wave * NT * 16 + j * 16 + lr] = a;
    }
    __syncthreads();
    if (wave == 0 && lq == 0) {
      float* dst = g.stats + (int64_t)tt * 2 * g.scs;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int c = j * 16 + lr, co = (j0 + j) * 16 + lr;
        if (j0 + j < L.nt_total && co < g.ycw) {
          const bool cv = co < g.Nn;
          dst[co] = cv ? s[j] : 0.f;
          dst[g.scs + co] = cv ? (red2[c] + red2[NT * 16 + c]) + (red2[2 * NT * 16 + c] + red2[3 * NT * 16 + c]) : 0.f;
        }
      }
    }
  }

#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int oy = oy0 + 2 * wave + (MT == 2 ? i : (i >> 1));
    if (oy >= g.Ho) continue;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const int ox = ox0 + (MT == 2 ? 0 : (i & 1) * 16) + lq * 4 + rg;
      if (ox >= g.Wo) continue;
      float* yo = y + (((int64_t)n * g.Ho + oy) * g.Wo + ox) * g.ycs;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int co = (j0 + j) * 16 + lr;
        if (j0 + j >= L.nt_total) continue;
        if (co < g.Nn) {
          float v = cat::apply_act(acc[i][j][rg] + (bias ? bias[co] : 0.f), g.act, g.slope);
          if (g.res) v += g.res[(((int64_t)n * g.Ho + oy) * g.Wo + ox) * g.rcs + co];
          yo[co] = v;
        } else if (co < g.ycw) {
          yo[co] = 0.f;
        }
      }
    }
  }
