// The 1x1 PixelGAN discriminator as a per-pixel MLP (gfx950).
//
// Reference: models/modules/discriminators.py:82-126 -- Conv2d(C0, C1, 1) -> LeakyReLU(0.2) -> Conv2d(C1, C2 = 2 C1, 1) -> norm -> LeakyReLU(0.2)
// -> Conv2d(C2, 1, 1).  Layer by layer that writes and re-reads h1 [M][C1], the pre-norm tensor z [M][C2] five times and the activated tensor;
// here only z ever reaches HBM:
//   pd_fwd1   persistent; W2 resident in LDS ([C2][C1 + 4], 132 KB at ndf 128: one workgroup per CU), 32-pixel tiles: x -> h1 (VALU, K = C0) into
//             LDS -> z = h1 W2^T on v_mfma_f32_32x32x2_f32 -> HBM, with (sum, M2) per channel merged over 8 tiles (Chan) into one table entry of
//             256 pixels; entries never straddle images.  cat_tnorm_finalize2 turns the table into scale / shift / mean / rstd.
//   pd_fwd3   out = w3 . lrelu(scale z + shift) + b3: 16 lanes per pixel, one pass over z.
//   pd_bwd1   one pass over z and dout: partial sums of dout a (net.5.weight), g and g zhat per channel and image; pd_bwd1_reduce (one wave per channel) adds them in a
//             fixed order, leaves the coefficient rows of dz and writes the gradients of net.5 and of the norm's affine.
//   pd_bwd2   persistent, 64-pixel tiles, 8 waves: dz and the recomputed h1 into LDS; dW2 += dz^T h1 (MFMA, accumulators held over the tile
//             loop), dh1 = dz W2 (MFMA, W2 streamed from L2), dp1 = dh1 lrelu'(p1) over h1 in LDS, then dW1 / db1 / db2 sums and dx on the
//             VALU.  <PARAMS, DX> are compile-time; pd_bwd2_reduce adds the per-workgroup partials in workgroup order.
// No float atomics anywhere: two runs give the same bits.
#include <algorithm>
#include <atomic>

#include "common.h"

namespace {
using cat::cdiv;

typedef float f16v __attribute__((ext_vector_type(16)));

constexpr int FT = 32;       // pixels per MFMA tile of pd_fwd1
constexpr int FSUB = 8;      // tiles merged into one statistics entry
constexpr int BT = 64;       // pixels per tile of pd_bwd2
constexpr int kMinWalk = 4;  // fewest tiles of a persistent workgroup
constexpr int NCOEF = 7;     // scale, shift, mean, rstd, scale * w3, mean(g), mean(g zhat)

__device__ __forceinline__ int pix_of(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }   // C/D row of register r, lane half h

__device__ __forceinline__ float lrelu(float v, float s) { return v > 0.f ? v : v * s; }

// One pixel's input into registers: zeros past C0 (pad lanes are never read) and for pixels past the tile.
__device__ __forceinline__ void load_x(const float* __restrict__ x, int64_t px, bool valid, int C0, int xcs, float (&xr)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) xr[k] = (valid && k < C0) ? x[px * xcs + k] : 0.f;
}

// h1 of one tile into hs[pix][ld].  Thread tid owns pixel tid >> 3 (its input in xr) and the channels (tid & 7) + 8 j; columns [C1, C1p) and
// pixels past the tile are written 0.  The 8 products are added in channel order (the lanes past C0 add exact zeros).
__device__ __forceinline__ void stage_h1(const float (&xr)[8], bool valid, const float* __restrict__ w1s, const float* __restrict__ b1s,
                                         float* __restrict__ hs, int C1, int C1p, int ld, float slope, int tid) {
  float* hp = hs + (tid >> 3) * ld;
#pragma unroll 2
  for (int c = tid & 7; c < C1p; c += 8) {
    float v = 0.f;
    if (c < C1 && valid) {
      const f4 wa = *reinterpret_cast<const f4*>(w1s + c * 8), wb = *reinterpret_cast<const f4*>(w1s + c * 8 + 4);
      v = b1s[c];
#pragma unroll
      for (int k = 0; k < 4; ++k) v = fmaf(wa[k], xr[k], v);
#pragma unroll
      for (int k = 0; k < 4; ++k) v = fmaf(wb[k], xr[4 + k], v);
      v = lrelu(v, slope);
    }
    hp[c] = v;
  }
}

__device__ __forceinline__ void stage_w1(const float* __restrict__ w1, const float* __restrict__ b1, float* __restrict__ w1s, float* __restrict__ b1s,
                                         int C0, int C1, int w1cs, int tid, int nthr) {
  for (int i = tid; i < C1 * 8; i += nthr) {
    const int c = i >> 3, k = i & 7;
    w1s[i] = k < C0 ? w1[c * w1cs + k] : 0.f;
  }
  for (int i = tid; i < C1; i += nthr) b1s[i] = b1[i];
}

// ------------------------------------------------------------------------------------------------------------------------------- forward
__global__ __launch_bounds__(256) void pd_fwd1(cat_pixeld_t p, int tiles, const float* __restrict__ x, const float* __restrict__ w1,
                                               const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                               float* __restrict__ z, float* __restrict__ table) {
  extern __shared__ f4 smem4[];
  float* sm = reinterpret_cast<float*>(smem4);
  const int C1 = p.C1, C2 = p.C2, ld = C1 + 4;
  float* w2s = sm;                    // [C2][ld]
  float* hs = w2s + C2 * ld;          // [FT][ld]
  float* w1s = hs + FT * ld;          // [C1][8]
  float* b1s = w1s + C1 * 8;          // [C1]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int q1 = C1 >> 2;
  for (int i = tid; i < C2 * q1; i += 256) {
    const int r = i / q1, c4 = i - r * q1;
    *reinterpret_cast<f4*>(w2s + r * ld + c4 * 4) = *reinterpret_cast<const f4*>(w2 + (int64_t)r * C1 + c4 * 4);
  }
  stage_w1(w1, b1, w1s, b1s, p.C0, C1, p.w1cs, tid, 256);
  const int ntl = C2 >> 5;      // 32-channel tiles; this wave owns tiles wv and wv + 4
  const bool has0 = wv < ntl, has1 = wv + 4 < ntl;
  const int c0 = wv * 32 + l31, c1 = (wv + 4) * 32 + l31;
  const float bias0 = (b2 && has0) ? b2[c0] : 0.f, bias1 = (b2 && has1) ? b2[c1] : 0.f;
  const int total = p.N * tiles;
  const int pix = tid >> 3;      // 256 threads = 32 pixels x 8 lanes
  int st = blockIdx.x, u = 0;
  bool live = st < total;
  float xr[8];
  if (live) {
    const int n = st / tiles, s = st - n * tiles;
    load_x(x, (int64_t)n * p.HW + s * (FT * FSUB) + pix, s * (FT * FSUB) + pix < p.HW, p.C0, p.xcs, xr);
  }
  float rsum0 = 0.f, rm20 = 0.f, rsum1 = 0.f, rm21 = 0.f, rn = 0.f;
  while (live) {
    const int n = st / tiles, s = st - n * tiles;
    const int px0 = s * (FT * FSUB) + u * FT;
    const int nvalid = min(FT, p.HW - px0);
    const int64_t base = (int64_t)n * p.HW + px0;
    if (u == 0) rsum0 = rm20 = rsum1 = rm21 = rn = 0.f;
    __syncthreads();      // the previous tile's h1 has been consumed
    stage_h1(xr, pix < nvalid, w1s, b1s, hs, C1, C1, ld, p.slope1, tid);
    __syncthreads();
    // the next tile of this workgroup: its input is fetched while this one is multiplied
    int nst = st, nu = u + 1;
    if (nu >= FSUB || px0 + FT >= p.HW) nst = st + gridDim.x, nu = 0;
    const bool nlive = nst < total;
    if (nlive) {
      const int nn = nst / tiles, ns = nst - nn * tiles;
      const int npx = ns * (FT * FSUB) + nu * FT + pix;
      load_x(x, (int64_t)nn * p.HW + npx, npx < p.HW, p.C0, p.xcs, xr);
    }
    f16v a0 = {0}, a1 = {0};
    if (has0) {
      const float* ap = hs + l31 * ld + 4 * h;
      const float* bp0 = w2s + c0 * ld + 4 * h;
      const float* bp1 = w2s + (has1 ? c1 : c0) * ld + 4 * h;
      // k order permuted alike for both operands: lane half h takes k = 8 j + 4 h + e
      if (has1) {
        for (int j0 = 0; j0 < (C1 >> 3); j0 += 2) {      // C1 % 16 == 0: two k groups per trip, their LDS reads issued together
          f4 av[2], bv0[2], bv1[2];
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) {
            av[jj] = *reinterpret_cast<const f4*>(ap + 8 * (j0 + jj));
            bv0[jj] = *reinterpret_cast<const f4*>(bp0 + 8 * (j0 + jj));
            bv1[jj] = *reinterpret_cast<const f4*>(bp1 + 8 * (j0 + jj));
          }
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[jj][e], bv0[jj][e], a0, 0, 0, 0);
              a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[jj][e], bv1[jj][e], a1, 0, 0, 0);
            }
          }
        }
      } else {
        for (int j0 = 0; j0 < (C1 >> 3); j0 += 2) {
          f4 av[2], bv0[2];
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) {
            av[jj] = *reinterpret_cast<const f4*>(ap + 8 * (j0 + jj));
            bv0[jj] = *reinterpret_cast<const f4*>(bp0 + 8 * (j0 + jj));
          }
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) {
#pragma unroll
            for (int e = 0; e < 4; ++e) a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[jj][e], bv0[jj][e], a0, 0, 0, 0);
          }
        }
      }
    }
    // epilogue: rows = pixels, column = this lane's channel; tile statistics merged into the entry's running (sum, M2)
    const float fn = (float)nvalid;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (!(t ? has1 : has0)) continue;
      const f16v& a = t ? a1 : a0;
      const float bias = t ? bias1 : bias0;
      const int c = t ? c1 : c0;
      float v[16], sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int pr = pix_of(r, h);
        v[r] = a[r] + bias;
        if (pr < nvalid) {
          z[(base + pr) * C2 + c] = v[r];
          sum += v[r];
        }
      }
      sum += __shfl_xor(sum, 32, 64);
      const float tm = sum / fn;
      float m2 = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (pix_of(r, h) < nvalid) m2 += (v[r] - tm) * (v[r] - tm);
      m2 += __shfl_xor(m2, 32, 64);
      float& rs = t ? rsum1 : rsum0;
      float& rm = t ? rm21 : rm20;
      if (rn > 0.f) {
        const float d = tm - rs / rn;
        rm += m2 + d * d * rn * fn / (rn + fn);
      } else {
        rm = m2;
      }
      rs += sum;
    }
    rn += fn;
    if (nu == 0 && h == 0) {      // the entry is complete
      float* dst = table + (int64_t)st * 2 * C2;
      if (has0) dst[c0] = rsum0, dst[C2 + c0] = rm20;
      if (has1) dst[c1] = rsum1, dst[C2 + c1] = rm21;
    }
    st = nst, u = nu, live = nlive;
  }
}

// 16 lanes per pixel; lane `sub` owns the channel quads sub, sub + 16, ... (at most 4)
__global__ __launch_bounds__(256) void pd_fwd3(cat_pixeld_t p, const float* __restrict__ z, const float* __restrict__ scale, const float* __restrict__ shift,
                                               const float* __restrict__ w3, const float* __restrict__ b3, float* __restrict__ out) {
  const int tid = threadIdx.x, slot = tid >> 4, sub = tid & 15;
  const int C2 = p.C2, nq = C2 >> 2;
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  f4 w[4], sc[4], sh[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = (sub + 16 * j < nq) ? *reinterpret_cast<const f4*>(w3 + (sub + 16 * j) * 4) : zero;
  const float bias = b3 ? b3[0] : 0.f;
  int curg = -1;
  const int64_t M = (int64_t)p.N * p.HW;
  for (int64_t px = (int64_t)blockIdx.x * 16 + slot; px < M; px += (int64_t)gridDim.x * 16) {
    const int g = p.groups > 1 ? (int)(px / p.HW) : 0;
    if (g != curg) {
      curg = g;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool v = sub + 16 * j < nq;
        sc[j] = v ? *reinterpret_cast<const f4*>(scale + (int64_t)g * C2 + (sub + 16 * j) * 4) : zero;
        sh[j] = v ? *reinterpret_cast<const f4*>(shift + (int64_t)g * C2 + (sub + 16 * j) * 4) : zero;
      }
    }
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (sub + 16 * j < nq) {
        const f4 zv = *reinterpret_cast<const f4*>(z + px * C2 + (sub + 16 * j) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf(w[j][e], lrelu(fmaf(sc[j][e], zv[e], sh[j][e]), p.slope2), acc);
      }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (sub == 0) *reinterpret_cast<f4*>(out + px * 4) = f4{acc + bias, 0.f, 0.f, 0.f};
  }
}

// ------------------------------------------------------------------------------------------------------------------------------- backward
// grid (b1_blocks, N); partial [(n * nb + b)][3][C2] (+ dout sums behind all of them)
__global__ __launch_bounds__(256) void pd_bwd1(cat_pixeld_t p, const float* __restrict__ z, const float* __restrict__ dout, const float* __restrict__ scale,
                                               const float* __restrict__ shift, const float* __restrict__ mean, const float* __restrict__ rstd,
                                               const float* __restrict__ w3, float* __restrict__ part, float* __restrict__ dpart) {
  __shared__ float red[16 * 3 * 256];
  __shared__ float dred[16];
  const int tid = threadIdx.x, slot = tid >> 4, sub = tid & 15;
  const int C2 = p.C2, nq = C2 >> 2, n = blockIdx.y, g = p.groups > 1 ? n : 0;
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  f4 w[4], sc[4], sh[4], mn[4], rs[4], aw[4], ag[4], agz[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool v = sub + 16 * j < nq;
    const int o = (sub + 16 * j) * 4;
    w[j] = v ? *reinterpret_cast<const f4*>(w3 + o) : zero;
    sc[j] = v ? *reinterpret_cast<const f4*>(scale + (int64_t)g * C2 + o) : zero;
    sh[j] = v ? *reinterpret_cast<const f4*>(shift + (int64_t)g * C2 + o) : zero;
    mn[j] = v ? *reinterpret_cast<const f4*>(mean + (int64_t)g * C2 + o) : zero;
    rs[j] = v ? *reinterpret_cast<const f4*>(rstd + (int64_t)g * C2 + o) : zero;
    aw[j] = ag[j] = agz[j] = zero;
  }
  float ad = 0.f;
  for (int pl = blockIdx.x * 16 + slot; pl < p.HW; pl += gridDim.x * 16) {
    const int64_t px = (int64_t)n * p.HW + pl;
    const float dv = dout[px * p.docs];
    ad += dv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (sub + 16 * j < nq) {
        const f4 zv = *reinterpret_cast<const f4*>(z + px * C2 + (sub + 16 * j) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float y = fmaf(sc[j][e], zv[e], sh[j][e]);
          const float d = y > 0.f ? 1.f : p.slope2;
          const float gg = dv * w[j][e] * d;
          aw[j][e] = fmaf(dv, y * d, aw[j][e]);
          ag[j][e] += gg;
          agz[j][e] = fmaf(gg, (zv[e] - mn[j][e]) * rs[j][e], agz[j][e]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (sub + 16 * j < nq) {
      const int o = (sub + 16 * j) * 4;
      *reinterpret_cast<f4*>(red + (slot * 3 + 0) * 256 + o) = aw[j];
      *reinterpret_cast<f4*>(red + (slot * 3 + 1) * 256 + o) = ag[j];
      *reinterpret_cast<f4*>(red + (slot * 3 + 2) * 256 + o) = agz[j];
    }
  }
  if (sub == 0) dred[slot] = ad;
  __syncthreads();
  const int64_t blk = (int64_t)n * gridDim.x + blockIdx.x;
  if (tid < C2) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      float s = 0.f;
      for (int sl = 0; sl < 16; ++sl) s += red[(sl * 3 + r) * 256 + tid];
      part[(blk * 3 + r) * C2 + tid] = s;
    }
  }
  if (tid == 0) {
    float s = 0.f;
    for (int sl = 0; sl < 16; ++sl) s += dred[sl];
    dpart[blk] = s;
  }
}

// grid C2 + 1, one wave each: workgroup c < C2 owns channel c -- its lanes stride over a group's partials and a fixed shuffle tree adds the 64
// lane sums (deterministic); workgroup C2 adds the dout sums
__global__ __launch_bounds__(64) void pd_bwd1_reduce(cat_pixeld_t p, int nb, const float* __restrict__ part, const float* __restrict__ dpart,
                                                     const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const float* __restrict__ w3, float* __restrict__ coef,
                                                     float* __restrict__ dw3, float* __restrict__ db3, float* __restrict__ dgamma,
                                                     float* __restrict__ dbeta, int accumulate) {
  const int c = blockIdx.x, lane = threadIdx.x, C2 = p.C2;
  if (c == C2) {
    if (db3) {
      float s = 0.f;
      for (int i = lane; i < p.N * nb; i += 64) s += dpart[i];
      s = cat::wave_sum(s);
      if (lane == 0) db3[0] = accumulate ? db3[0] + s : s;
    }
    return;
  }
  const int per = p.N / p.groups;      // images per group
  const float cnt = (float)per * (float)p.HW;
  float tw = 0.f, tg = 0.f, tgz = 0.f;
  for (int g = 0; g < p.groups; ++g) {
    float sw = 0.f, sg = 0.f, sgz = 0.f;
    for (int i = g * per * nb + lane; i < (g + 1) * per * nb; i += 64) {
      sw += part[((int64_t)i * 3 + 0) * C2 + c];
      sg += part[((int64_t)i * 3 + 1) * C2 + c];
      sgz += part[((int64_t)i * 3 + 2) * C2 + c];
    }
    sw = cat::wave_sum(sw);
    sg = cat::wave_sum(sg);
    sgz = cat::wave_sum(sgz);
    if (lane == 0) {
      float* k = coef + (int64_t)g * NCOEF * C2 + c;
      const float s = scale[(int64_t)g * C2 + c];
      k[0] = s;
      k[C2] = shift[(int64_t)g * C2 + c];
      k[2 * C2] = mean[(int64_t)g * C2 + c];
      k[3 * C2] = rstd[(int64_t)g * C2 + c];
      k[4 * C2] = s * w3[c];
      k[5 * C2] = sg / cnt;
      k[6 * C2] = sgz / cnt;
    }
    tw += sw;
    tg += sg;
    tgz += sgz;
  }
  if (lane != 0) return;
  if (dw3) dw3[c] = accumulate ? dw3[c] + tw : tw;
  if (dgamma) dgamma[c] = accumulate ? dgamma[c] + tgz : tgz;
  if (dbeta) dbeta[c] = accumulate ? dbeta[c] + tg : tg;
}

// partial layout of one workgroup: dW2 [C2][C1] | db2 [C2] | db1 [C1] | dW1 [C1][8]
__host__ __device__ inline int pd_partial_floats(int C1, int C2) { return C2 * C1 + C2 + C1 + C1 * 8; }

template <bool PARAMS, bool DX>
__global__ __launch_bounds__(512) void pd_bwd2(cat_pixeld_t p, int tpi, const float* __restrict__ x, const float* __restrict__ z, const float* __restrict__ dout,
                                               const float* __restrict__ coef, const float* __restrict__ w1, const float* __restrict__ b1,
                                               const float* __restrict__ w2, float* __restrict__ dx, float* __restrict__ part) {
  extern __shared__ f4 smem4[];
  float* sm = reinterpret_cast<float*>(smem4);
  const int C1 = p.C1, C2 = p.C2, C1p = (C1 + 31) & ~31, ld1 = C1p + 4, ld2 = C2 + 4;
  float* dzs = sm;                      // [BT][ld2]
  float* hs = dzs + BT * ld2;           // [BT][ld1]   h1, later dp1
  float* cf = hs + BT * ld1;            // [NCOEF][C2]
  float* w1s = cf + NCOEF * C2;         // [C1][8]
  float* b1s = w1s + C1 * 8;            // [C1]
  float* xs = b1s + C1;                 // [BT][8]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, h = lane >> 5;
  stage_w1(w1, b1, w1s, b1s, p.C0, C1, p.w1cs, tid, 512);
  const int nti = C2 >> 5, ntj = C1p >> 5;      // dW2 tiles: nti x ntj (<= 32), this wave owns tiles wv, wv + 8, wv + 16, wv + 24
  f16v aw2[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) aw2[m] = f16v{0};
  float adb2 = 0.f, adb1 = 0.f, adw1[2] = {0.f, 0.f};
  const int nq = C2 >> 2;
  const int total = p.N * tpi;
  int curg = -1;
  for (int t = blockIdx.x; t < total; t += gridDim.x) {
    const int n = t / tpi, s = t - n * tpi;
    const int nvalid = min(BT, p.HW - s * BT);
    const int64_t base = (int64_t)n * p.HW + s * BT;
    const int g = p.groups > 1 ? n : 0;
    const int pix = tid >> 3;      // 512 threads = 64 pixels x 8 lanes
    const bool pv = pix < nvalid;
    float xr[8];
    load_x(x, base + pix, pv, p.C0, p.xcs, xr);
    const float dv = pv ? dout[(base + pix) * p.docs] : 0.f;
    xs[tid] = xr[tid & 7];
    if (g != curg) {
      curg = g;
      for (int i = tid; i < NCOEF * C2; i += 512) cf[i] = coef[(int64_t)g * NCOEF * C2 + i];
    }
    __syncthreads();
    // dz = scale (g - mean(g) - zhat mean(g zhat)),  g = dout w3 lrelu'(scale z + shift)
#pragma unroll 2
    for (int q = tid & 7; q < nq; q += 8) {      // this thread's pixel, the quads (tid & 7) + 8 j
      f4 o = {0.f, 0.f, 0.f, 0.f};
      if (pv) {
        const f4 zv = *reinterpret_cast<const f4*>(z + (base + pix) * C2 + q * 4);
        const f4 ksc = *reinterpret_cast<const f4*>(cf + q * 4), ksh = *reinterpret_cast<const f4*>(cf + C2 + q * 4);
        const f4 kmn = *reinterpret_cast<const f4*>(cf + 2 * C2 + q * 4), krs = *reinterpret_cast<const f4*>(cf + 3 * C2 + q * 4);
        const f4 kp = *reinterpret_cast<const f4*>(cf + 4 * C2 + q * 4), kg = *reinterpret_cast<const f4*>(cf + 5 * C2 + q * 4);
        const f4 kgz = *reinterpret_cast<const f4*>(cf + 6 * C2 + q * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float y = fmaf(ksc[e], zv[e], ksh[e]);
          const float d = y > 0.f ? 1.f : p.slope2;
          const float zh = (zv[e] - kmn[e]) * krs[e];
          o[e] = dv * d * kp[e] - ksc[e] * (kg[e] + zh * kgz[e]);
        }
      }
      *reinterpret_cast<f4*>(dzs + pix * ld2 + q * 4) = o;
    }
    stage_h1(xr, pv, w1s, b1s, hs, C1, C1p, ld1, p.slope1, tid);
    __syncthreads();
    if (PARAMS) {      // dW2[c2][c1] += sum_p dz[p][c2] h1[p][c1]: A = dz^T, B = h1, k = pixel
      int ao[4], bo[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int tt = min(wv + 8 * m, nti * ntj - 1), ti = tt / ntj, tj = tt - ti * ntj;
        ao[m] = h * ld2 + ti * 32 + l31;
        bo[m] = h * ld1 + tj * 32 + l31;
      }
      const int nmine = (nti * ntj - wv + 7) >> 3;      // tiles of this wave (wave-uniform)
#pragma unroll 2
      for (int k = 0; k < BT / 2; ++k) {
        const float* ap = dzs + 2 * k * ld2;
        const float* bp = hs + 2 * k * ld1;
#pragma unroll
        for (int m = 0; m < 4; ++m)
          if (m < nmine) aw2[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[ao[m]], bp[bo[m]], aw2[m], 0, 0, 0);
      }
    }
    // dh1[p][c1] = sum_c2 dz[p][c2] W2[c2][c1]: tile wv = (pixel half, 32 channels); W2 from L2
    f16v ah = {0};
    const int pi = wv / ntj, tj1 = wv - pi * ntj;
    const bool hast = wv < 2 * ntj;
    const int cc1 = tj1 * 32 + l31;
    if (hast) {
      const float* ap = dzs + (pi * 32 + l31) * ld2 + 4 * h;
      const bool cv = cc1 < C1;
      const float keep = cv ? 1.f : 0.f;
      const float* bp = w2 + (cv ? cc1 : 0) + (int64_t)4 * h * C1;
      for (int j0 = 0; j0 < (C2 >> 3); j0 += 2) {      // C2 % 32 == 0: two k groups per trip, 8 loads of W2 in flight
        f4 av[2];
        float bv[2][4];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          av[jj] = *reinterpret_cast<const f4*>(ap + 8 * (j0 + jj));
#pragma unroll
          for (int e = 0; e < 4; ++e) bv[jj][e] = bp[(int64_t)(8 * (j0 + jj) + e) * C1] * keep;      // padded columns (cc1 >= C1) read column 0 and drop it
        }
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
#pragma unroll
          for (int e = 0; e < 4; ++e) ah = __builtin_amdgcn_mfma_f32_32x32x2f32(av[jj][e], bv[jj][e], ah, 0, 0, 0);
        }
      }
    }
    __syncthreads();      // every wave is done reading h1
    if (hast) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float* hp = hs + (pi * 32 + pix_of(r, h)) * ld1 + cc1;
        *hp = ah[r] * (*hp > 0.f ? 1.f : p.slope1);      // lrelu keeps the sign of p1; padded columns and pixels hold 0 -> 0 * slope
      }
    }
    __syncthreads();
    if (PARAMS) {
      if (tid < C2) {
        float s2 = 0.f;
#pragma unroll 8
        for (int px = 0; px < BT; ++px) s2 += dzs[px * ld2 + tid];
        adb2 += s2;
      } else if (tid - 256 >= 0 && tid - 256 < C1) {
        float s1 = 0.f;
#pragma unroll 8
        for (int px = 0; px < BT; ++px) s1 += hs[px * ld1 + tid - 256];
        adb1 += s1;
      }
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int o = tid + 512 * m;
        if (o < C1 * 8) {
          const int c = o >> 3, k = o & 7;
          float s1 = 0.f;
#pragma unroll 8
          for (int px = 0; px < BT; ++px) s1 = fmaf(hs[px * ld1 + c], xs[px * 8 + k], s1);
          adw1[m] += s1;
        }
      }
    }
    if (DX) {
      const int k = tid & 7;
      if (pv && k < p.xcs) {
        float v = 0.f;
        if (k < p.C0)
#pragma unroll 8
          for (int c = 0; c < C1; ++c) v = fmaf(hs[pix * ld1 + c], w1s[c * 8 + k], v);
        dx[(base + pix) * p.xcs + k] = v;
      }
    }
    __syncthreads();
  }
  if (PARAMS) {
    float* dst = part + (int64_t)blockIdx.x * pd_partial_floats(C1, C2);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int tt = wv + 8 * m;
      if (tt < nti * ntj) {
        const int ti = tt / ntj, tj = tt - ti * ntj;
        const int c1 = tj * 32 + l31;
        if (c1 < C1) {
#pragma unroll
          for (int r = 0; r < 16; ++r) dst[(ti * 32 + pix_of(r, h)) * C1 + c1] = aw2[m][r];
        }
      }
    }
    dst += C2 * C1;
    if (tid < C2) dst[tid] = adb2;
    else if (tid - 256 >= 0 && tid - 256 < C1) dst[C2 + tid - 256] = adb1;
    dst += C2 + C1;
#pragma unroll
    for (int m = 0; m < 2; ++m)
      if (tid + 512 * m < C1 * 8) dst[tid + 512 * m] = adw1[m];
  }
}

__global__ __launch_bounds__(256) void pd_bwd2_reduce(cat_pixeld_t p, int nwg, const float* __restrict__ part, float* __restrict__ dw1, float* __restrict__ db1,
                                                      float* __restrict__ dw2, float* __restrict__ db2, int accumulate) {
  const int C1 = p.C1, C2 = p.C2, pf = pd_partial_floats(C1, C2);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= pf) return;
  float* dst;
  if (i < C2 * C1) {
    dst = dw2 + i;
  } else if (i < C2 * C1 + C2) {
    dst = db2 ? db2 + (i - C2 * C1) : nullptr;
  } else if (i < C2 * C1 + C2 + C1) {
    dst = db1 + (i - C2 * C1 - C2);
  } else {
    const int o = i - C2 * C1 - C2 - C1, c = o >> 3, k = o & 7;
    dst = k < p.w1cs ? dw1 + c * p.w1cs + k : nullptr;
  }
  if (!dst) return;
  float s = 0.f;
  for (int w = 0; w < nwg; ++w) s += part[(int64_t)w * pf + i];
  *dst = accumulate ? *dst + s : s;
}

int num_cus() {      // per device ordinal; racing first calls store the same value
  static std::atomic<int> cus[64];
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64) dev = 0;
  int v = cus[dev].load(std::memory_order_relaxed);
  if (!v) {
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    cus[dev].store(v, std::memory_order_relaxed);
  }
  return v;
}

bool geom_ok(const cat_pixeld_t* g) {
  return g && g->N > 0 && g->HW > 0 && g->C0 >= 1 && g->C0 <= 8 && g->C0 <= g->xcs && (g->xcs == 4 || g->xcs == 8) && g->C1 >= 16 && g->C1 <= 128 &&
         g->C1 % 16 == 0 && g->C2 == 2 * g->C1 && g->w1cs >= g->C0 && g->w1cs <= 8 && (g->groups == 1 || g->groups == g->N) && g->docs >= 4 &&
         g->docs % 4 == 0 && (int64_t)g->N * g->HW < (1ll << 31) / 4;
}

cat::LdsOptIn optin_fwd1, optin_b2[3];

}  // namespace

extern "C" {

int cat_pixeld_plan(const cat_pixeld_t* g, cat_pixeld_plan_t* plan) {
  CAT_REQUIRE(geom_ok(g) && plan, "pixeld plan: unsupported geometry");
  const int C1 = g->C1, C2 = g->C2, C1p = cat::round_up(C1, 32), cus = num_cus();
  plan->tile_px = FT * FSUB;
  plan->tiles = cdiv(g->HW, FT * FSUB);
  plan->fwd_lds = (int)sizeof(float) * (C2 * (C1 + 4) + FT * (C1 + 4) + C1 * 8 + C1);
  // a persistent workgroup pays for itself over several tiles (pd_fwd1 loads all of W2 into LDS, pd_bwd2 leaves a partial of every parameter
  // gradient behind): at least kMinWalk tiles each, at most what the CUs hold
  plan->fwd_grid = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv((int64_t)g->N * plan->tiles, kMinWalk), (int64_t)cus * (plan->fwd_lds <= 72 * 1024 ? 2 : 1)));
  plan->b1_blocks = std::max(1, std::min(cdiv(g->HW, 16), cdiv(4 * cus, g->N)));
  plan->b2_tiles = g->N * cdiv(g->HW, BT);
  plan->b2_lds = (int)sizeof(float) * (BT * (C2 + 4) + BT * (C1p + 4) + NCOEF * C2 + C1 * 8 + C1 + BT * 8);
  plan->b2_grid = std::max(1, std::min(cdiv(plan->b2_tiles, kMinWalk), cus));
  plan->table_floats = (int64_t)g->N * plan->tiles * 2 * C2;
  plan->ws1_floats = (int64_t)g->N * plan->b1_blocks * (3 * C2 + 1);
  plan->ws2_floats = (int64_t)plan->b2_grid * pd_partial_floats(C1, C2);
  return 0;
}

int cat_pixeld_fwd1(const cat_pixeld_t* g, const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* z,
                    float* table, cat_stream_t stream) {
  cat_pixeld_plan_t pl;
  if (int rc = cat_pixeld_plan(g, &pl)) return rc;
  CAT_REQUIRE(x && w1 && b1 && w2 && z && table, "pixeld fwd1: null pointer");
  cat::ProfScope prof("pixeld_fwd1", 2.0 * g->N * g->HW * g->C1 * (g->C2 + g->C0), 4.0 * g->N * g->HW * (g->C2 + g->xcs), stream);
  cat::lds_optin(optin_fwd1, reinterpret_cast<const void*>(pd_fwd1), 160 * 1024);
  pd_fwd1<<<pl.fwd_grid, 256, pl.fwd_lds, (hipStream_t)stream>>>(*g, pl.tiles, x, w1, b1, w2, b2, z, table);
  return cat::check_launch("pixeld_fwd1");
}

int cat_pixeld_fwd3(const cat_pixeld_t* g, const float* z, const float* scale, const float* shift, const float* w3, const float* b3,
                    float* out, cat_stream_t stream) {
  CAT_REQUIRE(geom_ok(g) && z && scale && shift && w3 && out, "pixeld fwd3: bad arguments");
  const int64_t M = (int64_t)g->N * g->HW;
  cat::ProfScope prof("pixeld_fwd3", 4.0 * M * g->C2, 4.0 * M * (g->C2 + 4), stream);
  const int grid = (int)std::min<int64_t>(cdiv(M, 16), (int64_t)num_cus() * 16);
  pd_fwd3<<<grid, 256, 0, (hipStream_t)stream>>>(*g, z, scale, shift, w3, b3, out);
  return cat::check_launch("pixeld_fwd3");
}

int cat_pixeld_bwd1(const cat_pixeld_t* g, const float* z, const float* dout, const float* scale, const float* shift, const float* mean,
                    const float* rstd, const float* w3, float* coef, float* dw3, float* db3, float* dgamma, float* dbeta, int accumulate,
                    float* ws, cat_stream_t stream) {
  cat_pixeld_plan_t pl;
  if (int rc = cat_pixeld_plan(g, &pl)) return rc;
  CAT_REQUIRE(z && dout && scale && shift && mean && rstd && w3 && coef && ws, "pixeld bwd1: null pointer");
  const int64_t M = (int64_t)g->N * g->HW;
  cat::ProfScope prof("pixeld_bwd1", 10.0 * M * g->C2, 4.0 * M * (g->C2 + 4), stream);
  float* dpart = ws + (int64_t)g->N * pl.b1_blocks * 3 * g->C2;
  pd_bwd1<<<dim3(pl.b1_blocks, g->N), 256, 0, (hipStream_t)stream>>>(*g, z, dout, scale, shift, mean, rstd, w3, ws, dpart);
  pd_bwd1_reduce<<<g->C2 + 1, 64, 0, (hipStream_t)stream>>>(*g, pl.b1_blocks, ws, dpart, scale, shift, mean, rstd, w3, coef, dw3, db3, dgamma, dbeta,
                                                     accumulate);
  return cat::check_launch("pixeld_bwd1");
}

int cat_pixeld_bwd2(const cat_pixeld_t* g, const float* x, const float* z, const float* dout, const float* coef, const float* w1,
                    const float* b1, const float* w2, float* dx, int params, float* dw1, float* db1, float* dw2, float* db2, int accumulate,
                    float* ws, cat_stream_t stream) {
  cat_pixeld_plan_t pl;
  if (int rc = cat_pixeld_plan(g, &pl)) return rc;
  CAT_REQUIRE(x && z && dout && coef && w1 && b1 && w2, "pixeld bwd2: null pointer");
  CAT_REQUIRE(dx || params, "pixeld bwd2: nothing to compute");
  CAT_REQUIRE(!params || (dw1 && db1 && dw2 && ws), "pixeld bwd2: parameter gradients need dw1, db1, dw2 and a workspace");
  const int64_t M = (int64_t)g->N * g->HW;
  cat::ProfScope prof("pixeld_bwd2", 2.0 * M * g->C1 * g->C2 * (params ? 2 : 1), 4.0 * M * (g->C2 + 2 * g->xcs + 4), stream);
  const int tpi = cdiv(g->HW, BT);
  const hipStream_t st = (hipStream_t)stream;
#define PD_B2(P, D, SLOT)                                                                                   \
  do {                                                                                                      \
    cat::lds_optin(optin_b2[SLOT], reinterpret_cast<const void*>(pd_bwd2<P, D>), 160 * 1024);               \
    pd_bwd2<P, D><<<pl.b2_grid, 512, pl.b2_lds, st>>>(*g, tpi, x, z, dout, coef, w1, b1, w2, dx, ws);       \
  } while (0)
  if (params && dx) PD_B2(true, true, 0);
  else if (params) PD_B2(true, false, 1);
  else PD_B2(false, true, 2);
#undef PD_B2
  if (params) {
    if (int rc = cat::check_launch("pixeld_bwd2")) return rc;
    pd_bwd2_reduce<<<cdiv(pd_partial_floats(g->C1, g->C2), 256), 256, 0, st>>>(*g, pl.b2_grid, ws, dw1, db1, dw2, db2, accumulate);
  }
  return cat::check_launch("pixeld_bwd2");
}

}  // extern "C"
