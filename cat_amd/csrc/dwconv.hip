// Depthwise convolution (groups == C, stride 1, k in {1,3,5,...}), NHWC, gfx950.  HBM/L2-bound direct kernels: one lane owns
// a float4 of channels of one pixel, the k*k taps are re-read from L1/L2 (neighbouring lanes share them), the
// filter lives in LDS as [tap][channel] so a tap is one ds_read_b128 per lane.
// Reference: the groups=midp ConvBNReLU conv of InvertedResidualChannels (models/modules/inception_modules.py:166-173).
#include "common.h"
#include <stdlib.h>

namespace {
using cat::cdiv;

constexpr int MAXW = 16384;  // taps * cs floats of LDS filter (dynamic LDS, <= 64 KB): k=5 up to 652 channels, k=7 up to 332

struct DwArgs {
  const float* x; const float* w; const float* bias; float* y;
  int N, H, W, C, xcs, Ho, Wo, ycs, kh, kw, pad, reflect;
  int cq;        // fwd: channel quads processed per pixel (the tensor, or a channel SLICE of a wider buffer: x / y point at its first channel)
  int act;       // fwd: fused epilogue activation
  float slope;
};

__device__ __forceinline__ void load_filter(float* sw, const float* w, int C, int cs, int taps) {
  for (int i = threadIdx.x; i < taps * cs; i += 256) {
    const int t = i / cs, c = i - t * cs;
    sw[i] = c < C ? w[c * taps + t] : 0.f;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void dw_fwd_kernel(DwArgs p) {
  extern __shared__ __attribute__((aligned(16))) float sw[];
  const int taps = p.kh * p.kw, nq = p.cq, fcs = p.cq * 4;
  load_filter(sw, p.w, p.C, fcs, taps);
  const int64_t total = (int64_t)p.N * p.Ho * p.Wo * nq;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int cq = (int)(i % nq);
    int64_t r = i / nq;
    const int ox = (int)(r % p.Wo);
    r /= p.Wo;
    const int oy = (int)(r % p.Ho);
    const int n = (int)(r / p.Ho);
    const int c = cq * 4;
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) {
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = c + e < p.C ? p.bias[c + e] : 0.f;
    }
    const float* xn = p.x + (int64_t)n * p.H * p.W * p.xcs + c;
    for (int ky = 0; ky < p.kh; ++ky) {
      int iy = oy - p.pad + ky;
      if (p.reflect) iy = cat::reflect_idx(iy, p.H);
      else if ((unsigned)iy >= (unsigned)p.H) continue;
      for (int kx = 0; kx < p.kw; ++kx) {
        int ix = ox - p.pad + kx;
        if (p.reflect) ix = cat::reflect_idx(ix, p.W);
        else if ((unsigned)ix >= (unsigned)p.W) continue;
        const f4 xv = *reinterpret_cast<const f4*>(xn + ((int64_t)iy * p.W + ix) * p.xcs);
        const f4 wv = *reinterpret_cast<const f4*>(sw + (ky * p.kw + kx) * fcs + c);
        acc += xv * wv;
      }
    }
    if (p.act != CAT_ACT_NONE) {
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = c + e < p.C ? cat::apply_act(acc[e], p.act, p.slope) : 0.f;
    }
    *reinterpret_cast<f4*>(p.y + (i / nq) * p.ycs + c) = acc;
  }
}

// Several depthwise convs of DIFFERENT kernel sizes over adjacent channel slices of one buffer as ONE launch (round 6: the frozen teacher's
// block, cat_amd/frozen.py -- its 1 x 1 / 3 x 3 / 5 x 5 depthwise convs with eval-mode BatchNorm folded in, plus the plain copy of the k = 1
// residual branch's hidden slice, were four launches of 10 - 32 us over the same 176-channel buffers).  Per channel quad a kernel size
// k in {1, 3, 5}; the filters sit in a 5 x 5 frame [25][cs] (k < 5: centred, the rest zero -- only the k x k window is read), a quad that is
// merely copied carries k = 1, centre weight 1, bias 0.  Lane = (pixel, quad): a pixel's quads are consecutive lanes (one coalesced row).
// The kernels are templates on the frame side F: F = 5 is what is described here (cat_dwconv2d_multi_fwd), F = 7 serves cat_dwconv2d_multi7_fwd --
// k in {1, 3, 5, 7}, a 7 x 7 frame [49][cs], the teacher of a distillation with the reference's default kernel sizes 3 5 7.
// cat_dwconv2d_multi_fwd launches this 1-D walk for planes of fewer than DW_MULTI_TILE_MIN_WG tile workgroups (and under CAT_DWMULTI_TILE=0);
// larger planes go to dw_multi_tile_kernel below.
struct DwMultiArgs {
  const float* x; const float* w25; const float* bias; float* y;
  int N, H, W, nq, xcs, ycs, reflect, act;
  float slope;
  // runs of consecutive quads with the same kernel size: threads are dealt out run by run ([run][pixel][quad of the run]), so a wave has ONE
  // kernel size (no divergence, fully unrolled tap loops: all k * k loads of a thread in flight at once)
  int nrun;
  int run_q0[CAT_DWMULTI_MAXRUN], run_nq[CAT_DWMULTI_MAXRUN], run_k[CAT_DWMULTI_MAXRUN];
  long long run_base[CAT_DWMULTI_MAXRUN + 1];      // first thread index of the run; [nrun] = total
};

__device__ __attribute__((aligned(16))) float g_zero[4] = {0.f, 0.f, 0.f, 0.f};      // global (not constant) address space: the loads stay global_load

// F: side of the filter frame (5: cat_dwconv2d_multi_fwd; 7: cat_dwconv2d_multi7_fwd), K <= F
template <int K, int F>
__device__ __forceinline__ f4 dw_multi_taps(const DwMultiArgs& p, const float* sw, const float* xn, int oy, int ox, int c, int cs, f4 acc) {
  constexpr int R = K / 2, O = F / 2 - R;
  int64_t offy[K];
  int offx[K];
  bool vy[K], vx[K];
#pragma unroll
  for (int t = 0; t < K; ++t) {
    int iy = oy - R + t, ix = ox - R + t;
    vy[t] = p.reflect || (unsigned)iy < (unsigned)p.H;
    vx[t] = p.reflect || (unsigned)ix < (unsigned)p.W;
    iy = p.reflect ? cat::reflect_idx(iy, p.H) : (vy[t] ? iy : 0);
    ix = p.reflect ? cat::reflect_idx(ix, p.W) : (vx[t] ? ix : 0);
    offy[t] = (int64_t)iy * p.W * p.xcs;
    offx[t] = ix * p.xcs;
  }
  f4 xv[K][K];
#pragma unroll
  for (int ky = 0; ky < K; ++ky)
#pragma unroll
    for (int kx = 0; kx < K; ++kx)      // out-of-plane taps load the zero line: never x * 0 (a non-finite pixel (0, 0) would turn every border output into NaN)
      xv[ky][kx] = *reinterpret_cast<const f4*>((vy[ky] && vx[kx]) ? xn + offy[ky] + offx[kx] : g_zero);
#pragma unroll
  for (int ky = 0; ky < K; ++ky)
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
      const f4 wv = *reinterpret_cast<const f4*>(sw + ((O + ky) * F + O + kx) * cs + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(xv[ky][kx][e], wv[e], acc[e]);
    }
  return acc;
}

template <int F>
__global__ __launch_bounds__(256) void dw_multi_fwd_kernel(DwMultiArgs p) {
  extern __shared__ __attribute__((aligned(16))) float sw[];      // [F * F][cs] frame, then [cs] bias
  constexpr int FT = F * F;
  const int cs = p.nq * 4;
  for (int i = threadIdx.x; i < FT * p.nq; i += 256) *reinterpret_cast<f4*>(sw + i * 4) = *reinterpret_cast<const f4*>(p.w25 + i * 4);
  for (int i = threadIdx.x; i < p.nq; i += 256)
    *reinterpret_cast<f4*>(sw + FT * cs + i * 4) = p.bias ? *reinterpret_cast<const f4*>(p.bias + i * 4) : f4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  const int64_t total = p.run_base[p.nrun];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int r = 0;
    while (r + 1 < p.nrun && i >= p.run_base[r + 1]) ++r;
    const int64_t j = i - p.run_base[r];
    const int rq = p.run_nq[r], k = p.run_k[r];
    const int cq = p.run_q0[r] + (int)(j % rq);
    int64_t pix = j / rq;
    const int64_t opix = pix;
    const int ox = (int)(pix % p.W);
    pix /= p.W;
    const int oy = (int)(pix % p.H);
    const int n = (int)(pix / p.H);
    const int c = cq * 4;
    f4 acc = *reinterpret_cast<const f4*>(sw + FT * cs + c);
    const float* xn = p.x + (int64_t)n * p.H * p.W * p.xcs + c;
    if (k == 1) acc = dw_multi_taps<1, F>(p, sw, xn, oy, ox, c, cs, acc);
    else if (k == 3) acc = dw_multi_taps<3, F>(p, sw, xn, oy, ox, c, cs, acc);
    else if (F == 5 || k == 5) acc = dw_multi_taps<5, F>(p, sw, xn, oy, ox, c, cs, acc);
    else acc = dw_multi_taps<F, F>(p, sw, xn, oy, ox, c, cs, acc);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = cat::apply_act(acc[e], p.act, p.slope);
    *reinterpret_cast<f4*>(p.y + opix * p.ycs + c) = acc;
  }
}

// The same conv for planes large enough to fill the chip (cat_dwconv2d_multi_fwd routes them here): the 1-D walk above re-reads the 25 taps
// of a 5 x 5 quad from L2 in workgroups five image rows apart (2.3 x the compulsory fetch on the 176-channel 64 x 64 teacher block).  Here one
// workgroup = 8 x 16 output pixels x one group of at most kDwGroup consecutive quads of one kernel size (common.h: dw_quad_groups), the
// (8 + k - 1) x (16 + k - 1) patch staged in LDS once: a pixel is fetched once per tile, plus halo.  No affine on staging, bias + activation in
// the epilogue, no statistics.  Thread = (pixel, quad parity within the group), as in the fused block's dwm_fwd_kernel.  Per output the
// arithmetic is dw_multi_taps': bias, then fmaf over the taps in (ky, kx) order.
constexpr int DWT_TH = 8, DWT_TW = 16;
// f4 per quad plane of a frame of side F (halo F - 1): + 2 spreads the staging stores of a pixel's 4 quads over the banks
template <int F> constexpr int DWT_PS = (DWT_TH + F - 1) * (DWT_TW + F - 1) + 2;
constexpr int DWT_GCS = cat::kDwGroup * 4;
template <int F> constexpr size_t DWT_LDS = (size_t)(cat::kDwGroup * DWT_PS<F> * 4 + (F * F + 1) * DWT_GCS) * sizeof(float);      // 17 KB at 4 quads, F = 5; 23 KB, F = 7

struct DwTileArgs {
  const float* x; const float* w25; const float* bias; float* y;
  int N, H, W, nq, xcs, ycs, reflect, act;
  float slope;
  int tiles_x, tiles, ng;
  unsigned char gq0[CAT_DWMULTI_MAXQ], gnq[CAT_DWMULTI_MAXQ], gks[CAT_DWMULTI_MAXQ];
};

template <int K, int F>
__device__ __forceinline__ void dw_multi_tile_body(const DwTileArgs& p, f4* tile, float* sw, int n, int oy0, int ox0, int q0, int gn) {
  constexpr int R = K / 2, O = F / 2 - R, PS = DWT_PS<F>, PR = DWT_TH + 2 * R, PC = DWT_TW + 2 * R, G = cat::kDwGroup;
  const int tid = threadIdx.x;
  constexpr int SIT = (PR * PC * G + 255) / 256;      // all of the thread's loads in flight before the first LDS store
  f4 xv[SIT];
#pragma unroll
  for (int it = 0; it < SIT; ++it) {
    const int i = tid + it * 256;
    xv[it] = f4{0.f, 0.f, 0.f, 0.f};      // out-of-plane taps of zero padding stay literal zeros: never x * 0 (dw_multi_taps)
    if (i < PR * PC * gn) {
      const int pix = i / gn, q = q0 + i - pix * gn;
      const int r = pix / PC, c = pix - r * PC;
      int iy = oy0 - R + r, ix = ox0 - R + c;
      bool v;
      if (p.reflect) {
        v = iy > -p.H && iy < 2 * p.H - 1 && ix > -p.W && ix < 2 * p.W - 1;      // beyond a ragged tile's mirror range: never read
        iy = cat::reflect_idx(iy, p.H);
        ix = cat::reflect_idx(ix, p.W);
      } else {
        v = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
      }
      if (v) xv[it] = *reinterpret_cast<const f4*>(p.x + (((int64_t)n * p.H + iy) * p.W + ix) * p.xcs + q * 4);
    }
  }
#pragma unroll
  for (int it = 0; it < SIT; ++it) {
    const int i = tid + it * 256;
    if (i < PR * PC * gn) tile[(i % gn) * PS + i / gn] = xv[it];
  }
  __syncthreads();
  const int px = tid & 127, half = tid >> 7, py = px / DWT_TW, pxx = px % DWT_TW;
  if (oy0 + py >= p.H || ox0 + pxx >= p.W) return;
#pragma unroll      // (a runtime loop over the quads keeps all 25 taps and weights of the next quad in flight: 200 registers)
  for (int k = 0; k < G / 2; ++k) {
    const int ql = half + 2 * k;
    if (ql >= gn) break;
    const f4* pl = tile + ql * PS;
    const float* wq = sw + ql * 4;
    f4 acc = *reinterpret_cast<const f4*>(sw + F * F * DWT_GCS + ql * 4);
#pragma unroll
    for (int ky = 0; ky < K; ++ky)
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const f4 xq = pl[(py + ky) * PC + pxx + kx];
        const f4 wv = *reinterpret_cast<const f4*>(wq + ((O + ky) * F + O + kx) * DWT_GCS);
        acc = __builtin_elementwise_fma(xq, wv, acc);
      }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = cat::apply_act(acc[e], p.act, p.slope);
    *reinterpret_cast<f4*>(p.y + (((int64_t)n * p.H + oy0 + py) * p.W + ox0 + pxx) * p.ycs + (q0 + ql) * 4) = acc;
  }
}

template <int F>
__global__ __launch_bounds__(256) void dw_multi_tile_kernel(DwTileArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int FT = F * F;
  f4* tile = reinterpret_cast<f4*>(smem);             // [G][DWT_PS<F>] one plane per quad of the group
  float* sw = smem + cat::kDwGroup * DWT_PS<F> * 4;      // [F * F][DWT_GCS] frame, then [DWT_GCS] bias
  int tt, grp;
  cat::dw_tile_group(blockIdx.x, p.N * p.tiles, p.ng, tt, grp);
  const int q0 = p.gq0[grp], gn = p.gnq[grp], k = p.gks[grp];
  const int n = tt / p.tiles, t = tt - n * p.tiles;
  const int oy0 = (t / p.tiles_x) * DWT_TH, ox0 = (t % p.tiles_x) * DWT_TW;
  const int cs = p.nq * 4;
  for (int i = threadIdx.x; i < (FT + 1) * gn; i += 256) {
    const int tap = i / gn, c = (q0 + i - tap * gn) * 4;
    const f4 v = tap < FT ? *reinterpret_cast<const f4*>(p.w25 + tap * cs + c)
                          : (p.bias ? *reinterpret_cast<const f4*>(p.bias + c) : f4{0.f, 0.f, 0.f, 0.f});
    *reinterpret_cast<f4*>(sw + tap * DWT_GCS + (i - tap * gn) * 4) = v;
  }
  if (k == 1) dw_multi_tile_body<1, F>(p, tile, sw, n, oy0, ox0, q0, gn);
  else if (k == 3) dw_multi_tile_body<3, F>(p, tile, sw, n, oy0, ox0, q0, gn);
  else if (F == 5 || k == 5) dw_multi_tile_body<5, F>(p, tile, sw, n, oy0, ox0, q0, gn);
  else dw_multi_tile_body<F, F>(p, tile, sw, n, oy0, ox0, q0, gn);
}

// Fewest workgroups (tiles x quad groups) for which cat_dwconv2d_multi_fwd takes the tile kernel: four per CU of the 256.  Below, the tile
// kernel's fixed cost per workgroup (staging, a barrier) buys nothing -- the plane sits in L2 -- and the 1-D walk's finer lanes fill more CUs.
constexpr int64_t DW_MULTI_TILE_MIN_WG = 1024;

// dxp[n,py,px,c] = sum_k dy[n, py+pe-ky, px+pe-kx, c] * w[c,ky,kx]; (Hin,Win,pe) = (H+2p,W+2p,0) for reflect, (H,W,p) for zero pad.
__global__ __launch_bounds__(256) void dw_dgrad_kernel(DwArgs p, int Hin, int Win, int pe, int dxcs) {
  extern __shared__ __attribute__((aligned(16))) float sw[];
  const int taps = p.kh * p.kw, nq = dxcs / 4;
  load_filter(sw, p.w, p.C, dxcs, taps);
  const int64_t total = (int64_t)p.N * Hin * Win * nq;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int cq = (int)(i % nq);
    int64_t r = i / nq;
    const int px = (int)(r % Win);
    r /= Win;
    const int py = (int)(r % Hin);
    const int n = (int)(r / Hin);
    const int c = cq * 4;
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    const float* dn = p.x + (int64_t)n * p.Ho * p.Wo * p.xcs + c;  // p.x = dy here
    for (int ky = 0; ky < p.kh; ++ky) {
      const int oy = py + pe - ky;
      if ((unsigned)oy >= (unsigned)p.Ho) continue;
      for (int kx = 0; kx < p.kw; ++kx) {
        const int ox = px + pe - kx;
        if ((unsigned)ox >= (unsigned)p.Wo) continue;
        const f4 gv = *reinterpret_cast<const f4*>(dn + ((int64_t)oy * p.Wo + ox) * p.xcs);
        const f4 wv = *reinterpret_cast<const f4*>(sw + (ky * p.kw + kx) * dxcs + c);
        acc += gv * wv;
      }
    }
    *reinterpret_cast<f4*>(p.y + i * 4) = acc;
  }
}

// dw[c][tap] partials: lanes = (pixel-lane, channel quad); each lane keeps one float4 accumulator per tap of ONE filter row
// (blockIdx.y = ky) to bound registers at kw*4; block-reduced through LDS; partial [nb][taps][cs] in ws.
template <int KW>
__global__ __launch_bounds__(256) void dw_wgrad_kernel(DwArgs p, float* __restrict__ part, int nb, int ppl) {
  __shared__ f4 red[256];
  const int nq = p.xcs / 4;
  const int tid = threadIdx.x, cq = tid % nq, pl = tid / nq;
  const int ky = blockIdx.y, b = blockIdx.x;
  const int64_t P = (int64_t)p.N * p.Ho * p.Wo;
  const int64_t per = (P + nb - 1) / nb;
  const int64_t pbeg = b * per, pend = pbeg + per < P ? pbeg + per : P;
  f4 acc[KW];
#pragma unroll
  for (int k = 0; k < KW; ++k) acc[k] = f4{0.f, 0.f, 0.f, 0.f};
  if (pl < ppl) {
    for (int64_t q = pbeg + pl; q < pend; q += ppl) {
      const int ox = (int)(q % p.Wo);
      const int64_t r = q / p.Wo;
      const int oy = (int)(r % p.Ho);
      const int n = (int)(r / p.Ho);
      int iy = oy - p.pad + ky;
      if (p.reflect) iy = cat::reflect_idx(iy, p.H);
      else if ((unsigned)iy >= (unsigned)p.H) continue;
      const f4 gv = *reinterpret_cast<const f4*>(p.y + q * p.ycs + cq * 4);  // p.y = dy here (read only)
      const float* xr = p.x + ((int64_t)n * p.H + iy) * p.W * p.xcs + cq * 4;
#pragma unroll
      for (int kx = 0; kx < KW; ++kx) {
        int ix = ox - p.pad + kx;
        if (p.reflect) ix = cat::reflect_idx(ix, p.W);
        else if ((unsigned)ix >= (unsigned)p.W) continue;
        acc[kx] += gv * *reinterpret_cast<const f4*>(xr + (int64_t)ix * p.xcs);
      }
    }
  }
#pragma unroll
  for (int kx = 0; kx < KW; ++kx) {
    __syncthreads();
    red[tid] = acc[kx];
    __syncthreads();
    if (pl == 0) {
      f4 s = acc[kx];
      for (int j = 1; j < ppl; ++j) s += red[j * nq + cq];
      *reinterpret_cast<f4*>(part + ((int64_t)b * p.kh * KW + ky * KW + kx) * p.xcs + cq * 4) = s;
    }
  }
}

__global__ void dw_wgrad_final_kernel(const float* __restrict__ part, float* __restrict__ dw, int C, int cs, int taps, int nb,
                                      int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C * taps) return;
  const int c = i / taps, t = i - c * taps;
  float s = 0.f;
  for (int b = 0; b < nb; ++b) s += part[((int64_t)b * taps + t) * cs + c];
  dw[i] = accumulate ? dw[i] + s : s;
}

constexpr int kEwCap = 8192;   // most workgroups of an element walk (cat::ew_grid)

int dw_check(const cat_conv_t* g) {
  CAT_REQUIRE(g->Cin == g->Cout && g->stride == 1, "dwconv: needs Cin == Cout, stride 1");
  CAT_REQUIRE(g->xcs % 4 == 0 && g->ycs % 4 == 0 && g->xcs >= g->Cin && g->ycs >= g->Cout, "dwconv: bad pixel stride");
  CAT_REQUIRE(g->kh * g->kw * (g->xcs > g->ycs ? g->xcs : g->ycs) <= MAXW, "dwconv: filter does not fit the LDS stage (k*k*cs <= %d)", MAXW);
  CAT_REQUIRE(g->Ho == g->H + 2 * g->pad - g->kh + 1 && g->Wo == g->W + 2 * g->pad - g->kw + 1, "dwconv: inconsistent output size");
  CAT_REQUIRE(g->pad_mode == CAT_PAD_ZERO || (g->pad < g->H && g->pad < g->W), "dwconv: reflect pad must be < input size");
  return 0;
}

DwArgs dw_args(const cat_conv_t* g) {
  DwArgs a{};
  a.N = g->N; a.H = g->H; a.W = g->W; a.C = g->Cin; a.xcs = g->xcs; a.Ho = g->Ho; a.Wo = g->Wo; a.ycs = g->ycs;
  a.kh = g->kh; a.kw = g->kw; a.pad = g->pad; a.reflect = g->pad_mode == CAT_PAD_REFLECT;
  return a;
}

struct DwWgPlan { int nb, ppl; };
DwWgPlan dw_wg_plan(const cat_conv_t* g) {
  DwWgPlan p;
  p.ppl = 256 / (g->xcs / 4);
  const int64_t P = (int64_t)g->N * g->Ho * g->Wo;
  int nb = cdiv(1024, g->kh);
  const int maxb = cdiv(P, (int64_t)p.ppl * 16);
  if (nb > maxb) nb = maxb;
  if (nb < 1) nb = 1;
  p.nb = nb;
  return p;
}

}  // namespace

extern "C" {

int cat_dwconv2d_fwd(const cat_conv_t* g, const float* x, const float* w, const float* bias, float* y, cat_stream_t stream) {
  if (int e = dw_check(g)) return e;
  DwArgs a = dw_args(g);
  a.x = x; a.w = w; a.bias = bias; a.y = y;
  // a channel SLICE of wider buffers: ycw (0 = whole tensor) gives the channels-with-padding this call owns; x / y point at its first one
  const int own = g->ycw > 0 ? g->ycw : g->ycs;
  CAT_REQUIRE(own % 4 == 0 && own >= g->Cin && own <= g->ycs && own <= g->xcs, "dwconv: bad channel slice (ycw=%d)", g->ycw);
  a.cq = own / 4;
  a.act = g->act;
  a.slope = g->slope;
  cat::ProfScope prof("dwconv_fwd", 2.0 * g->N * g->Ho * g->Wo * g->Cin * g->kh * g->kw, 2 * 4.0 * (double)g->N * g->Ho * g->Wo * own, stream);
  dw_fwd_kernel<<<cat::ew_grid((int64_t)g->N * g->Ho * g->Wo * a.cq, kEwCap), 256, (size_t)g->kh * g->kw * own * sizeof(float), (hipStream_t)stream>>>(a);
  return cat::check_launch("dwconv2d_fwd");
}

}  // extern "C"

namespace {

// cat_dwconv2d_multi_fwd (F = 5) and cat_dwconv2d_multi7_fwd (F = 7): one routing rule, one set of limits
template <int F>
int dw_multi_launch(const cat_dwmulti_t* g, const float* x, const float* w25, const float* bias, float* y, cat_stream_t stream) {
  CAT_REQUIRE(g->N > 0 && g->H > 0 && g->W > 0 && g->nq > 0 && g->nq <= CAT_DWMULTI_MAXQ, "dwconv multi: bad geometry (nq=%d)", g->nq);
  CAT_REQUIRE((g->xcs & 3) == 0 && (g->ycs & 3) == 0 && g->xcs >= 4 * g->nq && g->ycs >= 4 * g->nq, "dwconv multi: pixel strides");
  DwMultiArgs a{};
  a.x = x; a.w25 = w25; a.bias = bias; a.y = y;
  a.N = g->N; a.H = g->H; a.W = g->W; a.nq = g->nq; a.xcs = g->xcs; a.ycs = g->ycs; a.reflect = g->reflect; a.act = g->act; a.slope = g->slope;
  double taps = 0.0;
  const int64_t npix = (int64_t)g->N * g->H * g->W;
  a.nrun = 0;
  a.run_base[0] = 0;
  for (int q = 0; q < g->nq; ++q) {
    const int k = g->ks[q];
    CAT_REQUIRE(k == 1 || k == 3 || k == 5 || (F == 7 && k == 7), "dwconv multi: kernel size %d of quad %d", k, q);
    CAT_REQUIRE(!g->reflect || (k / 2 < g->H && k / 2 < g->W), "dwconv multi: reflect padding wider than the plane");
    taps += 4.0 * k * k;
    if (a.nrun == 0 || a.run_k[a.nrun - 1] != k) {
      CAT_REQUIRE(a.nrun < CAT_DWMULTI_MAXRUN, "dwconv multi: more than %d runs of equal kernel size", CAT_DWMULTI_MAXRUN);
      a.run_q0[a.nrun] = q;
      a.run_nq[a.nrun] = 0;
      a.run_k[a.nrun] = k;
      ++a.nrun;
    }
    ++a.run_nq[a.nrun - 1];
  }
  for (int r = 0; r < a.nrun; ++r) a.run_base[r + 1] = a.run_base[r] + npix * a.run_nq[r];
  const double pix = (double)npix;
  cat::ProfScope prof("dwconv_fwd", 2.0 * pix * taps, 2 * 4.0 * pix * 4 * g->nq, stream);
  static const int tile_on = getenv("CAT_DWMULTI_TILE") ? atoi(getenv("CAT_DWMULTI_TILE")) : 1;      // 0: always the 1-D walk (A/B runs)
  DwTileArgs t{};
  t.tiles_x = cdiv(g->W, DWT_TW);
  t.tiles = t.tiles_x * cdiv(g->H, DWT_TH);
  t.ng = cat::dw_quad_groups(g->ks, g->nq, t.gq0, t.gnq);
  if (tile_on && (int64_t)g->N * t.tiles * t.ng >= DW_MULTI_TILE_MIN_WG && (int64_t)g->N * t.tiles * t.ng < (int64_t)2147483647) {
    t.x = x; t.w25 = w25; t.bias = bias; t.y = y;
    t.N = g->N; t.H = g->H; t.W = g->W; t.nq = g->nq; t.xcs = g->xcs; t.ycs = g->ycs; t.reflect = g->reflect; t.act = g->act; t.slope = g->slope;
    for (int k = 0; k < t.ng; ++k) t.gks[k] = (unsigned char)g->ks[t.gq0[k]];
    dw_multi_tile_kernel<F><<<g->N * t.tiles * t.ng, 256, DWT_LDS<F>, (hipStream_t)stream>>>(t);
    return cat::check_launch("dwconv2d_multi_fwd");
  }
  dw_multi_fwd_kernel<F><<<cat::ew_grid(npix * g->nq, kEwCap), 256, (size_t)(F * F + 1) * 4 * g->nq * sizeof(float), (hipStream_t)stream>>>(a);
  return cat::check_launch("dwconv2d_multi_fwd");
}

}  // namespace

extern "C" {

int cat_dwconv2d_multi_fwd(const cat_dwmulti_t* g, const float* x, const float* w25, const float* bias, float* y, cat_stream_t stream) {
  return dw_multi_launch<5>(g, x, w25, bias, y, stream);
}

int cat_dwconv2d_multi7_fwd(const cat_dwmulti_t* g, const float* x, const float* w49, const float* bias, float* y, cat_stream_t stream) {
  return dw_multi_launch<7>(g, x, w49, bias, y, stream);
}

int cat_dwconv2d_dgrad(const cat_conv_t* g, const float* dy, const float* w, float* dx, int dxcs, cat_stream_t stream) {
  if (int e = dw_check(g)) return e;
  CAT_REQUIRE(dxcs % 4 == 0 && dxcs >= g->Cin && g->kh * g->kw * dxcs <= MAXW, "dwconv dgrad: bad dxcs");
  DwArgs a = dw_args(g);
  a.x = dy; a.xcs = g->ycs; a.w = w; a.y = dx;
  cat::ProfScope prof("dwconv_dgrad", 2.0 * g->N * g->Ho * g->Wo * g->Cin * g->kh * g->kw, 2 * 4.0 * (double)g->N * g->Ho * g->Wo * g->ycs, stream);
  const bool refl = g->pad_mode == CAT_PAD_REFLECT;
  const int Hin = refl ? g->H + 2 * g->pad : g->H, Win = refl ? g->W + 2 * g->pad : g->W, pe = refl ? 0 : g->pad;
  dw_dgrad_kernel<<<cat::ew_grid((int64_t)g->N * Hin * Win * (dxcs / 4), kEwCap), 256, (size_t)g->kh * g->kw * dxcs * sizeof(float), (hipStream_t)stream>>>(a, Hin, Win, pe,
                                                                                                                                            dxcs);
  return cat::check_launch("dwconv2d_dgrad");
}

size_t cat_dwconv2d_wgrad_ws_bytes(const cat_conv_t* g) {
  return (size_t)dw_wg_plan(g).nb * g->kh * g->kw * g->xcs * sizeof(float);
}

int cat_dwconv2d_wgrad(const cat_conv_t* g, const float* x, const float* dy, float* dw, int accumulate, void* ws, cat_stream_t stream) {
  if (int e = dw_check(g)) return e;
  CAT_REQUIRE(ws && g->xcs == g->ycs && g->xcs <= 1024, "dwconv wgrad: needs workspace and xcs == ycs <= 1024");
  DwArgs a = dw_args(g);
  a.x = x; a.y = const_cast<float*>(dy);
  const DwWgPlan pl = dw_wg_plan(g);
  hipStream_t s = (hipStream_t)stream;
  cat::ProfScope prof("dwconv_wgrad", 2.0 * g->N * g->Ho * g->Wo * g->Cin * g->kh * g->kw, 2 * 4.0 * (double)g->N * g->Ho * g->Wo * g->ycs, stream);
  dim3 grid(pl.nb, g->kh);
  switch (g->kw) {
    case 1: dw_wgrad_kernel<1><<<grid, 256, 0, s>>>(a, (float*)ws, pl.nb, pl.ppl); break;
    case 3: dw_wgrad_kernel<3><<<grid, 256, 0, s>>>(a, (float*)ws, pl.nb, pl.ppl); break;
    case 5: dw_wgrad_kernel<5><<<grid, 256, 0, s>>>(a, (float*)ws, pl.nb, pl.ppl); break;
    case 7: dw_wgrad_kernel<7><<<grid, 256, 0, s>>>(a, (float*)ws, pl.nb, pl.ppl); break;
    default: CAT_REQUIRE(false, "dwconv wgrad: kw %d unsupported", g->kw);
  }
  dw_wgrad_final_kernel<<<cdiv(g->Cin * g->kh * g->kw, 256), 256, 0, s>>>((const float*)ws, dw, g->Cin, g->xcs, g->kh * g->kw, pl.nb,
                                                                            accumulate);
  return cat::check_launch("dwconv2d_wgrad");
}

}  // extern "C"
