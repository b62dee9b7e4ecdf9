// Implicit-GEMM convolution for gfx950 on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32), NHWC.
//
//   fwd   : y[M = N*Ho*Wo][Cout]      = im2col(x)[M][K] * W^T[K][Cout]          K = kh*kw*cin4
//   dgrad : dx[M = class pixels][Cin] = col(dy)[M][K']  * Wt[K'][Cin]           K' = taps(class)*cout4
//           (stride-2 problems are split into stride*stride parity classes so that no MFMA work is spent on
//            taps that cannot contribute; the same kernel is nn.ConvTranspose2d's forward)
//   wgrad : dw[Cout][K]               = dy^T[Cout][M] * im2col(x)[M][K]          split over M, partials in ws
//
// One workgroup = 256 threads = 4 wave64, one wave per SIMD; wave tile = (MT*16) x (NT*16) accumulators of
// 16x16x4 MFMAs; BK = 16.  Operand tiles are staged global -> VGPR -> LDS with a one-chunk register prefetch
// (loads for chunk t+1 are in flight while chunk t is on the matrix pipe), LDS is double buffered, one barrier per
// chunk.  "K-contiguous" tiles ([row][16 k]) use an XOR swizzle that is conflict-free for both the float4 store
// (row = tid>>2, quad = tid&3) and the ds_read_b128 fragment read (row = lane&15, quad = lane>>4);
// "N-contiguous" tiles ([16 k][cols + 4]) are read with ds_read_b32 at a row stride == 4 (mod 8) floats.
// Ragged channel counts (pruned students: 4..17, 56, 82 ...) never touch HBM layout beyond the 4-float pixel
// stride: the N edge is handled by 16-wide tile variants chosen per layer, the K edge by zero-filled quads.
#include "common.h"
#include <limits.h>
#include <stdlib.h>

namespace {

using cat::cdiv;

struct IgemmArgs {
  const float* a;     // activation operand (x for fwd/wgrad, dy for dgrad)
  const float* b;     // weights (fwd/dgrad) or dy (wgrad)
  const float* bias;  // optional
  float* out;         // y / dx / dw-or-workspace
  int N, H, W, Cin, xcs;
  int Ho, Wo, Cout, ycs;
  int kh, kw, stride, pad, reflect;
  int padw;      // forward only: implicit padding along W (== pad except through cat_conv2d_fwd_rect: 1 x 7 / 7 x 1 / 1 x 3 / 3 x 1 filters)
  int act;
  float slope;
  int cw;        // channels [Cvalid, cw) of the output pixel get zeros
  int c4;        // per-tap K extent of the walk (fwd/dgrad: may be rounded up to 16 so that a chunk never straddles taps)
  int cval;      // channels that may actually be read per pixel (round_up(C, 4)); quads beyond it come from the zero page
  int K;         // fwd/wgrad: kh*kw*cin4
  int M;         // fwd/wgrad: N*Ho*Wo
  int wvec;      // weight rows can be read as float4
  int wcs;       // weight floats per (cout, tap)
  // dgrad
  int Hin, Win, pad_eff, ocs;
  // wgrad
  int nsplit, mchunk, direct, accumulate;
  // split-K (fwd32 / dgrad when the output tile grid cannot fill the chip): blockIdx.y (fwd) / blockIdx.z (dgrad) = K slice of
  // `kchunks` chunks; raw partial sums go to part[slice][pixel][channel], splitk_reduce_kernel adds bias / activation
  int ksplit, kchunks;
  float* part;
  const float* bt;  // dgrad: filters transposed to [Cin][taps][Cout] (cat_conv2d_dgrad_t), or null
  long long* dbg;  // diagnostic build only (cat::kDiag, CAT_DBG): per-phase shader-clock totals of one wave
  // cat_conv2d_fwd_ex only (the EX instantiations of the forward kernels; the others never read these)
  int dil;           // filter dilation: tap (ky, kx) reads input pixel (oy * stride - pad + ky * dil, ...)
  const float* res;  // optional residual, added BEFORE the activation: res[m * rcs + col]
  int rcs;
};

__device__ __forceinline__ int swz(int r, int q) { return (r * 4 + (q ^ ((r >> 1) & 3))) * 4; }

__device__ __forceinline__ f4 ldg4(const float* p) { return *reinterpret_cast<const f4*>(p); }

// Out-of-range / padding elements are read from this zero page instead of being branched around: every lane always
// issues its load, so the compiler can count outstanding loads (s_waitcnt vmcnt(N)) and keep a whole chunk in flight.
// (`v ? load : 0` compiles to exec-masked branches with a vmcnt(0) behind each load: fully serialised latency.)
__device__ __attribute__((aligned(16))) float g_zero_page[4] = {0.f, 0.f, 0.f, 0.f};  // global (not constant) address space: keeps loads global_load
__device__ __forceinline__ f4 ldg4_or_zero(bool valid, const float* p) { return ldg4(valid ? p : g_zero_page); }
__device__ __forceinline__ f4 ldw4_or_zero(bool valid, bool vec, const float* wp, int ci, int cin) {
  if (vec) return ldg4(valid ? wp : g_zero_page);
  f4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = *((valid && ci + e < cin) ? wp + e : g_zero_page);
  return v;
}

// ------------------------------------------------------------------------------------------------ shared tile code
template <int MT, int NT>
__device__ __forceinline__ void zero_acc(f4 (&acc)[MT][NT]) {
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
}

// The 16-deep MFMA block of one wave tile; fragments are f4 (K-contiguous tiles) or float[4] (N-contiguous tiles) per 16 rows.
// BFIRST: the B fragment goes in as the MFMA's FIRST operand, which leaves the accumulators transposed (see store_pixel_t).
template <bool BFIRST, int MT, int NT, typename FA, typename FB>
__device__ __forceinline__ void mfma_block(const FA (&fa)[MT], const FB (&fb)[NT], f4 (&acc)[MT][NT]) {
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j)
        acc[i][j] = BFIRST ? __builtin_amdgcn_mfma_f32_16x16x4f32(fb[j][t], fa[i][t], acc[i][j], 0, 0, 0)
                           : __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][t], fb[j][t], acc[i][j], 0, 0, 0);
}

template <int MT, int NT>
__device__ __forceinline__ void mma_kcontig_a_kcontig_b(const float* A, const float* B, int arow0, int brow0, int lane,
                                                       f4 (&acc)[MT][NT]) {
  const int lr = lane & 15, lq = lane >> 4;
  f4 fa[MT], fb[NT];
#pragma unroll
  for (int i = 0; i < MT; ++i) fa[i] = *reinterpret_cast<const f4*>(A + swz(arow0 + i * 16 + lr, lq));
#pragma unroll
  for (int j = 0; j < NT; ++j) fb[j] = *reinterpret_cast<const f4*>(B + swz(brow0 + j * 16 + lr, lq));
  mfma_block<false>(fa, fb, acc);
}

// [row][32 k] tiles of the BK = 32 kernels: same XOR swizzle idea as swz over the eight quads of a row
__device__ __forceinline__ int swz32(int r, int q) { return (r * 8 + (q ^ ((r >> 1) & 7))) * 4; }

// fragments of 16-deep half h of a [row][32 k] tile (ds_read_b128)
template <int N>
__device__ __forceinline__ void read_kcontig32(const float* T, int row0, int lane, int h, f4 (&f)[N]) {
  const int lr = lane & 15, lq = lane >> 4;
#pragma unroll
  for (int i = 0; i < N; ++i) f[i] = *reinterpret_cast<const f4*>(T + swz32(row0 + i * 16 + lr, lq + 4 * h));
}

// fragments of k-rows row0 .. row0 + 15 of an N-contiguous tile [k][LD] without row padding (ds_read_b32): the 16-column group of row r is
// XOR-ed with (r >> 2) & 3 (== lq for the four rows a lane reads) instead
template <int LD, int N>
__device__ __forceinline__ void read_ncontig(const float* T, int row0, int col0, int lane, float (&f)[N][4]) {
  const int lr = lane & 15, lq = lane >> 4;
#pragma unroll
  for (int j = 0; j < N; ++j)
#pragma unroll
    for (int t = 0; t < 4; ++t) f[j][t] = T[(row0 + lq * 4 + t) * LD + ((col0 + j * 16 + lr) ^ (lq << 4))];
}

// one 32-deep chunk, A and B tiles [row][32 k]
template <bool BFIRST, int MT, int NT>
__device__ __forceinline__ void mma32_kcontig_a_kcontig_b(const float* A, const float* B, int arow0, int brow0, int lane, f4 (&acc)[MT][NT]) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    f4 fa[MT], fb[NT];
    read_kcontig32(A, arow0, lane, h, fa);
    read_kcontig32(B, brow0, lane, h, fb);
    mfma_block<BFIRST>(fa, fb, acc);
  }
}

// one 32-deep chunk, A tile [row][32 k], B tile [32 k][BN] with XOR-ed column groups
template <bool BFIRST, int BN, int MT, int NT>
__device__ __forceinline__ void mma32_kcontig_a_ncontig_b(const float* A, const float* B, int arow0, int bcol0, int lane, f4 (&acc)[MT][NT]) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    f4 fa[MT];
    float fb[NT][4];
    read_kcontig32(A, arow0, lane, h, fa);
    read_ncontig<BN>(B, h * 16, bcol0, lane, fb);
    mfma_block<BFIRST>(fa, fb, acc);
  }
}

// the filter-tap walk moves one tap on, row-major over (ky, kx)
__device__ __forceinline__ void next_tap(int& ky, int& kx, int kw) {
  if (++kx == kw) {
    kx = 0;
    ++ky;
  }
}

// m -> (n, y, x) of a pixel-major [N][H][W] index space (HW = H * W).  Rows beyond the tile's M are decoded as pixel 0 by the callers
// (`rv ? m : 0`): their loads are parked or masked, but the address arithmetic stays in range.
struct Pixel { int n, y, x; };
__device__ __forceinline__ Pixel decode_pixel(int m, int HW, int W) {
  const int n = m / HW, rem = m - n * HW;
  const int y = rem / W;
  return Pixel{n, y, rem - y * W};
}

// One chunk of both operand tiles DMA-ed straight into LDS (buffer_load_dwordx4 ... lds): wave w's instruction i writes the 256 floats
// (64 lanes x 16 bytes, lane-linear) at tile + (w * 4 + i) * 256.  voff = per-lane byte offsets (0x80000000: beyond num_records, the
// buffer unit returns zeros), so = wave-uniform byte offset of the chunk.
typedef __attribute__((address_space(3))) void* lds_t;
__device__ __forceinline__ void dma_chunk(__amdgpu_buffer_rsrc_t rA, __amdgpu_buffer_rsrc_t rB, float* tA, float* tB, int wave,
                                          const unsigned (&voffA)[4], const unsigned (&voffB)[4], unsigned soA, unsigned soB) {
  float* dA = tA + wave * 4 * 256;
  float* dB = tB + wave * 4 * 256;
#pragma unroll
  for (int i = 0; i < 4; ++i) __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (lds_t)(dA + i * 256), 16, voffA[i], soA, 0, 0);
#pragma unroll
  for (int i = 0; i < 4; ++i) __builtin_amdgcn_raw_ptr_buffer_load_lds(rB, (lds_t)(dB + i * 256), 16, voffB[i], soB, 0, 0);
}

// Row-major accumulators (lane (lr, lq) holds rows i * 16 + lq * 4 + 0..3 of column j * 16 + lr) of the forward kernels:
// out[m][col] = act(acc + bias[col]) for col < Cout, zeros for Cout <= col < cw.  m0 / n0 = first row / column of the WAVE tile.
template <int MT, int NT, bool EX = false>
__device__ __forceinline__ void store_rows(const IgemmArgs& p, const f4 (&acc)[MT][NT], int m0, int n0, int lane) {
  const int lr = lane & 15, lq = lane >> 4;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int col = n0 + j * 16 + lr;
    const bool cvalid = col < p.Cout;
    const float bias = (cvalid && p.bias) ? p.bias[col] : 0.f;
    if (!cvalid && col >= p.cw) continue;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int m = m0 + i * 16 + lq * 4 + rg;
        if (m < p.M) {
          float v = acc[i][j][rg] + bias;
          if (EX && cvalid && p.res) v += p.res[(int64_t)m * p.rcs + col];
          p.out[(int64_t)m * p.ycs + col] = cvalid ? cat::apply_act(v, p.act, p.slope) : 0.f;
        }
      }
    }
  }
}

// Transposed accumulators (mfma_block<true>): lane (lr, lq) holds channels j * 16 + lq * 4 + 0..3 of tile row (pixel) i * 16 + lr -- one
// pixel address and one float4 store per tile instead of four of each (round 6: -3.7 % on a 256 -> 256 3x3 forward).
// orow = the pixel of tile row i, c0 = first channel of the wave tile + lq * 4, C = valid channels; zeros for C <= c < cw.
// rrow (EX only) = the same pixel of the residual, or null.
template <int MT, int NT, bool EX = false>
__device__ __forceinline__ void store_pixel_t(const IgemmArgs& p, float* orow, const f4 (&acc)[MT][NT], int i, int c0, int C, bool vec,
                                              const float* rrow = nullptr) {
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int cj = c0 + j * 16;
    if (cj >= p.cw) continue;
    if (vec && cj + 3 < C) {
      f4 v = acc[i][j];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t = v[e] + (p.bias ? p.bias[cj + e] : 0.f);
        if (EX && rrow) t += rrow[cj + e];
        v[e] = cat::apply_act(t, p.act, p.slope);
      }
      *reinterpret_cast<f4*>(orow + cj) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = cj + e;
        if (c < C) {
          float t = acc[i][j][e] + (p.bias ? p.bias[c] : 0.f);
          if (EX && rrow) t += rrow[c];
          orow[c] = cat::apply_act(t, p.act, p.slope);
        } else if (c < p.cw) {
          orow[c] = 0.f;
        }
      }
    }
  }
}

// Stride-parity class of a dgrad problem (blockIdx.y = py * stride + px): the input pixels (iyf + a * s, ixf + b * s), a < Hc, b < Wc,
// of the (possibly padded) input plane receive only the filter taps (py + jy * s, px + jx * s), jy < nty, jx < ntx; class pixel (a, b)
// and class tap (jy, jx) meet at dy pixel (cy0 + a - jy, cx0 + b - jx).
struct DgradClass { int s, py, px, iyf, ixf, Hc, Wc, cy0, cx0, nty, ntx, Mc; };
__device__ __forceinline__ DgradClass dgrad_class(const IgemmArgs& p, int cls) {
  DgradClass c;
  c.s = p.stride;
  c.py = cls / c.s;
  c.px = cls % c.s;
  c.iyf = ((c.py - p.pad_eff) % c.s + c.s) % c.s;
  c.ixf = ((c.px - p.pad_eff) % c.s + c.s) % c.s;
  c.Hc = c.iyf < p.Hin ? (p.Hin - c.iyf + c.s - 1) / c.s : 0;
  c.Wc = c.ixf < p.Win ? (p.Win - c.ixf + c.s - 1) / c.s : 0;
  c.cy0 = (c.iyf + p.pad_eff - c.py) / c.s;
  c.cx0 = (c.ixf + p.pad_eff - c.px) / c.s;
  c.nty = c.py < p.kh ? (p.kh - c.py + c.s - 1) / c.s : 0;
  c.ntx = c.px < p.kw ? (p.kw - c.px + c.s - 1) / c.s : 0;
  c.Mc = p.N * c.Hc * c.Wc;
  return c;
}
// output pixel of class pixel m (< Mc) in the input plane, in pixels
__device__ __forceinline__ int64_t dgrad_out_pixel(const IgemmArgs& p, const DgradClass& c, int m) {
  const Pixel px = decode_pixel(m, c.Hc * c.Wc, c.Wc);
  return ((int64_t)px.n * p.Hin + (c.iyf + px.y * c.s)) * p.Win + (c.ixf + px.x * c.s);
}

// One weight-gradient element (filter co, column k = (tap, ci)): straight into dw (`direct`, optionally accumulating) or into this pixel
// slice's (blockIdx.y) workspace [slice][Cout][K]
__device__ __forceinline__ void store_dw(const IgemmArgs& p, int co, int k, int tap, int ci, int taps, float v) {
  if (p.direct) {
    if (ci < p.cval) {   // cval = writable channels per tap (Cin, or the padded extent when the storage is padded)
      float* dst = p.out + ((int64_t)co * taps + tap) * p.wcs + ci;
      *dst = p.accumulate ? *dst + v : v;
    }
  } else {
    p.out[((int64_t)blockIdx.y * p.Cout + co) * p.K + k] = v;
  }
}

// ------------------------------------------------------------------------------------------------ forward
// EX (cat_conv2d_fwd_ex): taps `dil` pixels apart and a residual in the epilogue; EX = false compiles to the code it was before
template <int MT, int NT, int WM, int WN, bool WVEC = false, int SCHED = 0, bool EX = false>
__global__ __launch_bounds__(256) void conv_fwd_kernel(IgemmArgs p) {
  constexpr int BM = WM * MT * 16, BN = WN * NT * 16;
  constexpr int AI = BM / 64, BI = (BN + 63) / 64;
  __shared__ __attribute__((aligned(16))) float smem[2 * (BM + BN) * 16];
  float* sA = smem;
  float* sB = smem + 2 * BM * 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int ntn = (p.Cout + BN - 1) / BN;
  const int bid = cat::xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (bid / ntn) * BM, n0 = (bid % ntn) * BN;
  const int q = tid & 3, r0 = tid >> 2;
  const int HoWo = p.Ho * p.Wo;
  const int taps = p.kh * p.kw;
  const int dil = EX ? p.dil : 1;

  int iy0[AI], ix0[AI];
  int64_t xoff[AI];
  bool rv[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    const int m = m0 + r0 + 64 * i;
    rv[i] = m < p.M;
    const Pixel o = decode_pixel(rv[i] ? m : 0, HoWo, p.Wo);
    iy0[i] = o.y * p.stride - p.pad;
    ix0[i] = o.x * p.stride - p.padw;
    xoff[i] = (int64_t)o.n * p.H * p.W * p.xcs;
  }
  const float* wrow[BI];
  bool bv[BI];
#pragma unroll
  for (int i = 0; i < BI; ++i) {
    const int r = r0 + 64 * i, co = n0 + r;
    bv[i] = r < BN && co < p.Cout;
    wrow[i] = p.b + (int64_t)(bv[i] ? co : 0) * taps * p.wcs;
  }

  // K walk of this thread's quad: k = kc*16 + q*4 = (tap, ci).  The walk is INCREMENTAL -- on gfx950 the fp32 MFMA runs at the
  // fp32 VALU rate on shared issue slots, so every vector instruction in this loop is paid in matrix throughput (measured:
  // 64 MFMA + ~250 VALU per chunk = 65 % of peak).  Steady state costs two pointer bumps per operand; only lanes whose quad
  // crosses a tap boundary take the (divergent, rare for wide layers) re-location branch.
  const bool aligned = (p.c4 & 15) == 0;
  int k = q * 4, ci, ky, kx;
  {
    const int tap = k / p.c4;
    ci = k - tap * p.c4;
    ky = tap / p.kw;
    kx = tap - ky * p.kw;
  }
  const float* pa[AI];
  bool va[AI];
  const float* pb[BI];
  auto locate = [&]() {
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      int iy = iy0[i] + ky * dil, ix = ix0[i] + kx * dil;
      const bool inr = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
      const int ry = cat::reflect_idx(iy, p.H), rx = cat::reflect_idx(ix, p.W);
      iy = p.reflect ? ry : (inr ? iy : 0);
      ix = p.reflect ? rx : (inr ? ix : 0);
      va[i] = rv[i] && (p.reflect || inr);
      pa[i] = p.a + xoff[i] + ((int64_t)iy * p.W + ix) * p.xcs + ci;
    }
  };
  locate();
#pragma unroll
  for (int i = 0; i < BI; ++i) pb[i] = wrow[i] + (int64_t)(ky * p.kw + kx) * p.wcs + ci;

  f4 ra[AI], rb[BI];
  auto gload = [&]() {   // loads the chunk the walk currently points at, then advances the walk by 16
    const bool kv = k < p.K && ci < p.cval;
#pragma unroll
    for (int i = 0; i < AI; ++i) ra[i] = ldg4_or_zero(va[i] && kv, pa[i]);
#pragma unroll
    for (int i = 0; i < BI; ++i) rb[i] = ldw4_or_zero(bv[i] && kv, WVEC, pb[i], ci, p.Cin);
    k += 16;
    ci += 16;
    if (aligned) {   // c4 % 16 == 0: all quads of a chunk sit in one tap, so this branch is wave-uniform (and rare)
      if (ci >= p.c4) {
        ci -= p.c4;
        next_tap(ky, kx, p.kw);
        locate();
#pragma unroll
        for (int i = 0; i < BI; ++i) pb[i] += 16 + p.wcs - p.c4;
      } else {
#pragma unroll
        for (int i = 0; i < AI; ++i) pa[i] += 16;
#pragma unroll
        for (int i = 0; i < BI; ++i) pb[i] += 16;
      }
    } else {         // ragged channel counts: lanes cross tap boundaries at different chunks -> re-locate every chunk, no divergence
      int adj = 16;
      while (ci >= p.c4) {   // one iteration unless c4 < 16
        ci -= p.c4;
        adj += p.wcs - p.c4;
        const bool w = ++kx == p.kw;
        kx = w ? 0 : kx;
        ky += w ? 1 : 0;
      }
      locate();
#pragma unroll
      for (int i = 0; i < BI; ++i) pb[i] += adj;
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < AI; ++i) *reinterpret_cast<f4*>(sA + buf * BM * 16 + swz(r0 + 64 * i, q)) = ra[i];
#pragma unroll
    for (int i = 0; i < BI; ++i)
      if (r0 + 64 * i < BN) *reinterpret_cast<f4*>(sB + buf * BN * 16 + swz(r0 + 64 * i, q)) = rb[i];
  };

  f4 acc[MT][NT];
  zero_acc(acc);

  const int nk = (p.K + 15) >> 4;
  gload();
  sstore(0);
  __syncthreads();
  // steady state: one basic block per chunk (prefetch of chunk kc+1 is unconditional; the last chunk is peeled) so that the
  // scheduler directives below can interleave the gather's address arithmetic / loads with the MFMA stream
  const bool pdbg = cat::kDiag && p.dbg != nullptr;      // compile-time false in the production library
  const bool dbg = pdbg && blockIdx.x == 9 && tid == 0;
  long long t_load = 0, t_mma = 0, t_store = 0, t_bar = 0;
  for (int kc = 0; kc + 1 < nk; ++kc) {
    const int buf = kc & 1;
    long long c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
    if (pdbg) { __builtin_amdgcn_sched_barrier(0); c0 = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); }
    gload();
    if (pdbg) { __builtin_amdgcn_sched_barrier(0); c1 = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); }
    mma_kcontig_a_kcontig_b<MT, NT>(sA + buf * BM * 16, sB + buf * BN * 16, wm * MT * 16, wn * NT * 16, lane, acc);
    __builtin_amdgcn_sched_barrier(0);   // keep the LDS stores (which wait for the prefetch) behind the MFMA stream
    if (pdbg) { c2 = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); }
    sstore(buf ^ 1);
    if (pdbg) { __builtin_amdgcn_sched_barrier(0); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); c3 = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); }
    if (SCHED == 1) {
#pragma unroll
      for (int g = 0; g < MT * NT * 4; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);  // 4 VALU
      }
    } else if (SCHED == 2) {
      __builtin_amdgcn_iglp_opt(0);
    }
    __syncthreads();
    if (pdbg) {
      __builtin_amdgcn_sched_barrier(0);
      c4 = __builtin_readcyclecounter();
      t_load += c1 - c0; t_mma += c2 - c1; t_store += c3 - c2; t_bar += c4 - c3;
    }
  }
  if (dbg) { p.dbg[0] = t_load; p.dbg[1] = t_mma; p.dbg[2] = t_store; p.dbg[3] = t_bar; p.dbg[4] = nk - 1; }
  mma_kcontig_a_kcontig_b<MT, NT>(sA + ((nk - 1) & 1) * BM * 16, sB + ((nk - 1) & 1) * BN * 16, wm * MT * 16, wn * NT * 16, lane, acc);

  store_rows<MT, NT, EX>(p, acc, m0 + wm * MT * 16, n0 + wn * NT * 16, lane);
}

// ------------------------------------------------------------------------------------------------ forward, BK = 32
// Same tiling as conv_fwd_kernel with 32-deep K chunks: the per-chunk fixed cost (pointer bumps, LDS stores, barrier, fragment
// read latency: ~700 shader clocks measured) is amortised over twice the MFMA work.  Used when the per-tap K extent is a
// multiple of 32 (so a chunk never straddles taps and the walk is wave-uniform) and the filter rows are float4-readable.
// Invalid rows / padding taps keep their pointer parked on the zero page (increment 0), so the steady state is one 64-bit add per
// load and nothing else on the vector ALU.
template <int MT, int NT, int WM, int WN, bool EX = false>
__global__ __launch_bounds__(256) void conv_fwd32_kernel(IgemmArgs p) {
  constexpr int BM = WM * MT * 16, BN = WN * NT * 16;
  constexpr int AI = BM / 32, BI = (BN + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sA = smem;
  float* sB = smem + 2 * BM * 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int ntn = (p.Cout + BN - 1) / BN;
  const int bid = cat::xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (bid / ntn) * BM, n0 = (bid % ntn) * BN;
  // staging map: waves 0-1 fetch the first 16 k of the chunk, waves 2-3 the second 16, so the (tap, channel) walk is uniform
  // inside every wave for ANY tap extent that is a multiple of 16 (a 32-chunk may straddle two taps, a 16-half never does)
  const int half = __builtin_amdgcn_readfirstlane(wave >> 1);
  const int q4 = tid & 3, q = half * 4 + q4, r0 = (tid & 127) >> 2;
  const int HoWo = p.Ho * p.Wo;
  const int taps = p.kh * p.kw;
  const int dil = EX ? p.dil : 1;

  int iy0[AI], ix0[AI];
  int64_t xoff[AI];
  bool rv[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    const int m = m0 + r0 + 32 * i;
    rv[i] = m < p.M;
    const Pixel o = decode_pixel(rv[i] ? m : 0, HoWo, p.Wo);
    iy0[i] = o.y * p.stride - p.pad;
    ix0[i] = o.x * p.stride - p.padw;
    xoff[i] = (int64_t)o.n * p.H * p.W * p.xcs;
  }
  const int nk_all = (p.K + 31) >> 5;   // a trailing half chunk reads zeros (tap >= taps)
  const int kbeg = p.ksplit > 1 ? (int)blockIdx.y * p.kchunks : 0;
  const int nk = p.ksplit > 1 ? min(nk_all, kbeg + p.kchunks) - kbeg : nk_all;
  // walk state: tap = (ky, kx), ci = channel of this quad inside the tap; advanced by 32 per chunk
  int tap, ci, ky, kx;
  {
    const int k = q * 4 + kbeg * 32;
    tap = k / p.c4;
    ci = k - tap * p.c4;
    ky = tap / p.kw;
    kx = tap - ky * p.kw;
  }
  const float* pa[AI];
  int inca[AI];
  auto locate = [&]() {
    const bool cv = ci < p.cval && tap < taps;
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      int iy = iy0[i] + ky * dil, ix = ix0[i] + kx * dil;
      const bool inr = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
      const int ry = cat::reflect_idx(iy, p.H), rx = cat::reflect_idx(ix, p.W);
      iy = p.reflect ? ry : (inr ? iy : 0);
      ix = p.reflect ? rx : (inr ? ix : 0);
      const bool v = rv[i] && (p.reflect || inr) && cv;
      pa[i] = v ? p.a + xoff[i] + ((int64_t)iy * p.W + ix) * p.xcs + ci : g_zero_page;
      inca[i] = v ? 32 : 0;
    }
  };
  locate();
  const float* brow[BI];
  const float* pb[BI];
  int incb[BI];
  bool bok[BI];
  auto locate_b = [&]() {
    const bool cv = ci < p.cval && tap < taps;
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      const bool v = bok[i] && cv;
      pb[i] = v ? brow[i] + (int64_t)tap * p.wcs + ci : g_zero_page;
      incb[i] = v ? 32 : 0;
    }
  };
#pragma unroll
  for (int i = 0; i < BI; ++i) {
    const int r = r0 + 32 * i, co = n0 + r;
    bok[i] = r < BN && co < p.Cout;
    brow[i] = p.b + (int64_t)(bok[i] ? co : 0) * taps * p.wcs;
  }
  locate_b();
  const bool padded = p.c4 != p.cval;   // tap extent rounded up: validity of a quad changes inside a tap

  f4 ra[AI], rb[BI];
  auto gload = [&]() {
#pragma unroll
    for (int i = 0; i < AI; ++i) ra[i] = ldg4(pa[i]);
#pragma unroll
    for (int i = 0; i < BI; ++i) rb[i] = ldg4(pb[i]);
    ci += 32;
    bool moved = padded;
    while (ci >= p.c4) {   // wave-uniform
      ci -= p.c4;
      ++tap;
      next_tap(ky, kx, p.kw);
      moved = true;
    }
    if (moved) {
      locate();
      locate_b();
    } else {
#pragma unroll
      for (int i = 0; i < AI; ++i) pa[i] += inca[i];
#pragma unroll
      for (int i = 0; i < BI; ++i) pb[i] += incb[i];
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < AI; ++i) *reinterpret_cast<f4*>(sA + buf * BM * 32 + swz32(r0 + 32 * i, q)) = ra[i];
#pragma unroll
    for (int i = 0; i < BI; ++i)
      if (r0 + 32 * i < BN) *reinterpret_cast<f4*>(sB + buf * BN * 32 + swz32(r0 + 32 * i, q)) = rb[i];
  };
  const int lr = lane & 15, lq = lane >> 4;
  f4 acc[MT][NT];
  zero_acc(acc);
  auto mma = [&](int buf) {
    mma32_kcontig_a_kcontig_b<false>(sA + buf * BM * 32, sB + buf * BN * 32, wm * MT * 16, wn * NT * 16, lane, acc);
  };

  gload();
  sstore(0);
  __syncthreads();
  for (int kc = 0; kc + 1 < nk; ++kc) {
    const int buf = kc & 1;
    gload();
    mma(buf);
    __builtin_amdgcn_sched_barrier(0);
    sstore(buf ^ 1);
    __syncthreads();
  }
  mma((nk - 1) & 1);

  if (p.ksplit > 1) {   // raw partial sums of this K slice
    float* part = p.part + (int64_t)blockIdx.y * p.M * p.ycs;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int col = n0 + wn * NT * 16 + j * 16 + lr;
      if (col >= p.Cout) continue;
#pragma unroll
      for (int i = 0; i < MT; ++i) {
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const int m = m0 + wm * MT * 16 + i * 16 + lq * 4 + rg;
          if (m < p.M) part[(int64_t)m * p.ycs + col] = acc[i][j][rg];
        }
      }
    }
    return;
  }
  store_rows<MT, NT, EX>(p, acc, m0 + wm * MT * 16, n0 + wn * NT * 16, lane);
}

// ------------------------------------------------------------------------------------------------ forward, BK = 32, direct-to-LDS staging
// conv_fwd32_kernel's 128 x 128 x 32 tiling with the operand tiles DMA-ed straight into LDS (buffer_load_dwordx4 ... lds): no staging
// VGPRs, no ds_write pass, and -- because the per-lane part of every address is a 32-bit voffset that only changes when the walk moves to
// the next filter tap, while the advance along the channels is an SGPR soffset -- no vector-ALU address arithmetic in the steady state.
// (On gfx950 the fp32 MFMA shares its issue slots with the vector ALU: 8 loads + 8 ds_write_b128 + ~40 VALU per 128 MFMAs cost the
// register-staged kernel ~15 % of the matrix pipe.)  A lane-linear LDS image is what the DMA writes, so the XOR swizzle of the [row][32 k]
// tiles is applied to the SOURCE quad each lane fetches (guide rule 21); the fragment reads keep conv_fwd32_kernel's swz32.
// Out-of-image / padding / tail lanes carry voffset 0x80000000: beyond num_records, the buffer unit returns zeros.
// Preconditions (host): Cin % 32 == 0 (a 32-chunk never straddles taps), float4-readable filters, tensors < 2 GB.
// 2 x 2 waves of 4 x 4 MFMA tiles.
template <bool EX = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv_fwd32d_kernel(IgemmArgs p) {
  constexpr int MT = 4, NT = 4, WN = 2, BM = 128, BN = 128;
  const int dil = EX ? p.dil : 1;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sA = smem;
  float* sB = smem + 2 * BM * 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int ntn = (p.Cout + BN - 1) / BN;
  const int bid = cat::xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (bid / ntn) * BM, n0 = (bid % ntn) * BN;
  const int HoWo = p.Ho * p.Wo, taps = p.kh * p.kw;
  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.a), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.b), 0, 0x7fffffff, 0x00020000);
  // staging map: wave w, instruction i -> rows (w * 4 + i) * 8 + (lane >> 3) of the tile, LDS slot lane & 7 <- source quad slot ^ swz(row)
  const int slot = lane & 7, lrow = lane >> 3;
  int iy0[4], ix0[4];
  unsigned abase[4], aq[4], voffA[4], voffB[4];
  bool rv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (wave * 4 + i) * 8 + lrow;
    const unsigned q = (unsigned)(slot ^ ((row >> 1) & 7));
    const int m = m0 + row;
    rv[i] = m < p.M;
    const Pixel o = decode_pixel(rv[i] ? m : 0, HoWo, p.Wo);
    iy0[i] = o.y * p.stride - p.pad;
    ix0[i] = o.x * p.stride - p.padw;
    abase[i] = (unsigned)o.n * (unsigned)(p.H * p.W) * (unsigned)p.xcs * 4u;
    aq[i] = q * 16u;
    const int co = n0 + row;
    voffB[i] = co < p.Cout ? (unsigned)co * (unsigned)(taps * p.wcs) * 4u + q * 16u : 0x80000000u;
  }
  auto locate = [&](int ky, int kx) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int iy = iy0[i] + ky * dil, ix = ix0[i] + kx * dil;
      const bool inr = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
      const int ry = cat::reflect_idx(iy, p.H), rx = cat::reflect_idx(ix, p.W);
      iy = p.reflect ? ry : (inr ? iy : 0);
      ix = p.reflect ? rx : (inr ? ix : 0);
      const bool v = rv[i] && (p.reflect || inr);
      voffA[i] = v ? abase[i] + (unsigned)(iy * p.W + ix) * (unsigned)p.xcs * 4u + aq[i] : 0x80000000u;
    }
  };
  int tap = 0, ky = 0, kx = 0, ci = 0;      // walk state of the NEXT chunk to fetch (wave-uniform)
  locate(0, 0);
  auto issue = [&](int buf) {
    const unsigned soA = (unsigned)ci * 4u, soB = (unsigned)(tap * p.wcs + ci) * 4u;
    dma_chunk(rA, rB, sA + buf * BM * 32, sB + buf * BN * 32, wave, voffA, voffB, soA, soB);
    ci += 32;
    if (ci >= p.c4) {      // next tap (wave-uniform, once per Cin / 32 chunks)
      ci = 0;
      ++tap;
      next_tap(ky, kx, p.kw);
      if (tap < taps) locate(ky, kx);
    }
  };
  const int lr = lane & 15, lq = lane >> 4;
  f4 acc[MT][NT];
  zero_acc(acc);
  auto mma = [&](int buf) {   // filters first: transposed accumulators, see the epilogue
    mma32_kcontig_a_kcontig_b<true>(sA + buf * BM * 32, sB + buf * BN * 32, wm * MT * 16, wn * NT * 16, lane, acc);
  };
  const int nk = taps * (p.c4 >> 5);
  issue(0);
  __builtin_amdgcn_s_waitcnt(0);     // vmcnt(0): the DMA has landed
  __syncthreads();
  for (int kc = 0; kc + 1 < nk; ++kc) {
    const int buf = kc & 1;
    issue(buf ^ 1);                   // in flight behind this chunk's MFMA stream; buf ^ 1 was released by the barrier below
    mma(buf);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }
  mma((nk - 1) & 1);

  // The filter fragment went in as the MFMA's FIRST operand: the accumulators are transposed (store_pixel_t)
  const bool vec = (p.ycs & 3) == 0 && (reinterpret_cast<uintptr_t>(p.out) & 15) == 0;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = m0 + wm * MT * 16 + i * 16 + lr;
    if (m >= p.M) continue;
    store_pixel_t<MT, NT, EX>(p, p.out + (int64_t)m * p.ycs, acc, i, n0 + wn * NT * 16 + lq * 4, p.Cout, vec,
                              (EX && p.res) ? p.res + (int64_t)m * p.rcs : nullptr);
  }
}

// ------------------------------------------------------------------------------------------------ dgrad
// blockIdx.y = parity class (py, px) of the forward stride.  N dimension = Cin, K = taps(class) * cout4.
template <int MT, int NT, int WM, int WN>
__global__ __launch_bounds__(256) void conv_dgrad_kernel(IgemmArgs p) {
  constexpr int BM = WM * MT * 16, BN = WN * NT * 16, LDB = BN + 4;
  constexpr int AI = BM / 64;
  constexpr int BQ = BN / 4;                 // float4 per k-row of the B tile
  constexpr int BI = (16 * BQ + 255) / 256;  // float4 per thread
  __shared__ __attribute__((aligned(16))) float smem[2 * (BM * 16 + 16 * LDB)];
  float* sA = smem;
  float* sB = smem + 2 * BM * 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const DgradClass cls = dgrad_class(p, blockIdx.y);
  const int K = cls.nty * cls.ntx * p.c4;
  const int ntn = (p.Cin + BN - 1) / BN;
  const int bid = cat::xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (bid / ntn) * BM, n0 = (bid % ntn) * BN;
  if (m0 >= cls.Mc) return;
  const int q = tid & 3, r0 = tid >> 2;
  const int HcWc = cls.Hc * cls.Wc;
  const int taps = p.kh * p.kw;

  int cy[AI], cx[AI];
  int64_t aoff[AI];
  bool rv[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    const int m = m0 + r0 + 64 * i;
    rv[i] = m < cls.Mc;
    const Pixel cp = decode_pixel(rv[i] ? m : 0, HcWc, cls.Wc);
    cy[i] = cls.cy0 + cp.y;
    cx[i] = cls.cx0 + cp.x;
    aoff[i] = (int64_t)cp.n * p.Ho * p.Wo * p.ycs;
  }

  // incremental K walk (see conv_fwd_kernel): A quad = (tap (jy,jx), co..co+3) of dy; B rows = 16 consecutive k of the chunk
  const bool aligned = (p.c4 & 15) == 0;
  const int nk_all = (K + 15) >> 4;
  const int kbeg = p.ksplit > 1 ? (int)blockIdx.z * p.kchunks : 0;
  const int nk = p.ksplit > 1 ? max(0, min(nk_all, kbeg + p.kchunks) - kbeg) : nk_all;
  int ka = q * 4 + kbeg * 16, aco, ajy, ajx;
  {
    const int tj = p.c4 ? ka / p.c4 : 0;
    aco = ka - tj * p.c4;
    ajy = cls.ntx ? tj / cls.ntx : 0;
    ajx = tj - ajy * cls.ntx;
  }
  const float* pa[AI];
  bool va[AI];
  auto locate_a = [&]() {
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      const int oy = cy[i] - ajy, ox = cx[i] - ajx;
      const bool inr = (unsigned)oy < (unsigned)p.Ho && (unsigned)ox < (unsigned)p.Wo;
      va[i] = rv[i] && inr;
      pa[i] = p.a + aoff[i] + ((int64_t)(inr ? oy : 0) * p.Wo + (inr ? ox : 0)) * p.ycs + aco;
    }
  };
  locate_a();
  int kb[BI], bco[BI], bjy[BI], bjx[BI], bci[BI];
  const float* pb[BI];
  bool vb[BI];
  auto locate_b = [&](int i) {
    const int ky = cls.py + bjy[i] * cls.s, kx = cls.px + bjx[i] * cls.s;
    vb[i] = bco[i] < p.Cout && bci[i] < p.Cin;
    pb[i] = p.b + ((int64_t)(vb[i] ? bco[i] : 0) * taps + ky * p.kw + kx) * p.wcs + bci[i];
  };
#pragma unroll
  for (int i = 0; i < BI; ++i) {
    const int idx = tid + 256 * i;
    const int kr = idx / BQ, nq = idx - kr * BQ;
    kb[i] = kr < 16 ? kr + kbeg * 16 : (1 << 30);   // rows >= 16 (thread has no work in this slot) never become valid
    const int kk = kr < 16 ? kr + kbeg * 16 : 0;
    const int tj = p.c4 ? kk / p.c4 : 0;
    bco[i] = kk - tj * p.c4;
    bjy[i] = cls.ntx ? tj / cls.ntx : 0;
    bjx[i] = tj - bjy[i] * cls.ntx;
    bci[i] = n0 + nq * 4;
    locate_b(i);
  }

  f4 ra[AI], rb[BI];
  auto gload = [&]() {
    const bool kva = ka < K && aco < p.cval;
#pragma unroll
    for (int i = 0; i < AI; ++i) ra[i] = ldg4_or_zero(va[i] && kva, pa[i]);
#pragma unroll
    for (int i = 0; i < BI; ++i) rb[i] = ldw4_or_zero(vb[i] && kb[i] < K, p.wvec, pb[i], bci[i], p.Cin);
    ka += 16;
    aco += 16;
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      kb[i] += 16;
      bco[i] += 16;
    }
    if (aligned) {   // wave-uniform: every quad / row of the chunk wraps to the next tap together
      if (aco >= p.c4) {
        aco -= p.c4;
        next_tap(ajy, ajx, cls.ntx);
        locate_a();
#pragma unroll
        for (int i = 0; i < BI; ++i) {
          bco[i] -= p.c4;
          next_tap(bjy[i], bjx[i], cls.ntx);
          locate_b(i);
        }
      } else {
#pragma unroll
        for (int i = 0; i < AI; ++i) pa[i] += 16;
#pragma unroll
        for (int i = 0; i < BI; ++i) {
          vb[i] = bco[i] < p.Cout && bci[i] < p.Cin;
          pb[i] += (int64_t)16 * taps * p.wcs;
        }
      }
    } else {
      while (aco >= p.c4) {
        aco -= p.c4;
        const bool w = ++ajx == cls.ntx;
        ajx = w ? 0 : ajx;
        ajy += w ? 1 : 0;
      }
      locate_a();
#pragma unroll
      for (int i = 0; i < BI; ++i) {
        while (bco[i] >= p.c4) {
          bco[i] -= p.c4;
          const bool w = ++bjx[i] == cls.ntx;
          bjx[i] = w ? 0 : bjx[i];
          bjy[i] += w ? 1 : 0;
        }
        locate_b(i);
      }
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < AI; ++i) *reinterpret_cast<f4*>(sA + buf * BM * 16 + swz(r0 + 64 * i, q)) = ra[i];
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      const int idx = tid + 256 * i;
      const int kr = idx / BQ, nq = idx - kr * BQ;
      if (kr < 16) *reinterpret_cast<f4*>(sB + buf * 16 * LDB + kr * LDB + nq * 4) = rb[i];
    }
  };

  f4 acc[MT][NT];
  zero_acc(acc);

  const int lr = lane & 15, lq = lane >> 4;
  if (nk > 0) {
    gload();
    sstore(0);
  }
  __syncthreads();
  for (int kc = 0; kc < nk; ++kc) {
    const int buf = kc & 1;
    if (kc + 1 < nk) gload();
    {
      const float* A = sA + buf * BM * 16;
      const float* B = sB + buf * 16 * LDB;
      f4 fa[MT];
      float fb[NT][4];
#pragma unroll
      for (int i = 0; i < MT; ++i) fa[i] = *reinterpret_cast<const f4*>(A + swz(wm * MT * 16 + i * 16 + lr, lq));
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) fb[j][t] = B[(lq * 4 + t) * LDB + wn * NT * 16 + j * 16 + lr];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][t], fb[j][t], acc[i][j], 0, 0, 0);
    }
    if (kc + 1 < nk) sstore(buf ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const int m = m0 + wm * MT * 16 + i * 16 + lq * 4 + rg;
      if (m >= cls.Mc) continue;
      const int64_t opix = dgrad_out_pixel(p, cls, m) * p.ocs;
      if (p.ksplit > 1) {   // raw partial sums of this K slice
        float* prow = p.part + (int64_t)blockIdx.z * p.N * p.Hin * p.Win * p.ocs + opix;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const int col = n0 + wn * NT * 16 + j * 16 + lr;
          if (col < p.Cin) prow[col] = acc[i][j][rg];
        }
        continue;
      }
      float* orow = p.out + opix;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int col = n0 + wn * NT * 16 + j * 16 + lr;
        if (col < p.Cin) {
          const float bias = p.bias ? p.bias[col] : 0.f;
          orow[col] = cat::apply_act(acc[i][j][rg] + bias, p.act, p.slope);
        } else if (col < p.cw) {
          orow[col] = 0.f;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ dgrad, BK = 32
// conv_dgrad_kernel with 32-deep K chunks and parked pointers (see conv_fwd32_kernel), for the wide layers that carry the
// discriminator's backward pass: Cout % 16 == 0 (every 16-half of a chunk sits inside one tap and c4 == Cout, so validity never
// changes inside a tap), float4-readable filter rows, BN % 64 == 0.  The N-contiguous B tile is [32 k][BN] WITHOUT row padding
// (2 x (BM + BN) x 32 floats = 64 KB at 128 x 128): the 16-column group of a row is XOR-ed with (row >> 2) & 3 instead, which puts the
// four k-rows a wave reads per ds_read_b32 (rows 4 apart) into four different 16-bank groups.
template <int MT, int NT, int WM, int WN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv_dgrad32_kernel(IgemmArgs p) {
  constexpr int BM = WM * MT * 16, BN = WN * NT * 16;
  static_assert(BN % 64 == 0 && 256 % (BN / 4) == 0, "B tile swizzle needs 64-column multiples");
  constexpr int AI = BM / 32;
  constexpr int BQ = BN / 4;          // float4 per k-row of the B tile
  constexpr int BR = 256 / BQ;        // k-rows staged per pass of the workgroup
  constexpr int BI = 32 / BR;         // float4 per thread
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sA = smem;
  float* sB = smem + 2 * BM * 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const DgradClass cls = dgrad_class(p, blockIdx.y);
  const int ntaps = cls.nty * cls.ntx, ntxd = cls.ntx > 0 ? cls.ntx : 1;
  const int K = ntaps * p.c4;
  const int ntn = (p.Cin + BN - 1) / BN;
  const int bid = cat::xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (bid / ntn) * BM, n0 = (bid % ntn) * BN;
  if (m0 >= cls.Mc) return;
  const int half = __builtin_amdgcn_readfirstlane(wave >> 1);
  const int q4 = tid & 3, q = half * 4 + q4, r0 = (tid & 127) >> 2;
  const int HcWc = cls.Hc * cls.Wc;
  const int taps = p.kh * p.kw;

  int cy[AI], cx[AI];
  int64_t aoff[AI];
  bool rv[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    const int m = m0 + r0 + 32 * i;
    rv[i] = m < cls.Mc;
    const Pixel cp = decode_pixel(rv[i] ? m : 0, HcWc, cls.Wc);
    cy[i] = cls.cy0 + cp.y;
    cx[i] = cls.cx0 + cp.x;
    aoff[i] = (int64_t)cp.n * p.Ho * p.Wo * p.ycs;
  }

  // A walk: this thread's quad = (class tap atj = (ajy, ajx), channels aco .. aco+3 of dy), advanced by 32 per chunk
  int atj, aco, ajy, ajx;
  {
    const int ka = q * 4;
    atj = ka / p.c4;
    aco = ka - atj * p.c4;
    ajy = atj / ntxd;
    ajx = atj - ajy * ntxd;
  }
  const float* pa[AI];
  int inca[AI];
  auto locate_a = [&]() {
    const bool tv = atj < ntaps;
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      const int oy = cy[i] - ajy, ox = cx[i] - ajx;
      const bool v = rv[i] && tv && (unsigned)oy < (unsigned)p.Ho && (unsigned)ox < (unsigned)p.Wo;
      pa[i] = v ? p.a + aoff[i] + ((int64_t)oy * p.Wo + ox) * p.ycs + aco : g_zero_page;
      inca[i] = v ? 32 : 0;
    }
  };
  locate_a();
  // B walk: k-row (class tap btj, filter bco) x float4 of input channels; one filter row = taps * wcs floats
  const int nq = tid % BQ, bci = n0 + nq * 4;
  const bool bcv = bci < p.Cin;
  const int bstep = 32 * taps * p.wcs;   // < 2^31 (checked on the host)
  int btj[BI], bco[BI];
  const float* pb[BI];
  int incb[BI];
  auto locate_b = [&](int i) {
    const int jy = btj[i] / ntxd, jx = btj[i] - jy * ntxd;
    const int ky = cls.py + jy * cls.s, kx = cls.px + jx * cls.s;
    const bool v = bcv && btj[i] < ntaps;
    pb[i] = v ? p.b + ((int64_t)bco[i] * taps + ky * p.kw + kx) * p.wcs + bci : g_zero_page;
    incb[i] = v ? bstep : 0;
  };
#pragma unroll
  for (int i = 0; i < BI; ++i) {
    const int kr = tid / BQ + BR * i;
    btj[i] = kr / p.c4;
    bco[i] = kr - btj[i] * p.c4;
    locate_b(i);
  }

  f4 ra[AI], rb[BI];
  auto gload = [&]() {
#pragma unroll
    for (int i = 0; i < AI; ++i) ra[i] = ldg4(pa[i]);
#pragma unroll
    for (int i = 0; i < BI; ++i) rb[i] = ldg4(pb[i]);
    aco += 32;
    if (aco >= p.c4) {   // wave-uniform: the 16 k of this wave's half sit in one tap
      do {
        aco -= p.c4;
        ++atj;
        next_tap(ajy, ajx, ntxd);
      } while (aco >= p.c4);
      locate_a();
    } else {
#pragma unroll
      for (int i = 0; i < AI; ++i) pa[i] += inca[i];
    }
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      bco[i] += 32;
      if (bco[i] >= p.c4) {   // wave-uniform as well (a wave stages rows of one 16-group per pass)
        do {
          bco[i] -= p.c4;
          ++btj[i];
        } while (bco[i] >= p.c4);
        locate_b(i);
      } else {
        pb[i] += incb[i];
      }
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < AI; ++i) *reinterpret_cast<f4*>(sA + buf * BM * 32 + swz32(r0 + 32 * i, q)) = ra[i];
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      const int kr = tid / BQ + BR * i;
      *reinterpret_cast<f4*>(sB + buf * 32 * BN + kr * BN + ((nq * 4) ^ (((kr >> 2) & 3) << 4))) = rb[i];
    }
  };

  f4 acc[MT][NT];
  zero_acc(acc);

  const int lr = lane & 15, lq = lane >> 4;
  auto mma = [&](int buf) {
    mma32_kcontig_a_ncontig_b<false, BN>(sA + buf * BM * 32, sB + buf * 32 * BN, wm * MT * 16, wn * NT * 16, lane, acc);
  };

  const int nk = (K + 31) >> 5;   // a trailing half chunk has tap == ntaps: parked on the zero page
  if (nk > 0) {
    gload();
    sstore(0);
    __syncthreads();
    for (int kc = 0; kc + 1 < nk; ++kc) {
      const int buf = kc & 1;
      gload();
      mma(buf);
      __builtin_amdgcn_sched_barrier(0);
      sstore(buf ^ 1);
      __syncthreads();
    }
    mma((nk - 1) & 1);
  }

#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const int m = m0 + wm * MT * 16 + i * 16 + lq * 4 + rg;
      if (m >= cls.Mc) continue;
      float* orow = p.out + dgrad_out_pixel(p, cls, m) * p.ocs;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int col = n0 + wn * NT * 16 + j * 16 + lr;
        if (col < p.Cin) {
          const float bias = p.bias ? p.bias[col] : 0.f;
          orow[col] = cat::apply_act(acc[i][j][rg] + bias, p.act, p.slope);
        } else if (col < p.cw) {
          orow[col] = 0.f;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ dgrad, BK = 32, direct-to-LDS staging
// conv_dgrad32_kernel with both operand tiles DMA-ed into LDS (see conv_fwd32d_kernel).  A = dy rows ([class pixel][32 k], source quad
// pre-swizzled); B = the filter slab [32 k][128 input channels], whose per-lane voffset NEVER changes: k = (class tap, filter co) only moves
// the SGPR soffset (+32 filters per chunk, a new tap offset when co wraps).  The 16-column-group XOR of the N-contiguous tile is applied
// to the source column each lane fetches.  Preconditions (host): Cout % 32 == 0, Cin % 4 == 0, float4-readable filters, tensors < 2 GB.
// BT: the filter operand comes from a copy transposed to [Cin][taps][Cout] (K-contiguous rows like the forward kernel's B tile: fragments
// are read with ds_read_b128 instead of sixteen ds_read_b32 per half chunk); its voffsets are constant as well.
template <bool BT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv_dgrad32d_kernel(IgemmArgs p) {
  constexpr int MT = 4, NT = 4, WN = 2, BM = 128, BN = 128;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sA = smem;
  float* sB = smem + 2 * BM * 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const DgradClass cls = dgrad_class(p, blockIdx.y);
  const int ntaps = cls.nty * cls.ntx;
  const int ntn = (p.Cin + BN - 1) / BN;
  const int bid = cat::xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (bid / ntn) * BM, n0 = (bid % ntn) * BN;
  if (m0 >= cls.Mc) return;
  const int HcWc = cls.Hc * cls.Wc, taps = p.kh * p.kw;
  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.a), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(BT ? p.bt : p.b), 0, 0x7fffffff, 0x00020000);
  // A staging map as in conv_fwd32d_kernel; B: wave w, instruction i -> k-rows (w * 4 + i) * 2 + (lane >> 5), float4 column lane & 31
  // (BT: rows = input channels, staged exactly like A)
  const int slot = lane & 7, lrow = lane >> 3;
  int cy[4], cx[4];
  unsigned abase[4], aq[4], voffA[4], voffB[4];
  bool rv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (wave * 4 + i) * 8 + lrow;
    const int m = m0 + row;
    rv[i] = m < cls.Mc;
    const Pixel cp = decode_pixel(rv[i] ? m : 0, HcWc, cls.Wc);
    cy[i] = cls.cy0 + cp.y;
    cx[i] = cls.cx0 + cp.x;
    abase[i] = (unsigned)cp.n * (unsigned)(p.Ho * p.Wo) * (unsigned)p.ycs * 4u;
    aq[i] = (unsigned)(slot ^ ((row >> 1) & 7)) * 16u;
    if (BT) {
      const int cin = n0 + row;
      voffB[i] = cin < p.Cin ? (unsigned)cin * (unsigned)(taps * p.Cout) * 4u + aq[i] : 0x80000000u;
    } else {
      const int kr = (wave * 4 + i) * 2 + (lane >> 5);
      const int csrc = ((lane & 31) * 4) ^ (((kr >> 2) & 3) << 4);          // source column of this LDS position
      voffB[i] = n0 + csrc < p.Cin ? (unsigned)kr * (unsigned)(taps * p.wcs) * 4u + (unsigned)(n0 + csrc) * 4u : 0x80000000u;
    }
  }
  auto locate = [&](int jy, int jx) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int oy = cy[i] - jy, ox = cx[i] - jx;
      const bool v = rv[i] && (unsigned)oy < (unsigned)p.Ho && (unsigned)ox < (unsigned)p.Wo;
      voffA[i] = v ? abase[i] + (unsigned)(oy * p.Wo + ox) * (unsigned)p.ycs * 4u + aq[i] : 0x80000000u;
    }
  };
  int tj = 0, jy = 0, jx = 0, co = 0;       // walk state of the NEXT chunk to fetch (wave-uniform)
  locate(0, 0);
  auto issue = [&](int buf) {
    const unsigned soA = (unsigned)co * 4u;
    const unsigned tapi = (unsigned)((cls.py + jy * cls.s) * p.kw + cls.px + jx * cls.s);
    const unsigned soB = BT ? (tapi * (unsigned)p.Cout + (unsigned)co) * 4u : ((unsigned)co * (unsigned)taps + tapi) * (unsigned)p.wcs * 4u;
    dma_chunk(rA, rB, sA + buf * BM * 32, sB + buf * 32 * BN, wave, voffA, voffB, soA, soB);
    co += 32;
    if (co >= p.c4) {
      co = 0;
      ++tj;
      next_tap(jy, jx, cls.ntx);
      if (tj < ntaps) locate(jy, jx);
    }
  };
  const int lr = lane & 15, lq = lane >> 4;
  f4 acc[MT][NT];
  zero_acc(acc);
  auto mma = [&](int buf) {   // filters first: transposed accumulators, see the epilogue
    const float* A = sA + buf * BM * 32;
    const float* B = sB + buf * 32 * BN;
    if (BT) mma32_kcontig_a_kcontig_b<true>(A, B, wm * MT * 16, wn * NT * 16, lane, acc);
    else mma32_kcontig_a_ncontig_b<true, BN>(A, B, wm * MT * 16, wn * NT * 16, lane, acc);
  };
  const int nk = ntaps * (p.c4 >> 5);
  if (nk > 0) {
    issue(0);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    for (int kc = 0; kc + 1 < nk; ++kc) {
      const int buf = kc & 1;
      issue(buf ^ 1);
      mma(buf);
      __builtin_amdgcn_s_waitcnt(0);
      __syncthreads();
    }
    mma((nk - 1) & 1);
  }
  // transposed accumulators (filter fragment = the MFMA's first operand): one class pixel per lane and tile row (store_pixel_t)
  const bool vec = (p.ocs & 3) == 0 && (reinterpret_cast<uintptr_t>(p.out) & 15) == 0;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = m0 + wm * MT * 16 + i * 16 + lr;
    if (m >= cls.Mc) continue;
    store_pixel_t(p, p.out + dgrad_out_pixel(p, cls, m) * p.ocs, acc, i, n0 + wn * NT * 16 + lq * 4, p.Cin, vec);
  }
}

// ------------------------------------------------------------------------------------------------ wgrad
// rows = Cout (BM), cols = K = taps*cin4 (BN), reduction over the pixels [y*mchunk, (y+1)*mchunk).
// (A 32-pixel-chunk variant of the 128 x 128 tile was measured 1.5 - 7 % SLOWER on every wide layer: this kernel is bound by the
// per-pixel gather arithmetic on the vector ALU, which a deeper chunk does not reduce, not by barriers.)
template <int MT, int NT, int WM, int WN>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(IgemmArgs p) {
  constexpr int BM = WM * MT * 16, BN = WN * NT * 16, LDA = BM + 4, LDB = BN + 4;
  constexpr int AQ = BM / 4, BQ = BN / 4;
  constexpr int AI = (16 * AQ + 255) / 256, BI = (16 * BQ + 255) / 256;
  __shared__ __attribute__((aligned(16))) float smem[2 * 16 * (LDA + LDB)];
  float* sA = smem;
  float* sB = smem + 2 * 16 * LDA;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int ntn = (p.K + BN - 1) / BN;
  const int c0 = (blockIdx.x / ntn) * BM, k0 = (blockIdx.x % ntn) * BN;
  const int mbeg = blockIdx.y * p.mchunk;
  const int mend = min(p.M, mbeg + p.mchunk);
  const int HoWo = p.Ho * p.Wo;
  const int cout4 = (p.Cout + 3) & ~3;
  const int taps = p.kh * p.kw;

  // B' columns are fixed per thread: (tap, ci) of the im2col matrix
  int bky[BI], bkx[BI], bci[BI], bpix[BI], bnq[BI];
  bool bcv[BI];
#pragma unroll
  for (int i = 0; i < BI; ++i) {
    const int idx = tid + 256 * i;
    bpix[i] = idx / BQ;
    bnq[i] = idx - bpix[i] * BQ;
    const int k = k0 + bnq[i] * 4;
    bcv[i] = bpix[i] < 16 && k < p.K;
    const int tap = bcv[i] ? k / p.c4 : 0;
    bci[i] = bcv[i] ? k - tap * p.c4 : 0;
    bky[i] = tap / p.kw;
    bkx[i] = tap - bky[i] * p.kw;
  }
  int apix[AI], acq[AI];
  bool acv[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    const int idx = tid + 256 * i;
    apix[i] = idx / AQ;
    acq[i] = idx - apix[i] * AQ;
    acv[i] = apix[i] < 16 && c0 + acq[i] * 4 < cout4;
  }

  // (n, oy, ox) of the pixel each B' lane gathers; advanced by 16 pixels per chunk without divisions
  int pn[BI], poy[BI], pox[BI];
#pragma unroll
  for (int i = 0; i < BI; ++i) {
    const Pixel o = decode_pixel(min(mbeg + bpix[i], p.M - 1), HoWo, p.Wo);
    pn[i] = o.n;
    poy[i] = o.y;
    pox[i] = o.x;
  }
  // NB: gload must be called with kc = 0, 1, 2, ... exactly once each, in order
  const float* pa[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) pa[i] = p.b + (int64_t)(mbeg + apix[i]) * p.ycs + c0 + acq[i] * 4;
  f4 ra[AI], rb[BI];
  auto gload = [&](int kc) {
    const int mb = mbeg + kc * 16;
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      ra[i] = ldg4_or_zero(acv[i] && mb + apix[i] < mend, pa[i]);
      pa[i] += 16 * p.ycs;
    }
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      const int m = mb + bpix[i];
      bool v = bcv[i] && m < mend;
      const int n = pn[i], oy = poy[i], ox = pox[i];
      pox[i] += 16;
      while (pox[i] >= p.Wo) {
        pox[i] -= p.Wo;
        if (++poy[i] >= p.Ho) {
          poy[i] = 0;
          ++pn[i];
        }
      }
      int iy = oy * p.stride - p.pad + bky[i], ix = ox * p.stride - p.pad + bkx[i];
      {  // branch-free: reflect -> mirrored index, zero padding -> invalid lane (reads the zero page)
        const bool inr = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        const int ry = cat::reflect_idx(iy, p.H), rx = cat::reflect_idx(ix, p.W);
        iy = p.reflect ? ry : (inr ? iy : 0);
        ix = p.reflect ? rx : (inr ? ix : 0);
        v = v && (p.reflect || inr);
      }
      rb[i] = ldg4_or_zero(v, p.a + (unsigned)(((n * p.H + iy) * p.W + ix) * p.xcs + bci[i]));   // < 2^32 elements (checked on the host)
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < AI; ++i)
      if (apix[i] < 16) *reinterpret_cast<f4*>(sA + buf * 16 * LDA + apix[i] * LDA + acq[i] * 4) = ra[i];
#pragma unroll
    for (int i = 0; i < BI; ++i)
      if (bpix[i] < 16) *reinterpret_cast<f4*>(sB + buf * 16 * LDB + bpix[i] * LDB + bnq[i] * 4) = rb[i];
  };

  f4 acc[MT][NT];
  zero_acc(acc);

  const int lr = lane & 15, lq = lane >> 4;
  const int nk = mend > mbeg ? (mend - mbeg + 15) >> 4 : 0;
  if (nk > 0) {
    gload(0);
    sstore(0);
  }
  __syncthreads();
  for (int kc = 0; kc < nk; ++kc) {
    const int buf = kc & 1;
    if (kc + 1 < nk) gload(kc + 1);
    {
      const float* A = sA + buf * 16 * LDA;
      const float* B = sB + buf * 16 * LDB;
      float fa[MT][4], fb[NT][4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int i = 0; i < MT; ++i) fa[i][t] = A[(lq * 4 + t) * LDA + wm * MT * 16 + i * 16 + lr];
#pragma unroll
        for (int j = 0; j < NT; ++j) fb[j][t] = B[(lq * 4 + t) * LDB + wn * NT * 16 + j * 16 + lr];
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][t], fb[j][t], acc[i][j], 0, 0, 0);
    }
    if (kc + 1 < nk) sstore(buf ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int k = k0 + wn * NT * 16 + j * 16 + lr;
    if (k >= p.K) continue;
    const int tap = k / p.c4, ci = k - tap * p.c4;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int co = c0 + wm * MT * 16 + i * 16 + lq * 4 + rg;
        if (co < p.Cout) store_dw(p, co, k, tap, ci, taps, acc[i][j][rg]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ wgrad, 32-pixel chunks, direct-to-LDS
// dw[co][tap][ci] for the wide zero-padded layers (the PatchGAN's 4x4 convs, the teacher's stride-2 convs): 128 filters x 128 columns of
// ONE tap per workgroup (Cin % 128 == 0), reduction over output pixels in chunks of 32 CONSECUTIVE PIXELS OF ONE OUTPUT ROW.  With that
// chunk shape the source address of tile row r (pixel ox0 + r) is (row base) + (per-lane constant): the row base is an SGPR soffset,
// so -- unlike conv_wgrad_kernel, whose (n, oy, ox) walk per 16-pixel chunk is what bounds it -- the steady state has no vector-ALU
// address arithmetic; both tiles are DMA-ed into LDS (see conv_fwd32d_kernel).  Chunks whose input row falls into the zero padding are
// skipped.  Tiles are [32 pixels][128] with the 16-column groups XOR-ed by (pixel >> 2) & 3 (applied to the source column), read with
// ds_read_b32 like conv_wgrad_kernel.  blockIdx.y = slice of output rows; partial sums go to ws[slice][co][K] (or straight to dw).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv_wgrad32d_kernel(IgemmArgs p, int rows_per, int cpr) {
  constexpr int MT = 4, NT = 4, WN = 2, BM = 128, BN = 128;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sA = smem;                   // dy tile   [2][32][128]
  float* sB = smem + 2 * 32 * BM;     // x  tile   [2][32][128]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int ntn = p.K / BN;
  const int c0 = (blockIdx.x / ntn) * BM, k0 = (blockIdx.x % ntn) * BN;
  const int tap = k0 / p.c4, ci0 = k0 - tap * p.c4;
  const int ky = tap / p.kw, kx = tap - ky * p.kw;
  const int R = p.N * p.Ho;
  const int rbeg = blockIdx.y * rows_per, rend = min(R, rbeg + rows_per);
  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.b), 0, 0x7fffffff, 0x00020000);   // dy
  // x, with the base moved back by `pad` pixels: the scalar row offset below then never needs the (negative) "- pad" term, and the per-lane
  // part stays non-negative; nothing is read in front of the tensor (those lanes are parked out of range)
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.a) - (int64_t)p.pad * p.xcs, 0, 0x7fffffff, 0x00020000);
  // staging map: wave w, instruction i -> tile rows (w * 4 + i) * 2 + (lane >> 5), float4 column lane & 31
  int trow[4];
  unsigned colA[4], colB[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    trow[i] = (wave * 4 + i) * 2 + (lane >> 5);
    const int csrc = ((lane & 31) * 4) ^ (((trow[i] >> 2) & 3) << 4);
    colA[i] = c0 + csrc < ((p.Cout + 3) & ~3) ? (unsigned)(c0 + csrc) * 4u : 0x80000000u;
    colB[i] = (unsigned)(ci0 + csrc) * 4u;
  }
  unsigned voffA[4], voffB[4];
  auto locate = [&](int ox0) {        // per-lane offsets of one row segment (change only with the segment's start column)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ox = ox0 + trow[i];
      const int ix = ox * p.stride - p.pad + kx;
      const bool pv = ox < p.Wo;
      voffA[i] = (pv && colA[i] != 0x80000000u) ? (unsigned)trow[i] * (unsigned)p.ycs * 4u + colA[i] : 0x80000000u;
      voffB[i] = (pv && (unsigned)ix < (unsigned)p.W) ? (unsigned)(trow[i] * p.stride + kx) * (unsigned)p.xcs * 4u + colB[i] : 0x80000000u;
    }
  };
  // chunk cursor: (output row rr, segment sg); rows whose input row iy lies in the padding contribute nothing
  int rr = rbeg, sg = 0;
  auto valid_row = [&](int r) {
    const int oy = r % p.Ho;
    return (unsigned)(oy * p.stride - p.pad + ky) < (unsigned)p.H;
  };
  auto skip = [&]() {
    while (rr < rend && !valid_row(rr)) ++rr;
  };
  skip();
  int cur_sg = -1;
  auto issue = [&](int buf) {
    if (sg != cur_sg) {
      locate(sg * 32);
      cur_sg = sg;
    }
    const int n = rr / p.Ho, oy = rr - n * p.Ho;
    const int iy = oy * p.stride - p.pad + ky;
    const unsigned soA = (unsigned)((n * p.Ho + oy) * p.Wo + sg * 32) * (unsigned)p.ycs * 4u;
    const unsigned soB = (unsigned)((n * p.H + iy) * p.W + sg * 32 * p.stride) * (unsigned)p.xcs * 4u;      // "- pad" lives in rB's base
    dma_chunk(rA, rB, sA + buf * 32 * BM, sB + buf * 32 * BN, wave, voffA, voffB, soA, soB);
    if (++sg == cpr) {
      sg = 0;
      ++rr;
      skip();
    }
  };
  const int lr = lane & 15, lq = lane >> 4;
  f4 acc[MT][NT];
  zero_acc(acc);
  auto mma = [&](int buf) {
    const float* A = sA + buf * 32 * BM;
    const float* B = sB + buf * 32 * BN;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float fa[MT][4], fb[NT][4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int row = h * 16 + lq * 4 + t;
#pragma unroll
        for (int i = 0; i < MT; ++i) fa[i][t] = A[row * BM + ((wm * MT * 16 + i * 16 + lr) ^ (lq << 4))];
#pragma unroll
        for (int j = 0; j < NT; ++j) fb[j][t] = B[row * BN + ((wn * NT * 16 + j * 16 + lr) ^ (lq << 4))];
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][t], fb[j][t], acc[i][j], 0, 0, 0);
    }
  };
  if (rr < rend) {
    issue(0);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    int buf = 0;
    while (rr < rend) {
      issue(buf ^ 1);
      mma(buf);
      __builtin_amdgcn_s_waitcnt(0);
      __syncthreads();
      buf ^= 1;
    }
    mma(buf);
  }
  const int taps = p.kh * p.kw;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int k = k0 + wn * NT * 16 + j * 16 + lr;
    const int ci = k - tap * p.c4;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int co = c0 + wm * MT * 16 + i * 16 + lq * 4 + rg;
        if (co < p.Cout) store_dw(p, co, k, tap, ci, taps, acc[i][j][rg]);
      }
    }
  }
}

// wt[ci][tap][co] = w[co][tap][ci]: 32 x 32 tiles through LDS, one (tap, tile) per workgroup
__global__ __launch_bounds__(256) void weight_transpose_kernel(const float* __restrict__ w, float* __restrict__ wt, int Cout, int Cin, int taps,
                                                               int wcs) {
  __shared__ float tile[32][33];
  const int tap = blockIdx.z, co0 = blockIdx.y * 32, ci0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int co = co0 + r, ci = ci0 + tx;
    tile[r][tx] = (co < Cout && ci < Cin) ? w[((int64_t)co * taps + tap) * wcs + ci] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int ci = ci0 + r, co = co0 + tx;
    if (ci < Cin && co < Cout) wt[((int64_t)ci * taps + tap) * Cout + co] = tile[tx][r];
  }
}

struct RedItem {
  const float* ws;
  float* dw;
  int nsplit, Cout, taps, wlim, wcs, c4, K, accumulate;
};

// dw[co][tap][ci] (+)= sum_z ws[z][co][tap*c4 + ci].  Workgroup = 16 channel quads x 16 split lanes: every thread sums its slices' float4 in
// increasing z (fixed order), the 16 lanes of a quad are then combined pairwise through LDS -- deterministic, and 16-byte loads with 16
// slices in flight per output instead of 4-byte loads with 4.
// wlim = channels written per tap (Cin for dense storage, the padded extent otherwise), wcs = storage stride per tap
__device__ __forceinline__ void wgrad_reduce_body(const RedItem& r, int64_t blk, f4* red) {
  const int cq = r.c4 >> 2;
  const int64_t total = (int64_t)r.Cout * r.taps * cq;
  const int64_t e = blk * 16 + (threadIdx.x & 15);
  const int zl = threadIdx.x >> 4;
  f4 s = {0.f, 0.f, 0.f, 0.f};
  int q = 0, tap = 0, co = 0;
  if (e < total) {
    q = (int)(e % cq);
    const int64_t ct = e / cq;
    tap = (int)(ct % r.taps);
    co = (int)(ct / r.taps);
    const float* src = r.ws + (int64_t)co * r.K + tap * r.c4 + q * 4;
    const int64_t zs = (int64_t)r.Cout * r.K;
    int z = zl;
    for (; z + 48 < r.nsplit; z += 64) {
      const f4 v0 = *reinterpret_cast<const f4*>(src + z * zs), v1 = *reinterpret_cast<const f4*>(src + (z + 16) * zs);
      const f4 v2 = *reinterpret_cast<const f4*>(src + (z + 32) * zs), v3 = *reinterpret_cast<const f4*>(src + (z + 48) * zs);
      s += v0;
      s += v1;
      s += v2;
      s += v3;
    }
    for (; z < r.nsplit; z += 16) s += *reinterpret_cast<const f4*>(src + z * zs);
  }
  red[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int st = 8; st >= 1; st >>= 1) {
    if (zl < st) red[threadIdx.x] += red[threadIdx.x + st * 16];
    __syncthreads();
  }
  if (zl == 0 && e < total) {
    const f4 v = red[threadIdx.x];
    float* d = r.dw + ((int64_t)co * r.taps + tap) * r.wcs + q * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (q * 4 + c < r.wlim) d[c] = r.accumulate ? d[c] + v[c] : v[c];
  }
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, int nsplit,
                                                           int Cout, int taps, int wlim, int wcs, int c4, int K, int accumulate) {
  __shared__ f4 red[256];
  wgrad_reduce_body(RedItem{ws, dw, nsplit, Cout, taps, wlim, wcs, c4, K, accumulate}, blockIdx.x, red);
}

// The partial sums of SEVERAL weight gradients reduced by one launch (cat_conv2d_wgrad_batch: the narrow layers of a fused block -- seven
// 5 - 8 us reduce launches per block were launch latency, not data).  Same arithmetic per item as wgrad_reduce_kernel (same lane / slice
// order): blocks [start[i], start[i + 1]) serve item i.
struct RedMany {
  RedItem it[CAT_WGRAD_BATCH_MAX];
  int start[CAT_WGRAD_BATCH_MAX + 1];
  int n;
};

__global__ __launch_bounds__(256) void wgrad_reduce_many_kernel(const RedMany m) {
  __shared__ f4 red[256];
  int i = 0;
#pragma unroll
  for (int k = 1; k < CAT_WGRAD_BATCH_MAX; ++k)
    if (k < m.n && (int)blockIdx.x >= m.start[k]) i = k;
  wgrad_reduce_body(m.it[i], (int64_t)blockIdx.x - m.start[i], red);
}

// ------------------------------------------------------------------------------------------------ host side
// The tiles of the generic forward / dgrad kernels by GEMM width n (Cout / Cin): ROW(n <=, MT, MT when M is small, NT, WM, WN).
// ONE table for the dispatch, the profiler names, default_bm and split_plan, so a tile rule cannot change in one of them only.
// Small M = few output pixels (e.g. the student's 64x64 trunk at batch 16 = 256 tiles of 256 rows): halve the M tile so that every CU
// holds 2+ workgroups and the per-chunk load / LDS / barrier latencies of one overlap the MFMA stream of another.  Measured: that helps the
// 16- and 32-wide rows (256-row default) and not the 48..96-wide ones, so only those two rows have a second tile; in every other row both
// columns name the same tile and nothing more is compiled.
// (N = 130 .. 192 -- the frozen teacher's 176-wide fused GEMM, SPADE's 170-wide heads -- would fill two 96-wide tiles better than two
// 128-wide ones, 8 % instead of 31 % padding at 176; not taken: the 176-wide layer is the frozen teacher's merged 1 x 1, served by the
// direct-to-LDS 128 x 128 tile ahead of this dispatch.)
#define CONV_TILES(ROW, ...)         \
  ROW(16, 4, 2, 1, 4, 1, __VA_ARGS__) \
  ROW(32, 4, 2, 2, 4, 1, __VA_ARGS__) \
  ROW(48, 2, 2, 3, 4, 1, __VA_ARGS__) \
  ROW(64, 2, 2, 4, 4, 1, __VA_ARGS__) \
  ROW(96, 2, 2, 6, 4, 1, __VA_ARGS__) \
  ROW(INT_MAX, 4, 4, 4, 2, 2, __VA_ARGS__)
// ... and of conv_wgrad_kernel by Cout: ROW(Cout <=, MT, NT, WM, WN), for the launch, the profiler names and wgrad_split
#define WGRAD_TILES(ROW, ...)         \
  ROW(16, 1, 4, 1, 4, __VA_ARGS__)    \
  ROW(32, 2, 4, 1, 4, __VA_ARGS__)    \
  ROW(48, 3, 4, 1, 4, __VA_ARGS__)    \
  ROW(64, 4, 4, 1, 4, __VA_ARGS__)    \
  ROW(96, 6, 2, 1, 4, __VA_ARGS__)    \
  ROW(INT_MAX, 4, 4, 2, 2, __VA_ARGS__)

#define CONV_TILE_LAUNCH(NMAX, MT, MTS, NT, WM, WN, n, smallm, LAUNCH) \
  if ((n) <= NMAX) {                                                   \
    if (smallm) LAUNCH(MTS, NT, WM, WN) else LAUNCH(MT, NT, WM, WN)     \
  } else
#define DISPATCH_TILE_N(n, smallm, LAUNCH) CONV_TILES(CONV_TILE_LAUNCH, n, smallm, LAUNCH) {}

struct TileShape { int bm, bn; };
static TileShape conv_tile(int n, bool smallm) {
#define CONV_TILE_SHAPE(NMAX, MT, MTS, NT, WM, WN, ...) \
  if (n <= NMAX) return TileShape{WM * (smallm ? MTS : MT) * 16, WN * NT * 16};
  CONV_TILES(CONV_TILE_SHAPE, )
#undef CONV_TILE_SHAPE
  return TileShape{};
}
static TileShape wgrad_tile(int cout) {
#define WGRAD_TILE_SHAPE(NMAX, MT, NT, WM, WN, ...) \
  if (cout <= NMAX) return TileShape{WM * MT * 16, WN * NT * 16};
  WGRAD_TILES(WGRAD_TILE_SHAPE, )
#undef WGRAD_TILE_SHAPE
  return TileShape{};
}

// the profiler family of a launch through DISPATCH_TILE_N(n, smallm, ...) / WGRAD_TILES: the kernel's prefix + the tile's MT x NT x WM x WN
#define CONV_TILE_NAME(NMAX, MT, MTS, NT, WM, WN, n, smallm, PFX) \
  (n) <= NMAX ? ((smallm) ? PFX #MTS "x" #NT "x" #WM "x" #WN : PFX #MT "x" #NT "x" #WM "x" #WN) :
#define TILE_NAME(PFX, n, smallm) (CONV_TILES(CONV_TILE_NAME, n, smallm, PFX) "")
#define WGRAD_TILE_NAME(NMAX, MT, NT, WM, WN, cout) (cout) <= NMAX ? "conv_wgrad_" #MT "x" #NT "x" #WM "x" #WN :

// out[pix][c] = act(sum_z part[z][pix][c] + bias[c]) for c < C; zeros for C <= c < cw
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                            float* __restrict__ out, int64_t P, int C, int cw, int cs, int ksplit, int act,
                                                            float slope) {
  const int nq = (cw + 3) >> 2;
  const int64_t total = P * nq;
  const int64_t zstride = P * cs;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % nq) * 4;
    const int64_t off = (i / nq) * cs + c;
    f4 s = {0.f, 0.f, 0.f, 0.f};
    if (c < C)
      for (int z = 0; z < ksplit; ++z) s += *reinterpret_cast<const f4*>(part + z * zstride + off);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (c + e < C) out[off + e] = cat::apply_act(s[e] + (bias ? bias[c + e] : 0.f), act, slope);
      else if (c + e < cw) out[off + e] = 0.f;
    }
  }
}

static int default_bm(int n) { return conv_tile(n, false).bm; }
// take the small-M column of CONV_TILES?  (Which rows have a tile of their own there is the table's business.)
static bool use_small_m(int M, int n) { return cdiv(M, default_bm(n)) < 768; }

// Split-K plan: when the (M, N) tile grid of the kernel the dispatcher would pick is far below the 256 CUs (the 4x8 .. 32x64
// pixel layers of the SPADE generators: M = 128 .. 8192 pixels against K = 25 * 1024), K is cut into slices of >= 4 chunks.
struct SplitPlan { int ksplit, kchunks; };
static SplitPlan split_plan(int M, int n, int nk) {
  SplitPlan p{1, nk};
  const TileShape t = conv_tile(n, use_small_m(M, n));
  const int tiles = cdiv(M, t.bm) * cdiv(n, t.bn);
  if (tiles >= 128 || nk < 16) return p;
  int ks = cdiv(512, tiles);
  if (ks > nk / 4) ks = nk / 4;
  if (ks < 2) return p;
  p.kchunks = cdiv(nk, ks);
  p.ksplit = cdiv(nk, p.kchunks);
  if (p.ksplit < 2) p = SplitPlan{1, nk};
  return p;
}

static void launch_splitk_reduce(const float* part, const float* bias, float* out, int64_t P, int C, int cw, int cs, int ksplit, int act,
                                 float slope, hipStream_t s) {
  splitk_reduce_kernel<<<cat::ew_grid(P * ((cw + 3) / 4), 4096), 256, 0, s>>>(part, bias, out, P, C, cw, cs, ksplit, act, slope);
}

// The tile kernels zero the lanes [C, cw) that fall inside their own column tiles, which always covers [C, round_up(C, 4)) -- every in-tree
// caller's cw.  A wider cw (the C-ABI allows any cw <= the pixel stride) can reach past the last tile: those quads are zeroed here.
__global__ __launch_bounds__(256) void zero_lanes_kernel(float* __restrict__ out, int64_t P, int cs, int c_lo, int cw) {
  const int nq = (cw - c_lo + 3) >> 2;
  const int64_t total = P * nq;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = c_lo + (int)(i % nq) * 4;
    float* o = out + (i / nq) * cs;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c + e < cw) o[c + e] = 0.f;
  }
}

static void zero_lanes_past_c4(float* out, int64_t P, int C, int cw, int cs, hipStream_t s) {
  const int c4 = (C + 3) & ~3;
  if (cw <= c4) return;
  zero_lanes_kernel<<<cat::ew_grid(P * ((cw - c4 + 3) / 4), 4096), 256, 0, s>>>(out, P, cs, c4, cw);
}

// dynamic LDS of the double-buffered 128 x 128 x 32 tiles
constexpr size_t kLds128 = (size_t)2 * (128 + 128) * 32 * sizeof(float);
// the direct-to-LDS kernels address a tensor with 32-bit byte offsets
static bool fits_2gb(int64_t floats) { return floats * 4 < (int64_t)2147483647; }

// weight floats per (cout, tap): 0 in the geometry = dense
static int weight_cs(const cat_conv_t* g) { return g->wcs > 0 ? g->wcs : g->Cin; }

// 2 x the layer's multiply-adds: what every pass (forward, input gradient, weight gradient) reports to the profiler
static double conv_flops(const cat_conv_t* g) { return 2.0 * (double)g->N * g->Ho * g->Wo * g->Cout * g->kh * g->kw * g->Cin; }

int fill_common(IgemmArgs& a, const cat_conv_t* g, int pad_w = -1, int dil = 1) {
  const int padw = pad_w >= 0 ? pad_w : g->pad;
  CAT_REQUIRE(g->N > 0 && g->H > 0 && g->W > 0 && g->Cin > 0 && g->Cout > 0, "conv: empty geometry");
  CAT_REQUIRE(g->stride == 1 || g->stride == 2, "conv: stride %d unsupported", g->stride);
  CAT_REQUIRE(g->xcs % 4 == 0 && g->ycs % 4 == 0, "conv: pixel strides must be multiples of 4 (xcs=%d ycs=%d)", g->xcs, g->ycs);
  CAT_REQUIRE(g->xcs >= ((g->Cin + 3) & ~3) && g->ycs >= ((g->Cout + 3) & ~3), "conv: pixel stride smaller than padded channel count");
  const int eh = dil * (g->kh - 1) + 1, ew = dil * (g->kw - 1) + 1;   // filter extent (== kh, kw without dilation)
  CAT_REQUIRE(g->Ho == (g->H + 2 * g->pad - eh) / g->stride + 1 && g->Wo == (g->W + 2 * padw - ew) / g->stride + 1,
              "conv: output size (%d,%d) inconsistent with geometry", g->Ho, g->Wo);
  CAT_REQUIRE(g->pad_mode == CAT_PAD_ZERO || (g->pad < g->H && padw < g->W), "conv: reflect pad must be < input size");
  a.N = g->N; a.H = g->H; a.W = g->W; a.Cin = g->Cin; a.xcs = g->xcs;
  a.Ho = g->Ho; a.Wo = g->Wo; a.Cout = g->Cout; a.ycs = g->ycs;
  a.kh = g->kh; a.kw = g->kw; a.stride = g->stride; a.pad = g->pad; a.padw = padw; a.reflect = g->pad_mode == CAT_PAD_REFLECT;
  a.act = g->act; a.slope = g->slope;
  a.wcs = weight_cs(g);
  CAT_REQUIRE(a.wcs >= g->Cin, "conv: wcs < Cin");
  a.wvec = (a.wcs % 4) == 0;
  a.M = g->N * g->Ho * g->Wo;
  a.dil = dil;
  return 0;
}

// per-tap K extent of the fwd / dgrad walk: rounding the channel count up to 16 keeps every 16-wide chunk inside one tap (uniform,
// division-free walk) at the price of zero-filled MFMA work -- taken when that padding is <= 12.5 %
int walk_extent(int c4) {
  const int c16 = (c4 + 15) & ~15;
  return (c16 - c4) * 8 <= c16 ? c16 : c4;
}

// pixel split of conv_wgrad_kernel: nsplit slices of mchunk pixels, partial sums per slice
struct WgradSplit { int nsplit, mchunk; };
WgradSplit wgrad_split(const cat_conv_t* g) {
  const int Cout = g->Cout, K = g->kh * g->kw * ((g->Cin + 3) & ~3);
  const TileShape t = wgrad_tile(Cout);
  const int tiles = cdiv(Cout, t.bm) * cdiv(K, t.bn);
  const int M = g->N * g->Ho * g->Wo;
  // tuning knobs, read per call: the workgroups the pixel split aims for, the fewest pixels per slice, the most slices
  const auto knob = [](const char* name, int least, int dflt) { const char* v = getenv(name); return v && atoi(v) >= least ? atoi(v) : dflt; };
  int ns = cdiv(knob("CAT_WGRAD_BLOCKS", 1, 1024), tiles);
  const int minchunk = knob("CAT_WGRAD_MINCHUNK", 16, 256), maxsplit = knob("CAT_WGRAD_MAXSPLIT", 1, 256);
  int maxs = M / minchunk > 0 ? M / minchunk : 1;
  if (maxs > maxsplit) maxs = maxsplit;
  if (ns > maxs) ns = maxs;
  if (ns < 1) ns = 1;
  WgradSplit sp;
  sp.mchunk = cat::round_up(cdiv(M, ns), 16);
  sp.nsplit = cdiv(M, sp.mchunk);
  return sp;
}

// CAT_SCHED scheduling experiments of the 128 x 128 tile: instantiated by the diagnostic build only
template <bool DIAG>
void launch_fwd_sched(int sched, int grid, const IgemmArgs& a, hipStream_t s) {
  if constexpr (DIAG) {
    if (sched == 1) conv_fwd_kernel<4, 4, 2, 2, true, 1><<<grid, 256, 0, s>>>(a);
    else conv_fwd_kernel<4, 4, 2, 2, true, 2><<<grid, 256, 0, s>>>(a);
  }
}

// a kernel that needs more than 64 KB of dynamic LDS: opted in once per instantiation and device, then launched
template <auto KERNEL, class... Extra>
static void launch_big_lds(dim3 grid, size_t lds, hipStream_t s, const IgemmArgs& a, Extra... extra) {
  static cat::LdsOptIn optin;
  cat::lds_optin(optin, (const void*)KERNEL, (int)lds);
  KERNEL<<<grid, 256, lds, s>>>(a, extra...);
}

// ---- One plan per pass.  plan_fwd / plan_dgrad / plan_wgrad map a geometry and what the caller supplies to the kernel family, its tile and
// split, the derived extents, the workspace bytes and the profiler family.  The workspace queries, cat_conv2d_dgrad_t_applicable and the
// launches below all read the SAME plan, so a workspace cannot be sized for one kernel while another launches into it.  The applicability
// predicates, the tile rules and the A/B switches (CAT_FWD_DIRECT, CAT_DGRAD_DIRECT, CAT_DGRAD_T, CAT_WGRAD_DIRECT, CAT_WGRAD_*) are
// consulted by the plans only.  Plain struct, no allocation: the eager SPADE step is bound by host issue time.
// Small: conv_smallco.hip (Cout <= 3, dgrad Cin <= 6); Direct32: the direct-to-LDS 128 x 128 tiles conv_{fwd,dgrad,wgrad}32d_kernel;
// Tile32: conv_fwd32_kernel over CONV_TILES / conv_dgrad32_kernel; Tile16: conv_{fwd,dgrad}_kernel over CONV_TILES / conv_wgrad_kernel over
// WGRAD_TILES; LdsTile: conv_twgrad.hip; PixelStream: conv_pwgrad.hip
enum class Kernel { Small, Direct32, Tile32, Tile16, LdsTile, PixelStream };
struct ConvPlan {
  Kernel kernel;
  const char* name;   // profiler family
  int split;          // slices reduced from the workspace (1 = none): fwd / dgrad of K, wgrad of the pixels (Direct32: of the output rows)
  int chunk;          // length of a slice: fwd / dgrad K chunks, wgrad Tile16 pixels, wgrad Direct32 output rows
  bool smallm;        // fwd / dgrad over CONV_TILES: the small-M column of the row
  bool direct;        // wgrad: the kernel writes dw itself (the one slice of Direct32 / Tile16) -- no workspace, no reduce
  bool t_ok;          // dgrad Direct32: the transposed-filter variant is on offer (cat_conv2d_dgrad_t)
  int cval, c4, K;    // IgemmArgs' channel and K extents
  int Hin, Win, pad_eff, mmax;   // dgrad: the plane written (reflect: the padded one, pad_eff = 0), pixels of the largest stride-parity class
  size_t ws_bytes;
};
static ConvPlan pick(ConvPlan p, Kernel kernel, const char* name, int split = 1, int chunk = 0) {
  p.kernel = kernel; p.name = name; p.split = split; p.chunk = chunk;
  return p;
}

// BK = 32 forward kernels: per-tap K extent a multiple of 16 (walk_extent allows <= 12.5 % zero padding), float4-readable filter rows
static bool fwd_bk32_ok(const cat_conv_t* g, int c4) {
  static const bool dbg_on = cat::kDiag && getenv("CAT_DBG");   // the per-phase clocks are in conv_fwd_kernel
  return (weight_cs(g) % 4) == 0 && (c4 & 15) == 0 && !dbg_on;
}

// has_ws: the caller passes a workspace (only then may K be split); plain: cat_conv2d_fwd / _ws, not the rect or ex entry points
static ConvPlan plan_fwd(const cat_conv_t* g, bool has_ws, bool plain) {
  ConvPlan p{};
  const int M = g->N * g->Ho * g->Wo, n = g->Cout;
  p.cval = (g->Cin + 3) & ~3;
  p.c4 = walk_extent(p.cval);
  p.K = g->kh * g->kw * p.c4;
  static const int fwd_direct = getenv("CAT_FWD_DIRECT") ? atoi(getenv("CAT_FWD_DIRECT")) : 1;
  if (plain && cat::smallco_applicable(g)) {
    p = pick(p, Kernel::Small, "conv_fwd_smallco", has_ws ? cat::smallco_fwd_ksplit(g) : 1);
  } else {
    const bool bk32 = fwd_bk32_ok(g, p.c4);
    const SplitPlan sp = bk32 && has_ws ? split_plan(M, n, (p.K + 31) >> 5) : SplitPlan{1, 0};
    p.smallm = use_small_m(M, n);
    // direct-to-LDS variant of the 128 x 128 tile: Cin % 32 == 0 (a chunk never straddles taps), no K split, 32-bit byte offsets
    if (fwd_direct && bk32 && sp.ksplit == 1 && n > 96 && (g->Cin & 31) == 0 && p.c4 == g->Cin && weight_cs(g) >= g->Cin &&
        fits_2gb((int64_t)g->N * g->H * g->W * g->xcs) && fits_2gb((int64_t)n * g->kh * g->kw * weight_cs(g)))
      p = pick(p, Kernel::Direct32, "conv_fwd32d_4x4x2x2");
    else if (bk32)
      p = pick(p, Kernel::Tile32, sp.ksplit > 1 ? TILE_NAME("conv_fwd32sk_", n, p.smallm) : TILE_NAME("conv_fwd32_", n, p.smallm), sp.ksplit, sp.kchunks);
    else
      p = pick(p, Kernel::Tile16, TILE_NAME("conv_fwd_", n, p.smallm));
  }
  p.ws_bytes = p.split > 1 ? (size_t)p.split * M * g->ycs * sizeof(float) : 0;
  return p;
}

// does the direct-to-LDS dgrad tile apply (and with it the transposed-filter variant)?
static bool dgrad32d_ok(const cat_conv_t* g) {
  static const int on = getenv("CAT_DGRAD_DIRECT") ? atoi(getenv("CAT_DGRAD_DIRECT")) : 1;
  const int wcs = weight_cs(g);
  return on && g->Cin > 96 && (wcs & 3) == 0 && g->Cout % 32 == 0 && g->Cin % 4 == 0 &&
         fits_2gb((int64_t)g->N * g->Ho * g->Wo * g->ycs) && fits_2gb((int64_t)g->Cout * g->kh * g->kw * wcs);
}

// has_ws: the caller passes a workspace of dxcs floats per pixel and slice (only then may K be split); has_wt: it passes the transposed
// filter; has_bias: it passes a bias (with g->act the fused epilogue, which the Cin <= 6 kernel does not have)
static ConvPlan plan_dgrad(const cat_conv_t* g, int dxcs, bool has_ws, bool has_wt, bool has_bias) {
  ConvPlan p{};
  const bool refl = g->pad_mode == CAT_PAD_REFLECT;
  const int st = g->stride < 1 ? 1 : g->stride, n = g->Cin;   // (the two queries do not validate the geometry)
  p.Hin = refl ? g->H + 2 * g->pad : g->H;
  p.Win = refl ? g->W + 2 * g->pad : g->W;
  p.pad_eff = refl ? 0 : g->pad;
  p.mmax = g->N * cdiv(p.Hin, st) * cdiv(p.Win, st);
  p.cval = (g->Cout + 3) & ~3;
  p.c4 = walk_extent(p.cval);
  static const int t_on = getenv("CAT_DGRAD_T") ? atoi(getenv("CAT_DGRAD_T")) : 1;
  // K is split at stride 1 only: one parity class, mmax = every pixel of the plane
  const SplitPlan sp = has_ws && st == 1 && g->N > 0 ? split_plan(p.mmax, n, (g->kh * g->kw * p.c4 + 15) >> 4) : SplitPlan{1, 0};
  p.smallm = use_small_m(p.mmax, n);
  if (sp.ksplit > 1)
    p = pick(p, Kernel::Tile16, TILE_NAME("conv_dgradsk_", n, p.smallm), sp.ksplit, sp.kchunks);
  else if (!has_bias && g->act == CAT_ACT_NONE && cat::smallci_dgrad_applicable(g))
    p = pick(p, Kernel::Small, "conv_dgrad_smallci");
  else if (dgrad32d_ok(g) && p.c4 == g->Cout)   // BK = 32, direct to LDS (the discriminator's and the teacher's wide layers)
    p = pick(p, Kernel::Direct32, has_wt ? "conv_dgrad32dt_4x4x2x2" : "conv_dgrad32d_4x4x2x2");
  else if (n > 96 && (weight_cs(g) % 4) == 0 && g->Cout % 16 == 0 && n % 4 == 0)
    p = pick(p, Kernel::Tile32, "conv_dgrad32_4x4x2x2");
  else
    p = pick(p, Kernel::Tile16, TILE_NAME("conv_dgrad_", n, p.smallm));
  p.t_ok = t_on && p.kernel == Kernel::Direct32;
  p.ws_bytes = p.split > 1 ? (size_t)p.split * g->N * p.Hin * p.Win * dxcs * sizeof(float) : 0;
  return p;
}

// direct-to-LDS wgrad (conv_wgrad32d_kernel): wide zero-padded layers whose 128-column K blocks lie inside one tap; returns the number
// of output-row slices (0 = not applicable)
static int wgrad32d_nsplit(const cat_conv_t* g, int* rows_per) {
  static const int on = getenv("CAT_WGRAD_DIRECT") ? atoi(getenv("CAT_WGRAD_DIRECT")) : 1;
  // (output rows that end in a partial 32-pixel segment are served: the segment's tail lanes are parked out of range)
  if (!on || g->Cout <= 96 || (g->Cin & 127) || g->pad_mode != CAT_PAD_ZERO || !fits_2gb((int64_t)g->N * g->H * g->W * g->xcs) ||
      !fits_2gb((int64_t)g->N * g->Ho * g->Wo * g->ycs) || weight_cs(g) < g->Cin)
    return 0;
  const int tiles = cdiv(g->Cout, 128) * (g->kh * g->kw * g->Cin / 128);
  const int R = g->N * g->Ho;
  // workgroups aimed at: ONE resident round (256 CUs x 2).  Round 6, conv_bench on the three PatchGAN layers: 512 -> 2067 / 555 / 554 us, 1024 (two
  // rounds, twice the partial-sum traffic) 2155 / 562 / 563, 768 / 1536 / 2048 slower still; with 512 tiles (conv4) the launch writes dw directly
  int ns = cdiv(512, tiles);
  if (ns > R) ns = R;
  if (ns < 1) ns = 1;
  *rows_per = cdiv(R, ns);
  return cdiv(R, *rows_per);
}

// The order of the weight-gradient paths is written here and nowhere else.  Two predicates lean on it: the wide direct tile does not ask
// again whether the Cout <= 3 kernels apply (they come first), and pwgrad_applicable (conv_pwgrad.hip) keeps its own copy of the wide direct
// tile's "Cout > 96 && Cin % 128 == 0", so that under CAT_WGRAD_DIRECT=0 those layers fall to the generic tile and not to it.
static ConvPlan plan_wgrad(const cat_conv_t* g) {
  ConvPlan p{};
  p.c4 = (g->Cin + 3) & ~3;
  p.K = g->kh * g->kw * p.c4;
  int rows_per = 0;
  if (cat::smallco_applicable(g)) {
    p = pick(p, Kernel::Small, "conv_wgrad_smallco", cat::smallco_wgrad_nblk(g));
  } else if (cat::twgrad_applicable(g)) {
    p = pick(p, Kernel::LdsTile, "conv_twgrad", cat::twgrad_nblk(g));
  } else if (cat::pwgrad_applicable(g)) {
    p = pick(p, Kernel::PixelStream, "conv_pwgrad", cat::pwgrad_nblk(g));
  } else if (const int nsd = wgrad32d_nsplit(g, &rows_per)) {
    p = pick(p, Kernel::Direct32, "conv_wgrad32d_4x4x2x2", nsd, rows_per);
  } else {
    const WgradSplit sp = wgrad_split(g);
    p = pick(p, Kernel::Tile16, WGRAD_TILES(WGRAD_TILE_NAME, g->Cout) "", sp.nsplit, sp.mchunk);
  }
  p.direct = p.split == 1 && (p.kernel == Kernel::Direct32 || p.kernel == Kernel::Tile16);
  p.ws_bytes = (size_t)p.split * g->Cout * p.K * sizeof(float);
  return p;
}

}  // namespace

extern "C" {

size_t cat_conv2d_fwd_ws_bytes(const cat_conv_t* g) {
  IgemmArgs a{};
  if (fill_common(a, g)) return 0;
  return plan_fwd(g, true, true).ws_bytes;
}

struct FwdEx { int dil; const float* res; int rcs; };   // cat_conv2d_fwd_ex: dilation + residual epilogue (the EX kernel instantiations)
static int conv_fwd_impl(const cat_conv_t* g, const float* x, const float* w, const float* bias, float* y, void* ws, cat_stream_t stream,
                         int pad_w = -1, const FwdEx* ex = nullptr) {
  IgemmArgs a{};
  if (int e = fill_common(a, g, pad_w, ex ? ex->dil : 1)) return e;
  const bool rect = pad_w >= 0 && pad_w != g->pad;
  const ConvPlan pl = plan_fwd(g, ws != nullptr, !rect && !ex);
  a.cval = pl.cval; a.c4 = pl.c4; a.K = pl.K;
  a.ksplit = pl.split; a.kchunks = pl.chunk; a.part = (float*)ws;
  if (ex) { a.res = ex->res; a.rcs = ex->rcs; }
  a.a = x; a.b = w; a.bias = bias; a.out = y;
  a.cw = g->ycw > g->Cout ? g->ycw : g->Cout;
  CAT_REQUIRE(a.cw <= g->ycs, "conv fwd: ycw > ycs");
  hipStream_t s = (hipStream_t)stream;
  zero_lanes_past_c4(y, a.M, a.Cout, a.cw, a.ycs, s);
  // diagnostic build only (common.h kDiag): scheduling experiments, an LDS pad that caps workgroups per CU, per-phase shader clocks
  static const int sched = (cat::kDiag && getenv("CAT_SCHED")) ? atoi(getenv("CAT_SCHED")) : 0;
  static const int lds_pad = (cat::kDiag && getenv("CAT_LDS_PAD")) ? atoi(getenv("CAT_LDS_PAD")) : 0;
  static const bool dbg_on = cat::kDiag && getenv("CAT_DBG");
  static long long* dbg_buf = nullptr;
  if (dbg_on && pl.kernel == Kernel::Tile16) {
    if (!dbg_buf) (void)hipMalloc(&dbg_buf, 64);
    (void)hipMemsetAsync(dbg_buf, 0, 64, s);
    a.dbg = dbg_buf;
  }
#define LAUNCH(MT, NT, WM, WN)                                                             \
  {                                                                                        \
    const int grid = cdiv(a.M, WM * MT * 16) * cdiv(a.Cout, WN * NT * 16);                 \
    /* the EX launches take neither the CAT_SCHED variants nor the CAT_LDS_PAD occupancy cap: those diagnostics cover the plain kernels only */ \
    if (ex && !a.wvec) conv_fwd_kernel<MT, NT, WM, WN, false, 0, true><<<grid, 256, 0, s>>>(a); \
    else if (ex) conv_fwd_kernel<MT, NT, WM, WN, true, 0, true><<<grid, 256, 0, s>>>(a);    \
    else if (!a.wvec) conv_fwd_kernel<MT, NT, WM, WN, false, 0><<<grid, 256, 0, s>>>(a);    \
    else if (WN == 2 && sched) launch_fwd_sched<cat::kDiag>(sched, grid, a, s);             \
    else conv_fwd_kernel<MT, NT, WM, WN, true, 0><<<grid, 256, lds_pad, s>>>(a);            \
  }
#define LAUNCH32(MT, NT, WM, WN)                                                                      \
  {                                                                                                   \
    const dim3 grid(cdiv(a.M, WM * MT * 16) * cdiv(a.Cout, WN * NT * 16), pl.split);                   \
    const size_t lds = (size_t)2 * (WM * MT * 16 + WN * NT * 16) * 32 * sizeof(float);                \
    if (ex) launch_big_lds<conv_fwd32_kernel<MT, NT, WM, WN, true>>(grid, lds, s, a);                  \
    else launch_big_lds<conv_fwd32_kernel<MT, NT, WM, WN>>(grid, lds, s, a);                           \
  }
  {
    cat::ProfScope prof(pl.name, conv_flops(g), 0.0, stream);
    const int grid128 = cdiv(a.M, 128) * cdiv(a.Cout, 128);
    switch (pl.kernel) {
      case Kernel::Small:
        if (int e = cat::smallco_fwd(g, x, w, bias, y, (float*)ws, pl.split, s)) return e;
        break;
      case Kernel::Direct32:
        if (ex) launch_big_lds<conv_fwd32d_kernel<true>>(grid128, kLds128, s, a);
        else launch_big_lds<conv_fwd32d_kernel<false>>(grid128, kLds128, s, a);
        break;
      case Kernel::Tile32: DISPATCH_TILE_N(a.Cout, pl.smallm, LAUNCH32) break;
      default: DISPATCH_TILE_N(a.Cout, pl.smallm, LAUNCH) break;
    }
    if (pl.split > 1) launch_splitk_reduce((const float*)ws, bias, y, a.M, a.Cout, a.cw, a.ycs, pl.split, a.act, a.slope, s);
  }
#undef LAUNCH32
#undef LAUNCH
  if (a.dbg) {
    long long h[8];
    (void)hipMemcpyAsync(h, dbg_buf, 64, hipMemcpyDeviceToHost, s);
    (void)hipStreamSynchronize(s);
    fprintf(stderr, "[cat dbg raw] %lld %lld %lld %lld %lld err=%s\n", h[0], h[1], h[2], h[3], h[4], hipGetErrorString(hipGetLastError()));
    if (h[4] > 0)
      fprintf(stderr, "[cat dbg] chunks=%lld  per chunk: gload %lld  ds_read+mfma %lld  wait+ds_write %lld  barrier %lld  (shader clocks)\n", h[4],
              h[0] / h[4], h[1] / h[4], h[2] / h[4], h[3] / h[4]);
  }
  return cat::check_launch("conv2d_fwd");
}

int cat_conv2d_fwd(const cat_conv_t* g, const float* x, const float* w, const float* bias, float* y, cat_stream_t stream) {
  return conv_fwd_impl(g, x, w, bias, y, nullptr, stream);
}

int cat_conv2d_fwd_ws(const cat_conv_t* g, const float* x, const float* w, const float* bias, float* y, void* ws, cat_stream_t stream) {
  return conv_fwd_impl(g, x, w, bias, y, ws, stream);
}

// Forward convolution with DIFFERENT implicit zero padding along H (g->pad) and W (pad_w): the 1 x 7 / 7 x 1 / 1 x 3 / 3 x 1 factorised
// filters of the FID InceptionV3 (metric/inception.py:177-268 over torchvision's InceptionC / D / E).  Same kernels as cat_conv2d_fwd: the
// im2col gather takes the column offset from pad_w.  Forward only (the metric network is never differentiated).
int cat_conv2d_fwd_rect(const cat_conv_t* g, int pad_w, const float* x, const float* w, const float* bias, float* y, cat_stream_t stream) {
  CAT_REQUIRE(pad_w >= 0 && g->pad_mode == CAT_PAD_ZERO, "conv fwd rect: zero padding only");
  return conv_fwd_impl(g, x, w, bias, y, nullptr, stream, pad_w);
}

// y = act(conv_dilated(x, w) + bias + res): the layers of the dilated residual network behind the cityscapes mIoU (metric/drn.py:78-125,
// 163-202) -- 3 x 3 filters with taps 2 / 4 pixels apart, and the last 1 x 1 of a bottleneck, whose shortcut is added BEFORE the ReLU
// (:116-123).  The tap geometry is computed once per tap in the kernels' locate(), so dilation costs nothing per MFMA.  Zero padding,
// forward / inference only.  dilation == 1 && res == NULL is cat_conv2d_fwd itself (same dispatch, same bits).
int cat_conv2d_fwd_ex(const cat_conv_t* g, int dilation, const float* x, const float* w, const float* bias, const float* res, int rcs,
                      float* y, cat_stream_t stream) {
  CAT_REQUIRE(dilation >= 1 && dilation <= 64, "conv fwd ex: dilation %d", dilation);
  CAT_REQUIRE(g->pad_mode == CAT_PAD_ZERO, "conv fwd ex: zero padding only");
  CAT_REQUIRE(dilation == 1 || g->stride == 1, "conv fwd ex: dilation > 1 needs stride 1");
  CAT_REQUIRE(!res || rcs >= g->Cout, "conv fwd ex: residual pixel stride %d < Cout", rcs);
  if (dilation == 1 && !res) return conv_fwd_impl(g, x, w, bias, y, nullptr, stream);
  const FwdEx ex{dilation, res, rcs};
  return conv_fwd_impl(g, x, w, bias, y, nullptr, stream, -1, &ex);
}

size_t cat_conv2d_dgrad_ws_bytes(const cat_conv_t* g, int dxcs) { return plan_dgrad(g, dxcs, true, false, false).ws_bytes; }

// the transposed-filter tile is offered where a caller holding a workspace would still get the direct-to-LDS tile (no K split)
int cat_conv2d_dgrad_t_applicable(const cat_conv_t* g) { return plan_dgrad(g, 0, true, true, false).t_ok ? 1 : 0; }

int cat_conv2d_weight_transpose(const cat_conv_t* g, const float* w, float* wt, cat_stream_t stream) {
  const int wcs = weight_cs(g);
  CAT_REQUIRE(g->Cin > 0 && g->Cout > 0 && wcs >= g->Cin, "weight transpose: bad geometry");
  const dim3 grid(cdiv(g->Cin, 32), cdiv(g->Cout, 32), g->kh * g->kw);
  weight_transpose_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(w, wt, g->Cout, g->Cin, g->kh * g->kw, wcs);
  return cat::check_launch("weight_transpose");
}

static int conv_dgrad_impl(const cat_conv_t* g, const float* dy, const float* w, const float* wt, const float* bias, float* dx, int dxcs, int dxcw,
                           void* ws, cat_stream_t stream) {
  IgemmArgs a{};
  if (int e = fill_common(a, g)) return e;
  const ConvPlan pl = plan_dgrad(g, dxcs, ws != nullptr, wt != nullptr, bias != nullptr);
  a.a = dy; a.b = w; a.bt = wt; a.bias = bias; a.out = dx;
  a.cval = pl.cval; a.c4 = pl.c4;
  a.Hin = pl.Hin; a.Win = pl.Win; a.pad_eff = pl.pad_eff;
  a.ksplit = pl.split; a.kchunks = pl.chunk; a.part = (float*)ws;
  a.cw = dxcw > g->Cin ? dxcw : g->Cin;
  a.ocs = dxcs;
  CAT_REQUIRE(dxcs >= a.cw, "conv dgrad: dxcw > dxcs");
  const int st = g->stride;
  const int64_t P = (int64_t)g->N * pl.Hin * pl.Win;
  hipStream_t s = (hipStream_t)stream;
  zero_lanes_past_c4(dx, P, a.Cin, a.cw, a.ocs, s);
  cat::ProfScope prof(pl.name, conv_flops(g), 0.0, stream);
  const dim3 grid128(cdiv(pl.mmax, 128) * cdiv(a.Cin, 128), st * st);
#define LAUNCH(MT, NT, WM, WN)                                                               \
  {                                                                                          \
    dim3 grid(cdiv(pl.mmax, WM * MT * 16) * cdiv(a.Cin, WN * NT * 16), st * st, pl.split);   \
    conv_dgrad_kernel<MT, NT, WM, WN><<<grid, 256, 0, s>>>(a);                                \
  }
  switch (pl.kernel) {
    case Kernel::Small: return cat::smallci_dgrad(g, dy, w, dx, dxcs, a.cw, s);
    case Kernel::Direct32:
      if (wt) launch_big_lds<conv_dgrad32d_kernel<true>>(grid128, kLds128, s, a);
      else launch_big_lds<conv_dgrad32d_kernel<false>>(grid128, kLds128, s, a);
      break;
    case Kernel::Tile32: launch_big_lds<conv_dgrad32_kernel<4, 4, 2, 2>>(grid128, kLds128, s, a); break;
    default: DISPATCH_TILE_N(a.Cin, pl.smallm, LAUNCH) break;
  }
#undef LAUNCH
  if (pl.split > 1) launch_splitk_reduce((const float*)ws, bias, dx, P, a.Cin, a.cw, a.ocs, pl.split, a.act, a.slope, s);
  return cat::check_launch("conv2d_dgrad");
}

int cat_conv2d_dgrad(const cat_conv_t* g, const float* dy, const float* w, const float* bias, float* dx, int dxcs, int dxcw,
                     cat_stream_t stream) {
  return conv_dgrad_impl(g, dy, w, nullptr, bias, dx, dxcs, dxcw, nullptr, stream);
}

int cat_conv2d_dgrad_ws(const cat_conv_t* g, const float* dy, const float* w, const float* bias, float* dx, int dxcs, int dxcw, void* ws,
                        cat_stream_t stream) {
  return conv_dgrad_impl(g, dy, w, nullptr, bias, dx, dxcs, dxcw, ws, stream);
}

int cat_conv2d_dgrad_t(const cat_conv_t* g, const float* dy, const float* w, const float* wt, const float* bias, float* dx, int dxcs, int dxcw,
                       cat_stream_t stream) {
  return conv_dgrad_impl(g, dy, w, wt, bias, dx, dxcs, dxcw, nullptr, stream);
}

size_t cat_conv2d_wgrad_ws_bytes(const cat_conv_t* g) { return plan_wgrad(g).ws_bytes; }

static int wgrad_reduce_blocks(const RedItem& r) { return (int)(((int64_t)r.Cout * r.taps * (r.c4 / 4) + 15) / 16); }

// One weight gradient.  `defer` != nullptr: the partial sums stay in ws, defer->red describes the reduction still owed (nsplit = 0: none, dw is
// final) and defer->ws_bytes what the plan asked of ws -- cat_conv2d_wgrad_batch reduces several of them with one launch.
struct WgradDeferred { RedItem red; size_t ws_bytes; };
static int wgrad_impl(const cat_conv_t* g, const float* x, const float* dy, float* dw, int accumulate, void* ws, cat_stream_t stream,
                      WgradDeferred* defer) {
  if (defer) defer->red.nsplit = 0;
  IgemmArgs a{};
  if (int e = fill_common(a, g)) return e;
  CAT_REQUIRE((int64_t)g->N * g->H * g->W * g->xcs < (int64_t)4294967295LL, "conv wgrad: activation larger than 2^32 elements");
  const ConvPlan pl = plan_wgrad(g);
  if (defer) defer->ws_bytes = pl.ws_bytes;
  CAT_REQUIRE(pl.direct || ws != nullptr, "conv wgrad: workspace required");
  a.a = x; a.b = dy;
  a.c4 = pl.c4;
  a.cval = a.wcs >= a.c4 ? a.c4 : g->Cin;   // channels written per tap
  a.K = pl.K;
  a.nsplit = pl.split; a.mchunk = pl.chunk;
  a.direct = pl.direct ? 1 : 0;
  a.accumulate = accumulate;
  a.out = pl.direct ? dw : (float*)ws;
  hipStream_t s = (hipStream_t)stream;
  cat::ProfScope prof(pl.name, conv_flops(g), 0.0, stream);
#define WGRAD_TILE_LAUNCH(NMAX, MT, NT, WM, WN, ...)                                                                              \
  if (a.Cout <= NMAX)                                                                                                             \
    conv_wgrad_kernel<MT, NT, WM, WN><<<dim3(cdiv(a.Cout, WM * MT * 16) * cdiv(a.K, WN * NT * 16), pl.split), 256, 0, s>>>(a);     \
  else
  int e = 0;
  switch (pl.kernel) {
    case Kernel::Small: e = cat::smallco_wgrad(g, x, dy, (float*)ws, s); break;
    case Kernel::LdsTile: e = cat::twgrad(g, x, dy, (float*)ws, s); break;
    case Kernel::PixelStream: e = cat::pwgrad(g, x, dy, (float*)ws, s); break;
    case Kernel::Direct32:
      launch_big_lds<conv_wgrad32d_kernel>(dim3(cdiv(a.Cout, 128) * (a.K / 128), pl.split), (size_t)2 * 2 * 32 * 128 * sizeof(float), s, a,
                                           pl.chunk, cdiv(g->Wo, 32));
      e = cat::check_launch("conv2d_wgrad");
      break;
    default:
      WGRAD_TILES(WGRAD_TILE_LAUNCH, ) {}
      e = cat::check_launch("conv2d_wgrad");
      break;
  }
#undef WGRAD_TILE_LAUNCH
  if (e || pl.direct) return e;
  const RedItem red{(const float*)ws, dw, pl.split, a.Cout, a.kh * a.kw, a.cval, a.wcs, a.c4, a.K, accumulate};
  if (defer) defer->red = red;
  else wgrad_reduce_kernel<<<wgrad_reduce_blocks(red), 256, 0, s>>>(red.ws, red.dw, red.nsplit, red.Cout, red.taps, red.wlim, red.wcs, red.c4, red.K, red.accumulate);
  return cat::check_launch("conv2d_wgrad_reduce");
}

int cat_conv2d_wgrad(const cat_conv_t* g, const float* x, const float* dy, float* dw, int accumulate, void* ws,
                     cat_stream_t stream) {
  return wgrad_impl(g, x, dy, dw, accumulate, ws, stream, nullptr);
}

// every item's part of the batch workspace starts on a 256-byte boundary
static size_t wgrad_batch_slot(size_t ws_bytes) { return (ws_bytes + 255) & ~(size_t)255; }

size_t cat_conv2d_wgrad_batch_ws_bytes(const cat_wgrad_item_t* items, int n) {
  size_t total = 0;
  for (int i = 0; i < n; ++i) total += wgrad_batch_slot(plan_wgrad(&items[i].g).ws_bytes);
  return total;
}

int cat_conv2d_wgrad_batch(const cat_wgrad_item_t* items, int n, void* ws, cat_stream_t stream) {
  CAT_REQUIRE(n >= 1 && n <= CAT_WGRAD_BATCH_MAX, "conv wgrad batch: 1 .. %d items", CAT_WGRAD_BATCH_MAX);
  CAT_REQUIRE(ws != nullptr, "conv wgrad batch: workspace required");
  RedMany many{};
  size_t off = 0;
  int blocks = 0;
  for (int i = 0; i < n; ++i) {
    WgradDeferred d{};
    if (int e = wgrad_impl(&items[i].g, items[i].x, items[i].dy, items[i].dw, items[i].accumulate, (char*)ws + off, stream, &d)) return e;
    off += wgrad_batch_slot(d.ws_bytes);
    if (d.red.nsplit > 0) {
      many.it[many.n] = d.red;
      many.start[many.n] = blocks;
      blocks += wgrad_reduce_blocks(d.red);
      ++many.n;
    }
  }
  if (many.n == 0) return 0;
  many.start[many.n] = blocks;
  wgrad_reduce_many_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(many);
  return cat::check_launch("conv2d_wgrad_reduce_many");
}

}  // extern "C"
