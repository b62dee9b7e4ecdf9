// The tail of the cityscapes mIoU (metric/mIoU_score.py:152-168, 174-247) on the GPU, NHWC fp32, gfx950.
//
//   seg_up_logsoftmax : nn.ConvTranspose2d(C, C, 2s, stride=s, padding=s/2, groups=C, bias=False) + nn.LogSoftmax(dim=1) in one pass.  With
//                       kernel = 2 * stride every output pixel meets at most 2 x 2 input pixels per channel, so one thread = one output
//                       pixel with all its C channels in registers; the C x 2s x 2s filter planes (from the checkpoint: `up.weight`, not
//                       assumed bilinear) sit in LDS as [ky][kx][channel].  Padding channels never enter the softmax and are written as 0.
//   seg_confusion     : resize_4d_tensor (PIL bilinear enlargement == F.interpolate(mode='bilinear', align_corners=False)) + argmax(axis=1)
//                       + fast_hist in one pass: one thread = one LABEL pixel, which interpolates the C log-probabilities from its 2 x 2 source
//                       pixels, takes the argmax (lowest index wins, numpy's rule) and counts (label, prediction) in the workgroup's LDS
//                       histogram; the workgroup adds its non-zero counters to the 64-bit global matrix at the end.  Integer sums: the result
//                       does not depend on the order.  The resized [N, C, Hl, Wl] map (159 MB per cityscapes image) never exists.
//                       A NaN log-probability never wins the comparison, so an all-NaN pixel resolves to class 0 (numpy's argmax returns
//                       the first NaN's index instead); log-softmax outputs of finite logits are never NaN.  At most 2^32 - 1 label pixels
//                       per call (32-bit LDS counters).
#include "common.h"

namespace {

constexpr int SEG_MAXQ = 8;   // channel quads a thread holds in registers: C <= 32

// NQ = round_up(C, 4) / 4.  wl = LDS image of the filters, [2s][2s][NQ * 4], padding channels 0.
template <int NQ>
__global__ __launch_bounds__(256) void seg_up_logsoftmax_kernel(const float* __restrict__ x, int xcs, int N, int h, int w, int C,
                                                                const float* __restrict__ wt, int s, float* __restrict__ y, int ycs) {
  extern __shared__ __attribute__((aligned(16))) float wl[];
  constexpr int CS = NQ * 4;
  const int K = 2 * s, KK = K * K, pad = s >> 1;
  for (int i = threadIdx.x; i < KK * CS; i += 256) wl[i] = 0.f;
  __syncthreads();
  for (int i = threadIdx.x; i < C * KK; i += 256) {
    const int c = i / KK, r = i - c * KK;
    wl[r * CS + c] = wt[i];
  }
  __syncthreads();
  const int H = h * s, W = w * s;
  const int64_t total = (int64_t)N * H * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int X = (int)(i % W);
    int64_t r = i / W;
    const int Y = (int)(r % H);
    const int n = (int)(r / H);
    const int iyh = (Y + pad) / s, kyh = (Y + pad) - iyh * s;
    const int ixh = (X + pad) / s, kxh = (X + pad) - ixh * s;
    f4 v[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) v[q] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int iy = iyh - a, ky = kyh + a * s;
      if ((unsigned)iy >= (unsigned)h) continue;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int ix = ixh - b, kx = kxh + b * s;
        if ((unsigned)ix >= (unsigned)w) continue;
        const float* xp = x + (((int64_t)n * h + iy) * w + ix) * xcs;
        const float* wp = wl + (ky * K + kx) * CS;
#pragma unroll
        for (int q = 0; q < NQ; ++q) v[q] += *reinterpret_cast<const f4*>(xp + q * 4) * *reinterpret_cast<const f4*>(wp + q * 4);
      }
    }
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (q * 4 + e < C) m = fmaxf(m, v[q][e]);
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (q * 4 + e < C) sum += expf(v[q][e] - m);
    const float lse = m + logf(sum);
    float* yp = y + i * ycs;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      f4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = q * 4 + e < C ? v[q][e] - lse : 0.f;   // padding channels stay exactly 0
      *reinterpret_cast<f4*>(yp + q * 4) = o;
    }
  }
}

// hist[n_classes * label + pred] += 1 for every label pixel with label < n_classes (255 = ignore, fast_hist :174-177).
// Source coordinates as torch's upsample_bilinear2d, align_corners = False (see resize_bilinear_kernel in eval_ops.hip).
template <int NQ>
__global__ __launch_bounds__(256) void seg_confusion_kernel(const float* __restrict__ lp, int lcs, int N, int h, int w, int C,
                                                            const unsigned char* __restrict__ label, int Hl, int Wl, int ncls,
                                                            long long* __restrict__ hist, unsigned char* __restrict__ pred, float sh, float sw) {
  extern __shared__ unsigned int cnt[];
  const int nbins = ncls * ncls;
  for (int i = threadIdx.x; i < nbins; i += 256) cnt[i] = 0u;
  __syncthreads();
  const bool same = h == Hl && w == Wl;   // resize_4d_tensor returns the map itself (:187-188)
  const int64_t total = (int64_t)N * Hl * Wl;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int X = (int)(i % Wl);
    int64_t r = i / Wl;
    const int Y = (int)(r % Hl);
    const int n = (int)(r / Hl);
    const float* base = lp + (int64_t)n * h * w * lcs;
    f4 v[NQ];
    if (same) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) v[q] = *reinterpret_cast<const f4*>(base + ((int64_t)Y * w + X) * lcs + q * 4);
    } else {
      float sy = sh * ((float)Y + 0.5f) - 0.5f, sx = sw * ((float)X + 0.5f) - 0.5f;
      sy = sy < 0.f ? 0.f : sy;
      sx = sx < 0.f ? 0.f : sx;
      int y0 = (int)sy, x0 = (int)sx;
      y0 = y0 < h - 1 ? y0 : h - 1;
      x0 = x0 < w - 1 ? x0 : w - 1;
      const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
      const float ly1 = sy - (float)y0, lx1 = sx - (float)x0, ly0 = 1.f - ly1, lx0 = 1.f - lx1;
      const float* p00 = base + ((int64_t)y0 * w + x0) * lcs;
      const float* p01 = base + ((int64_t)y0 * w + x1) * lcs;
      const float* p10 = base + ((int64_t)y1 * w + x0) * lcs;
      const float* p11 = base + ((int64_t)y1 * w + x1) * lcs;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const f4 v00 = *reinterpret_cast<const f4*>(p00 + q * 4), v01 = *reinterpret_cast<const f4*>(p01 + q * 4);
        const f4 v10 = *reinterpret_cast<const f4*>(p10 + q * 4), v11 = *reinterpret_cast<const f4*>(p11 + q * 4);
        v[q] = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
      }
    }
    int best = 0;
    float bv = v[0][0];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = q * 4 + e;
        if (c > 0 && c < C && v[q][e] > bv) {   // strict: the lowest index wins a tie (numpy's argmax)
          bv = v[q][e];
          best = c;
        }
      }
    if (pred) pred[i] = (unsigned char)best;
    const int lab = label[i];
    if (lab < ncls) atomicAdd(&cnt[ncls * lab + best], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nbins; i += 256) {
    const unsigned int c = cnt[i];
    if (c) atomicAdd(reinterpret_cast<unsigned long long*>(hist + i), (unsigned long long)c);
  }
}

int seg_grid(int64_t items, int per_block, int cap) {
  int64_t b = (items + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

extern "C" {

int cat_seg_up_logsoftmax(const float* x, int xcs, int N, int h, int w, int C, const float* up_w, int s, float* y, int ycs,
                          cat_stream_t stream) {
  const int C4 = (C + 3) & ~3, NQ = C4 / 4, K = 2 * s;
  CAT_REQUIRE(x && y && up_w && N > 0 && h > 0 && w > 0 && C > 0 && NQ <= SEG_MAXQ, "seg up: geometry (C <= %d)", SEG_MAXQ * 4);
  CAT_REQUIRE((xcs & 3) == 0 && (ycs & 3) == 0 && xcs >= C4 && ycs >= C4, "seg up: channel layout");
  CAT_REQUIRE(s >= 2 && (s & 1) == 0, "seg up: kernel 2s / stride s / padding s/2 with an even s (s=%d)", s);
  const size_t lds = (size_t)K * K * C4 * sizeof(float);
  CAT_REQUIRE(lds <= 64 * 1024, "seg up: filter planes (%zu bytes) exceed the LDS budget", lds);
  CAT_REQUIRE((int64_t)N * h * s * w * s * ycs < ((int64_t)1 << 40), "seg up: output too large");
  const int64_t total = (int64_t)N * h * s * w * s;
  cat::ProfScope prof("seg_up_logsoftmax", 0.0, 4.0 * ((double)N * h * w * xcs + (double)total * ycs), stream);
  const int grid = seg_grid(total, 1024, 4096);
  hipStream_t st = (hipStream_t)stream;
#define SEG_UP(Q) case Q: seg_up_logsoftmax_kernel<Q><<<grid, 256, lds, st>>>(x, xcs, N, h, w, C, up_w, s, y, ycs); break;
  switch (NQ) { SEG_UP(1) SEG_UP(2) SEG_UP(3) SEG_UP(4) SEG_UP(5) SEG_UP(6) SEG_UP(7) SEG_UP(8) }
#undef SEG_UP
  return cat::check_launch("seg_up_logsoftmax");
}

int cat_seg_confusion(const float* logp, int lcs, int N, int h, int w, int C, const unsigned char* label, int Hl, int Wl, int n_classes,
                      long long* hist, unsigned char* pred, cat_stream_t stream) {
  const int C4 = (C + 3) & ~3, NQ = C4 / 4;
  CAT_REQUIRE(logp && label && hist && N > 0 && h > 0 && w > 0 && Hl > 0 && Wl > 0 && C > 0 && NQ <= SEG_MAXQ, "seg confusion: geometry");
  CAT_REQUIRE((lcs & 3) == 0 && lcs >= C4, "seg confusion: channel layout");
  CAT_REQUIRE(n_classes >= C && n_classes <= 64, "seg confusion: C <= n_classes <= 64 (C=%d, n_classes=%d)", C, n_classes);
  const int64_t total = (int64_t)N * Hl * Wl;
  // the per-workgroup LDS counters are 32 bits wide: one call may not hand a workgroup 2^32 pixels (callers pass one batch per call)
  CAT_REQUIRE(total < ((int64_t)1 << 32), "seg confusion: %lld label pixels in one call (limit 2^32: call per batch)", (long long)total);
  cat::ProfScope prof("seg_confusion", 0.0, 4.0 * (double)N * h * w * lcs + (double)total, stream);
  const int grid = seg_grid(total, 2048, 2048);
  const size_t lds = (size_t)n_classes * n_classes * sizeof(unsigned int);
  hipStream_t st = (hipStream_t)stream;
  const float sh = (float)h / (float)Hl, sw = (float)w / (float)Wl;
#define SEG_CF(Q) \
  case Q: seg_confusion_kernel<Q><<<grid, 256, lds, st>>>(logp, lcs, N, h, w, C, label, Hl, Wl, n_classes, hist, pred, sh, sw); break;
  switch (NQ) { SEG_CF(1) SEG_CF(2) SEG_CF(3) SEG_CF(4) SEG_CF(5) SEG_CF(6) SEG_CF(7) SEG_CF(8) }
#undef SEG_CF
  return cat::check_launch("seg_confusion");
}

}  // extern "C"
