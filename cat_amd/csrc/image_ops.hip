// The generated image set of evaluate_model as uint8 on the device (cat_amd/metric/images.py): util.tensor2im (utils/util.py:58-88) and
// ToTensor + Normalize (metric/mIoU_score.py:28-51; FID's and KID's `/ 255`) as two streaming kernels.  One lane = one pixel: a 16-byte load
// and a 4-byte store per pixel at xcs == 4, the reverse on the way back.  The host formulas round every float32 operation on its own, so
// nothing here may contract into a fused multiply-add: x * 127.5 + 127.5 gives other bytes next to the integer boundaries.
#include "common.h"

#pragma clang fp contract(off)

namespace {

// out[img][y][x] = one dword, byte c = (uint8) clip((x_c + 1) / 2 * 255, 0, 255) truncated, bytes [C, 4) = 0.  fmaxf / fminf drop a NaN for
// their other operand: NaN -> 0, -inf -> 0, +inf -> 255.
__global__ __launch_bounds__(256) void image_quantize_kernel(const float* __restrict__ x, int xcs, int64_t npix, int C,
                                                            unsigned int* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
    const f4 v = *reinterpret_cast<const f4*>(x + i * xcs);
    unsigned int px = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float t = (v[e] + 1.0f) / 2.0f;
      t = t * 255.0f;
      t = fminf(fmaxf(t, 0.0f), 255.0f);
      px |= (e < C ? (unsigned int)(int)t : 0u) << (8 * e);
    }
    out[i] = px;
  }
}

// y[img][y][x][c] = ((u8_c / 255) - mean_c) / std_c for c < C, 0 for c in [C, 4): correctly rounded float32 division and subtraction
__global__ __launch_bounds__(256) void image_normalize_kernel(const unsigned int* __restrict__ u8, int64_t npix, int C, f4 mean, f4 stdv,
                                                             float* __restrict__ y, int ycs) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
    const unsigned int px = u8[i];
    f4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float t = (float)((px >> (8 * e)) & 255u) / 255.0f;
      t = t - mean[e];
      t = t / stdv[e];
      v[e] = e < C ? t : 0.0f;
    }
    *reinterpret_cast<f4*>(y + i * ycs) = v;
  }
}

}  // namespace

extern "C" {

int cat_image_quantize(const float* x, int xcs, int N, int H, int W, int C, unsigned char* out, long long img_off, cat_stream_t stream) {
  CAT_REQUIRE(x && out && N > 0 && H > 0 && W > 0 && C >= 1 && C <= 4 && xcs >= 4 && (xcs & 3) == 0 && img_off >= 0, "image quantize: layout");
  CAT_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 3) == 0, "image quantize: x must be 16-byte aligned, out 4-byte aligned");
  const int64_t npix = (int64_t)N * H * W;
  cat::ProfScope prof("image_quantize", 0.0, 20.0 * (double)npix, stream);
  image_quantize_kernel<<<cat::ew_grid(npix, 16384), 256, 0, (hipStream_t)stream>>>(x, xcs, npix, C,
                                                                          reinterpret_cast<unsigned int*>(out) + (int64_t)img_off * H * W);
  return cat::check_launch("image_quantize");
}

int cat_image_normalize(const unsigned char* u8, long long img_off, int N, int H, int W, int C, float mean0, float mean1, float mean2,
                        float mean3, float std0, float std1, float std2, float std3, float* y, int ycs, cat_stream_t stream) {
  CAT_REQUIRE(u8 && y && N > 0 && H > 0 && W > 0 && C >= 1 && C <= 4 && ycs >= 4 && (ycs & 3) == 0 && img_off >= 0, "image normalize: layout");
  CAT_REQUIRE(((uintptr_t)y & 15) == 0 && ((uintptr_t)u8 & 3) == 0, "image normalize: y must be 16-byte aligned, u8 4-byte aligned");
  const int64_t npix = (int64_t)N * H * W;
  cat::ProfScope prof("image_normalize", 0.0, 20.0 * (double)npix, stream);
  image_normalize_kernel<<<cat::ew_grid(npix, 16384), 256, 0, (hipStream_t)stream>>>(reinterpret_cast<const unsigned int*>(u8) + (int64_t)img_off * H * W, npix, C,
                                                                           f4{mean0, mean1, mean2, mean3}, f4{std0, std1, std2, std3}, y, ycs);
  return cat::check_launch("image_normalize");
}

}  // extern "C"
