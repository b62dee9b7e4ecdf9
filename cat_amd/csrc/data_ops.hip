// A training batch out of a device-resident image set (cat_amd/data.py) as ONE launch: gather by sample index, crop, horizontal flip, ToTensor +
// Normalize -- what data/base_dataset.py:85-129 composes per sample on the host -- written straight into the layout the step reads: the NHWC
// activation for images, [N, 1, Hc, Wc] for the label and instance maps.  The random draws stay on the host; they reach the kernel as int32
// codes in DEVICE memory (as in image_pool.hip), so a captured launch replays with the codes staged for that replay.
// One lane = one output pixel of one plane; blockIdx.y is the plane, so its descriptor is read with scalar loads.  Normalize's
// ((u / 255) - 0.5) / 0.5 rounds every float32 operation on its own, as torch does on the host: nothing here may contract or reassociate.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kDataCap = 16384;

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// codes row of sample n: [idx slot 0, idx slot 1, (x, y, flip) of plane 0, (x, y, flip) of plane 1, ...].  The host validates what it draws; the
// clamps only keep a bad code from reading outside the set.
__global__ __launch_bounds__(256) void data_batch_kernel(cat_data_batch_t t, const int32_t* __restrict__ codes) {
  const int p = blockIdx.y;
  const cat_data_plane_t d = t.plane[p];
  const unsigned int per = (unsigned int)(d.Hc * d.Wc), total = per * (unsigned int)t.N;      // < 2^31 (checked by the entry point): 32-bit divisions
  const int stride = 2 + 3 * t.planes;
  for (unsigned int i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const int n = (int)(i / per);
    const int rem = (int)(i - (unsigned int)n * per);
    const int r = rem / d.Wc, j = rem - r * d.Wc;
    const int32_t* row = codes + (int64_t)n * stride;
    const int idx = clampi(row[d.slot], d.M - 1);
    const int x = row[2 + 3 * p], y = row[3 + 3 * p], flip = row[4 + 3 * p];
    const int sy = clampi(y + r, d.H - 1);
    const int sx = clampi(flip ? x + d.Wc - 1 - j : x + j, d.W - 1);
    const int64_t s = ((int64_t)idx * d.H + sy) * d.W + sx;
    if (d.kind == CAT_DATA_IMAGE) {
      const unsigned int px = static_cast<const unsigned int*>(d.src)[s];
      f4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float u = (float)((px >> (8 * e)) & 255u) / 255.0f;
        u = u - 0.5f;
        u = u / 0.5f;
        v[e] = e < d.C ? u : 0.0f;
      }
      f4* out = reinterpret_cast<f4*>(static_cast<float*>(d.dst) + (int64_t)i * d.cs);
      out[0] = v;
      for (int q = 1; q < d.cs / 4; ++q) out[q] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    } else if (d.kind == CAT_DATA_LABEL) {
      const unsigned int u = static_cast<const unsigned char*>(d.src)[s];
      static_cast<float*>(d.dst)[i] = u == 255u ? t.unknown : (float)u;
    } else {
      static_cast<int32_t*>(d.dst)[i] = static_cast<const int32_t*>(d.src)[s];
    }
  }
}

}  // namespace

extern "C" {

int cat_data_batch(const cat_data_batch_t* t, const int32_t* codes, cat_stream_t stream) {
  CAT_REQUIRE(t != nullptr && codes != nullptr, "data_batch: null pointer");
  CAT_REQUIRE(t->planes >= 1 && t->planes <= CAT_DATA_MAXPLANES, "data_batch: %d planes (1 to %d)", t->planes, CAT_DATA_MAXPLANES);
  CAT_REQUIRE(t->N >= 0, "data_batch: N %d", t->N);
  if (t->N == 0) return 0;
  CAT_REQUIRE(((uintptr_t)codes & 3) == 0, "data_batch: codes must be 4-byte aligned");
  int64_t most = 0;
  double bytes = 4.0 * t->N * (2 + 3 * t->planes);
  for (int p = 0; p < t->planes; ++p) {
    const cat_data_plane_t& d = t->plane[p];
    CAT_REQUIRE(d.src != nullptr && d.dst != nullptr, "data_batch: plane %d: null pointer", p);
    CAT_REQUIRE(d.M > 0 && d.H > 0 && d.W > 0 && d.Hc > 0 && d.Wc > 0 && d.Hc <= d.H && d.Wc <= d.W, "data_batch: plane %d: crop %d x %d of %d images of %d x %d", p,
                d.Hc, d.Wc, d.M, d.H, d.W);
    CAT_REQUIRE(d.slot == 0 || d.slot == 1, "data_batch: plane %d: index slot %d", p, d.slot);
    const int64_t npix = (int64_t)t->N * d.Hc * d.Wc;
    CAT_REQUIRE((int64_t)d.M * d.H * d.W < ((int64_t)1 << 40) && npix < ((int64_t)1 << 31), "data_batch: plane %d: %lld output pixels (fewer than 2^31), %lld in the set", p,
                (long long)npix, (long long)d.M * d.H * d.W);
    if (d.kind == CAT_DATA_IMAGE) {
      CAT_REQUIRE((d.C == 1 || d.C == 3) && d.cs >= 4 && (d.cs & 3) == 0, "data_batch: plane %d: C %d (1 or 3), channel stride %d (a positive multiple of 4)", p, d.C, d.cs);
      CAT_REQUIRE(((uintptr_t)d.src & 3) == 0 && ((uintptr_t)d.dst & 15) == 0, "data_batch: plane %d: src must be 4-byte aligned, dst 16-byte aligned", p);
      bytes += (4.0 + 4.0 * d.cs) * (double)npix;
    } else if (d.kind == CAT_DATA_LABEL) {
      CAT_REQUIRE(((uintptr_t)d.dst & 3) == 0, "data_batch: plane %d: dst must be 4-byte aligned", p);
      bytes += 5.0 * (double)npix;
    } else {
      CAT_REQUIRE(d.kind == CAT_DATA_INT32, "data_batch: plane %d: kind %d", p, d.kind);
      CAT_REQUIRE(((uintptr_t)d.src & 3) == 0 && ((uintptr_t)d.dst & 3) == 0, "data_batch: plane %d: src and dst must be 4-byte aligned", p);
      bytes += 8.0 * (double)npix;
    }
    most = npix > most ? npix : most;
  }
  cat::ProfScope prof("data_batch", 0.0, bytes, stream);
  data_batch_kernel<<<dim3(cat::ew_grid(most, kDataCap), t->planes), 256, 0, (hipStream_t)stream>>>(*t, codes);
  return cat::check_launch("data_batch");
}

}  // extern "C"
