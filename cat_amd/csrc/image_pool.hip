// The CycleGAN image history pool (reference utils/image_pool.py:27-53) as ONE launch per query: the host decides what happens to each image of
// the batch (pass it on, swap it with a stored one, store it while the pool is still filling) and leaves the decisions as int32 codes in DEVICE
// memory; the kernel applies them.  A captured step therefore replays the pool: the launch is the same every time, the codes and the history
// buffer it reads are what changes.
// The reference's loop is sequential -- two images of a batch may hit one slot, a slot stored early in a batch may be swapped out later in it --
// and that order is kept by OWNERSHIP: a lane owns float4 element e of every image and of every slot, and walks the images of the batch itself.
// No element is touched by two lanes: no barrier, no atomic, no second launch.
#include "common.h"

namespace {

constexpr int kPoolCap = 2048;   // most workgroups of the element walk (cat::ew_grid): 8 per CU

// per4 = float4 elements of one image.  codes[i] is the same address for every lane (a uniform read); `pool` is read AND written, by the same
// lane in program order, so it carries no __restrict__.
__global__ __launch_bounds__(256) void image_pool_query_kernel(const f4* __restrict__ images, f4* pool, f4* __restrict__ out,
                                                               const int32_t* __restrict__ codes, int n, int pool_size, int64_t per4) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < per4; e += (int64_t)gridDim.x * 256) {
    for (int i = 0; i < n; ++i) {
      const int64_t code = codes[i];
      const int64_t s = code >= 0 ? code : -2 - code;      // pass (-1) -> -1: outside every pool
      f4 v = images[i * per4 + e];
      if (s >= 0 && s < pool_size) {                       // anything else is a pass (the host validates the codes before it uploads them)
        f4* slot = pool + s * per4 + e;
        if (code >= 0) {                                   // swap: the stored image goes out, this one takes its place
          const f4 old = *slot;
          *slot = v;
          v = old;
        } else {                                           // store: the pool is still filling
          *slot = v;
        }
      }
      out[i * per4 + e] = v;
    }
  }
}

}  // namespace

extern "C" {

int cat_image_pool_query(const float* images, float* pool, float* out, const int32_t* codes, int n, int pool_size, int64_t per,
                         cat_stream_t stream) {
  CAT_REQUIRE(n >= 0, "image_pool_query: n %d", n);
  if (n == 0) return 0;
  CAT_REQUIRE(images != nullptr && pool != nullptr && out != nullptr && codes != nullptr, "image_pool_query: null pointer");
  CAT_REQUIRE(per > 0 && (per & 3) == 0, "image_pool_query: %lld floats per image (a positive multiple of 4)", (long long)per);
  CAT_REQUIRE(pool_size >= 0, "image_pool_query: pool_size %d", pool_size);
  cat::ProfScope prof("image_pool", 0.0, 3.0 * (double)n * (double)per * 4, stream);
  image_pool_query_kernel<<<cat::ew_grid(per / 4, kPoolCap), 256, 0, (hipStream_t)stream>>>(
      reinterpret_cast<const f4*>(images), reinterpret_cast<f4*>(pool), reinterpret_cast<f4*>(out), codes, n, pool_size, per / 4);
  return cat::check_launch("image_pool_query");
}

}  // extern "C"
