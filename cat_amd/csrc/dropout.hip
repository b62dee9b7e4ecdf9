// Dropout of the InvertedResidualChannels branches (reference models/modules/inception_modules.py:144, :174): a counter-based
// generator (Philox4x32-10, the constants of ROCm's rocrand_philox4x32_10.h) keyed by a device-resident ticket, so that
//   * the mask of a block forward is reproducible in its backward pass without being stored (the fused block re-materialises the
//     hidden activations there), and
//   * a step replayed as a captured graph draws a fresh mask per replay: the ticket is written by a kernel (cat_rng_draw) that
//     advances a counter in device memory, never by the host at capture time.
// One apply kernel serves every call site: segments of a channel-concatenated NHWC buffer, each one Dropout module with its own logical
// channel count C and block index j; plain (y = x * keep * s) or materialising (y = act(x * scale + shift) * keep * s).
#include "common.h"

namespace {
using cat::cdiv;

struct U4 {
  uint32_t v[4];
};

__device__ __forceinline__ U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
  }
  U4 o;
  o.v[0] = c0;
  o.v[1] = c1;
  o.v[2] = c2;
  o.v[3] = c3;
  return o;
}

__device__ __forceinline__ uint32_t pick(const U4& r, uint32_t k) {
  return k == 0 ? r.v[0] : (k == 1 ? r.v[1] : (k == 2 ? r.v[2] : r.v[3]));
}

__device__ __forceinline__ U4 block_bits(uint64_t b, uint32_t j, uint32_t d, uint32_t k0, uint32_t k1) {
  return philox4x32_10((uint32_t)b, (uint32_t)(b >> 32), j, d, k0, k1);
}

// ONE thread: the ticket of a block forward and the counter advance (plain C++ loads and stores)
__global__ void rng_draw_kernel(int64_t* state, int* ticket) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const uint64_t seed = (uint64_t)state[0], ctr = (uint64_t)state[1];
  ticket[0] = (int)(uint32_t)ctr;
  ticket[1] = (int)(uint32_t)seed;
  ticket[2] = (int)(uint32_t)(seed >> 32);
  ticket[3] = 0;
  state[1] = (int64_t)(ctr + 1);
}

// (pixel, channel quad) walk; a quad of a segment with C % 4 != 0 straddles at most two Philox blocks
__global__ __launch_bounds__(256) void dropout_kernel(const cat_drop_t g, const float* x, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, const int* __restrict__ ticket, float* y,
                                                      unsigned total, int nq) {
  const uint32_t d = (uint32_t)ticket[0], k0 = (uint32_t)ticket[1], k1 = (uint32_t)ticket[2];
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const unsigned p = i / (unsigned)nq, q = i - p * (unsigned)nq;
    const int ch = (int)q * 4;
    // the segment of this quad; unrolled over the fixed table so that it is read from the kernel arguments, never indexed at run time
    bool in = false;
    int C = 0, cl = 0;
    uint32_t j = 0;
#pragma unroll
    for (int k = 0; k < CAT_DROP_MAXSEG; ++k) {
      if (k < g.nseg && ch >= g.seg[k].c0 && ch < g.seg[k].c0 + ((g.seg[k].c + 3) & ~3)) {
        in = true;
        C = g.seg[k].c;
        cl = ch - g.seg[k].c0;
        j = (uint32_t)g.seg[k].j;
      }
    }
    if (!in && !g.rest) continue;
    f4 v = *reinterpret_cast<const f4*>(x + (int64_t)p * g.xcs + ch);
    if (g.mode == CAT_DROP_NORM) {
      const int so = (int)(p / (unsigned)g.hw) * g.sstride + ch;
      const f4 sc = *reinterpret_cast<const f4*>(scale + so);
      const f4 sh = *reinterpret_cast<const f4*>(shift + so);
      v = v * sc + sh;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = cat::apply_act(v[e], g.act, g.slope);
    }
    if (in) {
      const uint64_t e0 = (uint64_t)p * (uint64_t)C + (uint64_t)cl;
      const int nv = min(4, C - cl);      // masked lanes of this quad (>= 1)
      const uint64_t b0 = e0 >> 2;
      const U4 r0 = block_bits(b0, j, d, k0, k1);
      const U4 r1 = ((e0 + nv - 1) >> 2) != b0 ? block_bits(b0 + 1, j, d, k0, k1) : r0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (e < nv) {
          const uint64_t el = e0 + e;
          const uint32_t r = (el >> 2) == b0 ? pick(r0, (uint32_t)(el & 3)) : pick(r1, (uint32_t)(el & 3));
          const bool keep = !g.drop_all && r >= g.thresh;
          v[e] = keep ? v[e] * g.s : 0.f;
        }
      }
    }
    *reinterpret_cast<f4*>(y + (int64_t)p * g.ycs + ch) = v;
  }
}

}  // namespace

extern "C" {

int cat_rng_draw(int64_t* state, int* ticket, cat_stream_t stream) {
  CAT_REQUIRE(state != nullptr && ticket != nullptr, "rng_draw: null pointer");
  rng_draw_kernel<<<1, 64, 0, (hipStream_t)stream>>>(state, ticket);
  return cat::check_launch("rng_draw");
}

int cat_dropout_apply(const cat_drop_t* g, const float* x, const float* scale, const float* shift, const int* ticket, float* y,
                      cat_stream_t stream) {
  CAT_REQUIRE(g != nullptr && x != nullptr && y != nullptr && ticket != nullptr, "dropout: null pointer");
  CAT_REQUIRE(g->npix > 0 && g->width > 0 && (g->width & 3) == 0, "dropout: empty geometry or width %d not a multiple of 4", g->width);
  CAT_REQUIRE((g->xcs & 3) == 0 && (g->ycs & 3) == 0 && g->width <= g->xcs && g->width <= g->ycs, "dropout: channel layout");
  CAT_REQUIRE(g->nseg >= 0 && g->nseg <= CAT_DROP_MAXSEG, "dropout: %d segments", g->nseg);
  CAT_REQUIRE(g->mode == CAT_DROP_PLAIN || g->mode == CAT_DROP_NORM, "dropout: mode %d", g->mode);
  CAT_REQUIRE(g->mode == CAT_DROP_PLAIN || (scale != nullptr && shift != nullptr && g->hw > 0 && g->sstride >= 0 && (g->sstride & 3) == 0),
              "dropout: normalising mode needs scale / shift");
  CAT_REQUIRE(g->mode == CAT_DROP_PLAIN || g->sstride == 0 || g->npix % g->hw == 0, "dropout: pixels per image");
  for (int k = 0; k < g->nseg; ++k) {
    const cat_dropseg_t& s = g->seg[k];
    CAT_REQUIRE(s.c > 0 && s.c0 >= 0 && (s.c0 & 3) == 0 && s.c0 + ((s.c + 3) & ~3) <= g->width, "dropout: segment %d outside the buffer", k);
    for (int m = 0; m < k; ++m)
      CAT_REQUIRE(s.c0 >= g->seg[m].c0 + ((g->seg[m].c + 3) & ~3) || g->seg[m].c0 >= s.c0 + ((s.c + 3) & ~3), "dropout: segments %d and %d overlap",
                  m, k);
  }
  const int nq = g->width / 4;
  const int64_t total = (int64_t)g->npix * nq;
  CAT_REQUIRE(total < (int64_t)4000000000LL, "dropout: tensor too large");
  CAT_REQUIRE((int64_t)g->npix * g->xcs < ((int64_t)1 << 40) && (int64_t)g->npix * g->ycs < ((int64_t)1 << 40), "dropout: tensor too large");
  cat::ProfScope prof(g->mode == CAT_DROP_NORM ? "dropout_norm" : "dropout", 0.0, 8.0 * (double)total * 4, stream);
  dropout_kernel<<<cat::ew_grid(total, 4096), 256, 0, (hipStream_t)stream>>>(*g, x, scale, shift, ticket, y, (unsigned)total, nq);
  return cat::check_launch("dropout");
}

}  // extern "C"
