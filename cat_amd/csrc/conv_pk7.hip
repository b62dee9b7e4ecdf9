// LDS-tile convolution with 7 x 7 segments: the cat_tconv_fwd contract (include/cat_hip.h) for launches that need a wider patch than
// tconv_kernel's (8 + 4) x (TW + 4) -- a segment with ks == 7, or taps further than 4 pixels apart (hl + hr > 4).  The reference's parser
// default is --kernel_sizes 3 5 7 (options/distill_options.py:100-104); with it every InvertedResidualChannels block has 7 x 7 first and
// second convs (models/modules/inception_modules.py:135-165), and its backward pass runs their input gradients with padv up to 6.
//
// The kernel body is conv_pk_tconv_main.h, the body of tconv_kernel: the K-concatenated segment walk, the staging affine + activation, the
// packed filter stream, the epilogue and the per-tile statistics are the same code.  What differs here:
//   * the patch is (8 + 6) x (16 + 6) pixels (TW = 16 only): 1232 staging slots, 5 per thread;
//   * the A-offset table of a chunk has 256 entries: a 7 x 7 segment has 49 x 4 = 196 (tap, quad) pairs per 16-channel chunk.
// LDS: 2 x 14 x 22 x 80 B + 2 KB of tables + the statistics scratch = at most 55 KB.
//
// A translation unit of its own: the code generation of conv_pk.hip is pinned (tests/test_codegen.py) and stays as it is; this file's
// table is tests/golden/codegen_conv_pk7.json.
#include "common.h"
#include "conv_pk_tile.h"

namespace cat_pk7 {

using namespace cat_pk;      // TH, PITCH, Launch, mma_groups (conv_pk_tile.h)

__device__ __attribute__((aligned(16))) float g_zero[4] = {0.f, 0.f, 0.f, 0.f};

constexpr int TW7 = 16, HALO7 = 6, KTAB7 = 256;

template <int NT, int TW>
__global__ __launch_bounds__(256) void tconv7_kernel(const cat_tconv_t g, const float* __restrict__ pack, const float* __restrict__ bias,
                                                     float* __restrict__ y, const Launch L) {
  constexpr int HALO = HALO7, KTAB = KTAB7;
  static_assert(49 * 4 <= KTAB && KTAB <= 256, "one table entry per (tap, quad) pair of a chunk, filled by one thread each");
#include "conv_pk_tconv_main.h"
}

}  // namespace cat_pk7

namespace cat_pk {

int tconv7_launch(const cat_tconv_t* g, const float* pack, const float* bias, float* y, cat_stream_t stream) {
  using namespace cat_pk7;
  CAT_REQUIRE(g->nseg >= 1 && g->nseg <= CAT_TCONV_MAXSEG, "tconv: %d segments", g->nseg);
  CAT_REQUIRE(g->N > 0 && g->H > 0 && g->W > 0 && g->Ho > 0 && g->Wo > 0 && g->Nn > 0, "tconv: empty geometry");
  CAT_REQUIRE((g->ycs & 3) == 0 && g->ycs >= g->Nn && g->ycw <= g->ycs, "tconv: bad output stride");
  CAT_REQUIRE(g->res == nullptr || g->rcs >= g->Nn, "tconv: residual stride");
  int hl = 0, hr = 0;
  double kflops = 0.0;
  for (int s = 0; s < g->nseg; ++s) {
    const cat_tseg_t& sg = g->seg[s];
    CAT_REQUIRE(sg.ks == 1 || sg.ks == 3 || sg.ks == 5 || sg.ks == 7, "tconv: kernel size %d unsupported", sg.ks);
    CAT_REQUIRE(sg.c4 > 0 && (sg.c4 & 3) == 0 && (sg.xcs & 3) == 0 && sg.xcs >= sg.c4, "tconv: segment %d channel layout", s);
    CAT_REQUIRE(sg.padv >= 0 && sg.padv <= HALO7, "tconv: segment %d padv", s);
    CAT_REQUIRE(sg.act == CAT_ACT_NONE || sg.act == CAT_ACT_RELU || sg.act == CAT_ACT_LRELU, "tconv: staging activation %d", sg.act);
    CAT_REQUIRE(!sg.reflect || (sg.ks <= g->H && sg.ks <= g->W), "tconv: reflect padding wider than the plane");
    CAT_REQUIRE((int64_t)g->N * g->H * g->W * sg.xcs < (int64_t)4294967295LL, "tconv: source larger than 2^32 elements");
    hl = sg.padv > hl ? sg.padv : hl;
    hr = sg.ks - 1 - sg.padv > hr ? sg.ks - 1 - sg.padv : hr;   // stays >= 0: a segment whose taps all lie left of the origin needs none
    CAT_REQUIRE(sg.cin > 0 && sg.cin <= sg.c4, "tconv: segment %d valid channel count", s);
    kflops += (double)sg.ks * sg.ks * sg.cin;
  }
  CAT_REQUIRE(hl + hr <= HALO7, "tconv: halo %d + %d exceeds the staged patch", hl, hr);
  CAT_REQUIRE(g->stats == nullptr || (g->act == CAT_ACT_NONE && g->res == nullptr && g->scs >= g->ycw), "tconv: statistics need a plain epilogue");
  Launch L;
  L.nt_total = cat::cdiv(g->Nn, 16);
  L.nblk = cat::cdiv(L.nt_total, 8);
  const int nt = cat::cdiv(L.nt_total, L.nblk);
  L.nblk = cat::cdiv(L.nt_total, nt);
  L.ablate = 0;
  L.hl = hl;
  L.tr = TH + hl + hr;
  L.tc = TW7 + hl + hr;
  L.tiles_x = cat::cdiv(g->Wo, TW7);
  L.tiles = L.tiles_x * cat::cdiv(g->Ho, TH);
  const int64_t grid = (int64_t)g->N * L.tiles * L.nblk;
  CAT_REQUIRE(grid < (int64_t)2147483647, "tconv: grid too large");
  const size_t lds = (size_t)2 * L.tr * L.tc * PITCH * sizeof(float) + 2 * KTAB7 * sizeof(int) + (g->stats ? (size_t)8 * nt * 16 * sizeof(float) : 0);
  CAT_REQUIRE(lds <= 96 * 1024, "tconv: %zu bytes of LDS (max 96 KB)", lds);
  hipStream_t s = (hipStream_t)stream;
  cat::ProfScope prof(g->nseg > 1 ? "conv_tconv7_multi" : "conv_tconv7", 2.0 * (double)g->N * g->Ho * g->Wo * (g->nvalid > 0 ? g->nvalid : g->Nn) * kflops, 0.0,
                      stream);
#define CAT_PK7_LAUNCH(NT)                                                                   \
  {                                                                                          \
    static cat::LdsOptIn optin;                                                              \
    cat::lds_optin(optin, (const void*)tconv7_kernel<NT, TW7>, 96 * 1024);                   \
    tconv7_kernel<NT, TW7><<<(int)grid, 256, lds, s>>>(*g, pack, bias, y, L);                \
  }
  switch (nt) {
    case 1: CAT_PK7_LAUNCH(1) break;
    case 2: CAT_PK7_LAUNCH(2) break;
    case 3: CAT_PK7_LAUNCH(3) break;
    case 4: CAT_PK7_LAUNCH(4) break;
    case 5: CAT_PK7_LAUNCH(5) break;
    case 6: CAT_PK7_LAUNCH(6) break;
    case 7: CAT_PK7_LAUNCH(7) break;
    default: CAT_PK7_LAUNCH(8) break;
  }
#undef CAT_PK7_LAUNCH
  return cat::check_launch("tconv7_fwd");
}

}  // namespace cat_pk
