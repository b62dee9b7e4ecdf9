// Shared device/host helpers for libcat_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/cat_hip.h"

typedef float f4 __attribute__((ext_vector_type(4)));

namespace cat {

// Timing diagnostics -- per-phase shader clocks (CAT_DBG), scheduling experiments (CAT_SCHED, CAT_LDS_PAD) and the ablation switches that make
// results WRONG by design (CAT_PK_ABLATE, CAT_Q_ABLATE) -- exist only in the DIAGNOSTIC build of the library: `python -m cat_amd._build --diag`
// compiles with -DCAT_DIAG into lib/libcat_hip_diag.so, which tools/debug/* load through CAT_LIB=diag.  In the production library every
// `kDiag && ...` condition is a compile-time false: the branches and their operands are not in the kernels.
#ifdef CAT_DIAG
constexpr bool kDiag = true;
#else
constexpr bool kDiag = false;
#endif

void set_error(const char* fmt, ...);
int check_launch(const char* what);

// Optional HIP-event timing of one entry-point call (enabled by cat_prof_enable): records an event pair on the
// launch stream around everything the enclosing scope enqueues, tagged with its algorithmic FLOPs / bytes.
class ProfScope {
 public:
  ProfScope(const char* family, double flops, double bytes, void* stream);
  ~ProfScope();

 private:
  bool active_;
  void* stream_;
  int idx_;
};

#define CAT_REQUIRE(cond, ...)            \
  do {                                    \
    if (!(cond)) {                        \
      cat::set_error(__VA_ARGS__);        \
      return -22;                         \
    }                                     \
  } while (0)

// Cout <= 4 direct convolutions (conv_smallco.hip)
bool smallco_applicable(const cat_conv_t* g);
int smallco_fwd_ksplit(const cat_conv_t* g);   // > 1: channel-split forward, needs ksplit * N*Ho*Wo*ycs floats of workspace
int smallco_fwd(const cat_conv_t* g, const float* x, const float* w, const float* bias, float* y, float* ws, int ksplit, hipStream_t s);
int smallco_wgrad_nblk(const cat_conv_t* g);
int smallco_wgrad(const cat_conv_t* g, const float* x, const float* dy, float* ws, hipStream_t s);
bool smallci_dgrad_applicable(const cat_conv_t* g);   // 4x4 / stride 2 / pad 1 conv with 3 or 6 input channels (PatchGAN's first layer)
int smallci_dgrad(const cat_conv_t* g, const float* dy, const float* w, float* dx, int dxcs, int dxcw, hipStream_t s);

// LDS-tile weight gradient of narrow stride-1 3x3 / 5x5 layers (conv_twgrad.hip)
bool twgrad_applicable(const cat_conv_t* g);
int twgrad_nblk(const cat_conv_t* g);
int twgrad(const cat_conv_t* g, const float* x, const float* dy, float* ws, hipStream_t s);   // partials [nblk][Cout][taps * round_up(Cin, 4)]

// pixel-streaming weight gradient of 1 x 1 layers with few channels and many pixels (conv_pwgrad.hip)
bool pwgrad_applicable(const cat_conv_t* g);
int pwgrad_nblk(const cat_conv_t* g);
int pwgrad(const cat_conv_t* g, const float* x, const float* dy, float* ws, hipStream_t s);   // partials [nblk][Cout][round_up(Cin, 4)]

// Opt a kernel in to more than 64 KB of dynamic LDS.  hipFuncSetAttribute applies to the CURRENT device only, so the "already
// done" flag of a call site is kept per device ordinal (a process may drive several GPUs, e.g. the 2-ranks-on-one-box tests).
struct LdsOptIn {
  unsigned long long done = 0ull;
};
static inline void lds_optin(LdsOptIn& st, const void* fn, int bytes) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev >= 0 && dev < 64 && ((st.done >> dev) & 1ull)) return;
  (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (dev >= 0 && dev < 64) st.done |= 1ull << dev;
}

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
static inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// Workgroups of a 256-lane grid-stride walk over `items`: clamp(cdiv(items, 256), 1, cap).
static inline int ew_grid(int64_t items, int cap) {
  const int64_t b = (items + 255) / 256;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// Column reductions and pixel walks over [P][cs] (norm.hip, spade.hip, elementwise.hip): a workgroup is ppl pixel lanes x zq channel quads
// (every access a float4, a wave touches whole pixels), nz such workgroups cover the nq quads of a pixel, nb of them share the pixels.
// nb aims at `target` workgroups over all `groups`, keeps at least min_pix pixels per pixel lane and stays within cap (INT_MAX: none).
struct ColPlan {
  int nq, nz, zq, ppl, nb;
};
static inline int col_blocks(int64_t P, int ppl, int groups_nz, int target, int min_pix, int cap) {
  int nb = cdiv(target, groups_nz);
  if (nb > cap) nb = cap;
  const int maxb = cdiv(P, (int64_t)ppl * min_pix);
  if (nb > maxb) nb = maxb;
  return nb < 1 ? 1 : nb;
}
static inline ColPlan col_plan(int64_t P, int cs, int groups, int target, int min_pix, int cap) {
  ColPlan p;
  p.nq = cs / 4;
  p.nz = cdiv(p.nq, 256);
  p.zq = cdiv(p.nq, p.nz);  // quads per z-block (<= 256)
  p.ppl = 256 / p.zq;
  p.nb = col_blocks(P, p.ppl, groups * p.nz, target, min_pix, cap);
  return p;
}

__device__ __forceinline__ float apply_act(float v, int act, float slope) {
  switch (act) {
    case CAT_ACT_RELU: return v > 0.f ? v : 0.f;
    case CAT_ACT_LRELU: return v > 0.f ? v : v * slope;
    case CAT_ACT_TANH: return tanhf(v);
    case CAT_ACT_RELU6: return fminf(fmaxf(v, 0.f), 6.f);
    default: return v;
  }
}

// derivative of the activation expressed through its OUTPUT y (all four are invertible enough for that)
__device__ __forceinline__ float act_grad_from_out(float y, int act, float slope) {
  switch (act) {
    case CAT_ACT_RELU: return y > 0.f ? 1.f : 0.f;
    case CAT_ACT_LRELU: return y > 0.f ? 1.f : slope;
    case CAT_ACT_TANH: return 1.f - y * y;
    case CAT_ACT_RELU6: return (y > 0.f && y < 6.f) ? 1.f : 0.f;      // hardtanh_backward: 0 at and beyond both bounds
    default: return 1.f;
  }
}

// One element of a scalar loss (cat_loss_fwd / cat_loss_multi_fwd) and its derivative in a: ka_loss.hip and loss_multi.hip evaluate these two and
// nothing else, which is what makes cat_loss_multi_* bit-identical to cat_loss_fwd/bwd term by term.  CAT_LOSS_MSE is the default arm.
__device__ __forceinline__ float loss_term(int kind, float a, float b, float t) {
  switch (kind) {
    case CAT_LOSS_L1: {      // t = beta of nn.SmoothL1Loss: d^2 / (2 beta) inside |d| < beta, |d| - beta / 2 outside; both arms computed, one select.
      // beta 0 is plain L1, bit for bit: |d| < 0 never holds and |d| - 0 is |d| (rbeta is uniform and loop-invariant, and keeps the unused arm finite)
      const float d = a - b, ad = fabsf(d), rbeta = t > 0.f ? 1.f / t : 0.f;
      return ad < t ? 0.5f * d * d * rbeta : ad - 0.5f * t;
    }
    case CAT_LOSS_LSGAN: return (a - t) * (a - t);
    case CAT_LOSS_HINGE_D_REAL: return -fminf(a - 1.f, 0.f);
    case CAT_LOSS_HINGE_D_FAKE: return -fminf(-a - 1.f, 0.f);
    case CAT_LOSS_NEG_MEAN: return -a;
    case CAT_LOSS_BCE_LOGITS: return (1.f - t) * a + fmaxf(-a, 0.f) + log1pf(expf(-fabsf(a)));   // BCE with logits against the constant target t
    case CAT_LOSS_MEAN: return a;
    default: return (a - b) * (a - b);
  }
}
__device__ __forceinline__ float loss_grad(int kind, float a, float b, float t) {
  switch (kind) {
    case CAT_LOSS_L1: {      // d / beta inside |d| < beta, sign(d) outside (beta 0: sign(d) everywhere, 0 at d = 0)
      const float d = a - b, rbeta = t > 0.f ? 1.f / t : 0.f;
      return fabsf(d) < t ? d * rbeta : (a > b ? 1.f : (a < b ? -1.f : 0.f));
    }
    case CAT_LOSS_LSGAN: return 2.f * (a - t);
    case CAT_LOSS_HINGE_D_REAL: return a - 1.f < 0.f ? -1.f : 0.f;   // torch.min(x-1, 0): ties send the gradient to ... see tests (measure zero)
    case CAT_LOSS_HINGE_D_FAKE: return -a - 1.f < 0.f ? 1.f : 0.f;
    case CAT_LOSS_NEG_MEAN: return -1.f;
    case CAT_LOSS_BCE_LOGITS: return 1.f / (1.f + expf(-a)) - t;   // sigmoid(a) - t
    case CAT_LOSS_MEAN: return 1.f;
    default: return 2.f * (a - b);
  }
}

__device__ __forceinline__ int reflect_idx(int i, int n) {
  i = i < 0 ? -i : i;
  return i >= n ? 2 * n - 2 - i : i;
}

// XCD-aware, bijective block remap (guide §5 T1): consecutive logical tiles land on one XCD's L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = bid & 7, idx = bid >> 3;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + idx;
}

// The depthwise tile kernels (block_norm.hip: dwm_fwd / dwm_bwd, dwconv.hip: dw_multi_tile) deal a tile's channel quads out over several
// workgroups: every quad of a depthwise conv -- its output, its tile statistics, its filter gradient -- is independent of every other.
// kDwGroup = most quads of one workgroup (a 12 x 20 patch of 4 quads is 15 KB of LDS: 4+ workgroups per CU even with dwm_bwd's two patches).
#ifndef CAT_DW_GROUP
#define CAT_DW_GROUP 4
#endif
constexpr int kDwGroup = CAT_DW_GROUP;
static_assert(kDwGroup >= 2 && kDwGroup <= 8 && (kDwGroup & (kDwGroup - 1)) == 0, "CAT_DW_GROUP: 2, 4 or 8");

// Groups = the runs of equal kernel size cut into pieces of at most kDwGroup quads, so a group has ONE kernel size (fully unrolled tap loops)
// and never straddles a run boundary.  q0 / gn: first quad and quad count of each group; returns the number of groups (<= nq).
static inline int dw_quad_groups(const int* ks, int nq, unsigned char* q0, unsigned char* gn) {
  int ng = 0;
  for (int q = 0; q < nq; ++q) {
    if (ng && ks[q] == ks[q - 1] && gn[ng - 1] < kDwGroup) {
      ++gn[ng - 1];
      continue;
    }
    q0[ng] = (unsigned char)q;
    gn[ng] = 1;
    ++ng;
  }
  return ng;
}

// Workgroup -> (tile, group), bijective on [0, ntiles * ng).  With ntiles % 8 == 0 each XCD (workgroup id mod 8) owns a contiguous
// eighth of the tiles and all their groups: the groups of a tile share cache lines, neighbouring tiles share their halo -- in one L2.
__device__ __forceinline__ void dw_tile_group(int bid, int ntiles, int ng, int& tt, int& grp) {
  if ((ntiles & 7) == 0) {
    const int idx = bid >> 3;
    tt = (bid & 7) * (ntiles >> 3) + idx / ng;
    grp = idx % ng;
  } else {
    tt = bid / ng;
    grp = bid % ng;
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// A ColPlan workgroup's lane: channel quad cq (cq_l within z-block z), pixel lane pl; inactive lanes only take part in the combine.
struct ColLanes {
  int cq_l, pl, cq;
  bool active;
};
__device__ __forceinline__ ColLanes col_lanes(int z, int zq, int ppl, int cs) {
  const int tid = threadIdx.x;
  ColLanes L;
  L.cq_l = tid % zq;
  L.pl = tid / zq;
  L.cq = z * zq + L.cq_l;
  L.active = L.pl < ppl && L.cq * 4 < cs;
  return L;
}

// Block combine of NS per-lane sums: through LDS, pixel lane 0 adds lanes 1 .. ppl-1 in that order (deterministic) and stores sum k of its
// quad at dst + k * cs + cq * 4.  The two-sum stats kernels accumulate in named f4s and hand over a copy: an array indexed in their pixel
// loops is promoted to registers only after unrolling, which costs them ~20 register moves.
template <int NS>
__device__ __forceinline__ void col_block_store(f4 (&s)[NS], f4 (*red)[256], const ColLanes& L, int zq, int ppl, int cs, float* dst) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < NS; ++k) red[k][tid] = s[k];
  __syncthreads();
  if (L.pl == 0 && L.cq * 4 < cs) {
    for (int j = 1; j < ppl; ++j) {
#pragma unroll
      for (int k = 0; k < NS; ++k) s[k] += red[k][j * zq + L.cq_l];
    }
    dst += L.cq * 4;
#pragma unroll
    for (int k = 0; k < NS; ++k) *reinterpret_cast<f4*>(dst + k * cs) = s[k];
  }
}

}  // namespace cat
