// Launch plans of the stand-alone norm (norm.hip: the three-launch kernels, norm_resident.hip: the one-launch kernels of small groups).
#pragma once
#include "common.h"

namespace cat {

struct NormPlan : ColPlan {
  int G, Pg, Ptot;      // Ptot = all pixels: a sharded batch norm's last group may hold fewer than Pg
  size_t part_off, scale_off, shift_off, c1_off, c2_off, bytes;
};

static inline NormPlan norm_plan(const cat_norm_t* g) {
  int G = g->mode == CAT_NORM_INSTANCE ? g->N : 1, Pg = g->mode == CAT_NORM_INSTANCE ? g->HW : g->N * g->HW;
  if (g->mode == CAT_NORM_BATCH && g->shards > 1) {      // torch.chunk(batch, shards): groups of ceil(N / shards) consecutive samples
    const int per = cdiv(g->N, g->shards);
    G = cdiv(g->N, per);
    Pg = per * g->HW;
  }
  NormPlan p{col_plan(Pg, g->cs, G, 2048, 16, 1024)};   // stats: ~2048 workgroups, at most 1024 per group, >= 16 pixels per pixel lane
  p.G = G;
  p.Pg = Pg;
  p.Ptot = g->N * g->HW;
  size_t off = 0;
  p.part_off = off; off += (size_t)p.G * p.nb * 2 * g->cs;
  p.scale_off = off; off += (size_t)p.G * g->cs;
  p.shift_off = off; off += (size_t)p.G * g->cs;
  p.c1_off = off; off += (size_t)p.G * g->cs;
  p.c2_off = off; off += (size_t)p.G * g->cs;
  p.bytes = off * sizeof(float);
  return p;
}

// The one-launch kernels (norm_resident.hip): one workgroup of 256 lanes holds every pixel of one group for a slab of zq channel quads in
// registers -- ppl = 256 / zq pixel lanes, at most K pixels each.  The slab narrows (4, 2, 1 quads) as the group grows, so that
// zq * pixels <= 256 * K always holds; nz slabs cover the nq quads of a pixel.  ok = 0: the geometry stays on the three launches.
// (32 pixels per lane were measured too: 245 VGPRs, and the forward pass 3 - 5 us SLOWER than the three launches wherever it needed them.)
constexpr int kResidentFwdK = 16, kResidentBwdK = 16;      // most float4 of x (forward) / of x and of dy (backward) per lane
constexpr size_t kResidentFwdNarrowFloats = (size_t)3 << 20;      // forward with one-quad slabs of a wider pixel: activations up to 12 MiB
struct ResidentPlan {
  int ok, zq, nz, K;
};
ResidentPlan norm_resident_plan(const NormPlan& p, int cs, int backward);      // honours cat_norm_set_resident
void norm_resident_fwd(const cat_norm_t* g, const NormPlan& p, const ResidentPlan& r, const float* x, const float* gamma, const float* beta,
                       float* y, float* save_mean, float* save_rstd, float* running_mean, float* running_var, int64_t* num_batches,
                       hipStream_t s);
// c1 / c2: the rows norm_bwd_param_kernel reads (several groups with parameter gradients) or NULL; dgamma / dbeta: one group only, or NULL
void norm_resident_bwd(const cat_norm_t* g, const NormPlan& p, const ResidentPlan& r, const float* x, const float* dy, const float* gamma,
                       const float* beta, const float* mean, const float* rstd, float* dx, float* c1, float* c2, float* dgamma, float* dbeta,
                       int accumulate, hipStream_t s);

}  // namespace cat
