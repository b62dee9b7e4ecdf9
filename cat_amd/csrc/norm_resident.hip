// InstanceNorm2d / BatchNorm2d (training statistics) of SMALL statistic groups in one launch, NHWC, gfx950 (cat_norm_fwd / cat_norm_bwd dispatch
// here, norm.hip).  When every pixel of a group fits in the registers of one workgroup, the three dependent launches of norm.hip -- partial sums,
// finalize, apply -- are one: a workgroup owns one group and one slab of zq channel quads (norm_plan.h: ResidentPlan), loads its slab once
// (forward: x; backward: x and dy), reduces it and writes the result.  Slabs are independent: no grid synchronisation, no workspace, no atomics.
//   forward   1 read + 1 write of the activation (three launches: 2 + 1);  mean, then the variance from deviations about that mean,
//             then y = act((x - mean) * gamma * rstd + beta)
//   backward  2 reads + 1 write                  (three launches: 4 + 1)
// Reductions have one fixed order (slab_sum), so two runs give the same bits.
#include "norm_plan.h"
#include <stdlib.h>

namespace {
using cat::cdiv;

// Sum over the pixel lanes of a slab, the same bits in every lane: an xor butterfly over the lanes of a wave that hold the same quad
// (lane & (zq - 1); float addition commutes, so both partners of a step get one value), then the four waves in order through LDS.
__device__ __forceinline__ f4 slab_sum(f4 v, f4 (*red)[4], int zq) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    if (o >= zq) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += __shfl_xor(v[e], o, 64);
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane < zq) red[wave][lane] = v;
  __syncthreads();
  const int q = threadIdx.x & (zq - 1);
  return ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
}

// grid: G * nz workgroups; consecutive slabs of a group share cache lines, so they go to one XCD's L2 (cat::xcd_remap)
template <int K>
__global__ __launch_bounds__(256) void norm_fwd_resident_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float* __restrict__ y,
                                                                float* __restrict__ save_mean, float* __restrict__ save_rstd,
                                                                float* __restrict__ running_mean, float* __restrict__ running_var,
                                                                int64_t* __restrict__ num_batches, int Pg, int Ptot, int C, int cs, int nz,
                                                                int zq, float eps, float momentum, int act, float slope) {
  __shared__ f4 red[2][4][4];
  const int wg = cat::xcd_remap(blockIdx.x, gridDim.x);
  const int g = wg / nz, ppl = 256 / zq;
  const cat::ColLanes L = cat::col_lanes(wg % nz, zq, ppl, cs);
  if (num_batches && wg == 0 && threadIdx.x == 0) *num_batches += 1;   // nn.BatchNorm2d.num_batches_tracked
  const int Pn = min(Pg, Ptot - g * Pg);      // (the last group of a sharded batch norm may be short)
  const int c = L.cq * 4;
  const size_t base = (size_t)g * Pg * cs + c;
  f4 v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int p = L.pl + k * ppl;
    v[k] = L.active && p < Pn ? *reinterpret_cast<const f4*>(x + base + (size_t)p * cs) : f4{0.f, 0.f, 0.f, 0.f};
  }
  f4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < K; ++k) s += v[k];      // tail pixels hold zeros
  const float inv = 1.f / (float)Pn;
  const f4 mean = slab_sum(s, red[0], zq) * inv;
  f4 q = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const f4 d = v[k] - mean;
    if (L.pl + k * ppl < Pn) q += d * d;
  }
  const f4 var = slab_sum(q, red[1], zq) * inv;
  f4 sc, sh;      // y = (x - mean) * sc + sh: the mean is in registers, so no x * scale + shift that cancels where |mean| >> std
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool cv = L.active && c + e < C;
    const float rstd = rsqrtf(var[e] + eps);
    sc[e] = cv ? (gamma ? gamma[c + e] : 1.f) * rstd : 0.f;
    sh[e] = cv ? (beta ? beta[c + e] : 0.f) : 0.f;
    if (cv && L.pl == 0) {
      save_mean[g * C + c + e] = mean[e];
      save_rstd[g * C + c + e] = rstd;
      if (running_mean && g == 0) {  // batch norm only; of a sharded one group 0 alone (replica 0 shares its buffers with the module)
        running_mean[c + e] = (1.f - momentum) * running_mean[c + e] + momentum * mean[e];
        const float unb = Pn > 1 ? var[e] * (float)Pn / (float)(Pn - 1) : var[e];
        running_var[c + e] = (1.f - momentum) * running_var[c + e] + momentum * unb;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int p = L.pl + k * ppl;
    f4 o = (v[k] - mean) * sc + sh;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = c + e < C ? cat::apply_act(o[e], act, slope) : 0.f;      // padding channels: zeros
    if (L.active && p < Pn) *reinterpret_cast<f4*>(y + base + (size_t)p * cs) = o;
  }
}

template <int K>
__global__ __launch_bounds__(256) void norm_bwd_resident_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                float* __restrict__ dx, float* __restrict__ c1, float* __restrict__ c2,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate, int Pg,
                                                                int Ptot, int C, int cs, int nz, int zq, int act, float slope) {
  __shared__ f4 red[2][4][4];
  const int wg = cat::xcd_remap(blockIdx.x, gridDim.x);
  const int g = wg / nz, ppl = 256 / zq;
  const cat::ColLanes L = cat::col_lanes(wg % nz, zq, ppl, cs);
  const int Pn = min(Pg, Ptot - g * Pg);
  const int c = L.cq * 4;
  const size_t base = (size_t)g * Pg * cs + c;
  f4 mu, rs, ga, be;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool cv = L.active && c + e < C;
    mu[e] = cv ? mean[g * C + c + e] : 0.f;
    rs[e] = cv ? rstd[g * C + c + e] : 0.f;
    ga[e] = cv ? (gamma ? gamma[c + e] : 1.f) : 0.f;
    be[e] = cv ? (beta ? beta[c + e] : 0.f) : 0.f;
  }
  f4 xh[K], gv[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int p = L.pl + k * ppl;
    const bool ok = L.active && p < Pn;
    xh[k] = ok ? *reinterpret_cast<const f4*>(x + base + (size_t)p * cs) : mu;      // xhat = 0, g = 0: adds nothing
    gv[k] = ok ? *reinterpret_cast<const f4*>(dy + base + (size_t)p * cs) : f4{0.f, 0.f, 0.f, 0.f};
  }
  f4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < K; ++k) {
    xh[k] = (xh[k] - mu) * rs;
    if (act != CAT_ACT_NONE) {
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[k][e] *= cat::act_grad_from_out(cat::apply_act(ga[e] * xh[k][e] + be[e], act, slope), act, slope);
    }
    s0 += gv[k];
    s1 += gv[k] * xh[k];
  }
  s0 = slab_sum(s0, red[0], zq);
  s1 = slab_sum(s1, red[1], zq);
  const float inv = 1.f / (float)Pn;
  const f4 m1 = s0 * inv, m2 = s1 * inv, sc = ga * rs;      // sc: zeros on padding channels
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int p = L.pl + k * ppl;
    f4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = c + e < C ? sc[e] * (gv[k][e] - m1[e] - xh[k][e] * m2[e]) : 0.f;
    if (L.active && p < Pn) *reinterpret_cast<f4*>(dx + base + (size_t)p * cs) = o;
  }
  if (L.active && L.pl == 0) {
    if (c1) {      // several groups: the per-group means norm_bwd_param_kernel sums over the groups
      *reinterpret_cast<f4*>(c1 + g * cs + c) = m1;
      *reinterpret_cast<f4*>(c2 + g * cs + c) = m2;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {      // one group: the parameter gradients are these sums
      if (c + e < C) {
        if (dgamma) dgamma[c + e] = accumulate ? dgamma[c + e] + s1[e] : s1[e];
        if (dbeta) dbeta[c + e] = accumulate ? dbeta[c + e] + s0[e] : s0[e];
      }
    }
  }
}

// Off unless asked for: the graphed GauGAN step measured 60.08 -> 58.61 ms with it, inside the 1.96 ms spread of its own three rounds, and the
// CycleGAN-style steps within theirs (profiles/norm_resident_bench.txt) -- the rule for a default is a gain beyond the spread.
int g_resident = -1;      // -1: not read from the environment yet
int resident_on() {
  if (g_resident < 0) g_resident = getenv("CAT_NORM_RESIDENT") ? (atoi(getenv("CAT_NORM_RESIDENT")) != 0) : 0;
  return g_resident;
}

}  // namespace

namespace cat {

ResidentPlan norm_resident_plan(const NormPlan& p, int cs, int backward) {
  ResidentPlan r{0, 0, 0, 0};
  const int kmax = backward ? kResidentBwdK : kResidentFwdK;
  if (!resident_on() || p.Pg > 256 * kmax) return r;
  const int nq = cs / 4;
  int zq = nq >= 3 ? 4 : nq;      // 16 channels = 64 contiguous bytes per pixel; narrower only when the group needs the pixel lanes
  while (cdiv(p.Pg, 256 / zq) > kmax) zq >>= 1;
  // One-quad slabs of a wider pixel use 16 bytes of every cache line they fetch, and the slabs of a line are different workgroups.  Measured
  // (profiles/norm_resident_bench.txt): the backward pass still gains at every size (two of its four reads go away), the forward pass is level
  // with the three launches up to 10.5 MB of activation and 1 - 4 us slower from 16.8 MB on -- it stays on the three launches above 12 MiB.
  if (!backward && zq == 1 && nq > 1 && (size_t)p.Ptot * cs > kResidentFwdNarrowFloats) return r;
  const int need = cdiv(p.Pg, 256 / zq);
  r.ok = 1;
  r.zq = zq;
  r.nz = cdiv(nq, zq);
  r.K = need <= 4 ? 4 : need <= 8 ? 8 : 16;
  return r;
}

void norm_resident_fwd(const cat_norm_t* g, const NormPlan& p, const ResidentPlan& r, const float* x, const float* gamma, const float* beta,
                       float* y, float* save_mean, float* save_rstd, float* running_mean, float* running_var, int64_t* num_batches,
                       hipStream_t s) {
  const dim3 grid(p.G * r.nz);
#define CAT_RES_FWD(KK)                                                                                                                  \
  norm_fwd_resident_kernel<KK><<<grid, 256, 0, s>>>(x, gamma, beta, y, save_mean, save_rstd, running_mean, running_var, num_batches, p.Pg, \
                                                    p.Ptot, g->C, g->cs, r.nz, r.zq, g->eps, g->momentum, g->act, g->slope)
  switch (r.K) {
    case 4: CAT_RES_FWD(4); break;
    case 8: CAT_RES_FWD(8); break;
    default: CAT_RES_FWD(16); break;
  }
#undef CAT_RES_FWD
}

void norm_resident_bwd(const cat_norm_t* g, const NormPlan& p, const ResidentPlan& r, const float* x, const float* dy, const float* gamma,
                       const float* beta, const float* mean, const float* rstd, float* dx, float* c1, float* c2, float* dgamma, float* dbeta,
                       int accumulate, hipStream_t s) {
  const dim3 grid(p.G * r.nz);
#define CAT_RES_BWD(KK)                                                                                                                    \
  norm_bwd_resident_kernel<KK><<<grid, 256, 0, s>>>(x, dy, gamma, beta, mean, rstd, dx, c1, c2, dgamma, dbeta, accumulate, p.Pg, p.Ptot, g->C, \
                                                    g->cs, r.nz, r.zq, g->act, g->slope)
  switch (r.K) {
    case 4: CAT_RES_BWD(4); break;
    case 8: CAT_RES_BWD(8); break;
    default: CAT_RES_BWD(16); break;
  }
#undef CAT_RES_BWD
}

}  // namespace cat

extern "C" {

int cat_norm_set_resident(int on) {
  const int prev = resident_on();
  g_resident = on != 0;
  return prev;
}

int cat_norm_resident_max_pixels(int backward) { return 256 * (backward ? cat::kResidentBwdK : cat::kResidentFwdK); }

int cat_norm_launches(const cat_norm_t* g, int backward, int with_param_grads) {
  const cat::NormPlan p = cat::norm_plan(g);
  const int resident = cat::norm_resident_plan(p, g->cs, backward).ok;
  if (backward) return (resident ? 1 : 3) + (with_param_grads && p.G > 1 ? 1 : 0);
  return resident ? 1 : 3;
}

}  // extern "C"
