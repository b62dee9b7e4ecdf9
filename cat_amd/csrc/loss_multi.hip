// The loss head of a multiscale discriminator in one launch each way: T mean-reduced scalar losses (the kinds of cat_loss_fwd, ka_loss.hip)
// over T unrelated NHWC tensors.  The GauGAN teacher step has num_D * (n_layers_D + 1) such terms on the generator side and 2 * num_D on the
// discriminator side, each a few microseconds of work: per term they cost two forward launches and one backward launch between dependent
// launches; here the whole table costs two forward launches (partials, then a fixed-order final sum) and one backward launch.
//
// The table travels BY VALUE in the kernel arguments (no device allocation, no host synchronisation: the calls can be captured).  Every
// workgroup finds its term by scanning the <= 16 block offsets, which are wave-uniform kernel-argument reads.  The arithmetic per term is the
// arithmetic of loss_partial_kernel / loss_final_kernel / loss_bwd_kernel: same quad loop, same wave / block sums in the same order, so the
// result does not depend on which other terms share the launch and is bit-identical run to run (no atomics at all).
#include "common.h"

namespace {

struct MultiArgs {
  cat_loss_term_t term[CAT_LOSS_MULTI_MAX];
  const float* gout[CAT_LOSS_MULTI_MAX];   // backward only: d total / d out[t], one float each
  int blk0[CAT_LOSS_MULTI_MAX + 1];        // first workgroup of every term; blk0[T] = grid size
  int T;
};

__device__ __forceinline__ int find_term(const MultiArgs& A, int bid) {
  int t = 0;
  while (t + 1 < A.T && bid >= A.blk0[t + 1]) ++t;
  return t;
}

__global__ __launch_bounds__(256) void loss_multi_partial_kernel(const MultiArgs A, float* __restrict__ part) {
  __shared__ float red[4];
  const int t = find_term(A, blockIdx.x);
  const cat_loss_term_t& L = A.term[t];
  const int lb = blockIdx.x - A.blk0[t], nb = A.blk0[t + 1] - A.blk0[t];
  const int nq = L.cs >> 2, C = L.C, kind = L.kind;
  const int64_t nquads = L.M * nq;
  const float* __restrict__ a = L.a;
  const float* __restrict__ b = L.b;
  float s = 0.f;
  for (int64_t i = (int64_t)lb * 256 + threadIdx.x; i < nquads; i += (int64_t)nb * 256) {
    const int c = (int)(i % nq) * 4;
    const f4 av = *reinterpret_cast<const f4*>(a + i * 4);
    f4 bv = {0.f, 0.f, 0.f, 0.f};
    if (b) bv = *reinterpret_cast<const f4*>(b + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c + e < C) s += cat::loss_term(kind, av[e], bv[e], L.target);
  }
  s = cat::wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// one workgroup per term: its partials in index order, then the mean over the M * C real elements
__global__ __launch_bounds__(256) void loss_multi_final_kernel(const MultiArgs A, const float* __restrict__ part, float* __restrict__ out) {
  __shared__ float red[4];
  const int t = blockIdx.x;
  const float* p = part + A.blk0[t];
  const int nb = A.blk0[t + 1] - A.blk0[t];
  float s = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) s += p[i];
  s = cat::wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[t] = (red[0] + red[1] + red[2] + red[3]) * (1.f / (float)((double)A.term[t].M * A.term[t].C));
}

// term[t].scale already holds scale_t / (M * C); terms without `da` own no workgroup
__global__ __launch_bounds__(256) void loss_multi_bwd_kernel(const MultiArgs A) {
  const int t = find_term(A, blockIdx.x);
  const cat_loss_term_t& L = A.term[t];
  const int lb = blockIdx.x - A.blk0[t], nb = A.blk0[t + 1] - A.blk0[t];
  const int nq = L.cs >> 2, C = L.C, kind = L.kind;
  const int64_t nquads = L.M * nq;
  const float* __restrict__ a = L.a;
  const float* __restrict__ b = L.b;
  float* __restrict__ da = L.da;
  const float g = A.gout[t][0] * L.scale;
  for (int64_t i = (int64_t)lb * 256 + threadIdx.x; i < nquads; i += (int64_t)nb * 256) {
    const int c = (int)(i % nq) * 4;
    const f4 av = *reinterpret_cast<const f4*>(a + i * 4);
    f4 bv = {0.f, 0.f, 0.f, 0.f};
    if (b) bv = *reinterpret_cast<const f4*>(b + i * 4);
    f4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = c + e < C ? g * cat::loss_grad(kind, av[e], bv[e], L.target) : 0.f;
    *reinterpret_cast<f4*>(da + i * 4) = o;
  }
}

int fwd_nb(const cat_loss_term_t& L) {      // cat_loss_fwd's grid: 1024 quads per workgroup, at most 1024 workgroups
  const int64_t b = (L.M * (L.cs / 4) + 1023) / 1024;
  return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}
int bwd_nb(const cat_loss_term_t& L) { return cat::ew_grid(L.M * (L.cs / 4), 4096); }

int check_terms(const cat_loss_term_t* terms, int T, const char* what) {
  CAT_REQUIRE(terms && T >= 1, "%s: empty table", what);
  for (int t = 0; t < T; ++t) {
    const cat_loss_term_t& L = terms[t];
    CAT_REQUIRE(L.a && L.kind >= 0 && L.kind <= CAT_LOSS_MEAN && L.M >= 1 && L.C >= 1 && L.cs % 4 == 0 && L.cs >= L.C, "%s: term %d: bad arguments", what, t);
    CAT_REQUIRE((L.kind != CAT_LOSS_L1 && L.kind != CAT_LOSS_MSE) || L.b, "%s: term %d: kind %d needs a second tensor", what, t, L.kind);
  }
  return 0;
}

}  // namespace

extern "C" {

size_t cat_loss_multi_ws_bytes(const cat_loss_term_t* terms, int T) {
  size_t n = 0;
  for (int t = 0; terms && t < T; ++t) n += (size_t)fwd_nb(terms[t]);
  return (n ? n : 1) * sizeof(float);
}

int cat_loss_multi_fwd(const cat_loss_term_t* terms, int T, float* out, void* ws, cat_stream_t stream) {
  if (int e = check_terms(terms, T, "loss_multi")) return e;
  CAT_REQUIRE(out && ws, "loss_multi: out / ws missing");
  double bytes = 0.0;
  for (int t = 0; t < T; ++t) bytes += 4.0 * terms[t].M * terms[t].cs * (terms[t].b ? 2 : 1);
  cat::ProfScope prof("loss_multi", 0.0, bytes, stream);
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)ws;
  for (int t0 = 0; t0 < T; t0 += CAT_LOSS_MULTI_MAX) {      // more terms than the table holds: one launch pair per chunk
    MultiArgs A = {};
    A.T = T - t0 < CAT_LOSS_MULTI_MAX ? T - t0 : CAT_LOSS_MULTI_MAX;
    for (int t = 0; t < A.T; ++t) {
      A.term[t] = terms[t0 + t];
      A.blk0[t + 1] = A.blk0[t] + fwd_nb(A.term[t]);
    }
    loss_multi_partial_kernel<<<A.blk0[A.T], 256, 0, s>>>(A, part);
    loss_multi_final_kernel<<<A.T, 256, 0, s>>>(A, part, out + t0);
    part += A.blk0[A.T];
  }
  return cat::check_launch("loss_multi_fwd");
}

int cat_loss_multi_bwd(const cat_loss_term_t* terms, int T, const float* const* gout, cat_stream_t stream) {
  if (int e = check_terms(terms, T, "loss_multi bwd")) return e;
  CAT_REQUIRE(gout, "loss_multi bwd: gout missing");
  double bytes = 0.0;
  for (int t = 0; t < T; ++t)
    if (terms[t].da) bytes += 4.0 * terms[t].M * terms[t].cs * (terms[t].b ? 3 : 2);
  cat::ProfScope prof("loss_multi", 0.0, bytes, stream);
  hipStream_t s = (hipStream_t)stream;
  MultiArgs A = {};
  for (int t = 0; t <= T; ++t) {
    if (t < T && terms[t].da) {
      CAT_REQUIRE(gout[t], "loss_multi bwd: term %d has da but no gout", t);
      A.term[A.T] = terms[t];
      A.term[A.T].scale = terms[t].scale / (float)((double)terms[t].M * terms[t].C);
      A.gout[A.T] = gout[t];
      A.blk0[A.T + 1] = A.blk0[A.T] + bwd_nb(terms[t]);
      ++A.T;
    }
    if (A.T == CAT_LOSS_MULTI_MAX || (t == T && A.T > 0)) {
      loss_multi_bwd_kernel<<<A.blk0[A.T], 256, 0, s>>>(A);
      A = MultiArgs{};
    }
  }
  return cat::check_launch("loss_multi_bwd");
}

}  // extern "C"
