// Kernel-alignment (KA) distillation loss and the scalar GAN / reconstruction losses, gfx950.
//
// KA(X, Y) = <Gx, Gy> / sqrt(<Gx,Gx> <Gy,Gy>),  Gx = X X^T (N x N over the batch), utils/common.py:38-46.
// The Gram is a pure HBM stream: N rows of D = C*H*W floats are read once.  Each wave owns a contiguous slice of D
// and accumulates the 16x16 Gram tiles with v_mfma_f32_16x16x4_f32 where BOTH operands are the same register
// (A[i][k] = B[k][i] = X[i][k]), so the matrix pipe does the N^2 work while the lanes only issue float4 loads:
// lane l loads X[row = l&15][k0 + 4*(l>>4) .. +3]  (4 lanes x 16 B = 64 contiguous bytes per row per load).
// Partials are written per workgroup and reduced by a single finalize block (deterministic).
// Backward: dX = gout * 2 * Cx X with the N x N matrix Cx = Gy/sqrt(sxx syy) - sxy Gx/(sxx^1.5 syy^0.5).
// Sharded form (cat_ka_sharded_*): the batch is cut like torch.chunk(batch, S) into shards of P = ceil(N / S) consecutive rows (the last may be
// short) and every kernel takes the shard from blockIdx.y -- the KA of each shard's own Gram pair, as S data-parallel replicas compute
// it, summed or averaged by one more single-block launch.  One shard (gridDim.y == 1) is the plain form, launch for launch.
#include "common.h"

namespace {
using cat::cdiv;

constexpr int KA_MAXN = 64;

template <int NT>
__global__ __launch_bounds__(256) void gram_kernel(const float* __restrict__ X, int64_t D, int Ntot, int P, float* __restrict__ part,
                                                   int64_t chunk) {
  // part: [gridDim.y][gridDim.x][NT*16][NT*16]; shard blockIdx.y = rows [y * P, min(Ntot, (y + 1) * P))
  const int N = min(P, Ntot - (int)blockIdx.y * P);
  X += (int64_t)blockIdx.y * P * D;
  part += (int64_t)blockIdx.y * gridDim.x * (NT * 16) * (NT * 16);
  __shared__ float red[4][NT * NT][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int64_t kbeg = ((int64_t)blockIdx.x * 4 + wave) * chunk;
  const int64_t kend = kbeg + chunk < D ? kbeg + chunk : D;
  f4 acc[NT][NT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
  const float* rowp[NT];
  bool rv[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int r = i * 16 + lr;
    rv[i] = r < N;
    rowp[i] = X + (int64_t)(rv[i] ? r : 0) * D + lq * 4;
  }
  for (int64_t k = kbeg; k < kend; k += 16) {
    f4 v[NT];
    const bool kv = k + lq * 4 < kend;  // chunk and D are multiples of 4
#pragma unroll
    for (int i = 0; i < NT; ++i) v[i] = (rv[i] && kv) ? *reinterpret_cast<const f4*>(rowp[i] + k) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[i][t], v[j][t], acc[i][j], 0, 0, 0);
  }
  // D[row = lq*4 + rg][col = lr] per tile -> LDS, then sum the 4 waves
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) red[wave][i * NT + j][(lq * 4 + rg) * 16 + lr] = acc[i][j][rg];
  __syncthreads();
  constexpr int NN = NT * 16;
  float* dst = part + (int64_t)blockIdx.x * NN * NN;
  for (int e = tid; e < NT * NT * 256; e += 256) {
    const int tile = e >> 8, o = e & 255;
    const float s = red[0][tile][o] + red[1][tile][o] + red[2][tile][o] + red[3][tile][o];
    const int ti = tile / NT, tj = tile - ti * NT;
    dst[(ti * 16 + (o >> 4)) * NN + tj * 16 + (o & 15)] = s;
  }
}

// ws layout (floats): G shard heads of hs = 4 + 2 * P * P floats, each [0..3] sxy, sxx, syy, ka | Gx[N*N] | Gy[N*N] (N = the shard's rows), then
// partX[G][nbx][NN*NN] | partY[G][nby][NN*NN]
// stage 1: Gx / Gy entries = sum of the per-workgroup partials; 16 entries x 16 partial-lanes per workgroup, four independent loads per lane and
// step, lanes combined pairwise through LDS in a fixed order (round 6: 64 entries x 4 lanes = 4 workgroups walked 2 x 128 dependent loads
// per lane: 43 us per loss term for 2 MB of partials)
__global__ __launch_bounds__(256) void ka_gram_reduce_kernel(float* __restrict__ ws, int Ntot, int P, int NN, int nbx, int nby) {
  __shared__ float red[2][256];
  const int sh = blockIdx.y, G = gridDim.y, N = min(P, Ntot - sh * P);
  const int64_t hs = 4 + 2 * (int64_t)P * P;
  float* Gx = ws + sh * hs + 4;
  float* Gy = Gx + N * N;
  const float* px = ws + G * hs + (int64_t)sh * nbx * NN * NN;
  const float* py = ws + G * hs + (int64_t)G * nbx * NN * NN + (int64_t)sh * nby * NN * NN;
  const int e = blockIdx.x * 16 + (threadIdx.x & 15), zl = threadIdx.x >> 4;
  float gx = 0.f, gy = 0.f;
  if (e < N * N) {
    const int i = e / N, j = e - i * N;
    const int64_t zs = (int64_t)NN * NN;
    const float* sx = px + i * NN + j;
    const float* sy = py + i * NN + j;
    int b = zl;
    for (; b + 48 < nbx; b += 64) {
      const float v0 = sx[b * zs], v1 = sx[(b + 16) * zs], v2 = sx[(b + 32) * zs], v3 = sx[(b + 48) * zs];
      gx += v0;
      gx += v1;
      gx += v2;
      gx += v3;
    }
    for (; b < nbx; b += 16) gx += sx[b * zs];
    b = zl;
    for (; b + 48 < nby; b += 64) {
      const float v0 = sy[b * zs], v1 = sy[(b + 16) * zs], v2 = sy[(b + 32) * zs], v3 = sy[(b + 48) * zs];
      gy += v0;
      gy += v1;
      gy += v2;
      gy += v3;
    }
    for (; b < nby; b += 16) gy += sy[b * zs];
  }
  red[0][threadIdx.x] = gx;
  red[1][threadIdx.x] = gy;
  __syncthreads();
#pragma unroll
  for (int st = 8; st >= 1; st >>= 1) {
    if (zl < st) {
      red[0][threadIdx.x] += red[0][threadIdx.x + st * 16];
      red[1][threadIdx.x] += red[1][threadIdx.x + st * 16];
    }
    __syncthreads();
  }
  if (zl == 0 && e < N * N) {
    Gx[e] = red[0][threadIdx.x];
    Gy[e] = red[1][threadIdx.x];
  }
}

// stage 2: ws[0..3] = sxy, sxx, syy, ka
__global__ __launch_bounds__(256) void ka_finalize_kernel(float* __restrict__ ws, int Ntot, int P, float* __restrict__ out) {
  __shared__ float red[3][256];
  const int N = min(P, Ntot - (int)blockIdx.x * P);
  ws += blockIdx.x * (4 + 2 * (int64_t)P * P);
  const float* Gx = ws + 4;
  const float* Gy = Gx + N * N;
  float sxy = 0.f, sxx = 0.f, syy = 0.f;
  for (int e = threadIdx.x; e < N * N; e += 256) {
    const float gx = Gx[e], gy = Gy[e];
    sxy += gx * gy;
    sxx += gx * gx;
    syy += gy * gy;
  }
  red[0][threadIdx.x] = sxy;
  red[1][threadIdx.x] = sxx;
  red[2][threadIdx.x] = syy;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
      red[2][threadIdx.x] += red[2][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float a = red[0][0], b = red[1][0], c = red[2][0];
    const float ka = a / sqrtf(b * c);
    ws[0] = a;
    ws[1] = b;
    ws[2] = c;
    ws[3] = ka;
    if (out) out[0] = ka;
  }
}

// out[0] = scale * (ka_0 + ka_1 + ...) in shard order: the sum of the replicas' terms, or their mean
__global__ void ka_combine_kernel(const float* __restrict__ ws, int G, int64_t hs, float scale, float* __restrict__ out) {
  if (threadIdx.x != 0) return;
  float s = 0.f;
  for (int g = 0; g < G; ++g) s += ws[g * hs + 3];
  out[0] = s * scale;
}

// dX[i][k] = gout * 2 * sum_j Cx[i][j] X[j][k]; one lane per float4 column, 8 output rows at a time.
__global__ __launch_bounds__(256) void ka_bwd_kernel(const float* __restrict__ X, int64_t D, int Ntot, int P, float gscale,
                                                     const float* __restrict__ gout, const float* __restrict__ ws, float* __restrict__ dX) {
  __shared__ float C[KA_MAXN * KA_MAXN];
  const int N = min(P, Ntot - (int)blockIdx.y * P);      // shard blockIdx.y: its rows of X / dX, its head of ws
  X += (int64_t)blockIdx.y * P * D;
  dX += (int64_t)blockIdx.y * P * D;
  ws += blockIdx.y * (4 + 2 * (int64_t)P * P);
  const float sxy = ws[0], sxx = ws[1], syy = ws[2];
  const float* Gx = ws + 4;
  const float* Gy = Gx + N * N;
  const float g = gout[0] * gscale;
  const float ca = g / sqrtf(sxx * syy), cb = g * sxy / (sxx * sqrtf(sxx * syy));
  for (int e = threadIdx.x; e < N * N; e += 256) C[e] = ca * Gy[e] - cb * Gx[e];
  __syncthreads();
  const int64_t nq = D / 4;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
    for (int i0 = 0; i0 < N; i0 += 8) {
      f4 acc[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = f4{0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < N; ++j) {
        const f4 xv = *reinterpret_cast<const f4*>(X + (int64_t)j * D + q * 4);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float c = i0 + i < N ? C[(i0 + i) * N + j] : 0.f;
          acc[i] += xv * c;
        }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (i0 + i < N) *reinterpret_cast<f4*>(dX + (int64_t)(i0 + i) * D + q * 4) = acc[i];
    }
  }
}

struct GramPlan { int NT, NN, nb; int64_t chunk; };
GramPlan gram_plan(int N, int64_t D) {
  GramPlan p;
  p.NT = cdiv(N, 16);
  p.NN = p.NT * 16;
  int64_t nb = D / (4 * 512);  // >= 512 floats of every row per wave
  if (nb > 512) nb = 512;
  if (nb < 1) nb = 1;
  p.nb = (int)nb;
  p.chunk = ((D + (int64_t)p.nb * 4 - 1) / ((int64_t)p.nb * 4) + 15) / 16 * 16;
  return p;
}
constexpr int KA_MAXNB = 512;

// the Grams of G shards of P rows (the last may be short) of the N rows of X: one launch
int launch_gram(const float* X, int64_t D, int N, int P, int G, float* part, const GramPlan& p, hipStream_t s) {
  const dim3 grid(p.nb, G);
  switch (p.NT) {
    case 1: gram_kernel<1><<<grid, 256, 0, s>>>(X, D, N, P, part, p.chunk); break;
    case 2: gram_kernel<2><<<grid, 256, 0, s>>>(X, D, N, P, part, p.chunk); break;
    case 3: gram_kernel<3><<<grid, 256, 0, s>>>(X, D, N, P, part, p.chunk); break;
    default: gram_kernel<4><<<grid, 256, 0, s>>>(X, D, N, P, part, p.chunk); break;
  }
  return cat::check_launch("ka_gram");
}

// forward and backward of G shards of P rows each; G == 1, P == N is the unsharded form
int ka_fwd(const float* X, int64_t Dx, const float* Y, int64_t Dy, int N, int P, int G, float scale, float* out, void* ws, hipStream_t s) {
  const GramPlan px = gram_plan(P, Dx), py = gram_plan(P, Dy);
  float* w = (float*)ws;
  const int64_t hs = 4 + 2 * (int64_t)P * P;
  float* partx = w + G * hs;
  float* party = partx + (int64_t)G * px.nb * px.NN * px.NN;
  if (int e = launch_gram(X, Dx, N, P, G, partx, px, s)) return e;
  if (int e = launch_gram(Y, Dy, N, P, G, party, py, s)) return e;
  ka_gram_reduce_kernel<<<dim3(cdiv(P * P, 16), G), 256, 0, s>>>(w, N, P, px.NN, px.nb, py.nb);
  ka_finalize_kernel<<<G, 256, 0, s>>>(w, N, P, G == 1 ? out : nullptr);
  if (G > 1) ka_combine_kernel<<<1, 64, 0, s>>>(w, G, hs, scale, out);
  return cat::check_launch("ka_finalize");
}

int ka_bwd(const float* X, int64_t Dx, int N, int P, int G, float scale, const float* gout, const void* ws, float* dX, hipStream_t s) {
  int64_t nb = (Dx / 4 + 255) / 256;
  if (nb > 4096) nb = 4096;
  ka_bwd_kernel<<<dim3((int)nb, G), 256, 0, s>>>(X, Dx, N, P, 2.f * scale, gout, (const float*)ws, dX);
  return cat::check_launch("ka_bwd");
}

// torch.chunk(batch of N, S): P rows per shard, G = the number of shards that hold any
void ka_shards(int N, int S, int& P, int& G) {
  P = cdiv(N, S);
  G = cdiv(N, P);
}

// ------------------------------------------------------------------------------------------------ scalar losses
__global__ __launch_bounds__(256) void loss_partial_kernel(int kind, const float* __restrict__ a, const float* __restrict__ b, float t,
                                                           int64_t nquads, int nq, int C, float* __restrict__ part) {
  __shared__ float red[4];
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nquads; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % nq) * 4;
    const f4 av = *reinterpret_cast<const f4*>(a + i * 4);
    f4 bv = {0.f, 0.f, 0.f, 0.f};
    if (b) bv = *reinterpret_cast<const f4*>(b + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c + e < C) s += cat::loss_term(kind, av[e], bv[e], t);
  }
  s = cat::wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ __launch_bounds__(256) void loss_final_kernel(const float* __restrict__ part, int nb, float inv_count, float* __restrict__ out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) s += part[i];
  s = cat::wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (red[0] + red[1] + red[2] + red[3]) * inv_count;
}
__global__ __launch_bounds__(256) void loss_bwd_kernel(int kind, const float* __restrict__ a, const float* __restrict__ b, float t,
                                                       int64_t nquads, int nq, int C, const float* __restrict__ gout, float scale,
                                                       float* __restrict__ da) {
  const float g = gout[0] * scale;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nquads; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % nq) * 4;
    const f4 av = *reinterpret_cast<const f4*>(a + i * 4);
    f4 bv = {0.f, 0.f, 0.f, 0.f};
    if (b) bv = *reinterpret_cast<const f4*>(b + i * 4);
    f4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = c + e < C ? g * cat::loss_grad(kind, av[e], bv[e], t) : 0.f;
    *reinterpret_cast<f4*>(da + i * 4) = o;
  }
}

int loss_nb(int64_t nquads) {
  int64_t b = (nquads + 1023) / 1024;
  return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

}  // namespace

extern "C" {

size_t cat_ka_ws_bytes(int N) {
  const int NN = cdiv(N, 16) * 16;
  return (size_t)(4 + 2 * N * N + 2 * (size_t)KA_MAXNB * NN * NN) * sizeof(float);
}

int cat_ka_fwd(const float* X, int64_t Dx, const float* Y, int64_t Dy, int N, float* out, void* ws, cat_stream_t stream) {
  CAT_REQUIRE(N >= 1 && N <= KA_MAXN, "ka: batch N=%d outside [1,%d]", N, KA_MAXN);
  CAT_REQUIRE(Dx % 4 == 0 && Dy % 4 == 0 && ws, "ka: row lengths must be multiples of 4");
  cat::ProfScope prof("ka_fwd", 2.0 * N * N * (double)(Dx + Dy), 4.0 * N * (double)(Dx + Dy), stream);
  return ka_fwd(X, Dx, Y, Dy, N, N, 1, 1.f, out, ws, (hipStream_t)stream);
}

int cat_ka_bwd(const float* X, int64_t Dx, int N, const float* gout, const void* ws, float* dX, cat_stream_t stream) {
  CAT_REQUIRE(N >= 1 && N <= KA_MAXN && Dx % 4 == 0, "ka bwd: bad arguments");
  cat::ProfScope prof("ka_bwd", 2.0 * N * N * (double)Dx, 8.0 * N * (double)Dx, stream);
  return ka_bwd(X, Dx, N, N, 1, 1.f, gout, ws, dX, (hipStream_t)stream);
}

size_t cat_ka_sharded_ws_bytes(int N, int S) {
  if (N < 1 || S < 1) return 0;
  int P, G;
  ka_shards(N, S, P, G);
  const int NN = cdiv(P, 16) * 16;
  return (size_t)G * (4 + 2 * (size_t)P * P + 2 * (size_t)KA_MAXNB * NN * NN) * sizeof(float);
}

int cat_ka_sharded_fwd(const float* X, int64_t Dx, const float* Y, int64_t Dy, int N, int S, int mean, float* out, void* ws,
                       cat_stream_t stream) {
  CAT_REQUIRE(N >= 1 && S >= 1, "ka sharded: N=%d rows in S=%d shards", N, S);
  int P, G;
  ka_shards(N, S, P, G);
  CAT_REQUIRE(P <= KA_MAXN, "ka sharded: %d rows per shard outside [1,%d]", P, KA_MAXN);
  CAT_REQUIRE(Dx % 4 == 0 && Dy % 4 == 0 && ws, "ka: row lengths must be multiples of 4");
  cat::ProfScope prof("ka_fwd", 2.0 * N * P * (double)(Dx + Dy), 4.0 * N * (double)(Dx + Dy), stream);
  return ka_fwd(X, Dx, Y, Dy, N, P, G, mean ? 1.f / (float)G : 1.f, out, ws, (hipStream_t)stream);
}

int cat_ka_sharded_bwd(const float* X, int64_t Dx, int N, int S, int mean, const float* gout, const void* ws, float* dX,
                       cat_stream_t stream) {
  CAT_REQUIRE(N >= 1 && S >= 1 && Dx % 4 == 0 && ws, "ka sharded bwd: bad arguments");
  int P, G;
  ka_shards(N, S, P, G);
  CAT_REQUIRE(P <= KA_MAXN, "ka sharded bwd: %d rows per shard outside [1,%d]", P, KA_MAXN);
  cat::ProfScope prof("ka_bwd", 2.0 * N * P * (double)Dx, 8.0 * N * (double)Dx, stream);
  return ka_bwd(X, Dx, N, P, G, mean ? 1.f / (float)G : 1.f, gout, ws, dX, (hipStream_t)stream);
}

size_t cat_loss_ws_bytes(int64_t M) { (void)M; return 1024 * sizeof(float); }

int cat_loss_fwd(int kind, const float* a, const float* b, float target, int64_t M, int C, int cs, float* out, void* ws,
                 cat_stream_t stream) {
  CAT_REQUIRE(kind >= 0 && kind <= CAT_LOSS_MEAN && cs % 4 == 0 && cs >= C && ws, "loss: bad arguments");
  CAT_REQUIRE((kind != CAT_LOSS_L1 && kind != CAT_LOSS_MSE) || b, "loss: kind %d needs a second tensor", kind);
  const int64_t nquads = M * (cs / 4);
  const int nb = loss_nb(nquads);
  cat::ProfScope prof("loss", 0.0, 4.0 * M * cs * (b ? 2 : 1), stream);
  hipStream_t s = (hipStream_t)stream;
  loss_partial_kernel<<<nb, 256, 0, s>>>(kind, a, b, target, nquads, cs / 4, C, (float*)ws);
  loss_final_kernel<<<1, 256, 0, s>>>((const float*)ws, nb, 1.f / (float)((double)M * C), out);
  return cat::check_launch("loss_fwd");
}

int cat_loss_bwd(int kind, const float* a, const float* b, float target, int64_t M, int C, int cs, const float* gout, float scale,
                 float* da, cat_stream_t stream) {
  CAT_REQUIRE(kind >= 0 && kind <= CAT_LOSS_MEAN && cs % 4 == 0 && cs >= C, "loss: bad arguments");
  const int64_t nquads = M * (cs / 4);
  int64_t nb = (nquads + 255) / 256;
  if (nb > 8192) nb = 8192;
  cat::ProfScope prof("loss", 0.0, 4.0 * M * cs * (b ? 3 : 2), stream);
  loss_bwd_kernel<<<(int)nb, 256, 0, (hipStream_t)stream>>>(kind, a, b, target, nquads, cs / 4, C, gout, scale / (float)((double)M * C), da);
  return cat::check_launch("loss_bwd");
}

}  // extern "C"
