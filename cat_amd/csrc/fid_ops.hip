// The tail of FID (metric/fid_score.py:217-275 and np.mean / np.cov before it) on the GPU, float64 on v_mfma_f64_16x16x4_f64, gfx950.
//
//   cat_fid_mean / cat_fid_stats   column means and the covariance np.cov(F, rowvar=False) of float32 features: centre first, then
//                                  Xc^T Xc / (n - 1).  The rows are widened and the mean subtracted on their way into LDS; only the 64 x 64
//                                  tiles on or above the diagonal are computed, every value is written to (i, j) and (j, i): sigma is
//                                  symmetric bit for bit.
//   cat_gemm_f64                   C = alpha * A * op(B) + beta_eye * I, row-major float64, any m, n, k >= 1: the one product the coupled
//                                  Newton-Schulz iteration for the matrix square root is made of (T = 1.5 I - 0.5 Z Y, Y <- Y T, Z <- T Z).
//   cat_f64_trace_sumsq, cat_f64_symmetrize, cat_fid_center   the small float64 kernels between the products.
//
// Tiles: mfma_f64.h.  An operand whose K index is contiguous in memory lies in LDS as KContig, one whose K index is the slow one as KMajor.
// Rows, columns and K indices beyond the matrix are staged as zeros.
//
// Order of every sum is fixed (the MFMA's walk over K, per-thread walks, fixed LDS trees, a fixed walk over per-block partials): no atomics,
// the same inputs give the same bits.  Every output element is written.
#include "mfma_f64.h"

namespace {

using cat::d4;

constexpr int FID_BK = cat::BK;          // K indices per staging step
constexpr int FID_CT = 64;               // covariance tile
using CovLds = cat::KMajor<FID_CT>;      // both operands of the covariance tile: the K index is the row of F
constexpr int FID_SS_ROWS = 16;          // rows per block of the sum-of-squares pass

// ------------------------------------------------------------------------------------------------------------------ column means
// grid cdiv(d, 64); 256 threads = 64 columns x 4 row groups; group g adds rows g, g + 4, ... in order, the 4 groups are added in order.
__global__ __launch_bounds__(256) void fid_mean_kernel(const float* __restrict__ F, int n, int d, double* __restrict__ mu) {
  __shared__ double part[4][64];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6, col = blockIdx.x * 64 + c;
  double s = 0.0;
  if (col < d)
    for (int r = g; r < n; r += 4) s += (double)F[(int64_t)r * d + col];
  part[g][c] = s;
  __syncthreads();
  if (g == 0 && col < d) mu[col] = (((part[0][c] + part[1][c]) + part[2][c]) + part[3][c]) / (double)n;
}

// ------------------------------------------------------------------------------------------------------------------ covariance
struct CovQuad {
  f4 v;
  bool in;      // a row of F (beyond n: zeros, NOT minus the mean)
};

__device__ __forceinline__ CovQuad cov_fetch(const float* __restrict__ F, int n, int d, int row, int col) {
  if (row >= n || col >= d) return CovQuad{f4{0.f, 0.f, 0.f, 0.f}, false};
  return CovQuad{*reinterpret_cast<const f4*>(F + (int64_t)row * d + col), true};
}

__device__ __forceinline__ void cov_stage(double* dst, const CovQuad& q, const double* m) {
#pragma unroll
  for (int e = 0; e < 4; ++e) dst[e] = q.in ? (double)q.v[e] - m[e] : 0.0;
}

// grid (T, T), T = cdiv(d, 64); blocks below the diagonal leave at once.  The K index is the row of F: 32 rows x 64 columns per operand
// and step = 512 float quads, two per thread (rows t >> 4 and (t >> 4) + 16, column quad t & 15, whose four means stay in registers).
__global__ __launch_bounds__(256) void fid_cov_kernel(const float* __restrict__ F, const double* __restrict__ mu, int n, int d,
                                                      double* __restrict__ sigma) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (tj < ti) return;
  __shared__ __attribute__((aligned(16))) double As[CovLds::SIZE];
  __shared__ __attribute__((aligned(16))) double Bs[CovLds::SIZE];
  const int t = threadIdx.x;
  const cat::TileCoords c(t);
  const int sr = t >> 4, sc = (t & 15) * 4;
  const int ca = ti * FID_CT + sc, cb = tj * FID_CT + sc;
  double ma[4], mb[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    ma[e] = ca < d ? mu[ca + e] : 0.0;      // d % 4 == 0: a quad is inside or outside as a whole
    mb[e] = cb < d ? mu[cb + e] : 0.0;
  }
  d4 acc[2][2] = {};
  CovQuad a0, a1, b0, b1;
  cat::pipeline((n + FID_BK - 1) / FID_BK,
      [&] {
        cov_stage(As + CovLds::index(sc, sr), a0, ma);
        cov_stage(As + CovLds::index(sc, sr + 16), a1, ma);
        cov_stage(Bs + CovLds::index(sc, sr), b0, mb);
        cov_stage(Bs + CovLds::index(sc, sr + 16), b1, mb);
      },
      [&](int kc) {
        const int r = kc * FID_BK + sr;
        a0 = cov_fetch(F, n, d, r, ca);
        a1 = cov_fetch(F, n, d, r + 16, ca);
        b0 = cov_fetch(F, n, d, r, cb);
        b1 = cov_fetch(F, n, d, r + 16, cb);
      },
      [&] { cat::mma_step(acc, As, Bs, CovLds(), CovLds(), c); });
  const double inv = 1.0 / (double)(n - 1);
  cat::for_each_acc(acc, c, [=](int, int, int, int lrow, int lcol, double g) {
    const int row = ti * FID_CT + lrow, col = tj * FID_CT + lcol;
    if (row < d && col < d && col >= row) {      // the diagonal tile's lower half is the mirror of its upper half
      const double v = g * inv;
      sigma[(int64_t)row * d + col] = v;
      if (col > row) sigma[(int64_t)col * d + row] = v;
    }
  });
}

// ------------------------------------------------------------------------------------------------------------------ GEMM
// One workgroup owns a (32 TM) x (32 TM) tile of C, each wave TM x TM MFMA tiles.  A: [m][k], K contiguous.  B: transB ? [n][k] : [k][n].
// Staging reads single doubles, consecutive threads consecutive addresses, so no alignment or leading-dimension rule is needed.
template <int TM>
__global__ __launch_bounds__(256) void fid_gemm_kernel(const double* __restrict__ A, int64_t lda, const double* __restrict__ B, int64_t ldb,
                                                       int transB, double* __restrict__ C, int64_t ldc, int m, int n, int k, double alpha,
                                                       double beta_eye) {
  constexpr int BT = 32 * TM;                      // tile rows = tile columns
  constexpr int NE = BT * FID_BK / 256;            // doubles per thread, operand and step
  using LK = cat::KContig<BT>;                     // A, and B if transB
  using LN = cat::KMajor<BT>;                      // B otherwise
  __shared__ __attribute__((aligned(16))) double As[LK::SIZE];
  __shared__ __attribute__((aligned(16))) double Bs[LK::SIZE > LN::SIZE ? LK::SIZE : LN::SIZE];
  const int t = threadIdx.x;
  const cat::TileCoords c(t);
  const int row0 = blockIdx.y * BT, col0 = blockIdx.x * BT;
  // K-contiguous operand: element e = t + 256 i is row e >> 5, k index e & 31.  [k][n] operand: k index e / BT, column e % BT.
  const int ar = t >> 5, ak = t & 31;
  const int bk = transB ? ak : t / BT, bc = transB ? ar : t % BT;
  constexpr int BSTEP = 256 / BT;                  // k indices between a thread's elements of a [k][n] operand
  const cat::Strided lb{transB ? LK::LD : 1, transB ? 1 : LN::LD};      // LDS strides of B's column and k index

  auto fetch_a = [&](int k0, int i) -> double {
    const int r = row0 + ar + 8 * i, kk = k0 + ak;
    return (r < m && kk < k) ? A[(int64_t)r * lda + kk] : 0.0;
  };
  auto fetch_b = [&](int k0, int i) -> double {
    if (transB) {
      const int c = col0 + bc + 8 * i, kk = k0 + bk;
      return (c < n && kk < k) ? B[(int64_t)c * ldb + kk] : 0.0;
    }
    const int c = col0 + bc, kk = k0 + bk + BSTEP * i;
    return (c < n && kk < k) ? B[(int64_t)kk * ldb + c] : 0.0;
  };

  d4 acc[TM][TM] = {};
  double va[NE], vb[NE];
  cat::pipeline((k + FID_BK - 1) / FID_BK,
      [=, &va, &vb] {      // scalars by value (mfma_f64.h): by reference the two B stores become one with a selected address
#pragma unroll
        for (int i = 0; i < NE; ++i) {
          As[LK::index(ar + 8 * i, ak)] = va[i];
          if (transB)
            Bs[LK::index(bc + 8 * i, bk)] = vb[i];
          else
            Bs[LN::index(bc, bk + BSTEP * i)] = vb[i];
        }
      },
      [&](int kc) {
#pragma unroll
        for (int i = 0; i < NE; ++i) {
          va[i] = fetch_a(kc * FID_BK, i);
          vb[i] = fetch_b(kc * FID_BK, i);
        }
      },
      [&] { cat::mma_step(acc, As, Bs, LK(), lb, c); });
  cat::for_each_acc(acc, c, [=](int, int, int, int lrow, int lcol, double g) {
    const int row = row0 + lrow, col = col0 + lcol;
    if (row < m && col < n) C[(int64_t)row * ldc + col] = alpha * g + (row == col ? beta_eye : 0.0);
  });
}

// ------------------------------------------------------------------------------------------------------------------ small kernels
// a block's 256 values added in a fixed tree; the result is valid in thread 0
__device__ __forceinline__ double block_sum_256(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  return red[0];
}

// sum of squares of FID_SS_ROWS rows of a [rows][cols] matrix per block -> part[block]
__global__ __launch_bounds__(256) void fid_sumsq_kernel(const double* __restrict__ A, int rows, int cols, int64_t lda, double* __restrict__ part) {
  __shared__ double red[256];
  const int r0 = blockIdx.x * FID_SS_ROWS;
  double s = 0.0;
  for (int r = r0; r < r0 + FID_SS_ROWS && r < rows; ++r)
    for (int c = threadIdx.x; c < cols; c += 256) {
      const double v = A[(int64_t)r * lda + c];
      s += v * v;
    }
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// one block: *trace = the trace of A (if A is given), *sumsq = the partials added in order (NaN if there are none)
__global__ __launch_bounds__(256) void fid_finish_kernel(const double* __restrict__ A, int n, int64_t lda, const double* __restrict__ part, int P,
                                                         double* __restrict__ trace, double* __restrict__ sumsq) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  if (A) {
    double tr = 0.0;
    for (int i = t; i < n; i += 256) tr += A[(int64_t)i * lda + i];
    tr = block_sum_256(tr, red);
    if (t == 0) *trace = tr;
    __syncthreads();
  }
  double s = 0.0;
  for (int p = t; p < P; p += 256) s += part[p];
  s = block_sum_256(s, red);
  if (t == 0) *sumsq = part ? s : __builtin_nan("");
}

// out = scale * (A + A^T) / 2; out may be A itself (every pair is read and written by one thread)
__global__ __launch_bounds__(256) void fid_symmetrize_kernel(const double* A, int n, int64_t lda, double scale, double* out, int64_t ldo) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= n || j < i) return;
  const double v = scale * (0.5 * (A[(int64_t)i * lda + j] + A[(int64_t)j * lda + i]));
  out[(int64_t)i * ldo + j] = v;
  out[(int64_t)j * ldo + i] = v;
}

// one block per row: Xc = F - mu in float64, part[row] = the row's sum of squares
__global__ __launch_bounds__(256) void fid_center_kernel(const float* __restrict__ F, const double* __restrict__ mu, int d, double* __restrict__ Xc,
                                                         double* __restrict__ part) {
  __shared__ double red[256];
  const int64_t base = (int64_t)blockIdx.x * d;
  double s = 0.0;
  for (int c = threadIdx.x; c < d; c += 256) {
    const double v = (double)F[base + c] - mu[c];
    Xc[base + c] = v;
    s += v * v;
  }
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

int fid_check_features(const float* F, int n, int d, const char* what) {
  CAT_REQUIRE(F, "%s: null pointer", what);
  CAT_REQUIRE(n >= 1 && d >= 1 && n <= 1 << 24 && d <= 1 << 20, "%s: geometry (n=%d, d=%d)", what, n, d);
  return 0;
}

}  // namespace

extern "C" {

int cat_fid_mean(const float* F, int n, int d, double* mu, cat_stream_t stream) {
  if (int e = fid_check_features(F, n, d, "fid_mean")) return e;
  CAT_REQUIRE(mu, "fid_mean: null pointer");
  fid_mean_kernel<<<cat::cdiv(d, 64), 256, 0, (hipStream_t)stream>>>(F, n, d, mu);
  return cat::check_launch("fid_mean");
}

int cat_fid_stats(const float* F, int n, int d, double* mu, double* sigma, cat_stream_t stream) {
  if (int e = fid_check_features(F, n, d, "fid_stats")) return e;
  CAT_REQUIRE(mu && sigma, "fid_stats: null pointer");
  CAT_REQUIRE(n >= 2, "fid_stats: a covariance needs at least 2 rows (n=%d)", n);
  CAT_REQUIRE((d & 3) == 0, "fid_stats: the feature width must be a multiple of 4 (d=%d)", d);
  CAT_REQUIRE(((uintptr_t)F & 15) == 0, "fid_stats: the feature matrix must be 16-byte aligned");
  const int T = cat::cdiv(d, FID_CT);
  CAT_REQUIRE(T <= 65535, "fid_stats: feature width too large (d=%d)", d);
  const double np = (double)cat::round_up(n, FID_BK), dp = (double)T * FID_CT;
  cat::ProfScope prof("fid_stats", np * dp * (dp + FID_CT), 2.0 * 4.0 * n * (double)d + 8.0 * d * (double)d, stream);
  hipStream_t st = (hipStream_t)stream;
  fid_mean_kernel<<<cat::cdiv(d, 64), 256, 0, st>>>(F, n, d, mu);
  fid_cov_kernel<<<dim3(T, T), 256, 0, st>>>(F, mu, n, d, sigma);
  return cat::check_launch("fid_stats");
}

int cat_gemm_f64(const double* A, int lda, const double* B, int ldb, int transB, double* C, int ldc, int m, int n, int k, double alpha,
                 double beta_eye, cat_stream_t stream) {
  CAT_REQUIRE(A && B && C, "gemm_f64: null pointer");
  CAT_REQUIRE(m >= 1 && n >= 1 && k >= 1, "gemm_f64: geometry (m=%d, n=%d, k=%d)", m, n, k);
  CAT_REQUIRE(transB == 0 || transB == 1, "gemm_f64: transB must be 0 or 1 (%d)", transB);
  CAT_REQUIRE(lda >= k && ldb >= (transB ? k : n) && ldc >= n, "gemm_f64: leading dimensions (lda=%d, ldb=%d, ldc=%d) for m=%d, n=%d, k=%d", lda,
              ldb, ldc, m, n, k);
  CAT_REQUIRE(C != A && C != B, "gemm_f64: C must not alias an operand");
  cat::ProfScope prof("gemm_f64", 2.0 * m * (double)n * k, 8.0 * ((double)m * k + (double)k * n + (double)m * n), stream);
  hipStream_t st = (hipStream_t)stream;
  // 64 x 64 tiles once they give every compute unit a workgroup; below that 32 x 32 tiles, so that a 120-row problem still spreads
  // over the chip (120 x 2048: 4 x 64 workgroups instead of 2 x 32)
  const int64_t big = (int64_t)cat::cdiv(m, 64) * cat::cdiv(n, 64);
  if (big >= 256) {
    CAT_REQUIRE(cat::cdiv(m, 64) <= 65535, "gemm_f64: too many rows (m=%d)", m);
    fid_gemm_kernel<2><<<dim3(cat::cdiv(n, 64), cat::cdiv(m, 64)), 256, 0, st>>>(A, lda, B, ldb, transB, C, ldc, m, n, k, alpha, beta_eye);
  } else {
    fid_gemm_kernel<1><<<dim3(cat::cdiv(n, 32), cat::cdiv(m, 32)), 256, 0, st>>>(A, lda, B, ldb, transB, C, ldc, m, n, k, alpha, beta_eye);
  }
  return cat::check_launch("gemm_f64");
}

size_t cat_f64_trace_sumsq_ws_bytes(int n) {
  if (n <= 0) return 0;
  return (size_t)((n + FID_SS_ROWS - 1) / FID_SS_ROWS) * sizeof(double);
}

int cat_f64_trace_sumsq(const double* A, int n, int lda, int want_sumsq, double* out, double* ws, cat_stream_t stream) {
  CAT_REQUIRE(A && out, "trace_sumsq: null pointer");
  CAT_REQUIRE(n >= 1 && lda >= n, "trace_sumsq: geometry (n=%d, lda=%d)", n, lda);
  CAT_REQUIRE(!want_sumsq || ws, "trace_sumsq: the sum of squares needs its workspace");
  hipStream_t st = (hipStream_t)stream;
  const int P = cat::cdiv(n, FID_SS_ROWS);
  if (want_sumsq) fid_sumsq_kernel<<<P, 256, 0, st>>>(A, n, n, lda, ws);
  fid_finish_kernel<<<1, 256, 0, st>>>(A, n, lda, want_sumsq ? ws : nullptr, want_sumsq ? P : 0, out, out + 1);
  return cat::check_launch("trace_sumsq");
}

int cat_f64_symmetrize(const double* A, int n, int lda, double scale, double* out, int ldo, cat_stream_t stream) {
  CAT_REQUIRE(A && out, "symmetrize: null pointer");
  CAT_REQUIRE(n >= 1 && n <= 65535 && lda >= n && ldo >= n, "symmetrize: geometry (n=%d, lda=%d, ldo=%d)", n, lda, ldo);
  fid_symmetrize_kernel<<<dim3(cat::cdiv(n, 256), n), 256, 0, (hipStream_t)stream>>>(A, n, lda, scale, out, ldo);
  return cat::check_launch("symmetrize");
}

size_t cat_fid_center_ws_bytes(int n) { return n <= 0 ? 0 : (size_t)n * sizeof(double); }

int cat_fid_center(const float* F, const double* mu, int n, int d, double* Xc, double* sumsq, double* ws, cat_stream_t stream) {
  if (int e = fid_check_features(F, n, d, "fid_center")) return e;
  CAT_REQUIRE(mu && Xc && sumsq && ws, "fid_center: null pointer");
  hipStream_t st = (hipStream_t)stream;
  fid_center_kernel<<<n, 256, 0, st>>>(F, mu, d, Xc, ws);
  fid_finish_kernel<<<1, 256, 0, st>>>(nullptr, 0, 0, ws, n, nullptr, sumsq);
  return cat::check_launch("fid_center");
}

}  // extern "C"
