// The MMD tail of the kernel inception distance (metric/kid_score.py:184-281) on the GPU, float64 on v_mfma_f64_16x16x4_f64, gfx950.
//
// For every subset s of S the reference builds three m x m polynomial kernels K = (gamma * A B^T + coef0)^degree -- (X, X), (Y, Y), (X, Y), rows
// of the feature matrices picked by index tables -- and _mmd2_and_variance reads only sums of them.  kid_poly_panel_kernel computes those sums
// and never writes a K:
//
//   grid (P, 4, S): P = ceil(m / 64) row panels x 4 products (XX, YY, XY and YX, whose row sums are the COLUMN sums of K_XY) x S subsets.
//   One workgroup (the 64 x 64 tile of mfma_f64.h, TM = 2) owns 64 rows of one product and walks all P column chunks of 64.  Per chunk the
//   Gram block accumulates over the whole feature width: the gathered float32 rows are widened to float64 on their way into LDS, both
//   operands K-contiguous.  The epilogue raises every Gram value to K in registers and adds it to the lane's row sums / sum of squares; rows
//   and columns at or beyond m are staged as zeros AND masked out of the epilogue (K of a zero Gram value is coef0^degree, not 0).
//
// Float64 because mmd2 is a difference of order 1e-2 between means of order 1..10, and the variance estimate cancels harder still: a float32
// restatement differs from the reference by up to 8e-5 relative in the variance.
//
// Order of every sum is fixed (per lane over chunks, xor butterflies inside a wave, a fixed walk over LDS between waves, kid_finish_kernel's
// fixed walk over the per-panel partials): no atomics, results repeat bit for bit.  An index outside its feature matrix reads nothing and
// poisons its row with NaN instead.
#include "mfma_f64.h"

namespace {

using cat::d2;
using cat::d4;

constexpr int KID_BM = 64;             // rows (and columns) of a block
constexpr int KID_BK = cat::BK;        // feature columns per staging step
using KidLds = cat::KContig<KID_BM>;   // both operands: the feature index is contiguous
constexpr int KID_SCALARS = 4;         // trace K_XY, sum K_XX^2, sum K_YY^2, sum K_XY^2

struct KidRow {
  const float* p;   // the gathered feature row, or nullptr
  float fill;       // what a nullptr row stages: 0 beyond m, NaN for an index outside the matrix
};

__device__ __forceinline__ KidRow kid_row(const float* base, int n, int d, const int* tab, int r, int m) {
  if (r >= m) return KidRow{nullptr, 0.f};
  const int idx = tab[r];
  if ((unsigned)idx >= (unsigned)n) return KidRow{nullptr, __builtin_nanf("")};
  return KidRow{base + (int64_t)idx * d, 0.f};
}

__device__ __forceinline__ f4 kid_fetch(const KidRow& row, int k, int d) {
  if (k >= d) return f4{0.f, 0.f, 0.f, 0.f};
  if (!row.p) return f4{row.fill, row.fill, row.fill, row.fill};
  return *reinterpret_cast<const f4*>(row.p + k);
}

__device__ __forceinline__ void kid_stage(double* dst, const f4& v) {
  *reinterpret_cast<d2*>(dst) = d2{(double)v[0], (double)v[1]};
  *reinterpret_cast<d2*>(dst + 2) = d2{(double)v[2], (double)v[3]};
}

// out: [S][6 * m + 4] doubles = row sums K_XX | diag K_XX | row sums K_YY | diag K_YY | row sums K_XY | column sums K_XY | the 4 scalars.
// ws : [S][4][P] per-panel partials of the scalars.
__global__ __launch_bounds__(256) void kid_poly_panel_kernel(const float* __restrict__ X, int nx, const float* __restrict__ Y, int ny, int d,
                                                             const int* __restrict__ gi, const int* __restrict__ ri, int m, int P, double gamma,
                                                             double coef0, int degree, double* __restrict__ out, double* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) double As[KidLds::SIZE];
  __shared__ __attribute__((aligned(16))) double Bs[KidLds::SIZE];
  __shared__ double red[2 * KID_BM];
  __shared__ double dg[KID_BM];
  __shared__ double wred[4];
  const int t = threadIdx.x;
  const cat::TileCoords c(t);
  const int panel = blockIdx.x, prod = blockIdx.y, s = blockIdx.z;
  const bool ax = prod == 0 || prod == 2, bx = prod == 0 || prod == 3;
  const float* A = ax ? X : Y;
  const float* B = bx ? X : Y;
  const int na = ax ? nx : ny, nb = bx ? nx : ny;
  const int* ta = (ax ? gi : ri) + (int64_t)s * m;
  const int* tb = (bx ? gi : ri) + (int64_t)s * m;
  const int row0 = panel * KID_BM;
  // a thread stages quads q = t and t + 256 of the 64 x 8 quads of a step: row q >> 3, feature quad q & 7
  const int sr0 = t >> 3, sr1 = sr0 + 32, sk = (t & 7) * 4;
  const KidRow a0 = kid_row(A, na, d, ta, row0 + sr0, m), a1 = kid_row(A, na, d, ta, row0 + sr1, m);
  if (t < KID_BM) dg[t] = 0.0;
  const int nk = (d + KID_BK - 1) / KID_BK;
  double rs[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
  double sq = 0.0;
  for (int cb = 0; cb < P; ++cb) {
    const int col0 = cb * KID_BM;
    const KidRow b0 = kid_row(B, nb, d, tb, col0 + sr0, m), b1 = kid_row(B, nb, d, tb, col0 + sr1, m);
    d4 acc[2][2] = {};
    f4 va0, va1, vb0, vb1;
    cat::pipeline(nk,
        [&] {
          kid_stage(As + KidLds::index(sr0, sk), va0);
          kid_stage(As + KidLds::index(sr1, sk), va1);
          kid_stage(Bs + KidLds::index(sr0, sk), vb0);
          kid_stage(Bs + KidLds::index(sr1, sk), vb1);
        },
        [&](int kc) {
          const int k = kc * KID_BK + sk;
          va0 = kid_fetch(a0, k, d);
          va1 = kid_fetch(a1, k, d);
          vb0 = kid_fetch(b0, k, d);
          vb1 = kid_fetch(b1, k, d);
        },
        [&] { cat::mma_step(acc, As, Bs, KidLds(), KidLds(), c); });
    cat::for_each_acc(acc, c, [&](int i, int r, int, int lrow, int lcol, double g) {
      const int grow = row0 + lrow, gcol = col0 + lcol;
      const double v = gamma * g + coef0;
      double k = v;
      for (int e = 1; e < degree; ++e) k *= v;
      const bool in = grow < m && gcol < m;
      k = in ? k : 0.0;
      rs[i][r] += k;
      sq += k * k;
      if (in && grow == gcol) dg[lrow] = k;
    });
  }
  // row sums: the 16 lanes that share a row, then the two waves that share it
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double v = rs[i][r];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
      if (c.fr == 0) red[c.wj * KID_BM + c.wi * 32 + i * 16 + c.fk + 4 * r] = v;
    }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) sq += __shfl_xor(sq, o, 64);
  if (c.lane == 0) wred[c.wave] = sq;
  __syncthreads();
  double* o = out + (int64_t)s * (6 * (int64_t)m + KID_SCALARS);
  if (t < KID_BM && row0 + t < m) {
    const double sum = red[t] + red[KID_BM + t];
    const int r = row0 + t;
    if (prod == 0) {
      o[r] = sum;
      o[(int64_t)m + r] = dg[t];
    } else if (prod == 1) {
      o[2 * (int64_t)m + r] = sum;
      o[3 * (int64_t)m + r] = dg[t];
    } else if (prod == 2) {
      o[4 * (int64_t)m + r] = sum;
    } else {
      o[5 * (int64_t)m + r] = sum;
    }
  }
  if (t == 0 && prod < 3) {
    double* w = ws + (int64_t)s * KID_SCALARS * P;
    w[(int64_t)(prod + 1) * P + panel] = ((wred[0] + wred[1]) + wred[2]) + wred[3];
    if (prod == 2) {
      double tr = 0.0;
      for (int i = 0; i < KID_BM; ++i) tr += dg[i];
      w[panel] = tr;
    }
  }
}

// the 4 scalars of every subset: the per-panel partials added in panel order
__global__ __launch_bounds__(256) void kid_finish_kernel(const double* __restrict__ ws, int S, int m, int P, double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= S * KID_SCALARS) return;
  const int s = i / KID_SCALARS, q = i - s * KID_SCALARS;
  const double* w = ws + (int64_t)i * P;
  double v = 0.0;
  for (int p = 0; p < P; ++p) v += w[p];
  out[(int64_t)s * (6 * (int64_t)m + KID_SCALARS) + 6 * (int64_t)m + q] = v;
}

}  // namespace

extern "C" {

size_t cat_kid_poly_sums_ws_bytes(int S, int m) {
  if (S <= 0 || m <= 0) return 0;
  return (size_t)S * KID_SCALARS * (size_t)((m + KID_BM - 1) / KID_BM) * sizeof(double);
}

int cat_kid_poly_sums(const float* X, int nx, const float* Y, int ny, int d, const int* gi, const int* ri, int S, int m, double gamma,
                      double coef0, int degree, double* out, double* ws, cat_stream_t stream) {
  CAT_REQUIRE(X && Y && gi && ri && out && ws, "kid: null pointer");
  CAT_REQUIRE(nx > 0 && ny > 0 && d > 0 && m > 0, "kid: geometry (nx=%d, ny=%d, d=%d, m=%d)", nx, ny, d, m);
  CAT_REQUIRE((d & 3) == 0, "kid: the feature width must be a multiple of 4 (d=%d)", d);
  CAT_REQUIRE((((uintptr_t)X | (uintptr_t)Y) & 15) == 0, "kid: feature matrices must be 16-byte aligned");
  CAT_REQUIRE(S > 0 && S <= 65535, "kid: 1 <= n_subsets <= 65535 (S=%d)", S);
  CAT_REQUIRE(degree >= 1, "kid: degree must be an integer >= 1 (degree=%d)", degree);
  const int P = (m + KID_BM - 1) / KID_BM;
  CAT_REQUIRE(P <= 65535 && (int64_t)S * KID_SCALARS <= (int64_t)1 << 30, "kid: subset too large (m=%d)", m);
  const double gram = 2.0 * 4.0 * (double)S * (double)P * KID_BM * (double)P * KID_BM * (double)d;
  cat::ProfScope prof("kid_poly_sums", gram, 4.0 * ((double)nx + (double)ny) * d + 8.0 * (double)S * (6.0 * m + KID_SCALARS), stream);
  hipStream_t st = (hipStream_t)stream;
  kid_poly_panel_kernel<<<dim3(P, 4, S), 256, 0, st>>>(X, nx, Y, ny, d, gi, ri, m, P, gamma, coef0, degree, out, ws);
  kid_finish_kernel<<<cat::cdiv((int64_t)S * KID_SCALARS, 256), 256, 0, st>>>(ws, S, m, P, out);
  return cat::check_launch("kid_poly_sums");
}

}  // extern "C"
