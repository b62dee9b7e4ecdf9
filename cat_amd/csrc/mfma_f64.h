// The float64 MFMA tile (v_mfma_f64_16x16x4_f64, gfx950) of kid_ops.hip and fid_ops.hip: fragment map, LDS operand layouts, K loop, accumulator walk.
//
// A workgroup is 256 threads = 4 waves as 2 x 2; a wave owns TM x TM MFMA tiles of 16 x 16, the workgroup a (32 TM) x (32 TM) block.  Operands
// are staged in LDS as doubles, BK = 32 K indices per step, the next step's operands fetched into registers while the current one is multiplied.
// What is fetched, how it is staged and what becomes of the accumulators is the kernel's business: lambdas.  A lambda is optimised on its own
// before it is inlined, where a scalar captured by reference is opaque memory: capture scalars by value where the code generated depends on it.
//
// f64 MFMA fragments: A[i][k] / B[k][j] with i, j = lane & 15 and k = lane >> 4, one double per lane; D[row][col] with col = lane & 15 and
// row = (lane >> 4) + 4 * reg -- not the float32 forms' (lane >> 4) * 4 + reg.
#pragma once
#include "common.h"

namespace cat {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int BK = 32;      // K indices per staging step

// LDS layouts of one operand of ROWS rows (or columns) x BK: index(row, k) in doubles.  The pads keep the one-double-per-lane operand reads
// of a half wave (16 rows x 2 k) on distinct banks: KContig puts rows 4 banks and k 2 banks apart, KMajor rows 2 banks and k 32 banks.
template <int ROWS>
struct KContig {      // the K index is contiguous in memory: [row][BK + 2]
  static constexpr int LD = BK + 2, SIZE = ROWS * LD;
  __device__ static constexpr int index(int row, int k) { return row * LD + k; }
};
template <int ROWS>
struct KMajor {       // the K index is the slow one: [k][ROWS + 16]
  static constexpr int LD = ROWS + 16, SIZE = BK * LD;
  __device__ static constexpr int index(int row, int k) { return k * LD + row; }
};
struct Strided {      // either of the two, picked at run time
  int row, k;
  __device__ int index(int r, int kk) const { return r * row + kk * k; }
};

struct TileCoords {
  int lane, wave, wi, wj, fr, fk;      // wave (wi, wj) of the 2 x 2; fragment row / column fr, fragment k index (and D row group) fk
  __device__ explicit TileCoords(int t) : lane(t & 63), wave(t >> 6), wi(wave >> 1), wj(wave & 1), fr(lane & 15), fk(lane >> 4) {}
};

// one staged step: acc += A (rows of the wave's TM tiles) x B (columns of the wave's TM tiles) over the BK indices in LDS
template <int TM, class LA, class LB>
__device__ __forceinline__ void mma_step(d4 (&acc)[TM][TM], const double* As, const double* Bs, const LA& la, const LB& lb, const TileCoords& c) {
#pragma unroll
  for (int ks = 0; ks < BK / 4; ++ks) {
    double a[TM], b[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      a[i] = As[la.index((c.wi * TM + i) * 16 + c.fr, ks * 4 + c.fk)];
      b[i] = Bs[lb.index((c.wj * TM + i) * 16 + c.fr, ks * 4 + c.fk)];
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TM; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
  }
}

// The K loop over nk steps: fetch(kc) loads step kc's operands into registers, stage() writes the fetched registers to LDS, mma() multiplies
// what is staged.  Two barriers per step; the fetch of step kc + 1 is in flight while step kc is multiplied.
template <class Stage, class Fetch, class Mma>
__device__ __forceinline__ void pipeline(int nk, Stage stage, Fetch fetch, Mma mma) {
  fetch(0);
  for (int kc = 0; kc < nk; ++kc) {
    __syncthreads();   // the previous step's operand reads are done
    stage();
    __syncthreads();
    if (kc + 1 < nk) fetch(kc + 1);
    mma();
  }
}

// f(i, reg, j, row, col, value) for every accumulator value of the thread, row / col inside the workgroup's block.  The order i -> reg -> j
// is part of the contract: sums taken in an epilogue repeat bit for bit because of it.
template <int TM, class F>
__device__ __forceinline__ void for_each_acc(const d4 (&acc)[TM][TM], const TileCoords& c, F f) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < TM; ++j) f(i, r, j, (c.wi * TM + i) * 16 + c.fk + 4 * r, (c.wj * TM + j) * 16 + c.fr, acc[i][j][r]);
}

}  // namespace cat
