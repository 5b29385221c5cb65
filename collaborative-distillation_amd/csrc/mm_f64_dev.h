// The fp64 matrix-core GEMM tile of the C x C products outside the solver (transform.hip, rotate.hip): one wave per 16 x 16 output tile
// on v_mfma_f64_16x16x4_f64, operands straight from global memory (C <= 512: every matrix is L2 resident), any even C -- rows, columns
// and k past C read as zero and are not written.  The k order is fixed: a result is a function of the inputs alone.  Private to csrc/.
#pragma once
#include "wct_common.h"

namespace {

// acc += A[i0 .. i0+15][0 .. C) B[0 .. C)[j0 .. j0+15]; A(r, k) and B(k, c) are called inside the matrix only.
// Result layout (as solve.hip tile_gemm): acc[reg] is row i0 + (lane >> 4) + 4 reg, column j0 + (lane & 15).
template <class FA, class FB>
__device__ __forceinline__ f64x4 tile_mm(FA A, FB B, int C, int i0, int j0, int lane, f64x4 acc) {
  const int li = lane & 15, kk = lane >> 4;
  const int ra = i0 + li, cb = j0 + li;
  for (int k0 = 0; k0 < C; k0 += 4) {
    const int k = k0 + kk;
    const double a = (ra < C && k < C) ? A(ra, k) : 0.0;
    const double b = (cb < C && k < C) ? B(k, cb) : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// this wave's tile of a grid of 4-wave workgroups over nt x nt tiles; false: no tile
__device__ __forceinline__ bool wave_tile(int C, int& i0, int& j0) {
  const int nt = (C + 15) >> 4;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= nt * nt) return false;
  i0 = (t / nt) * 16; j0 = (t % nt) * 16;
  return true;
}

inline unsigned tile_blocks(int C) { const unsigned nt = (unsigned)((C + 15) / 16); return (nt * nt + 3) / 4; }

}  // namespace
