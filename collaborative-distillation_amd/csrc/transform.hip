// The C x C part of the optimal-transport and AdaIN feature transforms (include/wct_hip_transform.h), on the device, in fp64 on
// v_mfma_f64_16x16x4_f64 like solve.hip.  Both are affine maps csF = M cF + b with
//     M = alpha T + (1 - alpha) I,   b = alpha (mu_s - T mu_c)
// so everything behind (M, b) -- the fold into the decoder's first convolution, the f16x3 convolutions -- is the WCT path's.
//
//   ot     T = S B^(-1/2) S,  B = sym(S cov_c S),  S = cov_s^(1/2) (the level's style slot):  the Monge map between the two
//          Gaussians (Olkin & Pukelsheim 1982) in the form that needs only S and ONE matrix function on the content side.
//            launch_ot_sandwich   P = cov_c S, then B = (S P + (S P)^T) / 2, cov_c formed on the fly from the raw moments
//            launch_eig           B^(-1/2) (solve.hip; B enters as the pseudo-moments n = 2, sum = 0, sumsq = B, which give cov = B
//                                 exactly, with the iteration schedule chosen for B: wct_api.hip OT_MAXIT, OT_GUESS)
//            launch_ot_assemble   Q = Z S, then T = S Q, M and b by one workgroup per 16 rows
//   adain  T = diag(sqrt((cov_s_ii + eps) / (cov_c_ii + eps))),  cov_s_ii = SUM_k S_ik^2:  one launch, no matrix function.
//
// GEMM tiles (mm_f64_dev.h): one wave per 16 x 16 output tile, operands straight from global memory (C <= 512: every matrix is L2
// resident), any even C -- rows, columns and k past C read as zero and are not written.  Every sum has a fixed order: results are
// functions of the inputs alone.
#include "wct_common.h"
#include "mm_f64_dev.h"

namespace {

// solve.hip cov_value: the unbiased covariance from the raw moments, the (min, max) entry for both halves
__device__ __forceinline__ double cov_entry(int r, int c, int C, double n, const double* sum, const double* sumsq) {
  const double mr = sum[r] / n, mc = sum[c] / n;
  const int lo = r < c ? r : c, hi = r < c ? c : r;
  return (sumsq[(size_t)lo * C + hi] - n * mr * mc) / (n - 1.0);
}

// D = L R  (COV: L = cov_c from the raw moments (n, sum, sumsq); otherwise L is a C x C matrix)
template <bool COV>
__global__ __launch_bounds__(256) void tr_gemm_kernel(int C, double n, const double* sum, const double* Lm, const double* R, double* D) {
  int i0, j0;
  if (!wave_tile(C, i0, j0)) return;
  const int lane = threadIdx.x & 63;
  f64x4 acc = f64x4{0., 0., 0., 0.};
  if (COV) acc = tile_mm([&](int r, int k) { return cov_entry(r, k, C, n, sum, Lm); }, [&](int k, int c) { return R[(size_t)k * C + c]; }, C, i0, j0, lane, acc);
  else acc = tile_mm([&](int r, int k) { return Lm[(size_t)r * C + k]; }, [&](int k, int c) { return R[(size_t)k * C + c]; }, C, i0, j0, lane, acc);
  const int li = lane & 15, kk = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = i0 + kk + 4 * r, col = j0 + li;
    if (row < C && col < C) D[(size_t)row * C + col] = acc[r];
  }
}

// B = (S P + (S P)^T) / 2: the tile of S P and the transposed tile of its mirror image in two accumulators, whose products and k
// order are each other's at mirrored positions -- B is symmetric bit for bit.  zeros[0 .. C) = 0: the pseudo-moments' `sum`.
__global__ __launch_bounds__(256) void ot_sandwich_kernel(int C, const double* S, const double* P, double* B, double* zeros) {
  if (blockIdx.x == 0)
    for (int j = threadIdx.x; j < C; j += 256) zeros[j] = 0.0;
  int i0, j0;
  if (!wave_tile(C, i0, j0)) return;
  const int lane = threadIdx.x & 63;
  const f64x4 z = f64x4{0., 0., 0., 0.};
  const f64x4 a1 = tile_mm([&](int r, int k) { return S[(size_t)r * C + k]; }, [&](int k, int c) { return P[(size_t)k * C + c]; }, C, i0, j0, lane, z);
  const f64x4 a2 = tile_mm([&](int r, int k) { return P[(size_t)k * C + r]; }, [&](int k, int c) { return S[(size_t)c * C + k]; }, C, i0, j0, lane, z);
  const int li = lane & 15, kk = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = i0 + kk + 4 * r, col = j0 + li;
    if (row < C && col < C) B[(size_t)row * C + col] = 0.5 * (a1[r] + a2[r]);
  }
}

// rows 16 blockIdx.x .. + 15 of T = S Q, M = alpha T + (1 - alpha) I and b = alpha (mu_s - T mu_c), mu_c = sum_c / n: the column
// tiles dealt round-robin to the four waves, the row dot products with mu_c summed over a wave's tiles, its 16 columns (butterfly)
// and the four waves in that fixed order (assemble_row_kernel's job for the S Z S form)
__global__ __launch_bounds__(256) void ot_assemble_kernel(int C, double alpha, const double* S, const double* Q, double n, const double* sum_c,
                                                            const double* mu_s, double* M, double* bvec) {
  __shared__ double red[4][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, kk = lane >> 4;
  const int nt = (C + 15) >> 4, i0 = blockIdx.x * 16;
  double dot[4] = {0., 0., 0., 0.};
  for (int tj = wave; tj < nt; tj += 4) {
    const int j0 = tj * 16, col = j0 + li;
    const f64x4 acc = tile_mm([&](int r, int k) { return S[(size_t)r * C + k]; }, [&](int k, int c) { return Q[(size_t)k * C + c]; }, C, i0, j0, lane,
                              f64x4{0., 0., 0., 0.});
    const double mc = col < C ? sum_c[col] / n : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = i0 + kk + 4 * r;
      if (row < C && col < C) M[(size_t)row * C + col] = alpha * acc[r] + (row == col ? 1.0 - alpha : 0.0);
      dot[r] += acc[r] * mc;    // rows and columns past C hold exact zeros
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double d = dot[r];
    for (int o = 8; o > 0; o >>= 1) d += __shfl_xor(d, o);
    if (li == 0) red[wave][kk + 4 * r] = d;
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    const int row = i0 + threadIdx.x;
    if (row < C) bvec[row] = alpha * (mu_s[row] - (((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x]));
  }
}

// AdaIN: one workgroup per channel a.  t = sqrt((SUM_k S[a][k]^2 + eps) / (cov_c[a][a] + eps)); row a of M; b[a]
__global__ __launch_bounds__(256) void adain_assemble_kernel(int C, double alpha, double eps, const double* S, const double* mu_s, double n, const double* sum_c,
                                                               const double* sumsq_c, double* M, double* bvec, int* info) {
  __shared__ double red[256];
  const int a = blockIdx.x, tid = threadIdx.x;
  double q = 0.;
  for (int k = tid; k < C; k += 256) { const double v = S[(size_t)a * C + k]; q += v * v; }
  red[tid] = q;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
  const double var_c = fmax(cov_entry(a, a, C, n, sum_c, sumsq_c), 0.0);   // round-off of a constant channel may land below zero
  const double t = sqrt((red[0] + eps) / (var_c + eps));
  for (int c = tid; c < C; c += 256) M[(size_t)a * C + c] = a == c ? alpha * t + (1.0 - alpha) : 0.0;
  if (tid == 0) {
    bvec[a] = alpha * (mu_s[a] - t * (sum_c[a] / n));
    if (a == 0 && info) *info = 0;     // no matrix function on the content side
  }
}

}  // namespace

size_t ot_workspace_bytes(int C) { return (2 * (size_t)C * C + (size_t)C) * sizeof(double); }

hipError_t launch_ot_sandwich(int C, double n, const double* sum_c, const double* sumsq_c, const double* S, double* B, double* zeros, double* tmp, hipStream_t s) {
  if (C < 2 || (C & 1) || C > 512 || n < 2) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tr_gemm_kernel<true>, dim3(tile_blocks(C)), dim3(256), 0, s, C, n, sum_c, sumsq_c, S, tmp);
  hipLaunchKernelGGL(ot_sandwich_kernel, dim3(tile_blocks(C)), dim3(256), 0, s, C, S, (const double*)tmp, B, zeros);
  return hipGetLastError();
}

hipError_t launch_ot_assemble(int C, double alpha, const double* S, const double* mu_s, const double* Z, double n, const double* sum_c, double* tmp,
                              double* M, double* b, hipStream_t s) {
  if (C < 2 || (C & 1) || C > 512 || n < 2) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tr_gemm_kernel<false>, dim3(tile_blocks(C)), dim3(256), 0, s, C, n, (const double*)nullptr, Z, S, tmp);
  hipLaunchKernelGGL(ot_assemble_kernel, dim3((unsigned)((C + 15) / 16)), dim3(256), 0, s, C, alpha, S, (const double*)tmp, n, sum_c, mu_s, M, b);
  return hipGetLastError();
}

hipError_t launch_adain_assemble(int C, double alpha, double eps, const double* S, const double* mu_s, double n, const double* sum_c, const double* sumsq_c,
                                 double* M, double* b, int* info_dev, hipStream_t s) {
  if (C < 2 || (C & 1) || C > 512 || n < 2) return hipErrorInvalidValue;
  hipLaunchKernelGGL(adain_assemble_kernel, dim3((unsigned)C), dim3(256), 0, s, C, alpha, eps, S, mu_s, n, sum_c, sumsq_c, M, b, info_dev);
  return hipGetLastError();
}
