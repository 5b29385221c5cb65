// The seeded rotation of style diversification (include/wct_hip_diverse.h): an orthogonal Z(C, seed, stream_id, tag, strength) that
// post-multiplies a level's style slot, F <- F Z.  F Z (F Z)^T = F F^T = cov_s: the colouring step reaches the same target covariance
// through a different square root (Wang et al., "Diversified Arbitrary Style Transfer via Deep Feature Perturbation", CVPR 2020).
// Everything in fp64 with fixed summation orders: Z is a function of its five arguments alone, bit for bit.
//
// Definition (tests/diverse_oracle.py restates it in numpy; the header states it for callers)
//   generator   Philox4x32-10 as noise.hip uses it: key (seed & 0xffffffff, seed >> 32), counter (i & 0xffffffff, i >> 32, stream_id,
//               0x524F5400 | tag) for block i, tag in 0..255.  The noise image has 0 in the last word: the two never share a stream.
//   G           C x C: element e = r C + c is word e & 3 of block e >> 2, g = (double)(int32_t)word * 2^-31  (exact)
//   s           strength / (2.0 * sqrt(2.0 * C / 3.0)), in IEEE double on the host, in that order: a kernel argument.  The entries
//               g_rc - g_cr have variance 2 / 3, so the spectral radius of A / strength is just under 1 (semicircle law)
//   A           r < c: A[r][c] = s * (g_rc - g_cr) -- the difference is exact, ONE rounding --, A[c][r] = 0 - A[r][c], A[r][r] = 0:
//               skew-symmetric bit for bit
//   Z           (I - A)(I + A)^(-1), the Cayley transform of A: orthogonal for every A, I at strength 0, rotation angles
//               2 atan(strength mu_k) for the eigenvalues +- i strength mu_k of A
// Evaluation
//   B = I - A A is symmetric positive definite with eigenvalues 1 + (strength mu_k)^2 in [1, 1 + strength^2 rho^2]; it is formed
//   symmetric bit for bit the way transform.hip's ot_sandwich_kernel forms its B (a tile and the transposed tile of its mirror image).
//   R = B^(-1/2) runs through launch_eig (solve.hip) on the pseudo-moments n = 2, sum = 0, sumsq = B, which give cov = B exactly --
//   always the multi-launch iteration with the covariance schedule (never the single-launch form, whose abort path would make the bits
//   depend on what else runs on the device; never the wide-model switch: Z must not depend on which modules a context has loaded).
//   U = (I - A) R is orthogonal -- U^T U = R (I + A)(I - A) R = R B R = I -- and Z = U U = (I - A)^2 B^(-1) = (I - A)(I + A)^(-1):
//   every factor is a function of A, so they all commute.
//   Strength exactly 0 writes the identity (and a zero A) with no solver.
#include "wct_common.h"
#include "mm_f64_dev.h"
#include "philox_dev.h"

namespace {

constexpr unsigned ROT_TAG_BASE = 0x524F5400u;   // "ROT\0": the counter's last word is this | tag

// g of element e of the C x C matrix G, as an exact integer (the 2^-31 is applied to the difference)
__device__ __forceinline__ long long rot_word(unsigned long long e, unsigned stream_id, unsigned tagword, unsigned k0, unsigned k1) {
  const unsigned long long i = e >> 2;
  const Philox4 r = philox4x32_10((unsigned)i, (unsigned)(i >> 32), stream_id, tagword, k0, k1);
  return (long long)(int)r.v[e & 3];
}

// one thread per element of A; the pair (r, c), r < c, is computed by both of its threads from the same two words
__global__ __launch_bounds__(256) void rot_skew_kernel(int C, unsigned k0, unsigned k1, unsigned stream_id, unsigned tagword, double s, double* A) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)C * C) return;
  const int r = (int)(e / C), c = (int)(e % C);
  if (r == c) { A[e] = 0.0; return; }
  const int lo = r < c ? r : c, hi = r < c ? c : r;
  const long long d = rot_word((unsigned long long)lo * C + hi, stream_id, tagword, k0, k1) - rot_word((unsigned long long)hi * C + lo, stream_id, tagword, k0, k1);
  const double up = s * ((double)d * 0x1p-31);    // |d| < 2^32: exact as a double, exact scaled; the product rounds once
  A[e] = r < c ? up : 0.0 - up;
}

// strength 0: Z = I and A = 0 exactly
__global__ __launch_bounds__(256) void rot_identity_kernel(int C, double* Z, double* A) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)C * C) return;
  Z[e] = e / C == e % C ? 1.0 : 0.0;
  if (A) A[e] = 0.0;
}

// B = I - (A A + (A A)^T) / 2, the two tiles' products and k order each other's at mirrored positions; zeros[0 .. C) = 0: the
// pseudo-moments' `sum`
__global__ __launch_bounds__(256) void rot_gram_kernel(int C, const double* A, double* B, double* zeros) {
  if (blockIdx.x == 0)
    for (int j = threadIdx.x; j < C; j += 256) zeros[j] = 0.0;
  int i0, j0;
  if (!wave_tile(C, i0, j0)) return;
  const int lane = threadIdx.x & 63;
  const f64x4 z = f64x4{0., 0., 0., 0.};
  const f64x4 a1 = tile_mm([&](int r, int k) { return A[(size_t)r * C + k]; }, [&](int k, int c) { return A[(size_t)k * C + c]; }, C, i0, j0, lane, z);
  const f64x4 a2 = tile_mm([&](int r, int k) { return A[(size_t)k * C + r]; }, [&](int k, int c) { return A[(size_t)c * C + k]; }, C, i0, j0, lane, z);
  const int li = lane & 15, kk = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = i0 + kk + 4 * r, col = j0 + li;
    if (row < C && col < C) B[(size_t)row * C + col] = (row == col ? 1.0 : 0.0) - 0.5 * (a1[r] + a2[r]);
  }
}

// D = L R (MINUS_A: D = (I - L) R = R - L R, the subtraction after the sum)
template <bool MINUS_A>
__global__ __launch_bounds__(256) void rot_gemm_kernel(int C, const double* L, const double* R, double* D) {
  int i0, j0;
  if (!wave_tile(C, i0, j0)) return;
  const int lane = threadIdx.x & 63;
  const f64x4 acc = tile_mm([&](int r, int k) { return L[(size_t)r * C + k]; }, [&](int k, int c) { return R[(size_t)k * C + c]; }, C, i0, j0, lane,
                            f64x4{0., 0., 0., 0.});
  const int li = lane & 15, kk = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = i0 + kk + 4 * r, col = j0 + li;
    if (row < C && col < C) D[(size_t)row * C + col] = MINUS_A ? R[(size_t)row * C + col] - acc[r] : acc[r];
  }
}

struct RotWs { double *A, *B, *U, *zeros, *res; void* eig; int* info; };

size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// s of the definition, in the order the header states it
double rotation_scale(int C, double strength) { return strength / (2.0 * sqrt(2.0 * C / 3.0)); }

RotWs rot_carve(int C, void* ws) {
  const size_t cc = (size_t)C * C;
  char* p = reinterpret_cast<char*>(ws);
  RotWs w;
  w.A = reinterpret_cast<double*>(p); p += up256(cc * sizeof(double));
  w.B = reinterpret_cast<double*>(p); p += up256(cc * sizeof(double));
  w.U = reinterpret_cast<double*>(p); p += up256(cc * sizeof(double));
  w.zeros = reinterpret_cast<double*>(p); p += up256((size_t)C * sizeof(double));
  w.res = reinterpret_cast<double*>(p); p += up256(eig_result_bytes(C));
  w.eig = p; p += up256(eig_workspace_bytes(C));
  w.info = reinterpret_cast<int*>(p);
  return w;
}

}  // namespace

size_t rotation_workspace_bytes(int C) {
  const size_t cc = (size_t)C * C;
  return 3 * up256(cc * sizeof(double)) + up256((size_t)C * sizeof(double)) + up256(eig_result_bytes(C)) + up256(eig_workspace_bytes(C)) + 256;
}

hipError_t launch_rotation_make(int C, unsigned long long seed, unsigned stream_id, unsigned tag, double strength, double* Z, double* skew, void* ws,
                                size_t ws_bytes, hipStream_t s) {
  if (C < 2 || (C & 1) || C > 512 || tag > 255u || !(strength >= 0.0) || !Z) return hipErrorInvalidValue;
  const size_t cc = (size_t)C * C;
  const unsigned eb = (unsigned)((cc + 255) / 256);
  if (strength == 0.0) {
    hipLaunchKernelGGL(rot_identity_kernel, dim3(eb), dim3(256), 0, s, C, Z, skew);
    return hipGetLastError();
  }
  if (!ws || ws_bytes < rotation_workspace_bytes(C)) return hipErrorOutOfMemory;
  const RotWs w = rot_carve(C, ws);
  hipLaunchKernelGGL(rot_skew_kernel, dim3(eb), dim3(256), 0, s, C, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), stream_id, ROT_TAG_BASE | tag,
                     rotation_scale(C, strength), w.A);
  if (skew) {
    hipError_t e = hipMemcpyAsync(skew, w.A, cc * sizeof(double), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(rot_gram_kernel, dim3(tile_blocks(C)), dim3(256), 0, s, C, (const double*)w.A, w.B, w.zeros);
  hipError_t e = launch_eig(C, 2.0, w.zeros, w.B, 1, w.res, w.info, w.eig, eig_workspace_bytes(C), s);
  if (e != hipSuccess) return e;
  const double* R = w.res + eig_result_F_offset((size_t)C);
  hipLaunchKernelGGL(rot_gemm_kernel<true>, dim3(tile_blocks(C)), dim3(256), 0, s, C, (const double*)w.A, R, w.U);
  hipLaunchKernelGGL(rot_gemm_kernel<false>, dim3(tile_blocks(C)), dim3(256), 0, s, C, (const double*)w.U, (const double*)w.U, Z);
  return hipGetLastError();
}

hipError_t launch_rotation_apply(int C, const double* F, const double* Z, double* out, hipStream_t s) {
  if (C < 2 || (C & 1) || C > 512 || !F || !Z || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rot_gemm_kernel<false>, dim3(tile_blocks(C)), dim3(256), 0, s, C, F, Z, out);
  return hipGetLastError();
}
