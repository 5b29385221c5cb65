// Colour preservation (include/wct_hip_color.h): whiten_and_color (PytorchWCT/util_wct.py:62-131) in three channels on image pixels
// -- fp64 raw moments, a 3 x 3 solve, one affine map per pixel -- and the luminance merge at the image edge.  Four streaming
// kernels on planar 3 x H x W fp32 data (12 B/px read for the moments, 24 B/px for the apply, 24 + 12 or 3 B/px for the merge) and
// one single-thread solve.
//
// A thread works on GROUPS of four consecutive element indices: one 16-byte access per plane where that plane's group address is
// 16-byte aligned, four 4-byte accesses otherwise (a view into a larger buffer; planes of an H W that is not a multiple of 4) -- the
// values land in the same registers either way, so what is summed where never depends on the address.
//
// Moments: tile T = indices [8192 T, 8192 (T + 1)); thread t of its workgroup takes groups 2048 T + t + 256 i, i = 0..7, and adds
// their <= 32 pixels in index order into nine fp64 accumulators (three sums, six products; (double)a * (double)b is exact);
// the 256 threads fold by a fixed tree (lanes 32, 16, .. 1 apart, then waves 0 + 1 + 2 + 3) into partial[T][9].  The second stage is
// ONE workgroup: thread t adds partials t, t + 256, ... in order, the same tree, thread 0 writes sum[3] and the symmetric sumsq[9].
// The tree is a function of H W alone; no atomics.
#include "wct_common.h"
#include <float.h>

namespace {

constexpr int CM_THREADS = 256, CM_ITERS = 8, CM_TILE = CM_THREADS * 4 * CM_ITERS;   // 8192 pixels per workgroup

// four consecutive floats from p, zero beyond `n` valid ones (n >= 1)
__device__ __forceinline__ f32x4 load_group(const float* p, int n) {
  if (n == 4 && (reinterpret_cast<size_t>(p) & 15) == 0) return *reinterpret_cast<const f32x4*>(p);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  v[0] = p[0];
  if (n > 1) v[1] = p[1];
  if (n > 2) v[2] = p[2];
  if (n > 3) v[3] = p[3];
  return v;
}

__device__ __forceinline__ void store_group(float* p, f32x4 v, int n) {
  if (n == 4 && (reinterpret_cast<size_t>(p) & 15) == 0) { *reinterpret_cast<f32x4*>(p) = v; return; }
  p[0] = v[0];
  if (n > 1) p[1] = v[1];
  if (n > 2) p[2] = v[2];
  if (n > 3) p[3] = v[3];
}

// fixed-order fold of nine doubles over a 256-thread workgroup; the result is valid in thread 0
__device__ __forceinline__ void block_fold9(double (&a)[9], double (*lds)[9]) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
    for (int j = 0; j < 9; ++j) a[j] += __shfl_down(a[j], off, 64);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0)
#pragma unroll
    for (int j = 0; j < 9; ++j) lds[wave][j] = a[j];
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int j = 0; j < 9; ++j) a[j] = ((lds[0][j] + lds[1][j]) + lds[2][j]) + lds[3][j];
}

__global__ __launch_bounds__(CM_THREADS) void color_moments_kernel(const float* __restrict__ img, long npix, double* __restrict__ partial) {
  __shared__ double lds[4][9];
  const long g0 = (long)blockIdx.x * (CM_THREADS * CM_ITERS) + threadIdx.x;
  f32x4 v[CM_ITERS][3];
#pragma unroll
  for (int i = 0; i < CM_ITERS; ++i) {
    const long p0 = (g0 + (long)i * CM_THREADS) * 4;
    const long left = npix - p0;
    if (left > 0) {
      const int n = left < 4 ? (int)left : 4;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[i][c] = load_group(img + (size_t)c * npix + p0, n);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};   // adding +0 changes no bit of an accumulator
    }
  }
  double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // s0 s1 s2 | q00 q01 q02 q11 q12 q22
#pragma unroll
  for (int i = 0; i < CM_ITERS; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double r = (double)v[i][0][k], g = (double)v[i][1][k], b = (double)v[i][2][k];
      a[0] += r; a[1] += g; a[2] += b;
      a[3] = fma(r, r, a[3]); a[4] = fma(r, g, a[4]); a[5] = fma(r, b, a[5]);
      a[6] = fma(g, g, a[6]); a[7] = fma(g, b, a[7]); a[8] = fma(b, b, a[8]);
    }
  block_fold9(a, lds);
  if (threadIdx.x == 0)
#pragma unroll
    for (int j = 0; j < 9; ++j) partial[(size_t)blockIdx.x * 9 + j] = a[j];
}

__global__ __launch_bounds__(CM_THREADS) void color_moments_final_kernel(const double* __restrict__ partial, long ntiles, double* __restrict__ sum,
                                                                         double* __restrict__ sumsq) {
  __shared__ double lds[4][9];
  double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (long T = threadIdx.x; T < ntiles; T += CM_THREADS)
#pragma unroll
    for (int j = 0; j < 9; ++j) a[j] += partial[(size_t)T * 9 + j];
  block_fold9(a, lds);
  if (threadIdx.x == 0) {
    sum[0] = a[0]; sum[1] = a[1]; sum[2] = a[2];
    sumsq[0] = a[3]; sumsq[1] = a[4]; sumsq[2] = a[5];
    sumsq[3] = a[4]; sumsq[4] = a[6]; sumsq[5] = a[7];
    sumsq[6] = a[5]; sumsq[7] = a[7]; sumsq[8] = a[8];
  }
}

// ---- solve: one thread, fp64 ------------------------------------------------------------------------------------------------------
// eigen-decomposition of a symmetric 3 x 3 matrix by cyclic Jacobi: S = V diag(lam) V^T (columns of V).  Rotations in the fixed
// order (0,1), (0,2), (1,2); stops when the off-diagonal part is exactly annihilated or after 24 sweeps (3 x 3 converges in ~6).
__device__ void jacobi3(double S[3][3], double V[3][3], double lam[3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 24; ++sweep) {
    const double off = S[0][1] * S[0][1] + S[0][2] * S[0][2] + S[1][2] * S[1][2];
    if (off == 0.0) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        const double apq = S[p][q];
        if (apq == 0.0) continue;
        const double theta = (S[q][q] - S[p][p]) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
        for (int k = 0; k < 3; ++k) {   // S <- S J
          const double skp = S[k][p], skq = S[k][q];
          S[k][p] = c * skp - s * skq;
          S[k][q] = s * skp + c * skq;
        }
        for (int k = 0; k < 3; ++k) {   // S <- J^T S
          const double spk = S[p][k], sqk = S[q][k];
          S[p][k] = c * spk - s * sqk;
          S[q][k] = s * spk + c * sqk;
        }
        S[p][q] = 0.0; S[q][p] = 0.0;
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  for (int i = 0; i < 3; ++i) lam[i] = S[i][i];
}

// mu = sum / n, Sigma = (sumsq - n mu mu^T) / (n - 1) + eps I, then F = Sigma^(+1/2) (power > 0) or Sigma^(-1/2)
__device__ void color_root(double n, const double* sum, const double* sumsq, double eps, bool inverse, double mu[3], double F[3][3]) {
  double S[3][3], V[3][3], lam[3];
  for (int i = 0; i < 3; ++i) mu[i] = sum[i] / n;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j) {
      const double cij = (sumsq[i * 3 + j] - n * mu[i] * mu[j]) / (n - 1.0) + (i == j ? eps : 0.0);
      S[i][j] = cij; S[j][i] = cij;
    }
  jacobi3(S, V, lam);
  double f[3];
  for (int i = 0; i < 3; ++i) {
    const double l = fmax(lam[i], DBL_MIN);   // Sigma + eps I is positive definite; round-off below a tiny eps must not make a NaN
    f[i] = inverse ? 1.0 / sqrt(l) : sqrt(l);
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) F[i][j] = (V[i][0] * f[0]) * V[j][0] + (V[i][1] * f[1]) * V[j][1] + (V[i][2] * f[2]) * V[j][2];
}

__global__ void color_solve_kernel(double n_c, const double* sum_c, const double* sumsq_c, double n_s, const double* sum_s, const double* sumsq_s,
                                   double eps, double* A, double* t) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double mu_c[3], mu_s[3], Fc[3][3], Fs[3][3], Am[3][3];
  color_root(n_c, sum_c, sumsq_c, eps, false, mu_c, Fc);
  color_root(n_s, sum_s, sumsq_s, eps, true, mu_s, Fs);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Am[i][j] = Fc[i][0] * Fs[0][j] + Fc[i][1] * Fs[1][j] + Fc[i][2] * Fs[2][j];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) A[i * 3 + j] = Am[i][j];
    t[i] = mu_c[i] - (Am[i][0] * mu_s[0] + Am[i][1] * mu_s[1] + Am[i][2] * mu_s[2]);
  }
}

// ---- apply: out_p = float(A x_p + t), fp64 inside -----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void color_apply_kernel(const float* in, long npix, const double* __restrict__ A, const double* __restrict__ t,
                                                          float* out) {
  const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= npix) return;
  const int n = npix - p0 < 4 ? (int)(npix - p0) : 4;
  f32x4 x[3], y[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) x[c] = load_group(in + (size_t)c * npix + p0, n);   // all reads before any write: in place is safe
  double a[9], b[3];
#pragma unroll
  for (int j = 0; j < 9; ++j) a[j] = A[j];
#pragma unroll
  for (int j = 0; j < 3; ++j) b[j] = t[j];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double x0 = (double)x[0][k], x1 = (double)x[1][k], x2 = (double)x[2][k];
#pragma unroll
    for (int r = 0; r < 3; ++r) y[r][k] = (float)fma(a[r * 3 + 2], x2, fma(a[r * 3 + 1], x1, fma(a[r * 3], x0, b[r])));
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) store_group(out + (size_t)c * npix + p0, y[c], n);
}

// ---- luma merge ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float luma(float r, float g, float b) { return __fmaf_rn(0.114f, b, __fmaf_rn(0.587f, g, __fmul_rn(0.299f, r))); }

// the conversion of misc.hip planar_to_u8_kernel: mul(255), + 0.5 with round_mode 1, clamp, truncation
__device__ __forceinline__ unsigned to_u8(float v, int round_mode) {
  float x = __fmul_rn(v, 255.0f);
  if (round_mode) x = __fadd_rn(x, 0.5f);
  x = fminf(fmaxf(x, 0.f), 255.f);     // NaN -> 0
  return (unsigned)x;                  // truncation toward zero
}

// groups of four FLAT output pixels q = y Wo + x; with Wo a multiple of 4 (every result of the cascade) a group lies in one row
__global__ __launch_bounds__(256) void luma_merge_kernel(const float* sty, int Ho, int Wo, const float* con, int Hc, int Wc, float* out_planar,
                                                         uint8_t* out_hwc, int round_mode) {
  const long npix = (long)Ho * Wo, q0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (q0 >= npix) return;
  const int n = npix - q0 < 4 ? (int)(npix - q0) : 4;
  const size_t cplane = (size_t)Hc * Wc;
  f32x4 s[3], c[3], o[3];
  if ((Wo & 3) == 0) {
    const long y = q0 / Wo, x = q0 - y * Wo;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      s[ch] = load_group(sty + (size_t)ch * npix + q0, 4);
      c[ch] = load_group(con + ch * cplane + (size_t)y * Wc + x, 4);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long q = q0 + (k < n ? k : 0);
      const long y = q / Wo, x = q - y * Wo;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        s[ch][k] = sty[(size_t)ch * npix + q];
        c[ch][k] = con[ch * cplane + (size_t)y * Wc + x];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float d = __fsub_rn(luma(s[0][k], s[1][k], s[2][k]), luma(c[0][k], c[1][k], c[2][k]));
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) o[ch][k] = __fadd_rn(c[ch][k], d);
  }
  if (out_planar) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) store_group(out_planar + (size_t)ch * npix + q0, o[ch], n);
  } else {
    unsigned b[12];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) b[k * 3 + ch] = to_u8(o[ch][k], round_mode);
    if (n == 4 && (reinterpret_cast<size_t>(out_hwc) & 3) == 0) {   // q0 * 3 is a multiple of 12: aligned with the base
      unsigned* dst = reinterpret_cast<unsigned*>(out_hwc + q0 * 3);
      dst[0] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
      dst[1] = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
      dst[2] = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k)   // unrolled and predicated: b[] stays in registers (an unaligned base, or the image's last group)
        if (k < n * 3) out_hwc[q0 * 3 + k] = (uint8_t)b[k];
    }
  }
}

unsigned group_blocks(long npix) { return (unsigned)(((npix + 3) / 4 + 255) / 256); }

}  // namespace

long color_moments_tiles(long npix) { return (npix + CM_TILE - 1) / CM_TILE; }
// the second stage's threads add ceil(tiles / 256) partials in sequence: 4096 at most keeps the contract's bound
long color_moments_max_pixels() { return (long)CM_TILE * CM_THREADS * 4096; }
size_t color_moments_workspace_bytes(long npix) { return (size_t)color_moments_tiles(npix) * 9 * sizeof(double); }

hipError_t launch_color_moments(const float* planar, long npix, double* sum, double* sumsq, void* workspace, size_t workspace_bytes, hipStream_t s) {
  // arguments are checked where they can be answered with a message (api_image.hip); this one guards the partials' bounds
  if (workspace_bytes < color_moments_workspace_bytes(npix)) return hipErrorInvalidValue;
  const long ntiles = color_moments_tiles(npix);
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(color_moments_kernel, dim3((unsigned)ntiles), dim3(CM_THREADS), 0, s, planar, npix, partial);
  hipLaunchKernelGGL(color_moments_final_kernel, dim3(1), dim3(CM_THREADS), 0, s, partial, ntiles, sum, sumsq);
  return hipGetLastError();
}

hipError_t launch_color_solve(double n_c, const double* sum_c, const double* sumsq_c, double n_s, const double* sum_s, const double* sumsq_s,
                              double eps, double* A, double* t, hipStream_t s) {
  hipLaunchKernelGGL(color_solve_kernel, dim3(1), dim3(64), 0, s, n_c, sum_c, sumsq_c, n_s, sum_s, sumsq_s, eps, A, t);
  return hipGetLastError();
}

hipError_t launch_color_apply(const float* in, long npix, const double* A, const double* t, float* out, hipStream_t s) {
  hipLaunchKernelGGL(color_apply_kernel, dim3(group_blocks(npix)), dim3(256), 0, s, in, npix, A, t, out);
  return hipGetLastError();
}

hipError_t launch_luma_merge(const float* stylised, int Ho, int Wo, const float* content, int Hc, int Wc, float* out_planar, uint8_t* out_hwc,
                             int round_mode, hipStream_t s) {
  hipLaunchKernelGGL(luma_merge_kernel, dim3(group_blocks((long)Ho * Wo)), dim3(256), 0, s, stylised, Ho, Wo, content, Hc, Wc, out_planar, out_hwc,
                     round_mode);
  return hipGetLastError();
}
