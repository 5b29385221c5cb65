// Guided-filter smoothing by the content image (include/wct_hip_smooth.h): He, Sun and Tang's guided image filter with a colour guide,
// the fast form of the smoothing step of Li et al. 2018.  Two stages, each a clipped box filter in two separable directions:
//
//   stage 1   vert<1>   reads the 3 source and 3 guide planes, forms the 21 products (I 3, p 3, I I^T 6, I p^T 9) in registers and
//                       writes their VERTICAL window sums as 21 fp64 planes                                   24 B/px in, 168 B/px out
//             horiz<1>  reads those, sums them along x, divides by the window's pixel count, solves the 3 x 3 system per pixel
//                       (Cholesky, fp64) and writes a (9) and b (3) as fp32 planes                           168 B/px in,  48 B/px out
//   stage 2   vert<2>   vertical window sums of the 12 planes of a, b as 12 fp64 planes                       48 B/px in,  96 B/px out
//             horiz<2>  sums along x, q = mean_a^T I + mean_b in fp64, rounded once; writes 3 fp32 planes or the uint8 HWC image
//                                                                                                       96 + 12 B/px in, 12 or 3 B/px out
// (every window sample is read twice, once entering and once leaving; the second read is 2r + 1 rows or columns behind the first and is
// counted above once, as the algorithmic traffic.)
//
// Vertical direction: one THREAD per (column, row segment), lanes on adjacent columns, so every access is a coalesced row piece.  A
// walker sums the window of its segment's first row in ascending row order and then, per row, adds the entering row y + r and drops the
// leaving row y - r - 1 (in that order).  Segments are smooth_vseg(r) = clamp(4 r, 128, 2048) rows: the restart costs 2r + 1 of those
// rows' work, and a shorter segment gives more walkers (a 3840-column image has only 3840 columns).
//
// Horizontal direction: one WAVE per (row, column segment of SM_HSEG = 4096), walking in chunks of 64 columns with lane l on column
// xc + l.  The running sum is kept in its difference form so that all loads are coalesced: lane l loads the entering sample v(x + r) and
// the leaving one v(x - r - 1), a Kogge-Stone scan over the 64 lanes (shifts 1, 2, .. 32) gives the prefix of (entering - leaving), and
// S(xc + l) = S(xc - 1) + prefix(l); lane 63's S is the next chunk's S(xc - 1).  The first S(x0 - 1) of a segment is the clipped window
// of column x0 - 1, summed with lane l taking lo + l, lo + l + 64, .. and folded by lanes 32, 16, .. 1 apart.
//
// What is added to what, in which order, is a function of (Ho, Wo, r) alone: no atomics, nothing depends on grid size, CU count or
// addresses.  All loads and stores are 4- or 8-byte accesses of single elements INSIDE the Ho x Wo image (the lanes of a row's last chunk
// that lie past its end load nothing and only carry the scan), so an unaligned view takes the same path as an aligned one.  A vertical sum is carried across at most 2 * 2047 updates behind the <= 2 r + 1 <= 4097 terms of its restart; a horizontal one
// takes one rounding per chunk in the carry (64 per segment) and six in the scan, behind a restart of ceil((2 r + 1) / 64) + 6 additions.
#include "wct_common.h"
#include <float.h>

namespace {

constexpr int SM_VTHREADS = 64;    // vertical walkers per workgroup: one wave, so that a narrow image still spreads over the CUs
constexpr int SM_HTHREADS = 256;   // four waves = four (row, segment) pairs per workgroup
constexpr int SM_HSEG = 4096;      // columns per horizontal restart

// the conversion of misc.hip planar_to_u8_kernel (and color.hip): mul(255), + 0.5 with round_mode 1, clamp, truncation
__device__ __forceinline__ unsigned to_u8(float v, int round_mode) {
  float x = __fmul_rn(v, 255.0f);
  if (round_mode) x = __fadd_rn(x, 0.5f);
  x = fminf(fmaxf(x, 0.f), 255.f);     // NaN -> 0
  return (unsigned)x;                  // truncation toward zero
}

template <int STAGE> struct Quant { static constexpr int N = STAGE == 1 ? 21 : 12; };

// one image row's sample of column x, added to (SIGN = +1) or dropped from (-1) the accumulators.  Stage 1: A = guide (row stride aW),
// B = source; quantities I0 I1 I2 | p0 p1 p2 | I0I0 I0I1 I0I2 I1I1 I1I2 I2I2 | I_i p_c at 12 + 3 i + c; every product of two fp32
// values is exact in fp64 and enters through one fma.  Stage 2: A = the 12 planes of (a, b).
template <int STAGE, int SIGN>
__device__ __forceinline__ void take_row(double (&acc)[Quant<STAGE>::N], const float* __restrict__ A, size_t aplane, int aW,
                                         const float* __restrict__ B, size_t bplane, int bW, int y, int x) {
  if constexpr (STAGE == 1) {
    const size_t ia = (size_t)y * aW + x, ib = (size_t)y * bW + x;
    const double s = SIGN;
    const double I0 = A[ia], I1 = A[aplane + ia], I2 = A[2 * aplane + ia];
    const double p0 = B[ib], p1 = B[bplane + ib], p2 = B[2 * bplane + ib];
    const double J0 = s * I0, J1 = s * I1, J2 = s * I2;   // exact: s is +-1
    acc[0] += J0; acc[1] += J1; acc[2] += J2;
    acc[3] += s * p0; acc[4] += s * p1; acc[5] += s * p2;
    acc[6] = fma(J0, I0, acc[6]); acc[7] = fma(J0, I1, acc[7]); acc[8] = fma(J0, I2, acc[8]);
    acc[9] = fma(J1, I1, acc[9]); acc[10] = fma(J1, I2, acc[10]); acc[11] = fma(J2, I2, acc[11]);
    acc[12] = fma(J0, p0, acc[12]); acc[13] = fma(J0, p1, acc[13]); acc[14] = fma(J0, p2, acc[14]);
    acc[15] = fma(J1, p0, acc[15]); acc[16] = fma(J1, p1, acc[16]); acc[17] = fma(J1, p2, acc[17]);
    acc[18] = fma(J2, p0, acc[18]); acc[19] = fma(J2, p1, acc[19]); acc[20] = fma(J2, p2, acc[20]);
  } else {
    const size_t ia = (size_t)y * aW + x;
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] += (double)SIGN * (double)A[k * aplane + ia];
  }
}

// V[k][y][x] = sum over the rows of the clipped window of y of quantity k at column x
template <int STAGE>
__global__ __launch_bounds__(SM_VTHREADS) void smooth_vert_kernel(const float* __restrict__ A, size_t aplane, int aW, const float* __restrict__ B,
                                                                  size_t bplane, int bW, int Ho, int Wo, int r, int vseg, double* __restrict__ V) {
  constexpr int NQ = Quant<STAGE>::N;
  const int x = blockIdx.x * SM_VTHREADS + threadIdx.x;
  if (x >= Wo) return;
  const int ys = blockIdx.y * vseg, ye = ys + vseg < Ho ? ys + vseg : Ho;
  const size_t plane = (size_t)Ho * Wo;
  double acc[NQ];
#pragma unroll
  for (int k = 0; k < NQ; ++k) acc[k] = 0.0;
  const int lo = ys - r > 0 ? ys - r : 0, hi = ys + r < Ho - 1 ? ys + r : Ho - 1;
  for (int yy = lo; yy <= hi; ++yy) take_row<STAGE, 1>(acc, A, aplane, aW, B, bplane, bW, yy, x);
  double* v = V + (size_t)ys * Wo + x;
#pragma unroll
  for (int k = 0; k < NQ; ++k) v[k * plane] = acc[k];
  for (int y = ys + 1; y < ye; ++y) {
    const int en = y + r, lv = y - r - 1;
    if (en < Ho) take_row<STAGE, 1>(acc, A, aplane, aW, B, bplane, bW, en, x);
    if (lv >= 0) take_row<STAGE, -1>(acc, A, aplane, aW, B, bplane, bW, lv, x);
    v += Wo;
#pragma unroll
    for (int k = 0; k < NQ; ++k) v[k * plane] = acc[k];
  }
}

__device__ __forceinline__ int window_count(int c, int r, int n) {
  const int lo = c - r > 0 ? c - r : 0, hi = c + r < n - 1 ? c + r : n - 1;
  return hi - lo + 1;
}

// stage 1: `out_ab` (12 fp32 planes) from the 21 window means; stage 2: out_planar or out_hwc from the 12 window means and the guide
template <int STAGE>
__global__ __launch_bounds__(SM_HTHREADS) void smooth_horiz_kernel(const double* __restrict__ V, int Ho, int Wo, int r, int nseg, double eps,
                                                                   float* __restrict__ out_ab, const float* guide, size_t gplane, int Wg,
                                                                   float* out_planar, uint8_t* out_hwc, int round_mode) {
  constexpr int NQ = Quant<STAGE>::N;
  const int lane = threadIdx.x & 63;
  const long wid = (long)blockIdx.x * (SM_HTHREADS / 64) + (threadIdx.x >> 6);
  if (wid >= (long)Ho * nseg) return;   // uniform over the wave
  const int y = (int)(wid / nseg), sg = (int)(wid - (long)y * nseg);
  const int x0 = sg * SM_HSEG, x1 = x0 + SM_HSEG < Wo ? x0 + SM_HSEG : Wo;
  const size_t plane = (size_t)Ho * Wo;
  const double* row = V + (size_t)y * Wo;

  double carry[NQ];   // S(xc - 1): the window sums of the column in front of the chunk
  {
    const int lo = x0 - 1 - r > 0 ? x0 - 1 - r : 0, hi = x0 - 1 + r < Wo - 1 ? x0 - 1 + r : Wo - 1;
#pragma unroll
    for (int k = 0; k < NQ; ++k) carry[k] = 0.0;
    for (int xx = lo + lane; xx <= hi; xx += 64)
#pragma unroll
      for (int k = 0; k < NQ; ++k) carry[k] += row[k * plane + xx];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
      for (int k = 0; k < NQ; ++k) carry[k] += __shfl_down(carry[k], off, 64);
#pragma unroll
    for (int k = 0; k < NQ; ++k) carry[k] = __shfl(carry[k], 0, 64);
  }
  const double ny = (double)window_count(y, r, Ho);

  for (int xc = x0; xc < x1; xc += 64) {
    const int x = xc + lane, xe = x + r, xd = x - r - 1;
    double S[NQ];
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
      const double e = xe < Wo ? row[k * plane + xe] : 0.0;
      const double l = xd >= 0 && xd < Wo ? row[k * plane + xd] : 0.0;   // xd >= Wo: a lane past the row's ragged end (x >= Wo, r < 62)
      S[k] = e - l;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1)
#pragma unroll
      for (int k = 0; k < NQ; ++k) {
        const double t = __shfl_up(S[k], off, 64);
        if (lane >= off) S[k] += t;
      }
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
      S[k] = carry[k] + S[k];
      carry[k] = __shfl(S[k], 63, 64);
    }
    if (x >= x1) continue;   // the row's ragged end: these lanes carried the scan and hold nothing to write
    const double inv = 1.0 / (ny * (double)window_count(x, r, Wo));   // every mean is sum * (1 / count)
    const size_t o = (size_t)y * Wo + x;
    if constexpr (STAGE == 1) {
      const double m0 = S[0] * inv, m1 = S[1] * inv, m2 = S[2] * inv;   // mean_I
      const double q0 = S[3] * inv, q1 = S[4] * inv, q2 = S[5] * inv;   // mean_p
      const double s00 = fma(-m0, m0, S[6] * inv) + eps, s01 = fma(-m0, m1, S[7] * inv), s02 = fma(-m0, m2, S[8] * inv);
      const double s11 = fma(-m1, m1, S[9] * inv) + eps, s12 = fma(-m1, m2, S[10] * inv), s22 = fma(-m2, m2, S[11] * inv) + eps;
      // Sigma = L L^T; the pivots are >= eps in exact arithmetic, and the floor keeps round-off under a tiny eps from making a NaN
      const double i00 = 1.0 / sqrt(fmax(s00, DBL_MIN));
      const double l10 = s01 * i00, l20 = s02 * i00;
      const double i11 = 1.0 / sqrt(fmax(fma(-l10, l10, s11), DBL_MIN));
      const double l21 = fma(-l20, l10, s12) * i11;
      const double i22 = 1.0 / sqrt(fmax(fma(-l21, l21, fma(-l20, l20, s22)), DBL_MIN));
      const double mp[3] = {q0, q1, q2};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double c0 = fma(-m0, mp[c], S[12 + c] * inv), c1 = fma(-m1, mp[c], S[15 + c] * inv), c2 = fma(-m2, mp[c], S[18 + c] * inv);   // cov_Ip column c
        const double z0 = c0 * i00, z1 = fma(-l10, z0, c1) * i11, z2 = fma(-l21, z1, fma(-l20, z0, c2)) * i22;
        const double a2 = z2 * i22, a1 = fma(-l21, a2, z1) * i11, a0 = fma(-l20, a2, fma(-l10, a1, z0)) * i00;
        const double b = mp[c] - fma(a2, m2, fma(a1, m1, a0 * m0));
        out_ab[(size_t)(0 + c) * plane + o] = (float)a0;
        out_ab[(size_t)(3 + c) * plane + o] = (float)a1;
        out_ab[(size_t)(6 + c) * plane + o] = (float)a2;
        out_ab[(size_t)(9 + c) * plane + o] = (float)b;
      }
    } else {
      const size_t g = (size_t)y * Wg + x;
      const double I0 = guide[g], I1 = guide[gplane + g], I2 = guide[2 * gplane + g];
      float q[3];
#pragma unroll
      for (int c = 0; c < 3; ++c)
        q[c] = (float)fma(S[6 + c] * inv, I2, fma(S[3 + c] * inv, I1, fma(S[c] * inv, I0, S[9 + c] * inv)));
      if (out_planar) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out_planar[(size_t)c * plane + o] = q[c];
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) out_hwc[o * 3 + c] = (uint8_t)to_u8(q[c], round_mode);
      }
    }
  }
}

}  // namespace

int smooth_vseg(int r) { const int s = 4 * r; return s < 128 ? 128 : s > 2048 ? 2048 : s; }
int smooth_hseg() { return SM_HSEG; }
size_t smooth_sums_bytes(long npix) { return (size_t)21 * sizeof(double) * (size_t)npix; }
size_t smooth_ab_bytes(long npix) { return (size_t)12 * sizeof(float) * (size_t)npix; }

hipError_t launch_guided_filter(const float* src, int Ho, int Wo, const float* guide, int Hg, int Wg, int r, double eps, float* out_planar,
                                uint8_t* out_hwc, int round_mode, double* sums, size_t sums_bytes, float* ab, size_t ab_bytes, hipStream_t s) {
  // arguments are checked where they can be answered with a message (api_image.hip); this one guards the intermediates' bounds
  const long npix = (long)Ho * Wo;
  if (sums_bytes < smooth_sums_bytes(npix) || ab_bytes < smooth_ab_bytes(npix)) return hipErrorInvalidValue;
  const int vseg = smooth_vseg(r), nseg = (Wo + SM_HSEG - 1) / SM_HSEG;
  const dim3 vgrid((unsigned)((Wo + SM_VTHREADS - 1) / SM_VTHREADS), (unsigned)((Ho + vseg - 1) / vseg));
  const dim3 hgrid((unsigned)(((long)Ho * nseg + SM_HTHREADS / 64 - 1) / (SM_HTHREADS / 64)));
  const size_t gplane = (size_t)Hg * Wg, plane = (size_t)npix;
  hipLaunchKernelGGL(smooth_vert_kernel<1>, vgrid, dim3(SM_VTHREADS), 0, s, guide, gplane, Wg, src, plane, Wo, Ho, Wo, r, vseg, sums);
  hipLaunchKernelGGL(smooth_horiz_kernel<1>, hgrid, dim3(SM_HTHREADS), 0, s, sums, Ho, Wo, r, nseg, eps, ab, nullptr, (size_t)0, 0, nullptr, nullptr, 0);
  hipLaunchKernelGGL(smooth_vert_kernel<2>, vgrid, dim3(SM_VTHREADS), 0, s, ab, plane, Wo, nullptr, (size_t)0, 0, Ho, Wo, r, vseg, sums);
  hipLaunchKernelGGL(smooth_horiz_kernel<2>, hgrid, dim3(SM_HTHREADS), 0, s, sums, Ho, Wo, r, nseg, eps, nullptr, guide, gplane, Wg, out_planar, out_hwc,
                     round_mode);
  return hipGetLastError();
}
