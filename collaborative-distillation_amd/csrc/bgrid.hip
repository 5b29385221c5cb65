// Proxy mode's bilateral grid (include/wct_hip_bgrid.h): the fit of a field of 3 x 4 affine colour maps from a reduced (content, result)
// pair, and the slice that applies the field to the full-resolution content.
//
//   fit     accum     one workgroup per (spatial vertex (j, i), row chunk c): a GATHER -- the vertex's support is the reduced pixels within
//                     one cell of it, nothing is scattered.  The x and y tent weights of the chunk go into LDS once.  Wave wv takes the
//                     z vertices k = wv, wv + 4, ..; its 64 lanes stride the chunk's pixels in row-major order, each with the 22 fp64
//                     sums (Gv 10, Rv 12) of vertex (k, j, i) in registers; a fold 32, 16, .. 1 lanes apart; lane 0 writes the
//                     chunk's partial.  The reduced image is small and is re-read
//                     from L2 by every vertex that it supports and every z wave: latency, not throughput
//           combine   adds the chunks in ascending order (skipped when no support is taller than one chunk)
//           blur      [1 2 1] / 4 along one axis, the edge vertex repeated; 3 x smooth launches, ping-pong
//           totals    slabs of 256 vertices, one wave each, then one wave over the slabs, whose lane 0 solves Ag
//           solve     one thread per vertex: Cholesky of Gv + lambda I, 3 right-hand sides, the single rounding to fp32
//   slice   one workgroup per 128 x 8 tile of full-resolution pixels, a thread per 4 adjacent pixels of a row.  The tile's vertex
//           footprint (all gz, 48 B per vertex) is staged into LDS once; a footprint above WCT_BGRID_LDS_VERTICES (a grid finer than
//           the pixels) is read from global memory instead -- the same template, every operation an explicit intrinsic, so both paths
//           give the same bits.  Content loads and planar stores are 16 bytes wide where the address allows, uint8 stores 4 bytes
//           wide; an unaligned view takes scalar accesses and the same arithmetic.  24 B (15 B with uint8 out) of HBM traffic per pixel.
//
// What is added to what, in which order, is a function of (h, w, gz, gh, gw, smooth) alone: no atomics, nothing depends on grid
// size, CU count or addresses.
#include "../../include/wct_hip_bgrid.h"
#include "wct_common.h"
#include <float.h>

namespace {

constexpr int BG_NS = 22;                         // distinct sums per vertex: Gv (4 x 4 symmetric) 10, Rv (4 x 3) 12
constexpr int BG_ROWS = WCT_BGRID_FIT_ROWS;
constexpr int BG_TW = WCT_BGRID_TILE_W, BG_TH = WCT_BGRID_TILE_H;
constexpr int BG_LDS_VERTS = WCT_BGRID_LDS_VERTICES;
constexpr int BG_WX = 256;                        // columns of a support whose tent weights the fit tabulates in LDS
constexpr int BG_SLAB = 256;                      // vertices per partial total

typedef float f32x4 __attribute__((ext_vector_type(4)));

// [lo, hi]: the samples of an axis (n samples, G vertices) that can have weight on vertex v -- u = (x + 0.5) / n (G - 1) in (v - 1, v + 1) --
// in integers and one sample generous on either side, so that no rounding of u can leave a weighted sample out
__host__ __device__ inline void bgrid_support(int v, int n, int G, int& lo, int& hi) {
  if (G == 1) { lo = 0; hi = n - 1; return; }
  const long a = (long)(v - 1) * n / (G - 1) - 1, b = ((long)(v + 1) * n + (G - 2)) / (G - 1);
  lo = a < 0 ? 0 : (int)a;
  hi = b > n - 1 ? n - 1 : (int)b;
}

struct Tent { int i0, i1; double f; };

// sample x of an axis with n samples and G vertices (the header's rule); monotone in x
__device__ __forceinline__ Tent tent_axis(int x, int n, int G) {
  const double u = __dmul_rn(__ddiv_rn(__dadd_rn((double)x, 0.5), (double)n), (double)(G - 1));
  const int top = G >= 2 ? G - 2 : 0;
  int i0 = (int)floor(u);
  if (i0 > top) i0 = top;
  Tent t;
  t.i0 = i0;
  t.i1 = i0 + 1 < G ? i0 + 1 : G - 1;
  t.f = __dsub_rn(u, (double)i0);
  return t;
}

__device__ __forceinline__ double guide_of(double R, double G, double B) {
  const double g = fma(0.114, B, fma(0.587, G, __dmul_rn(0.299, R)));
  return fmin(fmax(g, 0.0), 1.0);   // NaN -> 0
}

__device__ __forceinline__ Tent tent_z(double g, int gz) {
  const double u = __dmul_rn(g, (double)(gz - 1));
  const int top = gz >= 2 ? gz - 2 : 0;
  int i0 = (int)floor(u);
  if (i0 > top) i0 = top;
  Tent t;
  t.i0 = i0;
  t.i1 = i0 + 1 < gz ? i0 + 1 : gz - 1;
  t.f = __dsub_rn(u, (double)i0);
  return t;
}

// a sample's weight on vertex v of its axis (G = 1: i0 = i1 = 0 and f = 0, so 1)
__device__ __forceinline__ double tent_weight(const Tent& t, int v) {
  return (t.i0 == v ? 1.0 - t.f : 0.0) + (t.i1 == v ? t.f : 0.0);
}

// ---- fit --------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ void wave_fold(double (&acc)[BG_NS]) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
    for (int q = 0; q < BG_NS; ++q) acc[q] += __shfl_down(acc[q], off, 64);
}

__global__ __launch_bounds__(256) void bgrid_accum_kernel(const float* __restrict__ cl, const float* __restrict__ sl, int h, int w, int gz, int gh,
                                                          int gw, double* __restrict__ P) {
  const int j = blockIdx.x / gw, i = blockIdx.x - j * gw, c = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int xlo, xhi, ylo, yhi;
  bgrid_support(i, w, gw, xlo, xhi);
  bgrid_support(j, h, gh, ylo, yhi);
  const int ya = ylo + c * BG_ROWS, yb = ya + BG_ROWS < yhi + 1 ? ya + BG_ROWS : yhi + 1;
  const int rw = xhi - xlo + 1, nrows = yb - ya;   // nrows <= 0: a chunk past this vertex's support, all-zero partials
  // the tent weights of the chunk's rows and the support's columns, once per workgroup (a support wider than the table -- one vertex
  // across a large image -- evaluates its column weights in the loop)
  __shared__ double swy[BG_ROWS], swx[BG_WX];
  const bool tab = rw <= BG_WX;
  for (int t = threadIdx.x; t < nrows; t += blockDim.x) swy[t] = tent_weight(tent_axis(ya + t, h, gh), j);
  if (tab)
    for (int t = threadIdx.x; t < rw; t += blockDim.x) swx[t] = tent_weight(tent_axis(xlo + t, w, gw), i);
  __syncthreads();
  // lane l takes the chunk's pixels l, l + 64, .. in row-major order: (row, column) advance by (64 / rw, 64 % rw) with a carry
  const int dy = 64 / rw, dx = 64 - dy * rw, yy0 = lane / rw, xx0 = lane - yy0 * rw;
  const size_t plane = (size_t)h * w, nv = (size_t)gz * gh * gw;
  for (int k = wv; k < gz; k += nw) {
    double acc[BG_NS];
#pragma unroll
    for (int q = 0; q < BG_NS; ++q) acc[q] = 0.0;
    for (int yy = yy0, xx = xx0; yy < nrows;) {
      const int y = ya + yy, x = xlo + xx;
      const double wxy = swy[yy] * (tab ? swx[xx] : tent_weight(tent_axis(x, w, gw), i));
      if (wxy != 0.0) {   // the support is cut one pixel generously; a zero weight would add exact zeros
        const size_t o = (size_t)y * w + x;
        const double v[4] = {(double)cl[o], (double)cl[plane + o], (double)cl[2 * plane + o], 1.0};
        const double wt = tent_weight(tent_z(guide_of(v[0], v[1], v[2]), gz), k) * wxy;
        if (wt != 0.0) {
          const double s[3] = {(double)sl[o], (double)sl[plane + o], (double)sl[2 * plane + o]};
          int n = 0;
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            const double wa = wt * v[a];
#pragma unroll
            for (int b = a; b < 4; ++b, ++n) acc[n] = fma(wa, v[b], acc[n]);   // (0,0) (0,1) (0,2) (0,3) (1,1) .. (3,3)
          }
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            const double wa = wt * v[a];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) acc[10 + 3 * a + ch] = fma(wa, s[ch], acc[10 + 3 * a + ch]);
          }
        }
      }
      xx += dx; yy += dy;
      if (xx >= rw) { xx -= rw; ++yy; }
    }
    wave_fold(acc);
    if (lane == 0) {
      double* dst = P + ((size_t)c * nv + ((size_t)k * gh + j) * gw + i) * BG_NS;
#pragma unroll
      for (int q = 0; q < BG_NS; ++q) dst[q] = acc[q];
    }
  }
}

__global__ __launch_bounds__(256) void bgrid_combine_kernel(const double* __restrict__ P, long n, int nchunk, double* __restrict__ S) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  double a = 0.0;
  for (int c = 0; c < nchunk; ++c) a += P[(size_t)c * n + e];
  S[e] = a;
}

// axis 0: z, 1: y, 2: x
__global__ __launch_bounds__(256) void bgrid_blur_kernel(const double* __restrict__ src, int gz, int gh, int gw, int axis, double* __restrict__ dst) {
  const long n = (long)gz * gh * gw * BG_NS, e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const long v = e / BG_NS;
  const int i = (int)(v % gw), j = (int)((v / gw) % gh), k = (int)(v / ((long)gw * gh));
  const int pos = axis == 0 ? k : axis == 1 ? j : i, G = axis == 0 ? gz : axis == 1 ? gh : gw;
  const long stride = (axis == 0 ? (long)gh * gw : axis == 1 ? (long)gw : 1L) * BG_NS;
  const double lo = src[pos > 0 ? e - stride : e], hi = src[pos + 1 < G ? e + stride : e];
  dst[e] = 0.25 * ((lo + hi) + 2.0 * src[e]);
}

// L L^T = M (4 x 4 symmetric, lower triangle read); the pivots are >= lambda in exact arithmetic, the floor keeps round-off from a NaN
__device__ __forceinline__ void chol4(const double (&M)[4][4], double (&L)[4][4], double (&inv)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    double d = M[c][c];
#pragma unroll
    for (int p = 0; p < c; ++p) d = fma(-L[c][p], L[c][p], d);
    const double l = sqrt(fmax(d, DBL_MIN));
    L[c][c] = l;
    inv[c] = 1.0 / l;
#pragma unroll
    for (int r = c + 1; r < 4; ++r) {
      double t = M[r][c];
#pragma unroll
      for (int p = 0; p < c; ++p) t = fma(-L[r][p], L[c][p], t);
      L[r][c] = t * inv[c];
    }
  }
}

__device__ __forceinline__ void chol4_solve(const double (&L)[4][4], const double (&inv)[4], const double (&b)[4], double (&x)[4]) {
  double z[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    double t = b[a];
#pragma unroll
    for (int p = 0; p < a; ++p) t = fma(-L[a][p], z[p], t);
    z[a] = t * inv[a];
  }
#pragma unroll
  for (int a = 3; a >= 0; --a) {
    double t = z[a];
#pragma unroll
    for (int p = a + 1; p < 4; ++p) t = fma(-L[p][a], x[p], t);
    x[a] = t * inv[a];
  }
}

// the 22 sums -> M = Gv + lambda I (lower triangle)
__device__ __forceinline__ void gram_of(const double* s, double lambda, double (&M)[4][4]) {
  int n = 0;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = a; b < 4; ++b, ++n) M[b][a] = a == b ? s[n] + lambda : s[n];
}

__global__ __launch_bounds__(256) void bgrid_slab_kernel(const double* __restrict__ S, long nv, long nslab, double* __restrict__ T) {
  const int lane = threadIdx.x & 63;
  const long slab = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slab >= nslab) return;   // uniform over the wave
  double acc[BG_NS];
#pragma unroll
  for (int q = 0; q < BG_NS; ++q) acc[q] = 0.0;
  for (int t = 0; t < BG_SLAB / 64; ++t) {
    const long v = slab * BG_SLAB + t * 64 + lane;
    if (v < nv)
#pragma unroll
      for (int q = 0; q < BG_NS; ++q) acc[q] += S[(size_t)v * BG_NS + q];
  }
  wave_fold(acc);
  if (lane == 0)
#pragma unroll
    for (int q = 0; q < BG_NS; ++q) T[(size_t)slab * BG_NS + q] = acc[q];
}

// one wave: the totals over the slabs, then Ag = (Gg + lambda I)^-1 Rg into head[0 .. 12) as [a * 3 + ch]
__global__ __launch_bounds__(64) void bgrid_global_kernel(const double* __restrict__ T, long nslab, double lambda, double* __restrict__ head) {
  const int lane = threadIdx.x;
  double acc[BG_NS];
#pragma unroll
  for (int q = 0; q < BG_NS; ++q) acc[q] = 0.0;
  for (long s = lane; s < nslab; s += 64)
#pragma unroll
    for (int q = 0; q < BG_NS; ++q) acc[q] += T[(size_t)s * BG_NS + q];
  wave_fold(acc);
  if (lane != 0) return;
  double M[4][4], L[4][4], inv[4];
  gram_of(acc, lambda, M);
  chol4(M, L, inv);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const double b[4] = {acc[10 + ch], acc[13 + ch], acc[16 + ch], acc[19 + ch]};
    double x[4];
    chol4_solve(L, inv, b, x);
#pragma unroll
    for (int a = 0; a < 4; ++a) head[a * 3 + ch] = x[a];
  }
}

__global__ __launch_bounds__(256) void bgrid_solve_kernel(const double* __restrict__ S, long nv, double lambda, const double* __restrict__ head,
                                                          float* __restrict__ grid) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  double s[BG_NS];
#pragma unroll
  for (int q = 0; q < BG_NS; ++q) s[q] = S[(size_t)v * BG_NS + q];
  float* dst = grid + (size_t)v * 12;
  if (s[9] == 0.0) {   // the weight sum: no pixel reaches this vertex (nor, after the blur, its neighbours)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
      for (int a = 0; a < 4; ++a) dst[4 * ch + a] = (float)head[a * 3 + ch];
    return;
  }
  double M[4][4], L[4][4], inv[4];
  gram_of(s, lambda, M);
  chol4(M, L, inv);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    double b[4], x[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) b[a] = fma(lambda, head[a * 3 + ch], s[10 + 3 * a + ch]);
    chol4_solve(L, inv, b, x);
#pragma unroll
    for (int a = 0; a < 4; ++a) dst[4 * ch + a] = (float)x[a];
  }
}

// ---- slice ------------------------------------------------------------------------------------------------------------------------

// the conversion of misc.hip planar_to_u8_kernel (and color.hip): mul(255), + 0.5 with round_mode 1, clamp, truncation
__device__ __forceinline__ unsigned to_u8(float v, int round_mode) {
  float x = __fmul_rn(v, 255.0f);
  if (round_mode) x = __fadd_rn(x, 0.5f);
  x = fminf(fmaxf(x, 0.f), 255.f);     // NaN -> 0
  return (unsigned)x;                  // truncation toward zero
}

// acc += wt * (the 12 coefficients of one vertex); LDS: three 16-byte reads, global: twelve 4-byte ones (a grid has any 4-byte alignment)
template <bool LDS>
__device__ __forceinline__ void take_vertex(double (&acc)[12], double wt, const f32x4* sm, const float* __restrict__ grid, size_t vertex) {
  float a[12];
  if constexpr (LDS) {
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const f32x4 q = sm[vertex * 3 + t];
      a[4 * t] = q[0]; a[4 * t + 1] = q[1]; a[4 * t + 2] = q[2]; a[4 * t + 3] = q[3];
    }
  } else {
#pragma unroll
    for (int t = 0; t < 12; ++t) a[t] = grid[vertex * 12 + t];
  }
#pragma unroll
  for (int t = 0; t < 12; ++t) acc[t] = fma(wt, (double)a[t], acc[t]);
}

// one pixel: (jlo, ilo, nj, ni) is the LDS footprint's origin and extent (LDS), or (0, 0, gh, gw) (global)
template <bool LDS>
__device__ __forceinline__ void slice_pixel(float R32, float G32, float B32, const Tent& ty, int x, int W, int gz, int gw, int jlo, int ilo, int nj,
                                            int ni, const f32x4* sm, const float* __restrict__ grid, float (&out)[3]) {
  const double R = R32, G = G32, B = B32;
  const Tent tz = tent_z(guide_of(R, G, B), gz), tx = tent_axis(x, W, gw);
  const double wz[2] = {__dsub_rn(1.0, tz.f), tz.f}, wy[2] = {__dsub_rn(1.0, ty.f), ty.f}, wx[2] = {__dsub_rn(1.0, tx.f), tx.f};
  const int kz[2] = {tz.i0, tz.i1}, jy[2] = {ty.i0 - jlo, ty.i1 - jlo}, ix[2] = {tx.i0 - ilo, tx.i1 - ilo};
  double acc[12];
#pragma unroll
  for (int t = 0; t < 12; ++t) acc[t] = 0.0;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const double wzy = __dmul_rn(wz[a], wy[b]);
#pragma unroll
      for (int c = 0; c < 2; ++c)
        take_vertex<LDS>(acc, __dmul_rn(wzy, wx[c]), sm, grid, ((size_t)kz[a] * nj + jy[b]) * ni + ix[c]);
    }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) out[ch] = (float)fma(acc[4 * ch + 2], B, fma(acc[4 * ch + 1], G, fma(acc[4 * ch], R, acc[4 * ch + 3])));
}

__global__ __launch_bounds__(256) void bgrid_slice_kernel(const float* __restrict__ grid, int gz, int gh, int gw, const float* content, int H, int W,
                                                          float* out_planar, uint8_t* out_hwc, int round_mode, int lds_cap) {
  __shared__ f32x4 sm[BG_LDS_VERTS * 3];
  const int ntx = (W + BG_TW - 1) / BG_TW, tyi = blockIdx.x / ntx;
  const int x0 = (blockIdx.x - tyi * ntx) * BG_TW, y0 = tyi * BG_TH;
  const int x1 = x0 + BG_TW < W ? x0 + BG_TW : W, y1 = y0 + BG_TH < H ? y0 + BG_TH : H;
  // the tile's vertex footprint: tent_axis is monotone, so every pixel's two vertices lie between those of the tile's corners
  const int ilo = tent_axis(x0, W, gw).i0, ihi = tent_axis(x1 - 1, W, gw).i1;
  const int jlo = tent_axis(y0, H, gh).i0, jhi = tent_axis(y1 - 1, H, gh).i1;
  const int ni = ihi - ilo + 1, nj = jhi - jlo + 1;
  const bool lds = (long)gz * nj * ni <= (long)lds_cap;   // uniform over the workgroup; lds_cap <= BG_LDS_VERTS
  if (lds) {
    float* smf = reinterpret_cast<float*>(sm);
    const int row = ni * 12, total = gz * nj * row;
    for (int e = threadIdx.x; e < total; e += 256) {
      const int r = e / row, cc = e - r * row, k = r / nj, jj = r - k * nj;
      smf[e] = grid[(((size_t)k * gh + jlo + jj) * gw + ilo) * 12 + cc];
    }
    __syncthreads();
  }
  const int y = y0 + (threadIdx.x >> 5), xs = x0 + 4 * (threadIdx.x & 31);
  if (y >= H || xs >= W) return;
  const int n = W - xs < 4 ? W - xs : 4;
  const size_t plane = (size_t)H * W, o = (size_t)y * W + xs;
  float in[3][4], res[3][4];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float* p = content + ch * plane + o;
    if (n == 4 && (reinterpret_cast<size_t>(p) & 15) == 0) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(p);
      in[ch][0] = q[0]; in[ch][1] = q[1]; in[ch][2] = q[2]; in[ch][3] = q[3];
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) in[ch][t] = t < n ? p[t] : 0.f;
    }
  }
  const Tent ty = tent_axis(y, H, gh);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    float q[3] = {0.f, 0.f, 0.f};
    if (t < n) {
      if (lds) slice_pixel<true>(in[0][t], in[1][t], in[2][t], ty, xs + t, W, gz, gw, jlo, ilo, nj, ni, sm, grid, q);
      else slice_pixel<false>(in[0][t], in[1][t], in[2][t], ty, xs + t, W, gz, gw, 0, 0, gh, gw, sm, grid, q);
    }
    res[0][t] = q[0]; res[1][t] = q[1]; res[2][t] = q[2];
  }
  // every read of this thread's pixels is behind us, and no other thread reads them: out_planar may be the content itself
  if (out_planar) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float* p = out_planar + ch * plane + o;
      if (n == 4 && (reinterpret_cast<size_t>(p) & 15) == 0) {
        f32x4 q;
        q[0] = res[ch][0]; q[1] = res[ch][1]; q[2] = res[ch][2]; q[3] = res[ch][3];
        *reinterpret_cast<f32x4*>(p) = q;
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (t < n) p[t] = res[ch][t];
      }
    }
  } else {
    unsigned b[12];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) b[t * 3 + ch] = to_u8(res[ch][t], round_mode);
    uint8_t* p = out_hwc + o * 3;
    if (n == 4 && (reinterpret_cast<size_t>(p) & 3) == 0) {
      unsigned* dst = reinterpret_cast<unsigned*>(p);
      dst[0] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
      dst[1] = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
      dst[2] = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
    } else {
#pragma unroll
      for (int t = 0; t < 12; ++t)   // unrolled and predicated: b[] stays in registers
        if (t < n * 3) p[t] = (uint8_t)b[t];
    }
  }
}

}  // namespace

int bgrid_fit_chunks(int h, int gh) {
  int tallest = 1;
  for (int j = 0; j < gh; ++j) {
    int lo, hi;
    bgrid_support(j, h, gh, lo, hi);
    if (hi - lo + 1 > tallest) tallest = hi - lo + 1;
  }
  return (tallest + BG_ROWS - 1) / BG_ROWS;
}

namespace {
struct FitLayout { size_t nv, nslab, s0, s1, t, head, p, doubles; int nchunk; };
FitLayout fit_layout(int h, int gz, int gh, int gw) {
  FitLayout l;
  l.nv = (size_t)gz * gh * gw;
  l.nslab = (l.nv + BG_SLAB - 1) / BG_SLAB;
  l.nchunk = bgrid_fit_chunks(h, gh);
  l.s0 = 0;
  l.s1 = l.s0 + l.nv * BG_NS;
  l.t = l.s1 + l.nv * BG_NS;
  l.head = l.t + l.nslab * BG_NS;
  l.p = l.head + 16;
  l.doubles = l.p + (l.nchunk > 1 ? (size_t)l.nchunk * l.nv * BG_NS : 0);   // one chunk: the partial IS the sum
  return l;
}
}  // namespace

size_t bgrid_fit_workspace_bytes(int h, int gz, int gh, int gw) { return fit_layout(h, gz, gh, gw).doubles * sizeof(double); }

hipError_t launch_bgrid_fit(const float* cl, const float* sl, int h, int w, int gz, int gh, int gw, double eps, int smooth, float* grid, double* ws,
                            size_t ws_bytes, hipStream_t s) {
  // arguments are checked where they can be answered with a message (api_bgrid.hip); this one guards the workspace's bounds
  const FitLayout l = fit_layout(h, gz, gh, gw);
  if (ws_bytes < l.doubles * sizeof(double) || l.nchunk > 65535) return hipErrorInvalidValue;
  const long n = (long)l.nv * BG_NS;
  const unsigned eblocks = (unsigned)((n + 255) / 256);
  double *S = ws + l.s0, *S2 = ws + l.s1, *T = ws + l.t, *head = ws + l.head;
  const double lambda = eps * (double)h * (double)w / (double)l.nv;
  hipLaunchKernelGGL(bgrid_accum_kernel, dim3((unsigned)(gh * gw), (unsigned)l.nchunk), dim3(64 * (gz < 4 ? gz : 4)), 0, s, cl, sl, h, w, gz, gh, gw,
                     l.nchunk > 1 ? ws + l.p : S);
  if (l.nchunk > 1) hipLaunchKernelGGL(bgrid_combine_kernel, dim3(eblocks), dim3(256), 0, s, ws + l.p, n, l.nchunk, S);
  for (int pass = 0; pass < smooth; ++pass)
    for (int axis = 0; axis < 3; ++axis) {
      hipLaunchKernelGGL(bgrid_blur_kernel, dim3(eblocks), dim3(256), 0, s, S, gz, gh, gw, axis, S2);
      double* t = S; S = S2; S2 = t;
    }
  hipLaunchKernelGGL(bgrid_slab_kernel, dim3((unsigned)((l.nslab + 3) / 4)), dim3(256), 0, s, S, (long)l.nv, (long)l.nslab, T);
  hipLaunchKernelGGL(bgrid_global_kernel, dim3(1), dim3(64), 0, s, T, (long)l.nslab, lambda, head);
  hipLaunchKernelGGL(bgrid_solve_kernel, dim3((unsigned)((l.nv + 255) / 256)), dim3(256), 0, s, S, (long)l.nv, lambda, head, grid);
  return hipGetLastError();
}

hipError_t launch_bgrid_slice(const float* grid, int gz, int gh, int gw, const float* content, int H, int W, float* out_planar, uint8_t* out_hwc,
                              int round_mode, bool use_lds, hipStream_t s) {
  const long ntiles = (long)((W + BG_TW - 1) / BG_TW) * ((H + BG_TH - 1) / BG_TH);
  if (ntiles > 2147483647L) return hipErrorInvalidValue;
  const dim3 tiles((unsigned)ntiles);
  hipLaunchKernelGGL(bgrid_slice_kernel, tiles, dim3(256), 0, s, grid, gz, gh, gw, content, H, W, out_planar, out_hwc, round_mode,
                     use_lds ? BG_LDS_VERTS : 0);
  return hipGetLastError();
}
