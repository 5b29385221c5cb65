// K-means on NHWC fp32 feature maps (include/wct_hip_guided.h): the label maps of wct_stylize_guided when no segmentation exists.
// Distances are taken in per-image standardised space z_c = (x_c - sh_c) * sc_c (subtraction, then product: two fp32 roundings, never
// fused), d_k = sum_c (z_c - m_kc)^2 in fp32.  Kernels, all new:
//   kmeans_assign_kernel       one Lloyd step in one pass: label = arg-min_k d_k (lowest k on ties), and per workgroup the fp64 totals of z
//                              per label, the pixel counts and the sum of min d
//   kmeans_reduce_kernel       the workgroups' partials in a fixed order -> n[K], sum[K][C], cost
//   kmeans_next_kernel         next_k = sum_k / n_k, an empty cluster stays where it was
//   kmeans_seed_pass_kernel    one pass of the farthest-first start: min distance to the centres chosen so far, arg-max of it per workgroup
//   kmeans_seed_pick_kernel    the arg-max over the workgroups -> idx[j], centroids[j]
//   kmeans_standardise_kernel  (sh, sc) = (mean, 1 / sqrt(population variance)) from raw moments, sc = 0 for a dead channel
//   kmeans_expand_kernel       a level's label map at image resolution
//
// The assign pass.  A workgroup (256 threads) walks its chunk of the map in tiles of 64 pixels.  Phase 1: LP = 1 .. 16 neighbouring lanes
// share a pixel and read its channels as 16-byte loads, 16 lanes = 256 contiguous bytes, against the K x C centroid table in LDS (fp32,
// <= 16 KB; the 4 pixels of a wave read the same table words: a broadcast); every lane keeps K partial distances over its channels in
// ascending order, an xor butterfly over the LP lanes adds them -- the order is a function of C alone.  Phase 2: thread (slice, c) re-reads
// channel c of every nslice-th pixel of the tile (64 C floats, just read: cache hits, consecutive lanes = consecutive addresses), forms z
// again and adds it in fp64 to one of K registers chosen by the pixel's label (the other K - 1 get + 0.0, which is exact): no atomics
// on floating point anywhere.  Slices are added in order at the end; the grid is a function of the pixel count alone, so n, sum and cost
// are bitwise reproducible.  HBM traffic: the map once.
#include "wct_common.h"
#include <algorithm>

namespace {

constexpr int KM_TP = 64;        // pixels per tile
constexpr int KM_MAXK = 8;
constexpr int KM_MAXC = 512;
constexpr int KM_MAXWG = 1024;   // workgroups of a pass (4 per CU): the partials stay at 33 MB for K = 8, C = 512

// z = (x - sh) * sc: the subtraction first, then the product, both rounded to fp32
__device__ __forceinline__ float km_z(float x, float sh, float sc) {
#pragma clang fp contract(off)
  const float d = x - sh;
  return d * sc;
}

__device__ __forceinline__ unsigned long long km_shfl_xor_u64(unsigned long long v, int o) {
  const unsigned lo = __shfl_xor((unsigned)(v & 0xffffffffull), o), hi = __shfl_xor((unsigned)(v >> 32), o);
  return ((unsigned long long)hi << 32) | lo;
}

struct KmPlan {
  int LP, nslice, nwg;
  long chunk;
};

KmPlan km_plan(int C, long npix) {
  KmPlan p{};
  const int c4n = C >> 2;
  p.LP = 1;
  while (p.LP < 16 && p.LP < c4n) p.LP <<= 1;
  p.nslice = C >= 256 ? 1 : std::min(KM_TP, 256 / C);
  const long ntiles = (npix + KM_TP - 1) / KM_TP;
  const long nwg = std::min<long>(ntiles, KM_MAXWG);
  p.chunk = (ntiles + nwg - 1) / nwg * KM_TP;
  p.nwg = (int)((npix + p.chunk - 1) / p.chunk);
  return p;
}

struct KmArgs {
  const float* x;
  const double *shift, *scale, *cent;
  uint8_t* labels;       // may be null
  double* part;          // [nwg][K * C + K + 1]: sums | counts | cost
  int C, K, LP, nslice;
  long npix, chunk;
};

__global__ __launch_bounds__(256) void kmeans_assign_kernel(KmArgs a) {
  __shared__ __attribute__((aligned(16))) float m_s[KM_MAXK * KM_MAXC];
  __shared__ __attribute__((aligned(16))) float sh_s[KM_MAXC];
  __shared__ __attribute__((aligned(16))) float sc_s[KM_MAXC];
  __shared__ double red_s[KM_MAXK * 256];
  __shared__ float dmin_s[KM_TP];
  __shared__ int lab_s[KM_TP];
  __shared__ unsigned cnt_s[KM_MAXK];
  const int tid = threadIdx.x, C = a.C, K = a.K, c4n = C >> 2;
  for (int e = tid; e < K * C; e += 256) m_s[e] = (float)a.cent[e];
  for (int e = tid; e < C; e += 256) { sh_s[e] = (float)a.shift[e]; sc_s[e] = (float)a.scale[e]; }
  if (tid < KM_MAXK) cnt_s[tid] = 0u;
  __syncthreads();
  const int LP = a.LP, sub = tid & (LP - 1), grp = tid / LP, ngrp = 256 / LP;
  const int nslice = a.nslice;
  const bool active = C > 256 || tid < nslice * C;
  const int slice = C > 256 ? 0 : tid / C, c0 = C > 256 ? tid : tid - slice * C;
  double acc[2][KM_MAXK];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int k = 0; k < KM_MAXK; ++k) acc[j][k] = 0.;
  double cost = 0.;
  const long p0 = (long)blockIdx.x * a.chunk, p1 = min(a.npix, p0 + a.chunk);
  for (long pt = p0; pt < p1; pt += KM_TP) {
    const int tp = (int)min((long)KM_TP, p1 - pt);
    // phase 1: labels of the tile (the trip count is uniform over a wave: the butterfly below has every lane)
    for (int px = grp; px < KM_TP; px += ngrp) {
      const bool live = px < tp;
      float d[KM_MAXK];
#pragma unroll
      for (int k = 0; k < KM_MAXK; ++k) d[k] = 0.f;
      if (live) {
        const float* row = a.x + (pt + px) * C;
        for (int q = sub; q < c4n; q += LP) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * q);
          const f32x4 sh = *reinterpret_cast<const f32x4*>(sh_s + 4 * q), sc = *reinterpret_cast<const f32x4*>(sc_s + 4 * q);
          float z[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) z[i] = km_z(v[i], sh[i], sc[i]);
#pragma unroll
          for (int k = 0; k < KM_MAXK; ++k) {
            if (k < K) {
              const f32x4 m = *reinterpret_cast<const f32x4*>(m_s + k * C + 4 * q);
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const float t = z[i] - m[i];
                d[k] = fmaf(t, t, d[k]);
              }
            }
          }
        }
      }
      for (int o = 1; o < LP; o <<= 1) {
#pragma unroll
        for (int k = 0; k < KM_MAXK; ++k) d[k] += __shfl_xor(d[k], o);
      }
      if (sub == 0) {
        int best = 255;
        float bd = 0.f;
        if (live) {
          best = 0; bd = d[0];
#pragma unroll
          for (int k = 1; k < KM_MAXK; ++k)
            if (k < K && d[k] < bd) { bd = d[k]; best = k; }
          if (a.labels) a.labels[pt + px] = (uint8_t)best;
          atomicAdd(&cnt_s[best], 1u);
        }
        lab_s[px] = best;
        dmin_s[px] = bd;
      }
    }
    __syncthreads();
    // phase 2: fp64 totals of z per label; thread (slice, c0) owns channels c0 and c0 + 256 of the pixels slice, slice + nslice, ...
    if (active) {
      for (int px = slice; px < tp; px += nslice) {
        const int l = lab_s[px];
        const float* row = a.x + (pt + px) * C;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int c = c0 + 256 * j;
          if (c < C) {
            const double z = (double)km_z(row[c], sh_s[c], sc_s[c]);
#pragma unroll
            for (int k = 0; k < KM_MAXK; ++k) acc[j][k] += (l == k) ? z : 0.;
          }
        }
      }
    }
    if (tid < KM_TP) cost += (double)dmin_s[tid];
    __syncthreads();
  }
  const long E = (long)K * C + K + 1;
  double* dst = a.part + (size_t)blockIdx.x * E;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KM_MAXK; ++k) red_s[k * 256 + tid] = acc[j][k];
    __syncthreads();
    const int c = c0 + 256 * j;
    if (active && slice == 0 && c < C) {
      for (int k = 0; k < K; ++k) {
        double v = 0.;
        for (int s = 0; s < nslice; ++s) v += red_s[k * 256 + s * C + c0];
        dst[(long)k * C + c] = v;
      }
    }
  }
  if (tid < K) dst[(long)K * C + tid] = (double)cnt_s[tid];
  if (tid < 64) {                                           // wave 0 holds the tile costs, one pixel slot per lane
    for (int o = 1; o < 64; o <<= 1) cost += __shfl_xor(cost, o);
    if (tid == 0) dst[(long)K * C + K] = cost;
  }
}

// partials -> sum[K][C], n[K], cost in a fixed order (16 slices of the workgroup index, then the slices in order)
__global__ __launch_bounds__(256) void kmeans_reduce_kernel(const double* part, int nwg, int K, int C, double* n, double* sum, double* cost) {
  __shared__ double red[16][17];
  const int el = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const long E = (long)K * C + K + 1, e = (long)blockIdx.x * 16 + el;
  double v = 0.;
  if (e < E)
    for (int g = sl; g < nwg; g += 16) v += part[(size_t)g * E + e];
  red[sl][el] = v;
  __syncthreads();
  if (sl != 0 || e >= E) return;
  v = 0.;
#pragma unroll
  for (int q = 0; q < 16; ++q) v += red[q][el];
  if (e < (long)K * C) sum[e] = v;
  else if (e < (long)K * C + K) n[e - (long)K * C] = v;
  else cost[0] = v;
}

__global__ void kmeans_next_kernel(const double* cent, const double* n, const double* sum, int K, int C, double* next) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= K * C) return;
  const double nk = n[e / C];
  next[e] = nk > 0. ? sum[e] / nk : cent[e];
}

// ---- farthest-first start -----------------------------------------------------------------------------------------------------
// Pass j: d(z_p, centre_{j-1}) (centre_{-1} = 0: the norm), mind_p = min(mind_p, d) (pass 0: = d), and the arg-max of mind with the lowest
// pixel index on ties as the maximum of the 64-bit key (bits of mind | ~index): an integer maximum, any order gives the same answer.
struct KmSeedArgs {
  const float* x;
  const double *shift, *scale;
  float* mind;                 // [npix]
  int* idx;                    // [K]
  unsigned long long* part;    // [nwg]
  int C, LP, j, nwg;
  long npix, chunk;
};

__global__ __launch_bounds__(256) void kmeans_seed_pass_kernel(KmSeedArgs a) {
  __shared__ __attribute__((aligned(16))) float ctr_s[KM_MAXC];
  __shared__ __attribute__((aligned(16))) float sh_s[KM_MAXC];
  __shared__ __attribute__((aligned(16))) float sc_s[KM_MAXC];
  __shared__ unsigned long long best_s[4];
  const int tid = threadIdx.x, C = a.C, c4n = C >> 2;
  const long pc = a.j > 0 ? (long)a.idx[a.j - 1] : 0;
  for (int e = tid; e < C; e += 256) {
    const float sh = (float)a.shift[e], sc = (float)a.scale[e];
    sh_s[e] = sh; sc_s[e] = sc;
    ctr_s[e] = a.j > 0 ? km_z(a.x[pc * C + e], sh, sc) : 0.f;
  }
  __syncthreads();
  const int LP = a.LP, sub = tid & (LP - 1), grp = tid / LP, ngrp = 256 / LP;
  unsigned long long best = 0ull;
  const long p0 = (long)blockIdx.x * a.chunk, p1 = min(a.npix, p0 + a.chunk);
  for (long pt = p0; pt < p1; pt += KM_TP) {
    const int tp = (int)min((long)KM_TP, p1 - pt);
    for (int px = grp; px < KM_TP; px += ngrp) {
      const bool live = px < tp;
      float d = 0.f;
      if (live) {
        const float* row = a.x + (pt + px) * C;
        for (int q = sub; q < c4n; q += LP) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * q);
          const f32x4 sh = *reinterpret_cast<const f32x4*>(sh_s + 4 * q), sc = *reinterpret_cast<const f32x4*>(sc_s + 4 * q);
          const f32x4 m = *reinterpret_cast<const f32x4*>(ctr_s + 4 * q);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float t = km_z(v[i], sh[i], sc[i]) - m[i];
            d = fmaf(t, t, d);
          }
        }
      }
      for (int o = 1; o < LP; o <<= 1) d += __shfl_xor(d, o);
      if (live && sub == 0) {
        const long p = pt + px;
        if (a.j > 0) d = fminf(a.mind[p], d);
        a.mind[p] = d;
        const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(0xffffffffu - (unsigned)p);
        best = key > best ? key : best;
      }
    }
  }
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long other = km_shfl_xor_u64(best, o);
    best = other > best ? other : best;
  }
  if ((tid & 63) == 0) best_s[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    for (int q = 1; q < 4; ++q) best = best_s[q] > best ? best_s[q] : best;
    a.part[blockIdx.x] = best;
  }
}

__global__ __launch_bounds__(256) void kmeans_seed_pick_kernel(KmSeedArgs a, double* cent) {
  __shared__ unsigned long long best_s[4];
  const int tid = threadIdx.x, C = a.C;
  unsigned long long best = 0ull;
  for (int g = tid; g < a.nwg; g += 256) best = a.part[g] > best ? a.part[g] : best;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long other = km_shfl_xor_u64(best, o);
    best = other > best ? other : best;
  }
  if ((tid & 63) == 0) best_s[tid >> 6] = best;
  __syncthreads();
  best = best_s[0];
  for (int q = 1; q < 4; ++q) best = best_s[q] > best ? best_s[q] : best;
  long p = (long)(0xffffffffu - (unsigned)(best & 0xffffffffull));
  if (p >= a.npix) p = 0;                                   // cannot happen with a live pixel in every workgroup; keeps the gather in the map
  if (tid == 0) a.idx[a.j] = (int)p;
  for (int e = tid; e < C; e += 256) cent[(long)a.j * C + e] = (double)km_z(a.x[p * C + e], (float)a.shift[e], (float)a.scale[e]);
}

// ---- standardisation from raw moments ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void kmeans_standardise_kernel(const double* sum, const double* sumsq, int C, double n, double* shift, double* scale) {
#pragma clang fp contract(off)
  __shared__ double var_s[KM_MAXC];
  const int c = threadIdx.x;
  double mu = 0., var = 0.;
  if (c < C) {
    mu = sum[c] / n;
    const double q = sumsq[(size_t)c * C + c] / n, m2 = mu * mu;
    var = q - m2;
  }
  var_s[c] = c < C ? var : 0.;
  __syncthreads();
  for (int o = 256; o > 0; o >>= 1) {
    if (c < o) var_s[c] = fmax(var_s[c], var_s[c + o]);
    __syncthreads();
  }
  const double vmax = var_s[0];
  if (c < C) {
    shift[c] = mu;
    scale[c] = var > 1e-12 * vmax ? 1.0 / sqrt(var) : 0.;
  }
}

__global__ void kmeans_expand_kernel(const uint8_t* lab, int h, int w, int sh, uint8_t* out, int H, int W) {
  const long total = (long)H * W;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int y = (int)(e / W), x = (int)(e - (long)y * W);
    out[e] = lab[(long)min(y >> sh, h - 1) * w + min(x >> sh, w - 1)];
  }
}

bool km_shape_ok(int C, long npix, int K) { return C >= 4 && !(C & 3) && C <= KM_MAXC && npix >= 1 && npix < (1L << 31) && K >= 1 && K <= KM_MAXK; }

}  // namespace

size_t kmeans_assign_workspace_bytes(int C, long npix, int K) {
  const KmPlan p = km_plan(C, npix);
  return (size_t)p.nwg * ((size_t)K * C + K + 1) * sizeof(double);
}

hipError_t launch_kmeans_assign(const float* feat, int C, long npix, const double* shift, const double* scale, const double* cent, int K,
                                uint8_t* labels, double* n, double* sum, double* cost, double* next, void* ws, size_t ws_bytes, hipStream_t s) {
  if (!km_shape_ok(C, npix, K)) return hipErrorInvalidValue;
  if (ws_bytes < kmeans_assign_workspace_bytes(C, npix, K)) return hipErrorOutOfMemory;
  const KmPlan p = km_plan(C, npix);
  KmArgs a{};
  a.x = feat; a.shift = shift; a.scale = scale; a.cent = cent; a.labels = labels; a.part = reinterpret_cast<double*>(ws);
  a.C = C; a.K = K; a.LP = p.LP; a.nslice = p.nslice; a.npix = npix; a.chunk = p.chunk;
  hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)p.nwg), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const long E = (long)K * C + K + 1;
  hipLaunchKernelGGL(kmeans_reduce_kernel, dim3((unsigned)((E + 15) / 16)), dim3(256), 0, s, a.part, p.nwg, K, C, n, sum, cost);
  e = hipGetLastError();
  if (e != hipSuccess || !next) return e;
  hipLaunchKernelGGL(kmeans_next_kernel, dim3((unsigned)((K * C + 255) / 256)), dim3(256), 0, s, cent, n, sum, K, C, next);
  return hipGetLastError();
}

size_t kmeans_seed_workspace_bytes(long npix) { return ((size_t)npix * sizeof(float) + 255) / 256 * 256 + KM_MAXWG * sizeof(unsigned long long); }

hipError_t launch_kmeans_seed(const float* feat, int C, long npix, const double* shift, const double* scale, int K, double* cent, int* idx,
                              void* ws, size_t ws_bytes, hipStream_t s) {
  if (!km_shape_ok(C, npix, K)) return hipErrorInvalidValue;
  if (ws_bytes < kmeans_seed_workspace_bytes(npix)) return hipErrorOutOfMemory;
  const KmPlan p = km_plan(C, npix);
  KmSeedArgs a{};
  a.x = feat; a.shift = shift; a.scale = scale; a.idx = idx;
  a.mind = reinterpret_cast<float*>(ws);
  a.part = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(ws) + ((size_t)npix * sizeof(float) + 255) / 256 * 256);
  a.C = C; a.LP = p.LP; a.nwg = p.nwg; a.npix = npix; a.chunk = p.chunk;
  for (int j = 0; j < K; ++j) {
    a.j = j;
    hipLaunchKernelGGL(kmeans_seed_pass_kernel, dim3((unsigned)p.nwg), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kmeans_seed_pick_kernel, dim3(1), dim3(256), 0, s, a, cent);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_kmeans_standardise(const double* sum, const double* sumsq, int C, double n, double* shift, double* scale, hipStream_t s) {
  if (C < 1 || C > KM_MAXC || !(n >= 1)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kmeans_standardise_kernel, dim3(1), dim3(512), 0, s, sum, sumsq, C, n, shift, scale);
  return hipGetLastError();
}

hipError_t launch_kmeans_expand(const uint8_t* lab, int h, int w, int level, uint8_t* out, int H, int W, hipStream_t s) {
  if (h < 1 || w < 1 || H < 1 || W < 1 || level < 1 || level > 5) return hipErrorInvalidValue;
  const long total = (long)H * W;
  hipLaunchKernelGGL(kmeans_expand_kernel, dim3((unsigned)std::min(4096L, (total + 255) / 256)), dim3(256), 0, s, lab, h, w, level - 1, out, H, W);
  return hipGetLastError();
}
