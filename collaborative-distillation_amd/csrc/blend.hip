// Style interpolation and per-pixel style weights (wct_stylize_interp, wct_style_blend, wct_stylize_blend).
//   Tier 1 (uniform weights lambda_k): whiten_and_color is linear in the style statistics, so sum_k lambda_k WCT(fc, fs_k) is ONE
//   blended style slot (sum_k lambda_k S_k, sum_k lambda_k mu_s,k) followed by the unchanged single-style content path.
//   Tier 2 (weight maps w_k(p) in [0, 1], sum_k w_k <= 1): per level, the pooled maps w_k,L (area means over each feature pixel's
//   window), reliability-weighted content moments per k, and out_p = x_p + sum_k w_k,L(p) ((M_k x_p + b_k) - x_p).
// Kernels (all new; no single-style or regions kernel goes through here):
//   stats_blend_kernel       F = sum_k lambda_k F_k, mu = sum_k lambda_k mu_k in a fixed k order (lambda = e_0 gives slot 0 bit for bit)
//   weights_pool_kernel      the pooled level maps of levels 1..5 and per-block (V1, V2) partials; weights_reduce_kernel sums those in
//                            a fixed order; weights_check_kernel counts non-finite, out-of-range and over-unit-sum weights
//   moments_weighted_kernel  per-k raw fp64 moments (sum_p w x, sum_p w x x^T) of an NHWC map: the arithmetic of moments.hip
//   apply_mixed_kernel       out_p = x_p + sum_k w_k(p) ((M_k x_p + b_k) - x_p) on the fp32 matrix cores
#include "wct_common.h"
#include <algorithm>

namespace {

constexpr int BL_MAX = 8;

// ---- blended style slot -------------------------------------------------------------------------------------------------------
struct BlendArgs {
  const double* F[BL_MAX];
  const double* mu[BL_MAX];
  double lam[BL_MAX];
  double* Fo;
  double* muo;
  int K;
  long cc, C;
};

__global__ __launch_bounds__(256) void stats_blend_kernel(BlendArgs a) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < a.cc + a.C; e += (long)gridDim.x * 256) {
    const bool isF = e < a.cc;
    const long q = isF ? e : e - a.cc;
    double v = a.lam[0] * (isF ? a.F[0][q] : a.mu[0][q]);
    for (int k = 1; k < a.K; ++k) v = fma(a.lam[k], isF ? a.F[k][q] : a.mu[k][q], v);
    if (isF) a.Fo[q] = v;
    else a.muo[q] = v;
  }
}

// ---- pooled level maps, (V1, V2), validation ----------------------------------------------------------------------------------
struct WPool {
  const float* w;        // [K][H][W]
  int H, W, K;
  long HW;
  float* out[6];         // [level] -> [K][h_L * w_L]
  int h[6], wd[6], gx[6];
  int maxgx;
  double* part;          // [6][BL_MAX][maxgx][2]
};

__global__ __launch_bounds__(256) void weights_pool_kernel(WPool a) {
  __shared__ double red[2][256];
  const int level = blockIdx.z + 1, k = blockIdx.y, tid = threadIdx.x;
  if ((int)blockIdx.x >= a.gx[level]) return;              // whole workgroup
  const int s = 1 << (level - 1), wl = a.wd[level];
  const long n = (long)a.h[level] * wl;
  const float* src = a.w + (size_t)k * a.HW;
  float* dst = a.out[level] + (size_t)k * n;
  const double inv = 1.0 / ((double)s * s);
  double v1 = 0., v2 = 0.;
  for (long e = (long)blockIdx.x * 256 + tid; e < n; e += (long)a.gx[level] * 256) {
    const long i = e / wl, j = e - i * wl;
    double acc = 0.;
    for (int r = 0; r < s; ++r) {
      const float* row = src + (i * s + r) * (long)a.W + j * s;
      for (int c = 0; c < s; ++c) acc += row[c];
    }
    const float m = (float)(acc * inv);
    dst[e] = m;
    v1 += m;
    v2 += (double)m * m;
  }
  red[0][tid] = v1;
  red[1][tid] = v2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {
    double* p = a.part + (((size_t)level * BL_MAX + k) * a.maxgx + blockIdx.x) * 2;
    p[0] = red[0][0];
    p[1] = red[1][0];
  }
}

// partials of (level, k) -> vv[level][k][2], one workgroup each, fixed order
__global__ __launch_bounds__(256) void weights_reduce_kernel(WPool a, double* vv) {
  __shared__ double red[2][256];
  const int level = blockIdx.y + 1, k = blockIdx.x, tid = threadIdx.x;
  const double* p = a.part + ((size_t)level * BL_MAX + k) * a.maxgx * 2;
  double v1 = 0., v2 = 0.;
  for (int b = tid; b < a.gx[level]; b += 256) { v1 += p[2 * b]; v2 += p[2 * b + 1]; }
  red[0][tid] = v1;
  red[1][tid] = v2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {
    vv[((size_t)level * BL_MAX + k) * 2] = red[0][0];
    vv[((size_t)level * BL_MAX + k) * 2 + 1] = red[1][0];
  }
}

// cnt[0] non-finite values, cnt[1] finite values outside [0, 1], cnt[2] pixels whose weights sum to more than 1 + 1e-6 (integers: any
// order is exact)
__global__ __launch_bounds__(256) void weights_check_kernel(const float* w, long HW, int K, unsigned* cnt) {
  __shared__ unsigned c[3];
  if (threadIdx.x < 3) c[threadIdx.x] = 0u;
  __syncthreads();
  unsigned nf = 0, oor = 0, over = 0;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long)gridDim.x * 256) {
    double sum = 0.;
    for (int k = 0; k < K; ++k) {
      const float v = w[(size_t)k * HW + p];
      if (!isfinite(v)) { ++nf; continue; }
      if (v < 0.f || v > 1.f) ++oor;
      sum += v;
    }
    if (sum > 1.0 + 1e-6) ++over;
  }
  if (nf) atomicAdd(&c[0], nf);
  if (oor) atomicAdd(&c[1], oor);
  if (over) atomicAdd(&c[2], over);
  __syncthreads();
  if (threadIdx.x < 3 && c[threadIdx.x]) atomicAdd(cnt + threadIdx.x, c[threadIdx.x]);
}

// ---- per-k weighted moments ---------------------------------------------------------------------------------------------------
// grid = (pixel chunks, pair groups, K).  As moments_labeled_kernel (regions.hip): a workgroup (4 waves) walks its chunk in LDS tiles of
// MP pixels, wave w owns the 16 x 16 tile pairs pg * 4 PW + w + 4 j of the upper triangle, partials per (k, chunk), then a fixed-order
// reduction.  The operands are A = w x (the pixel's weight applied as the channel is read from LDS) and B = x; tiles whose weights are
// all zero are skipped before their features are loaded.  Two tiles in flight: the next tile's weights and features are loaded into
// registers while the current one is multiplied.  Arithmetic as moments.hip: F32 = fp32 products (w x rounded to fp32) on
// v_mfma_f32_16x16x4_f32 summed over a tile (<= 64 pixels), tile totals in fp64; F32 = false: exact fp64 products on v_mfma_f64_16x16x4_f64.
struct MomWArgs {
  const float* x;
  const float* w;        // [K][npix]
  int C, T, NP, Cs, MP, PW, NPC;
  long npix, chunk;
  double* part;          // [K][NPC][NP * 256 + T * 16]
};

constexpr int MW_PRE = 8;   // float4 per thread of one tile: MP * C / 4 <= 2048 for every (MP, C) of the plan

__device__ __forceinline__ int wrow_of(bool f32, int pk, int r) { return f32 ? 4 * pk + r : pk + 4 * r; }

template <int PW, bool F32>
__global__ __launch_bounds__(256, 2) void moments_weighted_kernel(MomWArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* lds = reinterpret_cast<float*>(smem);                      // [MP][Cs]
  float* wsh = lds + (size_t)a.MP * a.Cs;                           // [MP]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, pk = lane >> 4;
  const int pc = blockIdx.x, pg = blockIdx.y, k = blockIdx.z;
  const int MP = a.MP, Cs = a.Cs, c4n = a.C >> 2, nld = MP * c4n;
  const float* wk = a.w + (size_t)k * a.npix;
  int offA[PW], offB[PW], pidx[PW];
  bool diag[PW];
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < PW; ++j) {
    const int idx = pg * (4 * PW) + wave + 4 * j;
    offA[j] = offB[j] = c; pidx[j] = 0; diag[j] = false;
    if (idx < a.NP) {
      int I = 0, rem = idx;
      while (rem >= a.T - I) { rem -= a.T - I; ++I; }
      offA[j] = I * 16 + c; offB[j] = (I + rem) * 16 + c; pidx[j] = idx; diag[j] = rem == 0;
      cnt = j + 1;
    }
  }
  cnt = __builtin_amdgcn_readfirstlane(cnt);
  f64x4 acc[PW];
  double s[PW];
#pragma unroll
  for (int j = 0; j < PW; ++j) { acc[j] = f64x4{0., 0., 0., 0.}; s[j] = 0.; }
  for (int e = tid; e < MP * Cs; e += 256) lds[e] = 0.f;   // padding channels (C .. 16 T) stay zero
  const long p0 = (long)pc * a.chunk, p1 = min(a.npix, p0 + a.chunk);
  // registers of the tile in flight
  f32x4 pre[MW_PRE];
  float wreg = 0.f;
  auto fetch = [&](long pt) -> int {                        // weights of tile pt; its features too if any weight is non-zero
    wreg = 0.f;
    if (tid < MP && pt + tid < p1) wreg = wk[pt + tid];
    const int any = __syncthreads_or(wreg != 0.f);
    if (any) {
#pragma unroll
      for (int i = 0; i < MW_PRE; ++i) {
        const int e = tid + 256 * i;
        pre[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (e < nld) {
          const int px = e / c4n, q = e - px * c4n;
          if (pt + px < p1) pre[i] = *reinterpret_cast<const f32x4*>(a.x + (pt + px) * a.C + 4 * q);
        }
      }
    }
    return any;
  };
  int any = p0 < p1 ? fetch(p0) : 0;
  for (long pt = p0; pt < p1; pt += MP) {
    const int cur = any;
    __syncthreads();                                        // previous tile consumed
    if (cur) {
      if (tid < MP) wsh[tid] = wreg;
#pragma unroll
      for (int i = 0; i < MW_PRE; ++i) {
        const int e = tid + 256 * i;
        if (e < nld) {
          const int px = e / c4n, q = e - px * c4n;
          *reinterpret_cast<f32x4*>(lds + px * Cs + 4 * q) = pre[i];
        }
      }
    }
    __syncthreads();
    any = pt + MP < p1 ? fetch(pt + MP) : 0;                // next tile's loads in flight during this tile's products
    if (!cur) continue;
#pragma unroll
    for (int j = 0; j < PW; ++j) {
      if (j < cnt) {
        if constexpr (F32) {
          f32x4 f = f32x4{0.f, 0.f, 0.f, 0.f};
          float t = 0.f;
          for (int st = 0; st < MP; st += 4) {
            const float* row = lds + (st + pk) * Cs;
            const float av = row[offA[j]] * wsh[st + pk], bv = row[offB[j]];
            t += av;
            f = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, f, 0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[j][r] += (double)f[r];
          s[j] += (double)t;
        } else {
          for (int st = 0; st < MP; st += 4) {
            const float* row = lds + (st + pk) * Cs;
            const double av = (double)row[offA[j]] * (double)wsh[st + pk], bv = (double)row[offB[j]];
            s[j] += av;
            acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[j], 0, 0, 0);
          }
        }
      }
    }
  }
  const long stride = (long)a.NP * 256 + a.T * 16;
  double* dst = a.part + ((size_t)k * a.NPC + pc) * stride;
#pragma unroll
  for (int j = 0; j < PW; ++j) {
    if (j < cnt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[(size_t)pidx[j] * 256 + wrow_of(F32, pk, r) * 16 + c] = acc[j][r];
      if (diag[j]) {                                        // the diagonal tile's owner also owns the sums of its 16 channels
        double v = s[j];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (pk == 0) dst[(size_t)a.NP * 256 + offA[j]] = v;
      }
    }
  }
}

// partials -> sum[K][C], sumsq[K][C][C] in a fixed order (16 slices of the chunk index, then the slices in order).  Inside a diagonal
// tile only the upper half is taken and mirrored: (w x_a) x_b and (w x_b) x_a round differently in fp32, the result is exactly symmetric.
__global__ __launch_bounds__(256) void moments_weighted_reduce_kernel(MomWArgs a, double* sum, double* sumsq) {
  __shared__ double red[16][17];
  const int el = threadIdx.x & 15, sl = threadIdx.x >> 4, k = blockIdx.y;
  const long e = (long)blockIdx.x * 16 + el;
  const long nsq = (long)a.NP * 256, stride = nsq + a.T * 16;
  const double* base = a.part + (size_t)k * a.NPC * stride;
  double v = 0.;
  if (e < stride)
    for (int pc = sl; pc < a.NPC; pc += 16) v += base[(size_t)pc * stride + e];
  red[sl][el] = v;
  __syncthreads();
  if (sl != 0 || e >= stride) return;
  v = 0.;
#pragma unroll
  for (int q = 0; q < 16; ++q) v += red[q][el];
  const size_t C = a.C;
  if (e < nsq) {
    const int pair = (int)(e >> 8), r = (int)((e >> 4) & 15), cc = (int)(e & 15);
    int I = 0, rem = pair;
    while (rem >= a.T - I) { rem -= a.T - I; ++I; }
    const int J = I + rem;
    if (I == J && r > cc) return;
    const int ra = I * 16 + r, cb = J * 16 + cc;
    if (ra < a.C && cb < a.C) {
      sumsq[k * C * C + (size_t)ra * C + cb] = v;
      if (ra != cb) sumsq[k * C * C + (size_t)cb * C + ra] = v;
    }
  } else {
    const int ch = (int)(e - nsq);
    if (ch < a.C) sum[k * C + ch] = v;
  }
}

MomWArgs plan_weighted(int C, long npix) {
  MomWArgs a{};
  a.C = C; a.T = (C + 15) / 16; a.NP = a.T * (a.T + 1) / 2;
  a.Cs = (a.T & 1) ? a.T * 16 : a.T * 16 + 16;              // == 16 (mod 32) dwords: conflict-free operand reads
  a.MP = C <= 128 ? 64 : C <= 256 ? 32 : 16;
  a.PW = a.NP <= 8 ? 2 : 8;
  const int npg = (a.NP + 4 * a.PW - 1) / (4 * a.PW);
  a.npix = npix;
  long npc = std::max(1L, 1024L / npg);                     // ~1024 workgroups per k
  const long maxc = (npix + a.MP - 1) / a.MP;
  if (npc > maxc) npc = maxc;
  long chunk = (npix + npc - 1) / npc;
  a.chunk = (chunk + a.MP - 1) / a.MP * a.MP;
  a.NPC = (int)((npix + a.chunk - 1) / a.chunk);
  return a;
}

// ---- mixed apply --------------------------------------------------------------------------------------------------------------------
// A workgroup owns PT pixels (64 for C <= 128, 32 / 16 above) staged in LDS [PT][Cs] with their K weights; the (16 output channels x
// 16 pixels) items of the tile are dealt to the four waves.  Per item the result starts as x; per k with a non-zero weight in the tile
// (found with a 64-bit ballot): v_mfma_f32_16x16x4_f32 with A = M_k rows, B = the pixels, then res += w_k(p) (acc + b_k - x) on the
// accumulator columns in registers.  One read of x and the weights, one write of out.
struct ApplyMixArgs {
  const float* x;
  const float* w;        // [K][npix]
  const float* Mf;       // [K][Cp][Cp] fp32, zero padded
  const float* bf;       // [K][Cp]
  float* out;
  int C, Cp, Cs, PT, K;
  long npix;
};

__global__ __launch_bounds__(256) void apply_mixed_kernel(ApplyMixArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xs = reinterpret_cast<float*>(smem);                        // [PT][Cs]
  float* wts = xs + (size_t)a.PT * a.Cs;                             // [K][PT]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int PT = a.PT, Cs = a.Cs, Cp = a.Cp, C = a.C, c4n = C >> 2;
  const long p0 = (long)blockIdx.x * PT;
  const int npt = (int)min((long)PT, a.npix - p0);
  for (int e = tid; e < PT * (Cp >> 2); e += 256) {
    const int px = e / (Cp >> 2), q = e - px * (Cp >> 2);
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (px < npt && q < c4n) v = *reinterpret_cast<const f32x4*>(a.x + (p0 + px) * C + 4 * q);
    *reinterpret_cast<f32x4*>(xs + px * Cs + 4 * q) = v;
  }
  for (int e = tid; e < a.K * PT; e += 256) {
    const int k = e / PT, px = e - k * PT;
    wts[e] = px < npt ? a.w[(size_t)k * a.npix + p0 + px] : 0.f;
  }
  __syncthreads();
  unsigned present = 0;                                              // wave-uniform
  for (int k = 0; k < a.K; ++k)
    if (__ballot(lane < PT && wts[k * PT + (lane < PT ? lane : 0)] != 0.f)) present |= 1u << k;
  const int j = lane & 15, kq = lane >> 4;
  const int nO = Cp >> 4, nP = PT >> 4, nItems = nO * nP;
  for (int it = wave; it < nItems; it += 4) {
    const int ot = it / nP, ptile = it - ot * nP;
    const int o0 = ot * 16, px = ptile * 16 + j;
    const int oc = o0 + 4 * kq;
    const float* brow = xs + px * Cs + 4 * kq;
    const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + px * Cs + oc);
    f32x4 res = xv;
    unsigned pend = present;
    while (pend) {
      const int k = __builtin_ctz(pend);
      pend &= pend - 1;
      const float* arow = a.Mf + (size_t)k * Cp * Cp + (size_t)(o0 + j) * Cp + 4 * kq;
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < Cp; k0 += 16) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(arow + k0);
        const f32x4 bv = *reinterpret_cast<const f32x4*>(brow + k0);
#pragma unroll
        for (int st = 0; st < 4; ++st) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[st], bv[st], acc, 0, 0, 0);
      }
      // D layout: column = pixel (lane & 15), rows = output channels o0 + 4 (lane >> 4) + r
      const f32x4 bb = *reinterpret_cast<const f32x4*>(a.bf + (size_t)k * Cp + oc);
      const float wv = wts[k * PT + px];
      res += wv * (acc + bb - xv);
    }
    if (px < npt && oc < C) *reinterpret_cast<f32x4*>(a.out + (p0 + px) * C + oc) = res;
  }
}

// fp64 (M, b) of K maps -> fp32, zero padded to Cp
__global__ void mb_to_f32_mixed_kernel(const double* M, const double* b, int K, int C, int Cp, float* Mf, float* bf) {
  const long n = (long)K * Cp * Cp;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n + (long)K * Cp; e += (long)gridDim.x * blockDim.x) {
    if (e < n) {
      const int k = (int)(e / ((long)Cp * Cp)), r = (int)((e / Cp) % Cp), c = (int)(e % Cp);
      Mf[e] = (r < C && c < C) ? (float)M[(size_t)k * C * C + (size_t)r * C + c] : 0.f;
    } else {
      const long q = e - n;
      const int k = (int)(q / Cp), c = (int)(q % Cp);
      bf[q] = c < C ? (float)b[(size_t)k * C + c] : 0.f;
    }
  }
}

// sum_k *= f[k], sumsq_k *= f[k] (the (n_eff, scaled sums) form of the reliability-weighted covariance)
struct ScaleArgs { double f[BL_MAX]; };
__global__ __launch_bounds__(256) void scale_sums_kernel(double* sum, double* sumsq, int C, ScaleArgs a) {
  const int k = blockIdx.y;
  const long cc = (long)C * C;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < cc + C; e += (long)gridDim.x * 256) {
    if (e < cc) sumsq[k * cc + e] *= a.f[k];
    else sum[(long)k * C + (e - cc)] *= a.f[k];
  }
}

}  // namespace

hipError_t launch_stats_blend(int C, int K, const double* const* F, const double* const* mu, const double* lam, double* Fo, double* muo,
                              hipStream_t s) {
  if (C < 1 || K < 1 || K > BL_MAX) return hipErrorInvalidValue;
  BlendArgs a{};
  for (int k = 0; k < K; ++k) { a.F[k] = F[k]; a.mu[k] = mu[k]; a.lam[k] = lam[k]; }
  a.Fo = Fo; a.muo = muo; a.K = K; a.cc = (long)C * C; a.C = C;
  const long n = a.cc + C;
  hipLaunchKernelGGL(stats_blend_kernel, dim3((unsigned)std::min(1024L, (n + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

size_t weights_levels_workspace_bytes(int H, int W) {
  const long n5 = (long)(H >> 4) * (W >> 4);
  const long gx = std::min(1024L, (n5 * 256 + 255) / 256);  // level 1 has the most blocks: its map is 256 x level 5's
  return (size_t)6 * BL_MAX * gx * 2 * sizeof(double);
}

hipError_t launch_weights_levels(const float* w, int H, int W, int K, const int* h, const int* wd, float* const* out, double* vv,
                                 unsigned* cnt, void* ws, size_t ws_bytes, hipStream_t s) {
  if (K < 1 || K > BL_MAX || H < 16 || W < 16) return hipErrorInvalidValue;
  if (ws_bytes < weights_levels_workspace_bytes(H, W)) return hipErrorOutOfMemory;
  WPool a{};
  a.w = w; a.H = H; a.W = W; a.K = K; a.HW = (long)H * W;
  a.maxgx = 1;
  for (int level = 1; level <= 5; ++level) {
    const int sc = 1 << (level - 1);
    if ((long)h[level] * sc > H || (long)wd[level] * sc > W || h[level] < 1 || wd[level] < 1) return hipErrorInvalidValue;
    a.out[level] = out[level]; a.h[level] = h[level]; a.wd[level] = wd[level];
    a.gx[level] = (int)std::min(1024L, ((long)h[level] * wd[level] + 255) / 256);
    a.maxgx = std::max(a.maxgx, a.gx[level]);
  }
  if ((size_t)6 * BL_MAX * a.maxgx * 2 * sizeof(double) > ws_bytes) return hipErrorOutOfMemory;
  a.part = reinterpret_cast<double*>(ws);
  hipError_t e = hipMemsetAsync(cnt, 0, 4 * sizeof(unsigned), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(weights_check_kernel, dim3((unsigned)std::min(2048L, (a.HW + 255) / 256)), dim3(256), 0, s, w, a.HW, K, cnt);
  hipLaunchKernelGGL(weights_pool_kernel, dim3((unsigned)a.maxgx, (unsigned)K, 5u), dim3(256), 0, s, a);
  hipLaunchKernelGGL(weights_reduce_kernel, dim3((unsigned)K, 5u), dim3(256), 0, s, a, vv);
  return hipGetLastError();
}

size_t moments_weighted_workspace_bytes(int C, long npix, int K) {
  const MomWArgs a = plan_weighted(C, npix);
  return (size_t)K * a.NPC * ((size_t)a.NP * 256 + a.T * 16) * sizeof(double);
}

hipError_t launch_moments_weighted(const float* feat, int C, long npix, const float* w, int K, double* sum, double* sumsq, void* ws,
                                   size_t ws_bytes, hipStream_t s, bool f32_products) {
  if (C < 4 || (C & 3) || C > 512 || npix < 1 || K < 1 || K > BL_MAX) return hipErrorInvalidValue;
  if (ws_bytes < moments_weighted_workspace_bytes(C, npix, K)) return hipErrorOutOfMemory;
  MomWArgs a = plan_weighted(C, npix);
  if ((long)a.MP * (C >> 2) > 256L * MW_PRE) return hipErrorInvalidValue;
  a.x = feat; a.w = w; a.part = reinterpret_cast<double*>(ws);
  const int npg = (a.NP + 4 * a.PW - 1) / (4 * a.PW);
  const size_t lds = (size_t)a.MP * a.Cs * sizeof(float) + a.MP * sizeof(float);
  auto go = [&](auto kern) -> hipError_t {
    if (lds > 48 * 1024) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)a.NPC, (unsigned)npg, (unsigned)K), dim3(256), lds, s, a);
    return hipGetLastError();
  };
  note_moments_form('l', a.MP, (a.MP * (C >> 2) + 255) / 256, a.PW, false, f32_products);
  hipError_t e;
  if (a.PW == 2) e = f32_products ? go(moments_weighted_kernel<2, true>) : go(moments_weighted_kernel<2, false>);
  else e = f32_products ? go(moments_weighted_kernel<8, true>) : go(moments_weighted_kernel<8, false>);
  if (e != hipSuccess) return e;
  const long stride = (long)a.NP * 256 + a.T * 16;
  hipLaunchKernelGGL(moments_weighted_reduce_kernel, dim3((unsigned)((stride + 15) / 16), (unsigned)K), dim3(256), 0, s, a, sum, sumsq);
  return hipGetLastError();
}

size_t apply_mixed_workspace_bytes(int C, int K) {
  const size_t Cp = (size_t)(C + 15) / 16 * 16;
  return ((size_t)K * Cp * Cp + (size_t)K * Cp) * sizeof(float);
}

hipError_t launch_apply_mixed(const float* feat, int C, long npix, const float* w, int K, const double* M, const double* b, float* out,
                              void* ws, size_t ws_bytes, hipStream_t s) {
  if (C < 4 || (C & 3) || C > 512 || npix < 1 || K < 1 || K > BL_MAX) return hipErrorInvalidValue;
  if (ws_bytes < apply_mixed_workspace_bytes(C, K)) return hipErrorOutOfMemory;
  ApplyMixArgs a{};
  a.C = C; a.Cp = (C + 15) / 16 * 16; a.Cs = a.Cp + 4; a.K = K; a.npix = npix;
  a.PT = C <= 128 ? 64 : C <= 256 ? 32 : 16;
  a.x = feat; a.w = w; a.out = out;
  float* Mf = reinterpret_cast<float*>(ws);
  float* bf = Mf + (size_t)K * a.Cp * a.Cp;
  a.Mf = Mf; a.bf = bf;
  const long nconv = (long)K * a.Cp * a.Cp + (long)K * a.Cp;
  hipLaunchKernelGGL(mb_to_f32_mixed_kernel, dim3((unsigned)std::min(1024L, (nconv + 255) / 256)), dim3(256), 0, s, M, b, K, C, a.Cp, Mf, bf);
  const size_t lds = (size_t)a.PT * a.Cs * sizeof(float) + (size_t)K * a.PT * sizeof(float);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(apply_mixed_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(apply_mixed_kernel, dim3((unsigned)((npix + a.PT - 1) / a.PT)), dim3(256), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_scale_sums(double* sum, double* sumsq, int C, int K, const double* f, hipStream_t s) {
  if (K < 1 || K > BL_MAX) return hipErrorInvalidValue;
  ScaleArgs a{};
  for (int k = 0; k < K; ++k) a.f[k] = f[k];
  const long n = (long)C * C + C;
  hipLaunchKernelGGL(scale_sums_kernel, dim3((unsigned)std::min(256L, (n + 255) / 256), (unsigned)K), dim3(256), 0, s, sum, sumsq, C, a);
  return hipGetLastError();
}
