// Attention-weighted style statistics (include/wct_hip_attn.h): per content position the softmax-weighted mean and variance of the
// standardised style map.  Kernels:
//
//   attn_diag_kernel     raw moments -> the diagonal (M, b) of the standardised map, and (mu, sigma)
//   attn_unit_kernel     out_p = in_p / sqrt(|in_p|^2 + eps): 16 lanes per row, one pass, 16-byte accesses
//   attn_transpose_kernel, attn_whiten_kernel    the whitened map W (x - mu) in fp64 from the swap's whitening matrix
//   attn_vmax_kernel     partial maxima of |V|;  attn_vscale_kernel: the power-of-two scale of V^2 from them
//   attn_stats_kernel    the flash-attention forward: scores, online softmax, P.V and P.V^2 in f16x3 on 16x16x32 MFMAs
//   attn_apply_kernel    the elementwise result
//
// attn_stats_kernel.  A workgroup (4 waves) owns AT_QT = 64 queries -- 16 per wave, the wave's q^ rows split into registers (one
// 128-channel chunk: 32 VGPRs) -- and one slab of AT_CS = 128 value channels (blockIdx.y), and walks the keys in tiles of AT_KT = 32.
// Both products are SWAPPED so that a query is a lane's COLUMN from end to end and nothing but the maximum and the sum crosses lanes:
//   S^T = K^ Q^T     A = the key tile out of LDS ([hi | lo][8-channel group][key], 16-byte slots, plane stride 33), B = the wave's
//                    q^ registers.  Lane (li, kq) holds query li against keys 16 t + 4 kq + r  (t = 0, 1; r = 0 .. 3).
//   O^T = V^T P^T    B = those eight P values as they stand: the product's k index 8 kq + 4 t + r IS key 16 t + 4 kq + r, and the value
//                    tile is written to LDS in that order ([V hi | V lo | W hi | W lo][kq][channel] slots of 8 keys, W = s V^2).
//                    Lane (li, kq) holds channels 16 ct + 4 kq + r of query li: one 16-byte store per channel tile at the end.
// Per key tile: stage V / W (every thread 4 keys x 4 channels), per 128-channel chunk stage K^ (and, for C > 128, reload the q^
// registers), 24 score MFMAs, the softmax step in registers (exact expf; two shuffles for the maximum, two for the sum), 48 value MFMAs
// per wave.  Accumulators are rescaled only at a tile where some lane's maximum grew (a multiplication by exactly 1 otherwise: skipping
// it changes no bit).  Nothing is clamped; no SatTrack; no atomics.
#include "conv_f16_dev.h"
#include <algorithm>

// The header states evaluation orders operation by operation (wct_attn_apply is pinned bit for bit by a numpy emulation): no product may
// be fused into a following sum anywhere in this file.  The runtime's __fmul_rn / __fadd_rn do not see to that: they are inline
// functions compiled under the default contraction, so a product and a sum of theirs fuse after inlining (seen in the ISA: v_fma_f32).
// The four operators below are compiled under this pragma and stay apart.
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }

constexpr int AT_QT = 64, AT_KT = 32, AT_CS = 128, AT_THREADS = 256;
constexpr int AT_KP = 33;                      // key stride of one 8-channel group's plane, in 16-byte slots (staging stores 16 groups of one key)
constexpr int AT_KSLOTS = 2 * 16 * AT_KP;      // [hi | lo][16 groups of a 128-channel chunk][AT_KP]
constexpr int AT_VPLANE = 4 * AT_CS;           // [kq][channel] slots of one value plane
constexpr int AT_VSLOTS = 4 * AT_VPLANE;       // V hi | V lo | W hi | W lo
constexpr float AT_QSCALE = 4096.f;            // 2^12 on q^ and on k^ ...
constexpr float AT_SINV = 1.f / 16777216.f;    // ... 2^-24 on their product
constexpr float AT_PSCALE = 32768.f;           // 2^15 on P
static_assert(AT_QT == 16 * (AT_THREADS / 64) && AT_KT == 32 && AT_THREADS == 2 * AT_CS, "tile shapes the index arithmetic below assumes");

// the split of conv_f16_dev.h without its clamp: the caller's scale keeps |x| inside the f16 range; beyond it hi is infinite and lo NaN
__device__ __forceinline__ void split8_raw(const f32x4& a, const f32x4& b, float s, u32x4& hi, u32x4& lo) {
  { const HiLo t_ = split2(a[0] * s, a[1] * s); hi[0] = t_.hi; lo[0] = t_.lo; }
  { const HiLo t_ = split2(a[2] * s, a[3] * s); hi[1] = t_.hi; lo[1] = t_.lo; }
  { const HiLo t_ = split2(b[0] * s, b[1] * s); hi[2] = t_.hi; lo[2] = t_.lo; }
  { const HiLo t_ = split2(b[2] * s, b[3] * s); hi[3] = t_.hi; lo[3] = t_.lo; }
}
__device__ __forceinline__ float pair_sum(unsigned hi, unsigned lo) {   // (hi0 + lo0) + (hi1 + lo1) of two packed pairs, in fp32
  const f16x2 h = __builtin_bit_cast(f16x2, hi), l = __builtin_bit_cast(f16x2, lo);
  return add_rn(add_rn((float)h[0], (float)l[0]), add_rn((float)h[1], (float)l[1]));
}

__global__ __launch_bounds__(256) void attn_diag_kernel(int C, double n, double eps, const double* __restrict__ sum, const double* __restrict__ sumsq,
                                                        double* __restrict__ M, double* __restrict__ b, double* __restrict__ mu_out,
                                                        double* __restrict__ sigma_out) {
  const int a = blockIdx.x, tid = threadIdx.x;
  const double mu = sum[a] / n;
  const double var = fmax((sumsq[(size_t)a * C + a] - n * mu * mu) / (n - 1.0), 0.0);   // round-off of a constant channel may land below zero
  const double sigma = sqrt(var + eps);
  for (int c = tid; c < C; c += 256) M[(size_t)a * C + c] = a == c ? 1.0 / sigma : 0.0;
  if (tid == 0) {
    b[a] = -mu / sigma;
    if (mu_out) { mu_out[a] = mu; sigma_out[a] = sigma; }
  }
}

__global__ __launch_bounds__(256) void attn_unit_kernel(const float* __restrict__ in, long n, int C, float* __restrict__ out) {
  const int sub = threadIdx.x & 15, c4n = C >> 2;
  const long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool live = row < n;
  const f32x4* src = reinterpret_cast<const f32x4*>(in + (size_t)(live ? row : 0) * C);
  f32x4 x[8];
  double n2 = 0.0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = sub + 16 * j;
    x[j] = (live && i < c4n) ? src[i] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) n2 = fma((double)x[j][e], (double)x[j][e], n2);
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) n2 += __shfl_xor(n2, o, 64);   // a butterfly: the 16 lanes of a row end with one value
  const float r = (float)(1.0 / sqrt(n2 + 1e-12));                // WCT_ATTN_EPS
  if (!live) return;
  f32x4* dst = reinterpret_cast<f32x4*>(out + (size_t)row * C);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = sub + 16 * j;
    if (i < c4n) dst[i] = f32x4{mul_rn(x[j][0], r), mul_rn(x[j][1], r), mul_rn(x[j][2], r), mul_rn(x[j][3], r)};
  }
}

// max over a workgroup of non-negative values (a NaN operand is ignored by fmaxf); valid in thread 0
__device__ __forceinline__ float block_max(float m, float* red) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(256) void attn_vmax_kernel(const f32x4* __restrict__ v, long n4, float* __restrict__ part) {
  __shared__ float red[4];
  float m = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const f32x4 x = v[i];
    m = fmaxf(fmaxf(m, fabsf(x[0])), fabsf(x[1]));
    m = fmaxf(fmaxf(m, fabsf(x[2])), fabsf(x[3]));
  }
  m = block_max(m, red);
  if (threadIdx.x == 0) part[blockIdx.x] = m;
}

// scale[0] = 2^(14 - e), scale[1] = 2^(e - 14), e = floor(log2 fl(vmax^2)) kept in -60 .. 40
__global__ __launch_bounds__(256) void attn_vscale_kernel(const float* __restrict__ part, int n, float* __restrict__ scale) {
  __shared__ float red[4];
  float m = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, part[i]);
  m = block_max(m, red);
  if (threadIdx.x == 0) {
    int e = (int)((__float_as_uint(mul_rn(m, m)) >> 23) & 0xffu) - 127;
    e = e < -60 ? -60 : (e > 40 ? 40 : e);
    scale[0] = __uint_as_float((unsigned)(127 + 14 - e) << 23);
    scale[1] = __uint_as_float((unsigned)(127 - 14 + e) << 23);
  }
}

// queries [q0, q1) of Q against every key; grid (query tiles, value slabs)
__global__ __launch_bounds__(AT_THREADS, 2) void attn_stats_kernel(const float* __restrict__ Q, int q0, int q1, const float* __restrict__ K,
                                                                const float* __restrict__ V, int Nk, int C, float tau_s,
                                                                const float* __restrict__ vscale, float* __restrict__ mean, float* __restrict__ var) {
  __shared__ u32x4 ldsK[AT_KSLOTS];
  __shared__ u32x4 ldsV[AT_VSLOTS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
  const int slab0 = blockIdx.y * AT_CS;
  const int slabC = C - slab0 < AT_CS ? C - slab0 : AT_CS;
  const int nct = (slabC + 15) >> 4;
  const int nchunks = (C + 127) >> 7;
  const long qrow_l = (long)q0 + (long)blockIdx.x * AT_QT + wave * 16 + li;
  const bool qlive = qrow_l < q1;
  const size_t qrow = (size_t)(qlive ? qrow_l : q1 - 1);      // a ragged tile's spare lanes repeat the last query and store nothing
  const float wscale = vscale[0], winv = vscale[1];

  u32x4 qh[4], ql[4];
  auto load_q = [&](int c0) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int c = c0 + 32 * ks + 8 * kq;
      f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f}, b = a;
      if (c < C) a = *reinterpret_cast<const f32x4*>(Q + qrow * C + c);
      if (c + 4 < C) b = *reinterpret_cast<const f32x4*>(Q + qrow * C + c + 4);
      split8_raw(a, b, AT_QSCALE, qh[ks], ql[ks]);
    }
  };
  if (nchunks == 1) load_q(0);

  f32x4 accV[8], accW[8];
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) accV[ct] = accW[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -__builtin_inff(), l_run = 0.f;

  const int nkt = (int)(((long)Nk + AT_KT - 1) / AT_KT);
  for (int kt = 0; kt < nkt; ++kt) {
    const long k0 = (long)kt * AT_KT;
    __syncthreads();   // the previous tile's reads of both LDS tiles are done

    // the value tile: thread (g, c) takes keys k0 + 4 g .. + 3 of channel slab0 + c, i.e. half g >> 2 of slot (kq = g & 3, c)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int u = tid + AT_THREADS * i, c = u & (AT_CS - 1), g = u >> 7;
      if (c < 16 * nct) {
        float x[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long key = k0 + 4 * g + r;
          x[r] = (c < slabC && key < Nk) ? V[(size_t)key * C + slab0 + c] : 0.f;
        }
        const HiLo v01 = split2(x[0], x[1]), v23 = split2(x[2], x[3]);
        const HiLo w01 = split2(mul_rn(mul_rn(x[0], x[0]), wscale), mul_rn(mul_rn(x[1], x[1]), wscale));
        const HiLo w23 = split2(mul_rn(mul_rn(x[2], x[2]), wscale), mul_rn(mul_rn(x[3], x[3]), wscale));
        u32x2* dst = reinterpret_cast<u32x2*>(ldsV + (g & 3) * AT_CS + c) + (g >> 2);
        dst[0 * 2 * AT_VPLANE] = u32x2{v01.hi, v23.hi};
        dst[1 * 2 * AT_VPLANE] = u32x2{v01.lo, v23.lo};
        dst[2 * 2 * AT_VPLANE] = u32x2{w01.hi, w23.hi};
        dst[3 * 2 * AT_VPLANE] = u32x2{w01.lo, w23.lo};
      }
    }

    f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    for (int ch = 0; ch < nchunks; ++ch) {
      if (ch) __syncthreads();   // the previous chunk's reads of the key tile are done
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int u = tid + AT_THREADS * i, G = u & 15, key = u >> 4;
        const int c = ch * 128 + 8 * G;
        const long kidx = k0 + key;
        f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f}, b = a;
        if (kidx < Nk) {
          const float* p = K + (size_t)kidx * C + c;
          if (c < C) a = *reinterpret_cast<const f32x4*>(p);
          if (c + 4 < C) b = *reinterpret_cast<const f32x4*>(p + 4);
        }
        u32x4 hi, lo;
        split8_raw(a, b, AT_QSCALE, hi, lo);
        ldsK[(0 * 16 + G) * AT_KP + key] = hi;
        ldsK[(1 * 16 + G) * AT_KP + key] = lo;
      }
      if (nchunks > 1) load_q(ch * 128);
      __syncthreads();
      const int cleft = C - ch * 128;
      const int nks = cleft >= 128 ? 4 : (cleft + 31) >> 5;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        if (ks < nks) {
          f16x8 ah[2], al[2];
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            ah[t] = __builtin_bit_cast(f16x8, ldsK[(0 * 16 + 4 * ks + kq) * AT_KP + 16 * t + li]);
            al[t] = __builtin_bit_cast(f16x8, ldsK[(1 * 16 + 4 * ks + kq) * AT_KP + 16 * t + li]);
          }
          const f16x8 bh = __builtin_bit_cast(f16x8, qh[ks]), bl = __builtin_bit_cast(f16x8, ql[ks]);
#pragma unroll
          for (int term = 0; term < 3; ++term)
#pragma unroll
            for (int t = 0; t < 2; ++t)
              s[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(term == 1 ? al[t] : ah[t], term == 2 ? bl : bh, s[t], 0, 0, 0);
        }
    }

    // the softmax step of query li over this lane's 8 keys and its three partner lanes' (li + 16, + 32, + 48)
    float p[8], mx = -__builtin_inff();
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long key = k0 + 16 * t + 4 * kq + r;
        p[4 * t + r] = key < Nk ? mul_rn(s[t][r], tau_s) : -__builtin_inff();   // a key past the end: weight exactly 0
        mx = fmaxf(mx, p[4 * t + r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    const float f = expf(m_run - m_new);    // 0 at the first tile, 1 where the maximum stands
    m_run = m_new;
    u32x4 ph, pl;
    float ls = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const HiLo t_ = split2(mul_rn(expf(p[2 * j] - m_new), AT_PSCALE), mul_rn(expf(p[2 * j + 1] - m_new), AT_PSCALE));
      ph[j] = t_.hi; pl[j] = t_.lo;
      ls = add_rn(ls, pair_sum(t_.hi, t_.lo));     // the sum of what multiplies V, not of the fp32 weights
    }
    ls = add_rn(ls, __shfl_xor(ls, 16, 64));
    ls = add_rn(ls, __shfl_xor(ls, 32, 64));
    l_run = add_rn(mul_rn(l_run, f), ls);
    if (__any(f != 1.f)) {
#pragma unroll
      for (int ct = 0; ct < 8; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) { accV[ct][r] = mul_rn(accV[ct][r], f); accW[ct][r] = mul_rn(accW[ct][r], f); }
    }

    const f16x8 bh = __builtin_bit_cast(f16x8, ph), bl = __builtin_bit_cast(f16x8, pl);
#pragma unroll
    for (int ct = 0; ct < 8; ++ct)
      if (ct < nct) {
        const int slot = kq * AT_CS + 16 * ct + li;
        const f16x8 vh = __builtin_bit_cast(f16x8, ldsV[0 * AT_VPLANE + slot]), vl = __builtin_bit_cast(f16x8, ldsV[1 * AT_VPLANE + slot]);
        const f16x8 wh = __builtin_bit_cast(f16x8, ldsV[2 * AT_VPLANE + slot]), wl = __builtin_bit_cast(f16x8, ldsV[3 * AT_VPLANE + slot]);
        accV[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, bh, accV[ct], 0, 0, 0);
        accW[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, bh, accW[ct], 0, 0, 0);
        accV[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl, bh, accV[ct], 0, 0, 0);
        accW[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, bh, accW[ct], 0, 0, 0);
        accV[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, bl, accV[ct], 0, 0, 0);
        accW[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, bl, accW[ct], 0, 0, 0);
      }
  }

  if (!qlive) return;
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) {
    const int c = slab0 + 16 * ct + 4 * kq;
    if (ct < nct && c < C) {
      f32x4 mo, vo;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float m = div_rn(accV[ct][r], l_run);
        const float e = mul_rn(div_rn(accW[ct][r], l_run), winv);
        const float v = sub_rn(e, mul_rn(m, m));
        mo[r] = m;
        vo[r] = v < 0.f ? 0.f : v;      // a NaN stays a NaN
      }
      *reinterpret_cast<f32x4*>(mean + qrow * C + c) = mo;
      *reinterpret_cast<f32x4*>(var + qrow * C + c) = vo;
    }
  }
}

// The whitened map W (x - mu) in fp64: a workgroup takes AW_PIX pixels, centres them in fp64 into LDS (mu = sum / n) and every thread owns
// output channels tid, tid + 256: C fused multiply-adds per (pixel, channel) in ascending k, one rounding to fp32 at the end.  W is read
// TRANSPOSED (attn_transpose_kernel) so that the threads of a wave read consecutive doubles.  The result of a pixel depends on its values
// (and on W, mu) alone.
constexpr int AW_PIX = 8;

__global__ __launch_bounds__(256) void attn_transpose_kernel(const double* __restrict__ M, int C, double* __restrict__ Mt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C * C) return;
  const int r = i / C, c = i - r * C;
  Mt[(size_t)c * C + r] = M[i];
}

__global__ __launch_bounds__(256) void attn_whiten_kernel(const float* __restrict__ x, long npix, int C, double n, const double* __restrict__ sum,
                                                          const double* __restrict__ Mt, float* __restrict__ out) {
  __shared__ double xs[AW_PIX * 512];
  const long p0 = (long)blockIdx.x * AW_PIX;
  for (int i = threadIdx.x; i < AW_PIX * C; i += 256) {
    const int p = i / C, k = i - p * C;
    xs[i] = p0 + p < npix ? (double)x[(size_t)(p0 + p) * C + k] - sum[k] / n : 0.0;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    double acc[AW_PIX];
#pragma unroll
    for (int p = 0; p < AW_PIX; ++p) acc[p] = 0.0;
    for (int k = 0; k < C; ++k) {
      const double m = Mt[(size_t)k * C + c];
#pragma unroll
      for (int p = 0; p < AW_PIX; ++p) acc[p] = fma(m, xs[p * C + k], acc[p]);
    }
#pragma unroll
    for (int p = 0; p < AW_PIX; ++p)
      if (p0 + p < npix) out[(size_t)(p0 + p) * C + c] = (float)acc[p];
  }
}

__global__ __launch_bounds__(256) void attn_apply_kernel(const f32x4* __restrict__ mean, const f32x4* __restrict__ var, const f32x4* __restrict__ cstd,
                                                         const f32x4* __restrict__ cF, long n4, int c4n, const double* __restrict__ mu_s,
                                                         const double* __restrict__ sigma_s, float alpha, float oma, f32x4* __restrict__ out) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n4) return;
  const int c = 4 * (int)(t % c4n);
  const f32x4 m = mean[t], v = var[t], z = cstd[t], x = cF[t];
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float sg = (float)sigma_s[c + e], mu = (float)mu_s[c + e];
    const float sd = (float)sqrt((double)v[e]);   // the correctly rounded fp32 root: an fp64 root rounded once more cannot differ from it
    const float y = add_rn(mul_rn(sg, add_rn(mul_rn(sd, z[e]), m[e])), mu);
    r[e] = add_rn(mul_rn(alpha, y), mul_rn(oma, x[e]));
  }
  out[t] = r;
}

}  // namespace

size_t attn_stat_bytes(int C) { return 2 * (size_t)C * sizeof(double) + (1024 + 2) * sizeof(float); }

hipError_t launch_attn_diag(int C, double n, double eps, const double* sum, const double* sumsq, double* M, double* b, double* mu_out, double* sigma_out,
                            hipStream_t s) {
  if (C < 4 || C > 512 || n < 2) return hipErrorInvalidValue;
  hipLaunchKernelGGL(attn_diag_kernel, dim3((unsigned)C), dim3(256), 0, s, C, n, eps, sum, sumsq, M, b, mu_out, sigma_out);
  return hipGetLastError();
}

hipError_t launch_attn_whiten(const float* x, long npix, int C, const double* sum, const double* M, double* Mt, float* out, hipStream_t s) {
  if (C < 4 || (C & 3) || C > 512 || npix < 2) return hipErrorInvalidValue;
  hipLaunchKernelGGL(attn_transpose_kernel, dim3((unsigned)((C * C + 255) / 256)), dim3(256), 0, s, M, C, Mt);
  hipLaunchKernelGGL(attn_whiten_kernel, dim3((unsigned)((npix + AW_PIX - 1) / AW_PIX)), dim3(256), 0, s, x, npix, C, (double)npix, sum, (const double*)Mt, out);
  return hipGetLastError();
}

hipError_t launch_attn_unit(const float* in, long n, int C, float* out, hipStream_t s) {
  if (C < 4 || (C & 3) || C > 512 || n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(attn_unit_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, s, in, n, C, out);
  return hipGetLastError();
}

hipError_t launch_attn_stats(const float* qhat, int Nq, const float* khat, const float* v, int Nk, int C, float tau, int query_chunk, float* mean,
                             float* var, float* scratch /* 1024 + 2 floats */, hipStream_t s) {
  if (Nq < 1 || Nk < 1 || C < 4 || (C & 3) || C > 512 || query_chunk < 1 || !(tau >= 0.f && tau <= 32.f)) return hipErrorInvalidValue;
  const long n4 = (long)Nk * (C >> 2);
  const int nparts = (int)std::min(1024L, (n4 + 255) / 256);
  hipLaunchKernelGGL(attn_vmax_kernel, dim3((unsigned)nparts), dim3(256), 0, s, reinterpret_cast<const f32x4*>(v), n4, scratch);
  hipLaunchKernelGGL(attn_vscale_kernel, dim3(1), dim3(256), 0, s, (const float*)scratch, nparts, scratch + 1024);
  const unsigned slabs = (unsigned)((C + AT_CS - 1) / AT_CS);
  int nlaunch = 0;
  for (long b = 0; b < Nq; b += query_chunk) {
    const long e = b + query_chunk < Nq ? b + query_chunk : Nq;
    hipLaunchKernelGGL(attn_stats_kernel, dim3((unsigned)((e - b + AT_QT - 1) / AT_QT), slabs), dim3(AT_THREADS), 0, s, qhat, (int)b, (int)e, khat, v,
                       Nk, C, tau * AT_SINV, (const float*)(scratch + 1024), mean, var);
    ++nlaunch;
  }
  char form[sizeof wct_launch_form.text];
  snprintf(form, sizeof form, "l%d.s%u", nlaunch, slabs);
  note_launch_text(form);
  return hipGetLastError();
}

hipError_t launch_attn_apply(const float* mean, const float* var, const float* c_std, const float* cF, long n, int C, const double* mu_s,
                             const double* sigma_s, float alpha, float* out, hipStream_t s) {
  if (n < 1 || C < 4 || (C & 3) || C > 512) return hipErrorInvalidValue;
  const long n4 = n * (C >> 2);
  hipLaunchKernelGGL(attn_apply_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const f32x4*>(mean),
                     reinterpret_cast<const f32x4*>(var), reinterpret_cast<const f32x4*>(c_std), reinterpret_cast<const f32x4*>(cF), n4, C >> 2, mu_s,
                     sigma_s, alpha, 1.0f - alpha, reinterpret_cast<f32x4*>(out));
  return hipGetLastError();
}
