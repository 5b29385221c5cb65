// Patch-based style swap (include/wct_hip_swap.h): the fused normalised cross-correlation + arg-max of every 3 x 3 query patch with
// every 3 x 3 key patch, and the gather that assembles the swapped map.  Four kernels:
//
//   swap_norm_kernel      rnorm[k] = 1 / sqrt(|patch_K(k)|^2 + eps): one thread per key, fp64 sum in (tap, channel) order
//   swap_init_kernel      the running (score, index) of every query := "nothing yet"
//   swap_match_kernel     one launch per key chunk: implicit GEMM [Nq x 9C] . [9C x Nk] in f16x3 on 16x16x32 MFMAs, arg-max fused
//   swap_final_kernel     running (score, index) -> idx[q], best[q]
//   swap_assemble_kernel  out = alpha * mean of the covering value patches + (1 - alpha) * base
//
// swap_match_kernel.  A workgroup (4 waves) owns a tile of 8 x 16 queries and walks key tiles of 8 x 16 keys; both tiles sit in LDS with
// their halo ring (10 x 18 pixels), one 32-channel chunk at a time, already split: [hi | lo][kq = 8-channel group][pixel] x 16 bytes, the
// operand format of the MFMA (lane (li, kq) reads pixel li's channels 8 kq .. 8 kq + 7).  The plane stride SW_NP = 186 slots (== 2 mod 8)
// makes the staging stores -- four lanes on the four groups of one pixel, pixels in sequence -- and the operand reads -- 16 lanes on 16
// consecutive pixels -- free of bank conflicts by the bank rule (not yet confirmed with a counter run).  The 3 x 3 window is nine shifted 32-deep products on those tiles: nothing like an im2col
// buffer exists.  Wave (wm, wn) holds the 4 query rows 4 wm .. x the 4 key rows 4 wn .. as 4 x 4 accumulator tiles of 16 x 16 (64 VGPRs): per
// tap 16 operand reads feed 48 MFMAs (hi.hi, hi.lo, lo.hi).  D[i][j] of tile (m, n) = <query (row 4 wm + m, column i), key (row 4 wn + n,
// column j)>, lane (li, kq) holds i = 4 kq + r, j = li.
// Every (query, key) pair accumulates in ONE accumulator in the order (chunk, dx, dy, term) wherever the two patches lie: the score is a
// function of the patches' values alone.  After the last chunk a lane folds its 64 scores (x rnorm of its 4 keys) into its running
// (best, index) per query by "greater score, then lower index"; at the end of the walk 16 lanes fold by the same rule through
// shuffles and one lane per query merges into the context's running value with a 64-bit atomic max of (ordered score bits << 32 |
// ~index): order-independent, so key tiles may be dealt to any number of workgroups (grid.y) and chunks to any number of launches.
#include "conv_f16_dev.h"
#include <limits.h>

namespace {

constexpr int SW_TY = 8, SW_TX = 16;                     // patches per tile (queries and keys alike)
constexpr int SW_HY = SW_TY + 2, SW_HX = SW_TX + 2;      // the tile's pixels: 10 x 18
constexpr int SW_NPIX = SW_HY * SW_HX;                   // 180
constexpr int SW_NP = 186;                               // plane stride in 16-byte slots, == 2 (mod 8)
constexpr int SW_CK = 32;                                // channels per chunk = K of one MFMA
constexpr int SW_THREADS = 256;
constexpr int SW_PLANES = 8 * SW_NP;                     // [hl 2][kq 4][SW_NP] slots per map tile
static_assert(SW_NP >= SW_NPIX && (SW_NP & 7) == 2, "plane stride");

// order-preserving map of a non-NaN float onto unsigned, and back
__device__ __forceinline__ unsigned f32_ord(float s) {
  const unsigned u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_f32(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }
constexpr unsigned long long SW_NONE = 0x00000000ffffffffull;   // below every score (the ordered bits of -inf are 0x007fffff); index 0

__global__ __launch_bounds__(256) void swap_norm_kernel(const float* __restrict__ K, int hs, int ws, int C, float* __restrict__ rnorm) {
  const int kw = ws - 2;
  const long nk = (long)(hs - 2) * kw;
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= nk) return;
  const int ky = (int)(k / kw), kx = (int)(k - (long)ky * kw);
  double n2 = 0.0;
  for (int dy = 0; dy < 3; ++dy)
    for (int dx = 0; dx < 3; ++dx) {
      const f32x4* p = reinterpret_cast<const f32x4*>(K + ((size_t)(ky + dy) * ws + kx + dx) * C);
      for (int c = 0; c < C / 4; ++c) {
        const f32x4 v = p[c];
        n2 = fma((double)v[0], (double)v[0], n2); n2 = fma((double)v[1], (double)v[1], n2);
        n2 = fma((double)v[2], (double)v[2], n2); n2 = fma((double)v[3], (double)v[3], n2);
      }
    }
  rnorm[k] = (float)(1.0 / sqrt(n2 + 1e-12));   // WCT_SWAP_EPS
}

__global__ __launch_bounds__(256) void swap_init_kernel(unsigned long long* run, long nq) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q < nq) run[q] = SW_NONE;
}

__global__ __launch_bounds__(256) void swap_final_kernel(const unsigned long long* __restrict__ run, long nq, int32_t* __restrict__ idx,
                                                         float* __restrict__ best) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const unsigned long long v = run[q];
  const unsigned hi = (unsigned)(v >> 32);
  idx[q] = (int32_t)(0xffffffffu - (unsigned)v);
  if (best) best[q] = hi ? ord_f32(hi) : __uint_as_float(0x7fc00000u);   // no score ever won (all NaN): NaN
}

// one 32-channel chunk of a 10 x 18 pixel window -> split planes.  Pixels outside the map and channels >= C are zeros: no valid
// (query, key) pair reads the former, and the latter add exact zeros.
__device__ __forceinline__ void stage_tile(const float* __restrict__ map, int mh, int mw, int C, int y0, int x0, int c0, u32x4* dst, int tid,
                                           SatTrack& sat) {
  for (int u = tid; u < SW_NPIX * 4; u += SW_THREADS) {
    const int kq = u & 3, px = u >> 2;
    const int py = px / SW_HX, pxx = px - py * SW_HX;
    const int y = y0 + py, x = x0 + pxx, c = c0 + 8 * kq;
    f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f}, b = a;
    if (y < mh && x < mw) {
      const float* p = map + ((size_t)y * mw + x) * C + c;
      if (c < C) a = *reinterpret_cast<const f32x4*>(p);
      if (c + 4 < C) b = *reinterpret_cast<const f32x4*>(p + 4);
    }
    f16x8 hi, lo;
    split8(a, b, hi, lo, sat);
    dst[(0 * 4 + kq) * SW_NP + px] = __builtin_bit_cast(u32x4, hi);
    dst[(1 * 4 + kq) * SW_NP + px] = __builtin_bit_cast(u32x4, lo);
  }
}

// keys [k0, k1) (key rows ky0 .. of the band, tiles ktx x kty of it) against every query
__global__ __launch_bounds__(SW_THREADS) void swap_match_kernel(const float* __restrict__ Q, int h, int w, const float* __restrict__ K, int hs, int ws,
                                                                int C, const float* __restrict__ rnorm, int k0, int k1, int ky0, int ktiles_x,
                                                                int nkt, int qtiles_x, unsigned long long* run, unsigned* sat_counter) {
  __shared__ u32x4 lds[2 * SW_PLANES];
  u32x4* const ldsQ = lds;
  u32x4* const ldsK = lds + SW_PLANES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kq = lane >> 4, wm = wave & 1, wn = wave >> 1;
  const int qty = blockIdx.x / qtiles_x, qtx = blockIdx.x - qty * qtiles_x;
  const int qy0 = qty * SW_TY, qx0 = qtx * SW_TX;
  const int qw = w - 2, kw = ws - 2, kh = hs - 2;
  const int nchunks = (C + SW_CK - 1) / SW_CK;
  SatTrack sat;

  float bs[4][4];
  int bi[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) { bs[m][r] = -__builtin_inff(); bi[m][r] = INT_MAX; }

  const u32x4* aQ = ldsQ + kq * SW_NP + (4 * wm) * SW_HX + li;
  const u32x4* aK = ldsK + kq * SW_NP + (4 * wn) * SW_HX + li;

  for (int kt = blockIdx.y; kt < nkt; kt += gridDim.y) {
    const int ktr = kt / ktiles_x;
    const int kty = ky0 + ktr * SW_TY, ktx = (kt - ktr * ktiles_x) * SW_TX;
    f32x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int cc = 0; cc < nchunks; ++cc) {
      __syncthreads();   // the previous chunk's reads are done
      stage_tile(Q, h, w, C, qy0, qx0, cc * SW_CK, ldsQ, tid, sat);
      stage_tile(K, hs, ws, C, kty, ktx, cc * SW_CK, ldsK, tid, sat);
      __syncthreads();
#pragma unroll
      for (int dx = 0; dx < 3; ++dx)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
          f16x8 ah[4], al[4], bh[4], bl[4];
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            ah[m] = __builtin_bit_cast(f16x8, aQ[(m + dy) * SW_HX + dx]);
            al[m] = __builtin_bit_cast(f16x8, aQ[4 * SW_NP + (m + dy) * SW_HX + dx]);
            bh[m] = __builtin_bit_cast(f16x8, aK[(m + dy) * SW_HX + dx]);
            bl[m] = __builtin_bit_cast(f16x8, aK[4 * SW_NP + (m + dy) * SW_HX + dx]);
          }
#pragma unroll
          for (int term = 0; term < 3; ++term)   // dependent MFMAs 16 apart
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
              for (int n = 0; n < 4; ++n)
                acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(term == 2 ? al[m] : ah[m], term == 1 ? bl[n] : bh[n], acc[m][n], 0, 0, 0);
        }
    }

    // this lane's 4 keys (rows 4 wn + n of the tile, column li) against its 16 queries, by the full rule: tiles come in no index order
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int kyy = kty + 4 * wn + n, kxx = ktx + li;
      const bool inmap = kyy < kh && kxx < kw;
      const int kidx = inmap ? kyy * kw + kxx : 0;   // inside the map: below Nk < 2^31
      const bool valid = inmap && kidx >= k0 && kidx < k1;
      const float rn = valid ? rnorm[kidx] : 0.f;
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float s = __fmul_rn(acc[m][n][r], rn) + 0.f;   // + 0: -0 and +0 are one score
          if (valid && (s > bs[m][r] || (s == bs[m][r] && kidx < bi[m][r]))) { bs[m][r] = s; bi[m][r] = kidx; }
        }
    }
  }

  // 16 lanes (li) hold the same queries over different keys
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float s = bs[m][r];
      int i = bi[m][r];
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {
        const float so = __shfl_xor(s, off, 64);
        const int io = __shfl_xor(i, off, 64);
        if (so > s || (so == s && io < i)) { s = so; i = io; }
      }
      const int qy = qy0 + 4 * wm + m, qx = qx0 + 4 * kq + r;
      if (li == 0 && i != INT_MAX && qy < h - 2 && qx < qw)
        atomicMax(run + (size_t)qy * qw + qx, ((unsigned long long)f32_ord(s) << 32) | (unsigned long long)(0xffffffffu - (unsigned)i));
    }
  sat.commit(sat_counter);
}

__global__ __launch_bounds__(256) void swap_assemble_kernel(const int32_t* __restrict__ idx, int h, int w, const float* __restrict__ V, int hs, int ws,
                                                            int C, const float* base, float alpha, float oma, float* out) {
  const int c4n = C >> 2;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)h * w * c4n) return;
  const int c4 = (int)(t % c4n);
  const long p = t / c4n;
  const int y = (int)(p / w), x = (int)(p - (long)y * w);
  const int qw = w - 2, kw = ws - 2;
  const int nk1 = (hs - 2) * kw - 1;
  const int qya = y - 2 > 0 ? y - 2 : 0, qyb = y < h - 3 ? y : h - 3;
  const int qxa = x - 2 > 0 ? x - 2 : 0, qxb = x < w - 3 ? x : w - 3;
  f32x4 sum = f32x4{0.f, 0.f, 0.f, 0.f};
  int cnt = 0;
  for (int qy = qya; qy <= qyb; ++qy)
    for (int qx = qxa; qx <= qxb; ++qx) {
      int k = idx[(size_t)qy * qw + qx];
      k = k < 0 ? 0 : (k > nk1 ? nk1 : k);
      const int ky = k / kw, kx = k - ky * kw;
      const f32x4 v = *reinterpret_cast<const f32x4*>(V + ((size_t)(ky + y - qy) * ws + kx + x - qx) * C + 4 * c4);
#pragma unroll
      for (int e = 0; e < 4; ++e) sum[e] = __fadd_rn(sum[e], v[e]);
      ++cnt;
    }
  const float n = (float)cnt;
  const size_t o = (size_t)p * C + 4 * c4;
  f32x4 b = f32x4{0.f, 0.f, 0.f, 0.f};
  if (base) b = *reinterpret_cast<const f32x4*>(base + o);
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float am = __fmul_rn(alpha, __fdiv_rn(sum[e], n));
    r[e] = base ? __fadd_rn(am, __fmul_rn(oma, b[e])) : am;
  }
  *reinterpret_cast<f32x4*>(out + o) = r;
}

}  // namespace

size_t swap_run_bytes(long nq) { return (size_t)nq * sizeof(unsigned long long); }
size_t swap_norm_bytes(long nk) { return (size_t)nk * sizeof(float); }

hipError_t launch_patch_match(const float* q, int h, int w, const float* k, int hs, int ws, int C, int key_chunk, int32_t* idx, float* best,
                              void* run, size_t run_bytes, float* rnorm, size_t norm_bytes, unsigned* sat, hipStream_t s) {
  // arguments are checked where they can be answered with a message (api_swap.hip); this one guards the intermediates' bounds
  const int qh = h - 2, qw = w - 2, kh = hs - 2, kw = ws - 2;
  const long nq = (long)qh * qw, nk = (long)kh * kw;
  if (qh < 1 || qw < 1 || kh < 1 || kw < 1 || nk > INT_MAX || key_chunk < 1 || (C & 3) || C < 4) return hipErrorInvalidValue;
  if (run_bytes < swap_run_bytes(nq) || norm_bytes < swap_norm_bytes(nk)) return hipErrorInvalidValue;
  unsigned long long* r = reinterpret_cast<unsigned long long*>(run);
  hipLaunchKernelGGL(swap_norm_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, s, k, hs, ws, C, rnorm);
  hipLaunchKernelGGL(swap_init_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, r, nq);
  const int qtiles_x = (qw + SW_TX - 1) / SW_TX, qtiles_y = (qh + SW_TY - 1) / SW_TY;
  const int ktiles_x = (kw + SW_TX - 1) / SW_TX;
  const long qtiles = (long)qtiles_x * qtiles_y;
  int nlaunch = 0, nkt_first = 0, split_first = 0, nkt_last = 0, split_last = 0;
  for (long c0 = 0; c0 < nk; c0 += key_chunk) {
    const long c1 = c0 + key_chunk < nk ? c0 + key_chunk : nk;
    const int ky0 = (int)(c0 / kw), ky1 = (int)((c1 - 1) / kw);          // the band of key rows the chunk touches
    const int nkt = ((ky1 - ky0 + 1 + SW_TY - 1) / SW_TY) * ktiles_x;
    // key tiles are dealt to grid.y workgroups per query tile, enough for ~1024 workgroups where the sizes allow (a function of the sizes alone)
    long split = (1024 + qtiles - 1) / qtiles;
    if (split > nkt) split = nkt;
    if (split > 65535) split = 65535;
    hipLaunchKernelGGL(swap_match_kernel, dim3((unsigned)qtiles, (unsigned)split), dim3(SW_THREADS), 0, s, q, h, w, k, hs, ws, C, rnorm, (int)c0,
                       (int)c1, ky0, ktiles_x, nkt, qtiles_x, r, sat);
    if (!nlaunch++) { nkt_first = nkt; split_first = (int)split; }
    nkt_last = nkt; split_last = (int)split;
  }
  // "prof_forms": q<query tiles>.l<launches>.<key tiles>/<grid.y> of the first launch.<the same of the last> (include/wct_hip.h)
  char form[sizeof wct_launch_form.text];
  snprintf(form, sizeof form, "q%ld.l%d.%d/%d.%d/%d", qtiles, nlaunch, nkt_first, split_first, nkt_last, split_last);
  note_launch_text(form);
  hipLaunchKernelGGL(swap_final_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, r, nq, idx, best);
  return hipGetLastError();
}

hipError_t launch_patch_assemble(const int32_t* idx, int h, int w, const float* v, int hs, int ws, int C, const float* base, float alpha, float* out,
                                 hipStream_t s) {
  if (h < 3 || w < 3 || hs < 3 || ws < 3 || (C & 3) || C < 4 || (!base && alpha != 1.f)) return hipErrorInvalidValue;
  const long n = (long)h * w * (C >> 2);
  hipLaunchKernelGGL(swap_assemble_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, idx, h, w, v, hs, ws, C, base, alpha, 1.0f - alpha, out);
  return hipGetLastError();
}
