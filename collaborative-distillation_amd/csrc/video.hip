// Video mode (include/wct_hip_video.h): the tracking step of a level's content sums, the motion-adaptive recursive blend of the output,
// and the end-of-frame store (previous content crop, previous output, pending -> running sums).  Nothing here clamps or counts: the
// f16x3 range flag is the cascade's business.
#include "../../include/wct_hip_video.h"
#include "wct_common.h"

#include <cfloat>
#include <climits>

namespace {

// ---- tracking ---------------------------------------------------------------------------------------------------------------------
constexpr int TRK_THREADS = 1024, TRK_SLOTS = 512;   // one slot per channel of the widest level

// r + rate (c - r) as three separately rounded operations.  Plain operators under the pragma: the __d*_rn functions are inline bodies
// compiled under the translation unit's contraction mode, and the compiler did fuse their product and sum into one fma here.
__device__ __forceinline__ double track_ema(double r, double c, double rate) {
#pragma clang fp contract(off)
  const double d = c - r;
  const double m = rate * d;
  return r + m;
}

// run / pend: [rs C | rss C*C] of the level.  A deciding launch is ONE workgroup: every thread has read what it needs of `sum` behind
// the barriers before any thread rewrites it.
__global__ __launch_bounds__(TRK_THREADS) void clip_track_kernel(int C, double n, int decide, double rate, double cut_thr, const double* run,
                                                                 double* pend, double* sum, double* sumsq, int* flags) {
  __shared__ double red[2][TRK_SLOTS];
  __shared__ int s_cut;
  const int t = threadIdx.x;
  if (decide) {
    if (t < TRK_SLOTS) {
      double a = 0.0, v = 0.0;
      if (t < C) {
        const double mu_c = sum[t] / n, mu_r = run[t] / n, dm = mu_c - mu_r;
        a = dm * dm;
        v = run[(size_t)C + (size_t)t * C + t] / n - mu_r * mu_r;
      }
      red[0][t] = a;
      red[1][t] = v;
    }
    __syncthreads();
    for (int s = TRK_SLOTS / 2; s >= 1; s >>= 1) {   // pairwise over all 512 slots: the order does not even depend on C
      if (t < s) { red[0][t] += red[0][t + s]; red[1][t] += red[1][t + s]; }
      __syncthreads();
    }
    if (t == 0) {
      const double D = red[0][0] / fmax(red[1][0], DBL_MIN);
      const int cut = (flags[0] == 0 || !(D <= cut_thr)) ? 1 : 0;   // NaN: a cut
      flags[1] = cut;
      s_cut = cut;
    }
  } else if (t == 0) {
    s_cut = flags[1];
  }
  __syncthreads();
  const bool take = s_cut != 0 || rate == 1.0;
  const size_t total = (size_t)C + (size_t)C * C;
  for (size_t i = (size_t)blockIdx.x * TRK_THREADS + t; i < total; i += (size_t)gridDim.x * TRK_THREADS) {
    double* src = i < (size_t)C ? sum + i : sumsq + (i - C);
    const double c = *src;
    const double r = take ? c : track_ema(run[i], c, rate);
    pend[i] = r;
    *src = r;
  }
}

// ---- small vector helpers -----------------------------------------------------------------------------------------------------------
// four consecutive floats of which the first n exist; vec: p is 16-byte aligned and n == 4
__device__ __forceinline__ f32x4 ld4(const float* p, int n, bool vec) {
  if (vec) return *reinterpret_cast<const f32x4*>(p);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < n) v[k] = p[k];
  return v;
}
__device__ __forceinline__ void st4(float* p, f32x4 v, int n, bool vec) {
  if (vec) { *reinterpret_cast<f32x4*>(p) = v; return; }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < n) p[k] = v[k];
}

// ---- end of a frame: prev_content <- the content's crop, prev_out <- out (Wo a multiple of 4: groups of four lie in one row), then
//      running <- pending and frames += 1 by the workgroups behind the image's
__global__ __launch_bounds__(256) void clip_store_kernel(const float* content, int Hc, int Wc, const float* out, int Ho, int Wo, float* prev_content,
                                                         float* prev_out, int vec_c, int vec_o, unsigned img_blocks, const double* pend, double* run,
                                                         size_t nd, int* flags) {
  if (blockIdx.x < img_blocks) {
    const long row_groups = Wo >> 2, plane_groups = (long)Ho * row_groups, groups = 3 * plane_groups;
    const size_t cplane = (size_t)Hc * Wc;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)img_blocks * 256) {
      const long ch = g / plane_groups, rem = g - ch * plane_groups, y = rem / row_groups, xg = rem - y * row_groups;
      st4(prev_out + g * 4, ld4(out + g * 4, 4, vec_o), 4, true);
      st4(prev_content + g * 4, ld4(content + ch * cplane + (size_t)y * Wc + 4 * xg, 4, vec_c), 4, true);
    }
    return;
  }
  const unsigned b = blockIdx.x - img_blocks, nb = gridDim.x - img_blocks;
  for (size_t i = (size_t)b * 256 + threadIdx.x; i < nd; i += (size_t)nb * 256) run[i] = pend[i];
  if (b == 0 && threadIdx.x == 0 && flags[0] < INT_MAX) flags[0] += 1;
}

// ---- blend ----------------------------------------------------------------------------------------------------------------------------
constexpr int TB_W = 64, TB_H = 16;                                                      // output tile: 256 threads x 4 pixels of a row
constexpr int TB_EW = TB_W + 2 * WCT_CLIP_MAX_RADIUS, TB_EH = TB_H + 2 * WCT_CLIP_MAX_RADIUS;   // the tile with its halo at the largest radius

// the conversion of misc.hip planar_to_u8_kernel (and color.hip): mul(255), + 0.5 with round_mode 1, clamp, truncation
__device__ __forceinline__ unsigned to_u8(float v, int round_mode) {
  float x = __fmul_rn(v, 255.0f);
  if (round_mode) x = __fadd_rn(x, 0.5f);
  x = fminf(fmaxf(x, 0.f), 255.f);     // NaN -> 0
  return (unsigned)x;                  // truncation toward zero
}

// Four floats of row clamp(y + vy) of an Ho x Wo plane from column x + vx on, each column clamped to the row; the first n exist.  The clamp
// makes any vector safe; inside the row the four are consecutive at a 4-byte alignment (include/wct_hip_motion.h, Compensated blend).
__device__ __forceinline__ f32x4 ld4_moved(const float* plane, int Ho, int Wo, int y, int x, int n, int vy, int vx) {
  const float* row = plane + (size_t)min(max(y + vy, 0), Ho - 1) * Wo;
  const int xs = x + vx;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (n == 4 && xs >= 0 && xs + 3 < Wo) {
    __builtin_memcpy(&v, row + xs, sizeof v);
    return v;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < n) v[k] = row[min(max(xs + k, 0), Wo - 1)];
  return v;
}

// vec_c / vec_o: the content / the four Ho x Wo images take 16-byte accesses (Wo, and for vec_c Wc, multiples of 4; aligned bases).
// MV: prev and pout are read through the field mv[.][nbx][2] of 8 x 8 blocks -- a group of four pixels starts at a multiple of 4, so it
// lies in one block and has one vector.  Without MV neither mv nor nbx is looked at: that instantiation is video mode's kernel as it was.
template <bool MV>
__global__ __launch_bounds__(256) void temporal_blend_kernel(const float* cur, int Hc, int Wc, const float* prev, const float* sty, const float* pout,
                                                             int Ho, int Wo, float blend, float two_s2, int r, const int* cut_flag, float* out,
                                                             uint8_t* out_hwc, int round_mode, int vec_c, int vec_o, const int16_t* mv, int nbx) {
  __shared__ __attribute__((aligned(16))) float e[TB_EH][TB_EW];    // squared content difference over the tile and its halo; 0 outside the image
  __shared__ __attribute__((aligned(16))) float hs[TB_EH][TB_W];    // its horizontal window sums
  const int tid = threadIdx.x, tx0 = blockIdx.x * TB_W, ty0 = blockIdx.y * TB_H;
  const int row = tid >> 4, xg = tid & 15, y = ty0 + row, x = tx0 + 4 * xg;
  const size_t plane = (size_t)Ho * Wo, cplane = (size_t)Hc * Wc;
  const bool live = y < Ho && x < Wo;
  const int n = live ? (Wo - x < 4 ? Wo - x : 4) : 0;
  const int cut = cut_flag ? *cut_flag : 0;      // uniform over the grid
  float wgt[4] = {0.f, 0.f, 0.f, 0.f};
  if (!cut) {
    const int hx = (r + 3) & ~3;                 // the halo in x rounded up to whole groups of four: every group stays aligned
    const int eh = TB_H + 2 * r, gw = (TB_W + 2 * hx) >> 2;
    for (int idx = tid; idx < eh * gw; idx += 256) {
      const int gy = idx / gw, gx = idx - gy * gw;
      const int yy = ty0 - r + gy, xx = tx0 - hx + 4 * gx;    // xx is a multiple of 4: a group is left of the image or starts inside [0, ...)
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      if (yy >= 0 && yy < Ho && xx >= 0 && xx < Wo) {
        const int m = Wo - xx < 4 ? Wo - xx : 4;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const f32x4 a = ld4(cur + ch * cplane + (size_t)yy * Wc + xx, m, vec_c);
          f32x4 b;
          if constexpr (MV) {
            const int16_t* v = mv + ((size_t)(yy >> 3) * nbx + (xx >> 3)) * 2;
            b = ld4_moved(prev + ch * plane, Ho, Wo, yy, xx, m, v[0], v[1]);
          } else {
            b = ld4(prev + ch * plane + (size_t)yy * Wo + xx, m, vec_o);
          }
          const f32x4 d = a - b;                 // both 0 past the row's end
          acc += d * d;
        }
      }
      *reinterpret_cast<f32x4*>(&e[gy][4 * gx]) = acc;
    }
    __syncthreads();
    for (int idx = tid; idx < eh * TB_W; idx += 256) {
      const int gy = idx >> 6, xl = idx & (TB_W - 1);
      float s = 0.f;
      for (int dx = 0; dx <= 2 * r; ++dx) s += e[gy][hx - r + xl + dx];   // ascending x
      hs[gy][xl] = s;
    }
    __syncthreads();
    if (live) {
      const int cy = min(y + r, Ho - 1) - max(y - r, 0) + 1;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float s = 0.f;
        for (int dy = 0; dy <= 2 * r; ++dy) s += hs[row + dy][4 * xg + k];   // ascending y
        const int cx = min(x + k + r, Wo - 1) - max(x + k - r, 0) + 1;
        const float d = s / (float)(cx * cy);
        wgt[k] = blend * expf(-d / two_s2);
      }
    }
  }
  if (!live) return;
  const bool v4 = vec_o && n == 4;
  const size_t o0 = (size_t)y * Wo + x;
  f32x4 o[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const f32x4 s = ld4(sty + ch * plane + o0, n, v4);
    if (cut) {
      o[ch] = s;
    } else {
      f32x4 p;
      if constexpr (MV) {
        const int16_t* v = mv + ((size_t)(y >> 3) * nbx + (x >> 3)) * 2;
        p = ld4_moved(pout + ch * plane, Ho, Wo, y, x, n, v[0], v[1]);
      } else {
        p = ld4(pout + ch * plane + o0, n, v4);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) o[ch][k] = s[k] + wgt[k] * (p[k] - s[k]);
    }
    st4(out + ch * plane + o0, o[ch], n, v4);
  }
  if (out_hwc) {
    unsigned b[12];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) b[k * 3 + ch] = to_u8(o[ch][k], round_mode);
    if (n == 4 && (Wo & 3) == 0 && (reinterpret_cast<size_t>(out_hwc) & 3) == 0) {   // o0 * 3 is then a multiple of 12
      unsigned* dst = reinterpret_cast<unsigned*>(out_hwc + o0 * 3);
      dst[0] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
      dst[1] = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
      dst[2] = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k)   // unrolled and predicated: b[] stays in registers
        if (k < n * 3) out_hwc[o0 * 3 + k] = (uint8_t)b[k];
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

}  // namespace

int blend_tile_w() { return TB_W; }
int blend_tile_h() { return TB_H; }

hipError_t launch_clip_track(int C, double n, int decide, double rate, double cut_thr, const double* run, double* pend, double* sum, double* sumsq,
                             int* flags, hipStream_t s) {
  if (C < 1 || C > TRK_SLOTS) return hipErrorInvalidValue;
  const size_t total = (size_t)C + (size_t)C * C;
  const unsigned blocks = decide ? 1u : (unsigned)std::min<size_t>((total + TRK_THREADS - 1) / TRK_THREADS, 64);
  hipLaunchKernelGGL(clip_track_kernel, dim3(blocks), dim3(TRK_THREADS), 0, s, C, n, decide, rate, cut_thr, run, pend, sum, sumsq, flags);
  return hipGetLastError();
}

hipError_t launch_clip_store(const float* content, int Hc, int Wc, const float* out, int Ho, int Wo, float* prev_content, float* prev_out,
                             const double* pend, double* run, size_t nd, int* flags, hipStream_t s) {
  unsigned img_blocks = 0;
  int vec_c = 0, vec_o = 0;
  if (content) {
    if (Ho < 1 || Wo < 4 || (Wo & 3) || Ho > Hc || Wo > Wc || !aligned16(prev_content) || !aligned16(prev_out)) return hipErrorInvalidValue;
    const long groups = 3L * Ho * (Wo >> 2);
    img_blocks = (unsigned)std::min<long>((groups + 255) / 256, 4096);
    vec_c = (Wc & 3) == 0 && aligned16(content);
    vec_o = aligned16(out);
  }
  const unsigned commit_blocks = (unsigned)std::min<size_t>(std::max<size_t>((nd + 255) / 256, 1), 64);
  hipLaunchKernelGGL(clip_store_kernel, dim3(img_blocks + commit_blocks), dim3(256), 0, s, content, Hc, Wc, out, Ho, Wo, prev_content, prev_out, vec_c,
                     vec_o, img_blocks, pend, run, nd, flags);
  return hipGetLastError();
}

hipError_t launch_temporal_blend(const float* cur, int Hc, int Wc, const float* prev, const float* sty, const float* pout, int Ho, int Wo, float blend,
                                 float sigma, int r, const int* cut_flag, float* out, uint8_t* out_hwc, int round_mode, hipStream_t s) {
  if (Ho < 1 || Wo < 1 || Ho > Hc || Wo > Wc || r < 0 || r > WCT_CLIP_MAX_RADIUS) return hipErrorInvalidValue;
  const int quad = (Wo & 3) == 0;
  const int vec_c = quad && (Wc & 3) == 0 && aligned16(cur);
  const int vec_o = quad && aligned16(prev) && aligned16(sty) && aligned16(pout) && aligned16(out);
  const dim3 grid((unsigned)((Wo + TB_W - 1) / TB_W), (unsigned)((Ho + TB_H - 1) / TB_H));
  hipLaunchKernelGGL(temporal_blend_kernel<false>, grid, dim3(256), 0, s, cur, Hc, Wc, prev, sty, pout, Ho, Wo, blend, 2.0f * sigma * sigma, r, cut_flag,
                     out, out_hwc, round_mode, vec_c, vec_o, static_cast<const int16_t*>(nullptr), 0);
  return hipGetLastError();
}

hipError_t launch_motion_blend(const float* cur, int Hc, int Wc, const float* prev, const float* sty, const float* pout, int Ho, int Wo, float blend,
                               float sigma, int r, const int* cut_flag, float* out, uint8_t* out_hwc, int round_mode, const int16_t* mv, int nbx,
                               hipStream_t s) {
  if (!mv) return launch_temporal_blend(cur, Hc, Wc, prev, sty, pout, Ho, Wo, blend, sigma, r, cut_flag, out, out_hwc, round_mode, s);
  if (Ho < 1 || Wo < 1 || Ho > Hc || Wo > Wc || r < 0 || r > WCT_CLIP_MAX_RADIUS || nbx != (Wo + 7) / 8) return hipErrorInvalidValue;
  const int quad = (Wo & 3) == 0;
  const int vec_c = quad && (Wc & 3) == 0 && aligned16(cur);
  const int vec_o = quad && aligned16(sty) && aligned16(out);      // prev and pout are gathered: their alignment does not matter
  const dim3 grid((unsigned)((Wo + TB_W - 1) / TB_W), (unsigned)((Ho + TB_H - 1) / TB_H));
  hipLaunchKernelGGL(temporal_blend_kernel<true>, grid, dim3(256), 0, s, cur, Hc, Wc, prev, sty, pout, Ho, Wo, blend, 2.0f * sigma * sigma, r, cut_flag,
                     out, out_hwc, round_mode, vec_c, vec_o, mv, nbx);
  return hipGetLastError();
}
