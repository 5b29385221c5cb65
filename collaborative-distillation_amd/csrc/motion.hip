// Motion compensation (include/wct_hip_motion.h): the luma pyramid as packed bytes, and the block search of one pyramid level on the
// packed-byte SAD instruction.  Integer arithmetic behind the luma: nothing here rounds, clamps an activation or counts.  The compensated
// blend is video.hip's kernel with a field (temporal_blend_kernel<true>).
#include "../../include/wct_hip_motion.h"
#include "wct_common.h"

namespace {

// ---- luma and pyramid ---------------------------------------------------------------------------------------------------------------
constexpr int PY_W = 64, PY_H = 16;     // the level-0 tile of a workgroup: 256 threads x 4 pixels of a row; 2^3 divides both
constexpr int PY_DW = PY_W / 4;         // ... in dwords

struct PyrArgs { int levels; int H[4], W[4], pitch[4]; unsigned off[4]; };

// (0.299 r + 0.587 g) + 0.114 b as three products and two sums, each rounded on its own, then the uint8 conversion of video.hip to_u8 with
// rounding.  Plain operators under the pragma, as video.hip track_ema: the compiler fuses the bodies of the __f*_rn functions.
__device__ __forceinline__ unsigned luma_u8(float r, float g, float b) {
#pragma clang fp contract(off)
  const float pr = 0.299f * r;
  const float pg = 0.587f * g;
  const float pb = 0.114f * b;
  const float t0 = pr + pg;
  const float t = t0 + pb;
  float x = t * 255.0f;
  x = x + 0.5f;
  x = fminf(fmaxf(x, 0.f), 255.f);      // NaN -> 0
  return (unsigned)x;                   // truncation toward zero
}

// four pixels of the next level from two rows of eight bytes (a0 a1 / b0 b1: dwords): (a + b + c + d + 2) >> 2 per 2 x 2 cell
__device__ __forceinline__ unsigned down4(unsigned a0, unsigned a1, unsigned b0, unsigned b1) {
  unsigned o = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned a = k < 2 ? a0 : a1, b = k < 2 ? b0 : b1;
    const int sh = (2 * k & 3) * 8;
    const unsigned s = ((a >> sh) & 255u) + ((a >> (sh + 8)) & 255u) + ((b >> sh) & 255u) + ((b >> (sh + 8)) & 255u) + 2u;
    o |= (s >> 2) << (8 * k);
  }
  return o;
}

// bytes k >= n of a dword cleared (n in 1 .. 4)
__device__ __forceinline__ unsigned keep_bytes(unsigned v, int n) { return n >= 4 ? v : v & ((1u << (8 * n)) - 1u); }

// One workgroup = one 16 x 64 tile of level 0 and everything above it: the tile's origin is a multiple of 8 at every level, so level k of
// the tile is a (16 >> k) x (64 >> k) tile of level k, made from the LDS copy of level k - 1.  One pass over the fp32 planes, one launch.
__global__ __launch_bounds__(256) void motion_pyramid_kernel(const float* img, int Hc, int Wc, PyrArgs a, uint8_t* pyr) {
  __shared__ unsigned t[4][PY_H][PY_DW];
  const int tid = threadIdx.x, tx0 = blockIdx.x * PY_W, ty0 = blockIdx.y * PY_H;
  {
    const int row = tid >> 4, xg = tid & 15, y = ty0 + row, x = tx0 + 4 * xg;
    unsigned pk = 0;
    if (y < a.H[0] && x < a.W[0]) {
      const size_t cplane = (size_t)Hc * Wc;
      const float* p = img + (size_t)y * Wc + x;
      const int n = a.W[0] - x < 4 ? a.W[0] - x : 4;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < n) pk |= luma_u8(p[k], p[cplane + k], p[2 * cplane + k]) << (8 * k);
      *reinterpret_cast<unsigned*>(pyr + a.off[0] + (size_t)y * a.pitch[0] + x) = pk;     // x + 3 < pitch: the padding is written as zeros
    }
    t[0][row][xg] = pk;
  }
  for (int k = 1; k < a.levels; ++k) {      // uniform
    __syncthreads();
    const int dw = PY_DW >> k, rows = PY_H >> k;
    if (tid < dw * rows) {
      const int row = tid / dw, xg = tid - row * dw, y = (ty0 >> k) + row, x = (tx0 >> k) + 4 * xg;
      unsigned pk = 0;
      if (y < a.H[k] && x < a.W[k]) {
        pk = down4(t[k - 1][2 * row][2 * xg], t[k - 1][2 * row][2 * xg + 1], t[k - 1][2 * row + 1][2 * xg], t[k - 1][2 * row + 1][2 * xg + 1]);
        pk = keep_bytes(pk, a.W[k] - x);
        *reinterpret_cast<unsigned*>(pyr + a.off[k] + (size_t)y * a.pitch[k] + x) = pk;
      }
      t[k][row][xg] = pk;
    }
  }
}

__global__ __launch_bounds__(256) void motion_unpad_kernel(const uint8_t* pyr, PyrArgs a, uint8_t* out) {
  size_t base = 0;
  for (int k = 0; k < a.levels; ++k) {
    const size_t n = (size_t)a.H[k] * a.W[k];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
      const size_t y = i / a.W[k], x = i - y * a.W[k];
      out[base + i] = pyr[a.off[k] + y * a.pitch[k] + x];
    }
    base += n;
  }
}

// ---- block search ---------------------------------------------------------------------------------------------------------------------
// A workgroup of 256 lanes holds BPW blocks of LPB lanes each; a lane is one candidate.  The top level has up to 1 + 15^2 = 226
// candidates per block: one block, every lane.  A finer level has 10: sixteen blocks of sixteen lanes.
// Per block in LDS, as dwords of four packed bytes:
//   cur  [8][2]     the block, zero outside its clip
//   zero [8][3]     finer levels: the co-located block of the previous image (the (0, 0) candidate need not lie in the window); the third
//                   dword of a row is padding for the aligner
//   win  [S][WP]    the search window of the previous image, S = 8 + 2 range at the top and 10 = 8 + 2 at a finer level, zero outside the
//                   image; WP dwords per row so that the aligner's three dwords exist for every candidate offset
constexpr int SR_TOP_S = WCT_MOTION_BLOCK + 2 * WCT_MOTION_MAX_RANGE, SR_TOP_WP = 7;     // 22 rows; byte offset <= 14 -> dwords 3, 4, 5
constexpr int SR_FINE_S = WCT_MOTION_BLOCK + 2, SR_FINE_WP = 3;                          // 10 rows; byte offset <= 2 -> dwords 0, 1, 2
constexpr int SR_TOP_DW = 16 + SR_TOP_S * SR_TOP_WP, SR_FINE_DW = 16 + 24 + SR_FINE_S * SR_FINE_WP;
constexpr int SR_FINE_BPW = 16;

struct SearchArgs { int H, W, pitch; unsigned off; int nby, nbx, pnby, pnbx, range, penalty; };

// four bytes of row gy of a level from column gx on, 0 where (gy, gx + k) is outside the image or k >= n
__device__ __forceinline__ unsigned gather4(const uint8_t* img, const SearchArgs& a, int gy, int gx, int n) {
  unsigned v = 0;
  if (gy < 0 || gy >= a.H) return 0;
  const uint8_t* row = img + a.off + (size_t)gy * a.pitch;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < n && gx + k >= 0 && gx + k < a.W) v |= (unsigned)row[gx + k] << (8 * k);
  return v;
}

// SAD of the bh x bw block against the eight-byte rows that start `ox` bytes into row `oy` of src (pitch P dwords): per row two dwords
// brought to the byte offset by the aligner, the bytes outside the clip masked, two packed-byte SADs
__device__ __forceinline__ unsigned block_sad(const unsigned* cur, const unsigned* src, int P, int oy, int ox, int bh, unsigned mlo, unsigned mhi) {
  const unsigned* row = src + oy * P + (ox >> 2);
  const unsigned sh = (unsigned)ox & 3u;
  unsigned acc = 0;
#pragma unroll
  for (int r = 0; r < WCT_MOTION_BLOCK; ++r) {
    if (r < bh) {
      const unsigned d0 = row[r * P], d1 = row[r * P + 1], d2 = row[r * P + 2];
      const unsigned lo = __builtin_amdgcn_alignbyte(d1, d0, sh) & mlo, hi = __builtin_amdgcn_alignbyte(d2, d1, sh) & mhi;
      acc = __builtin_amdgcn_sad_u8(lo, cur[2 * r], acc);
      acc = __builtin_amdgcn_sad_u8(hi, cur[2 * r + 1], acc);
    }
  }
  return acc;
}

template <bool TOP>
__global__ __launch_bounds__(256) void motion_search_kernel(const uint8_t* pcur, const uint8_t* pprev, SearchArgs a, const int16_t* mvp, int16_t* mvo,
                                                            const int* cut_flag) {
  constexpr int LPB = TOP ? 256 : 256 / SR_FINE_BPW, BPW = 256 / LPB, DW = TOP ? SR_TOP_DW : SR_FINE_DW, WP = TOP ? SR_TOP_WP : SR_FINE_WP;
  __shared__ unsigned lds[BPW * DW];
  __shared__ unsigned skey[BPW];
  const int tid = threadIdx.x, lb = tid / LPB, c = tid - lb * LPB;
  const int nb = a.nby * a.nbx, b = blockIdx.x * BPW + lb;
  const bool live = b < nb;
  if (cut_flag && *cut_flag) {                   // uniform over the grid: the field of a cut is zero
    if (live && c == 0) { mvo[2 * b] = 0; mvo[2 * b + 1] = 0; }
    return;
  }
  const int by = live ? b / a.nbx : 0, bx = live ? b - by * a.nbx : 0;
  const int y0 = by * WCT_MOTION_BLOCK, x0 = bx * WCT_MOTION_BLOCK;
  const int bh = min(WCT_MOTION_BLOCK, a.H - y0), bw = min(WCT_MOTION_BLOCK, a.W - x0);
  const int R = TOP ? a.range : 1, S = WCT_MOTION_BLOCK + 2 * R;
  int py = 0, px = 0;                            // finer levels: twice the parent's vector
  if (!TOP && live) {
    const int16_t* v = mvp + ((size_t)min(by >> 1, a.pnby - 1) * a.pnbx + min(bx >> 1, a.pnbx - 1)) * 2;
    py = 2 * v[0];
    px = 2 * v[1];
  }
  unsigned* cur = lds + lb * DW;
  unsigned* zero = cur + 16;                     // finer levels only
  unsigned* win = cur + (TOP ? 16 : 40);
  if (c == 0) skey[lb] = 0xFFFFFFFFu;
  if (live) {
    for (int i = c; i < 16; i += LPB) {
      const int r = i >> 1, h = i & 1;
      cur[i] = r < bh ? gather4(pcur, a, y0 + r, x0 + 4 * h, bw - 4 * h) : 0u;
    }
    if (!TOP)
      for (int i = c; i < 24; i += LPB) {
        const int r = i / 3, h = i - 3 * r;
        zero[i] = (r < bh && h < 2) ? gather4(pprev, a, y0 + r, x0 + 4 * h, bw - 4 * h) : 0u;
      }
    for (int i = c; i < S * WP; i += LPB) {
      const int r = i / WP, h = i - r * WP;
      win[i] = gather4(pprev, a, y0 + py - R + r, x0 + px - R + 4 * h, S - 4 * h);
    }
  }
  __syncthreads();
  const int side = 2 * R + 1, ncand = 1 + side * side;
  unsigned key = 0xFFFFFFFFu;
  if (live && c < ncand) {
    int vy = 0, vx = 0, oy = R, ox = R;          // candidate 0: the zero vector -- at the top level the window's centre
    const unsigned* src = win;
    int P = WP;
    if (c > 0) {
      const int i = c - 1, dy = i / side - R, dx = i - (i / side) * side - R;
      vy = py + dy; vx = px + dx; oy = dy + R; ox = dx + R;
    } else if (!TOP) {
      src = zero; P = 3; oy = 0; ox = 0;
    }
    if (y0 + vy >= 0 && y0 + bh + vy <= a.H && x0 + vx >= 0 && x0 + bw + vx <= a.W) {      // admissible: everything it reads is image
      const unsigned mlo = keep_bytes(0xFFFFFFFFu, bw), mhi = bw > 4 ? keep_bytes(0xFFFFFFFFu, bw - 4) : 0u;
      const unsigned cost = block_sad(cur, src, P, oy, ox, bh, mlo, mhi) + (unsigned)a.penalty * (unsigned)(abs(vy) + abs(vx));
      key = (cost << 8) | (unsigned)c;
    }
  }
#pragma unroll
  for (int o = (LPB < 64 ? LPB : 64) / 2; o >= 1; o >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, o));
  if ((tid & ((LPB < 64 ? LPB : 64) - 1)) == 0) atomicMin(&skey[lb], key);
  __syncthreads();
  if (live && c == 0) {
    const int w = (int)(skey[lb] & 255u);        // candidate 0 is always admissible: a key exists
    int vy = 0, vx = 0;
    if (w > 0) {
      const int i = w - 1;
      vy = py + i / side - R;
      vx = px + (i - (i / side) * side) - R;
    }
    mvo[2 * b] = (int16_t)vy;
    mvo[2 * b + 1] = (int16_t)vx;
  }
}

PyrArgs pyr_args(const MotionLayout& l) {
  PyrArgs a{};
  a.levels = l.levels;
  for (int k = 0; k < l.levels; ++k) {
    a.H[k] = l.lv[k].H; a.W[k] = l.lv[k].W; a.pitch[k] = l.lv[k].pitch; a.off[k] = (unsigned)l.lv[k].pyr_off;
  }
  return a;
}

}  // namespace

bool motion_layout(int Ho, int Wo, int levels, MotionLayout& l) {
  if (levels < 1 || levels > WCT_MOTION_MAX_LEVELS || Ho < (1 << (levels - 1)) || Wo < (1 << (levels - 1))) return false;
  l = MotionLayout{};
  l.levels = levels;
  size_t pyr = 0, mv = 0;
  int H = Ho, W = Wo;
  for (int k = 0; k < levels; ++k, H >>= 1, W >>= 1) {
    MotionLevel& v = l.lv[k];
    v.H = H; v.W = W; v.pitch = (W + 3) & ~3;
    v.nby = (H + WCT_MOTION_BLOCK - 1) / WCT_MOTION_BLOCK; v.nbx = (W + WCT_MOTION_BLOCK - 1) / WCT_MOTION_BLOCK;
    v.pyr_off = pyr; v.mv_off = mv;
    pyr += (size_t)H * v.pitch;
    mv += (size_t)v.nby * v.nbx * 2;
  }
  if (pyr > 0xFFFFFFFFu) return false;
  l.pyr_bytes = (pyr + 255) & ~(size_t)255;
  l.mv_count = mv;
  return true;
}

hipError_t launch_motion_pyramid(const float* img, int Hc, int Wc, const MotionLayout& l, uint8_t* pyr, hipStream_t s) {
  if (l.levels < 1 || l.levels > WCT_MOTION_MAX_LEVELS || l.lv[0].H > Hc || l.lv[0].W > Wc || (reinterpret_cast<size_t>(pyr) & 3)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((l.lv[0].W + PY_W - 1) / PY_W), (unsigned)((l.lv[0].H + PY_H - 1) / PY_H));
  hipLaunchKernelGGL(motion_pyramid_kernel, grid, dim3(256), 0, s, img, Hc, Wc, pyr_args(l), pyr);
  return hipGetLastError();
}

hipError_t launch_motion_unpad(const uint8_t* pyr, const MotionLayout& l, uint8_t* out, hipStream_t s) {
  const size_t n = (size_t)l.lv[0].H * l.lv[0].W;
  hipLaunchKernelGGL(motion_unpad_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, s, pyr, pyr_args(l), out);
  return hipGetLastError();
}

hipError_t launch_motion_search(const uint8_t* pyr_cur, const uint8_t* pyr_prev, const MotionLayout& l, int level, int range, int penalty,
                                const int16_t* mv_parent, int16_t* mv_out, const int* cut_flag, hipStream_t s) {
  if (level < 0 || level >= l.levels || range < 0 || range > WCT_MOTION_MAX_RANGE || penalty < 0 || penalty > 255) return hipErrorInvalidValue;
  const bool top = level == l.levels - 1;
  if (!top && !mv_parent) return hipErrorInvalidValue;
  const MotionLevel& v = l.lv[level];
  SearchArgs a{v.H, v.W, v.pitch, (unsigned)v.pyr_off, v.nby, v.nbx, top ? 0 : l.lv[level + 1].nby, top ? 0 : l.lv[level + 1].nbx, range, penalty};
  const long nb = (long)v.nby * v.nbx;
  if (top)
    hipLaunchKernelGGL(motion_search_kernel<true>, dim3((unsigned)nb), dim3(256), 0, s, pyr_cur, pyr_prev, a, mv_parent, mv_out, cut_flag);
  else
    hipLaunchKernelGGL(motion_search_kernel<false>, dim3((unsigned)((nb + SR_FINE_BPW - 1) / SR_FINE_BPW)), dim3(256), 0, s, pyr_cur, pyr_prev, a, mv_parent,
                       mv_out, cut_flag);
  return hipGetLastError();
}
