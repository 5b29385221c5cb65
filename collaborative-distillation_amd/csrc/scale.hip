// Scale control (include/wct_hip_scale.h): the float resampler R and the pyramid merge M between two levels of the cascade, on planar
// 3 x h x w fp32.  ONE kernel, two instantiations: R alone, and M = R(a - g b) + g c with the difference formed while the source is
// staged and the fine map added in the epilogue, so that M reads each of its three inputs once and writes its result once.
//
// Behind the weights' launch, one workgroup of 256 threads makes one tile of tw x th output samples of one colour plane (blockIdx.z):
//
//   weights   a launch of its own in front (scale_weights_kernel): one thread per output column / row of the IMAGE evaluates that
//             sample's taps in fp64 (centre, bounds, filter, the sum, the division -- the rule of the header, no fixed-point step) and
//             leaves them rounded ONCE to fp32 in a table, <= k = 2 ceil(support) + 1 taps per sample; a tile copies its rows of the
//             two tables into LDS.  (Evaluated per tile instead, the 2 x 17 fp64 filter values and divisions of a 4:1 reduction's
//             sample cost a tile more than its sums: the tiles of one tile column share their column weights 135 x 3 times in a 4K
//             frame.)  The table is the caller's scratch, rewritten by every launch: nothing is cached, evicted or uploaded, hence
//             nothing that could synchronise or move under a captured graph.
//   stage     the source window of the tile -- rows [r0, r1) x columns [c0, c1), the union of its taps -- goes through LDS `sr` rows
//             at a time: 16-byte loads where a row piece is 16-byte aligned (every piece of the cascade's own buffers is), single
//             floats at the window's ragged ends and for a 4-byte-only alignment.  A chunk is at most SC_BATCH pieces per thread, all
//             loaded into registers before the first goes to LDS, and the loads are issued EARLY: the first chunk's (and the merge's
//             fine samples) in front of the copy of the weights, every later chunk's in front of the h-pass of the chunk before.  A
//             tile's lifetime is load latency, so what a CU has in flight is (resident workgroups) x (a tile's window): the template
//             parameter NB keeps the staging registers to what the window needs and SC_STAGE_FLOATS keeps the chunk small, both for
//             occupancy (the one lever that moved the measured rate).  M stores fma(-g, b, a).
//   h-pass    T[r][x] = SUM_t wh[x][t] * S[r][xs[x] - c0 + t]: one thread per (four staged rows, output column), fp32 fma from 0 in
//             ascending tap order.  S is skewed by one float per 64 (skew()) so that the lanes of a reduction, which read a multiple of
//             two floats apart, do not meet on a bank.  T (the horizontally resampled window, rwin x tw) stays in LDS between the passes.
//   v-pass    out[y][x .. x + 3] = SUM_t wv[y][t] * T[ys[y] - r0 + t][x .. x + 3]: one thread per four adjacent outputs, a 16-byte LDS
//             read per tap, four fp32 fma chains from 0 in ascending tap order; M adds fma(g, c, .); 16-byte stores where aligned.
//
// Every output sample is one thread's two fma chains in tap order: the value is a function of the four sizes, the filter and the
// inputs alone -- the tile shape (chosen below from the sizes to fit LDS) changes which thread computes a sample, never how.  No atomics.
//
// Bounds.  Global reads stay inside [r0, r1) x [c0, c1), which the tap bounds clip to the image; the widest window any tile can have
// follows from the sizes ((tile - 1) * scale + 2 * support + 1 samples, see window_bound) and sizes the LDS arrays on the host, and a
// tile whose window would not fit -- none can -- returns before it touches LDS.
#include "wct_common.h"
#include <cmath>

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_TILE_W = 64, SC_TILE_H = 16;   // the tile of every axis that shrinks by at most SC_NARROW_FS; tests/test_scale_gpu.py names them
constexpr int SC_TILE_W_NARROW = 32;            // columns per tile when the width shrinks by more
constexpr double SC_NARROW_FS = 8.0;
constexpr int SC_WIN_ROWS = 168;                // rows of T at most: the tile height halves until its window fits
constexpr int SC_STAGE_FLOATS = 4096;           // floats staged at once at most: LDS is occupancy, and occupancy is bytes in flight
constexpr int SC_BATCH = 8;                     // 16-byte loads a thread has in flight while it stages (the merge, with two sources: half as many pairs)
constexpr int SC_LDS_BYTES = 65536;

struct ScaleArgs {
  const float *a, *b, *c;   // b, c: the merge's coarse and fine maps (MERGE only)
  float* out;
  float *wx, *wy;           // the launch's weight tables, in the caller's scratch (scale_table_bytes)
  int2 *xt, *yt;
  int H, W, oH, oW, filter;
  float gain;
  double sx, fsx, supx, sy, fsy, supy;   // per axis: in / out, max(scale, 1), S * fs
  int tw, tw_shift, th, kh, kv, swin, sstr, rwin, sr;   // sstr: floats between two staged rows (skewed, see skew())
};

// taps [lo, hi) of output sample i: the window of the header, clipped to the axis
__device__ __forceinline__ void tap_bounds(int i, double scale, double support, int in, int& lo, int& hi) {
#pragma clang fp contract(off)
  const double centre = (i + 0.5) * scale;
  int a = (int)(centre - support + 0.5), b = (int)(centre + support + 0.5);
  lo = a < 0 ? 0 : a;
  hi = b > in ? in : b;
}

__device__ __forceinline__ double filter_at(double x, int filter) {
#pragma clang fp contract(off)
  if (x < 0.0) x = -x;
  if (filter == RESIZE_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
  constexpr double a = -0.5;   // Keys
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
  if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
  return 0.0;
}

// the n weights of output sample i: fp64 throughout, each divided by the fp64 sum of all of them (ascending), rounded once
__device__ void tap_weights(int i, double scale, double fs, int lo, int n, int filter, float* w) {
#pragma clang fp contract(off)
  const double centre = (i + 0.5) * scale;
  double ww = 0.0;
  for (int t = 0; t < n; ++t) ww += filter_at((lo + t - centre + 0.5) / fs, filter);
  for (int t = 0; t < n; ++t) {
    const double v = filter_at((lo + t - centre + 0.5) / fs, filter);
    w[t] = (float)(ww != 0.0 ? v / ww : v);
  }
}

__device__ __forceinline__ bool is_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the weight tables of one launch: row i of wx (kh floats) / wy (kv floats) holds the taps of output column / row i, xt / yt its
// (first tap, tap count).  One thread per output index.
__global__ __launch_bounds__(SC_THREADS) void scale_weights_kernel(ScaleArgs p) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i >= p.oW + p.oH) return;
  const bool col = i < p.oW;
  const int j = col ? i : i - p.oW;
  const int K = col ? p.kh : p.kv;
  int lo, hi;
  tap_bounds(j, col ? p.sx : p.sy, col ? p.supx : p.supy, col ? p.W : p.H, lo, hi);
  const int n = hi - lo < K ? hi - lo : K;   // hi - lo <= 2 ceil(support) + 1 = K
  tap_weights(j, col ? p.sx : p.sy, col ? p.fsx : p.fsy, lo, n, p.filter, (col ? p.wx : p.wy) + (size_t)j * K);
  (col ? p.xt : p.yt)[j] = make_int2(lo, n);
}

// sample e of a staged row lives at e + e / 64: lanes that read 64 floats apart (adjacent outputs of a 2:1, 4:1, 8:1 .. reduction read 2, 4,
// 8 .. floats apart, so lanes 32, 16, 8 .. apart meet on one bank) are moved to neighbouring banks
__device__ __forceinline__ int skew(int e) { return e + (e >> 6); }

// NB: 16-byte pieces a thread stages per chunk (launch_scale picks the smallest that covers the chunk: registers are occupancy)
template <bool MERGE, int NB>
__global__ __launch_bounds__(SC_THREADS) void scale_resample_kernel(ScaleArgs p) {
  extern __shared__ __align__(16) float sc_lds[];
  float* T = sc_lds;                    // [rwin][tw]; rows are 16-byte aligned (tw is a multiple of 4)
  float* S = T + p.rwin * p.tw;         // [sr][sstr], skewed
  float* wh = S + p.sr * p.sstr;        // [tw][kh]
  float* wv = wh + p.tw * p.kh;         // [th][kv]
  int* xs = reinterpret_cast<int*>(wv + p.th * p.kv);   // first tap and tap count of every column / row of the tile
  int* xn = xs + p.tw;
  int* ys = xn + p.tw;
  int* yn = ys + p.th;

  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * p.tw, y0 = blockIdx.y * p.th;
  const int nx = p.oW - x0 < p.tw ? p.oW - x0 : p.tw, ny = p.oH - y0 < p.th ? p.oH - y0 : p.th;
  const size_t iplane = (size_t)p.H * p.W, oplane = (size_t)p.oH * p.oW;
  const float* A = p.a + blockIdx.z * iplane;
  const float* B = MERGE ? p.b + blockIdx.z * iplane : nullptr;
  const float* Cf = MERGE ? p.c + blockIdx.z * oplane : nullptr;
  float* O = p.out + blockIdx.z * oplane;

  // the tile's source window: tap bounds are monotone in the output index, so the first and the last sample span it
  int c0, c1, r0, r1, unused;
  tap_bounds(x0, p.sx, p.supx, p.W, c0, unused);
  tap_bounds(x0 + nx - 1, p.sx, p.supx, p.W, unused, c1);
  tap_bounds(y0, p.sy, p.supy, p.H, r0, unused);
  tap_bounds(y0 + ny - 1, p.sy, p.supy, p.H, unused, r1);
  const int cw = c1 - c0, rh = r1 - r0;
  const int slots = (cw + 3) / 4 + 1;   // 4-float pieces per staged row, the partial ones at both ends included
  if (cw > p.swin || rh > p.rwin || p.sr * slots > SC_THREADS * NB) return;   // uniform; launch_scale's bounds cover every tile

  // a chunk of <= sr window rows from global memory into registers (load) and from there into S (store): apart, so that the loads are
  // in flight under whatever stands between the two -- the weights for the first chunk, the previous chunk's h-pass for the others
  float4 va[NB], vb[NB];
  int prow[NB], pcol[NB];   // the piece's row in the chunk (-1: none) and its first column in the window (-3 .. cw - 1)
  auto load = [&](int rc) {
    const int nr = rh - rc < p.sr ? rh - rc : p.sr;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      const int it = k * SC_THREADS + tid;
      prow[k] = -1;
      if (it < nr * slots) {
        const int r = it / slots, sl = it - r * slots;
        const size_t row = (size_t)(r0 + rc + r) * p.W + c0;
        const float* ra = A + row;
        const float* rb = MERGE ? B + row : nullptr;
        const int lead = (int)((4 - ((reinterpret_cast<uintptr_t>(ra) >> 2) & 3)) & 3);   // floats in front of the row's first 16-byte boundary
        const int g = (lead ? lead - 4 : 0) + 4 * sl;
        prow[k] = r; pcol[k] = g;
        if (g >= 0 && g + 3 < cw && (!MERGE || is_aligned16(rb + g))) {
          va[k] = *reinterpret_cast<const float4*>(ra + g);
          if (MERGE) vb[k] = *reinterpret_cast<const float4*>(rb + g);
        } else {   // the window's ragged ends, and rows of a 4-byte-only alignment
          float t[4], u[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bool in = g + j >= 0 && g + j < cw;
            t[j] = in ? ra[g + j] : 0.f;
            u[j] = MERGE && in ? rb[g + j] : 0.f;
          }
          va[k] = make_float4(t[0], t[1], t[2], t[3]);
          vb[k] = make_float4(u[0], u[1], u[2], u[3]);
        }
      }
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int k = 0; k < NB; ++k)
      if (prow[k] >= 0) {
        float q[4] = {va[k].x, va[k].y, va[k].z, va[k].w};
        if (MERGE) {
          q[0] = fmaf(-p.gain, vb[k].x, q[0]); q[1] = fmaf(-p.gain, vb[k].y, q[1]); q[2] = fmaf(-p.gain, vb[k].z, q[2]); q[3] = fmaf(-p.gain, vb[k].w, q[3]);
        }
        float* s = S + prow[k] * p.sstr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int e = pcol[k] + j;
          if (e >= 0 && e < cw) s[skew(e)] = q[j];
        }
      }
  };

  load(0);
  // this thread's four adjacent outputs (the tile has at most 256 such groups), and the merge's fine samples for them: read now, used last
  const int gshift = p.tw_shift - 2, gpr = p.tw >> 2;
  const int ty = tid >> gshift, og = tid & (gpr - 1), ox = x0 + 4 * og;
  const bool active = ty < ny && ox < p.oW;
  const size_t o = (size_t)(y0 + ty) * p.oW + ox;
  const int valid = p.oW - ox < 4 ? p.oW - ox : 4;
  float f[4] = {0.f, 0.f, 0.f, 0.f};
  if (MERGE && active) {
    if (valid == 4 && is_aligned16(Cf + o)) {
      const float4 v = *reinterpret_cast<const float4*>(Cf + o);
      f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
    } else {
      for (int k = 0; k < valid; ++k) f[k] = Cf[o + k];
    }
  }

  // the tile's rows of the two weight tables (scale_weights_kernel), whole rows of k floats: taps past a sample's count are never read
  for (int i = tid; i < nx * p.kh; i += SC_THREADS) wh[i] = p.wx[(size_t)x0 * p.kh + i];
  for (int i = tid; i < ny * p.kv; i += SC_THREADS) wv[i] = p.wy[(size_t)y0 * p.kv + i];
  for (int i = tid; i < nx + ny; i += SC_THREADS) {
    const bool col = i < nx;
    const int j = col ? i : i - nx;
    const int2 t = col ? p.xt[x0 + j] : p.yt[y0 + j];
    (col ? xs : ys)[j] = t.x;
    (col ? xn : yn)[j] = t.y;
  }

  for (int rc = 0; rc < rh; rc += p.sr) {
    const int nr = rh - rc < p.sr ? rh - rc : p.sr;
    store();
    __syncthreads();   // S holds rows rc .. rc + nr (and, the first time, the weights are there)
    if (rc + p.sr < rh) load(rc + p.sr);
    // h-pass: four rows of one output column per thread, so that a weight is read once for four products
    for (int it = tid; it < ((nr + 3) >> 2) << p.tw_shift; it += SC_THREADS) {
      const int r = (it >> p.tw_shift) << 2, tx = it & (p.tw - 1);
      if (tx < nx) {
        const int e0 = xs[tx] - c0, n = xn[tx];
        const float* w = wh + tx * p.kh;
        int ro[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) ro[j] = (r + j < nr ? r + j : nr - 1) * p.sstr;   // a row past the chunk repeats its last one and is not kept
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < n; ++t) {
          const int e = skew(e0 + t);
          const float wt = w[t];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] = fmaf(wt, S[ro[j] + e], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (r + j < nr) T[((rc + r + j) << p.tw_shift) + tx] = acc[j];
      }
    }
    __syncthreads();   // S is free for the next rows; after the last chunk T is complete
  }

  if (!active) return;
  const float* w = wv + ty * p.kv;
  const float4* t4 = reinterpret_cast<const float4*>(T + ((ys[ty] - r0) << p.tw_shift)) + og;
  const int n = yn[ty];
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);   // columns of a ragged tile past the image's edge carry whatever T held there and are not stored
  for (int t = 0; t < n; ++t) {
    const float4 v = t4[t * gpr];
    const float wt = w[t];
    acc.x = fmaf(wt, v.x, acc.x); acc.y = fmaf(wt, v.y, acc.y); acc.z = fmaf(wt, v.z, acc.z); acc.w = fmaf(wt, v.w, acc.w);
  }
  float q[4] = {acc.x, acc.y, acc.z, acc.w};
  if (MERGE) {
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = fmaf(p.gain, f[k], q[k]);
  }
  if (valid == 4 && is_aligned16(O + o)) {
    *reinterpret_cast<float4*>(O + o) = make_float4(q[0], q[1], q[2], q[3]);
  } else {
    for (int k = 0; k < valid; ++k) O[o + k] = q[k];
  }
}

// samples of the source axis that `tile` adjacent outputs can touch at most: the first one's window starts no earlier than
// centre_0 - support - 0.5, the last one's ends no later than centre_0 + (tile - 1) scale + support + 0.5
int window_bound(int tile, double scale, double support) { return (int)std::ceil((tile - 1) * scale + 2.0 * support) + 2; }

}  // namespace

int scale_tile_w() { return SC_TILE_W; }
int scale_tile_h() { return SC_TILE_H; }

namespace {
int axis_taps(int in, int out, int filter) {   // k = 2 ceil(support) + 1: no sample has more taps
  const double scale = (double)in / (double)out;
  return (int)std::ceil((filter == RESIZE_BICUBIC ? 2.0 : 1.0) * (scale > 1.0 ? scale : 1.0)) * 2 + 1;
}
}  // namespace

// [xt oW int2 | yt oH int2 | wx oW * kh floats | wy oH * kv floats]
size_t scale_table_bytes(int H, int W, int oH, int oW, int filter) {
  return ((size_t)oW + oH) * sizeof(int2) + ((size_t)oW * axis_taps(W, oW, filter) + (size_t)oH * axis_taps(H, oH, filter)) * sizeof(float);
}

hipError_t launch_scale(const float* a, const float* b, const float* c, float gain, int H, int W, float* out, int oH, int oW, int filter, void* tab,
                        size_t tab_bytes, hipStream_t s) {
  // arguments are checked where they can be answered with a message (api_image.hip); this one guards what the kernel's bounds rest on
  if (!a || !out || H < 1 || W < 1 || oH < 1 || oW < 1 || (filter != RESIZE_BILINEAR && filter != RESIZE_BICUBIC) || (b == nullptr) != (c == nullptr) ||
      !tab || tab_bytes < scale_table_bytes(H, W, oH, oW, filter))
    return hipErrorInvalidValue;
  ScaleArgs p{};
  p.a = a; p.b = b; p.c = c; p.out = out;
  p.H = H; p.W = W; p.oH = oH; p.oW = oW; p.filter = filter; p.gain = gain;
  const double S = filter == RESIZE_BICUBIC ? 2.0 : 1.0;
  p.sx = (double)W / (double)oW; p.fsx = p.sx > 1.0 ? p.sx : 1.0; p.supx = S * p.fsx;
  p.sy = (double)H / (double)oH; p.fsy = p.sy > 1.0 ? p.sy : 1.0; p.supy = S * p.fsy;
  p.kh = axis_taps(W, oW, filter);
  p.kv = axis_taps(H, oH, filter);
  p.xt = reinterpret_cast<int2*>(tab);
  p.yt = p.xt + oW;
  p.wx = reinterpret_cast<float*>(p.yt + oH);
  p.wy = p.wx + (size_t)oW * p.kh;
  p.tw = p.fsx > SC_NARROW_FS ? SC_TILE_W_NARROW : SC_TILE_W;
  p.tw_shift = p.tw == 64 ? 6 : 5;
  p.th = SC_TILE_H;
  while (p.th > 1 && window_bound(p.th, p.sy, p.supy) > SC_WIN_ROWS) p.th >>= 1;
  p.swin = window_bound(p.tw, p.sx, p.supx);
  p.rwin = window_bound(p.th, p.sy, p.supy);
  const long fixed = (long)p.rwin * p.tw + (long)p.tw * p.kh + (long)p.th * p.kv + 2L * (p.tw + p.th);   // 4-byte words besides the stage
  p.sstr = p.swin + (p.swin >> 6) + 1;
  long room = SC_LDS_BYTES / 4 - fixed;
  if (room > SC_STAGE_FLOATS) room = SC_STAGE_FLOATS;
  p.sr = (int)(room / p.sstr);
  if (p.sr > p.rwin) p.sr = p.rwin;
  const int pieces = SC_THREADS * (b ? SC_BATCH / 2 : SC_BATCH), slots = (p.swin + 3) / 4 + 1;   // a chunk is one round of the staging threads
  if (p.sr > pieces / slots) p.sr = pieces / slots;
  if (p.sr < 1) return hipErrorInvalidValue;   // an axis shrinking by more than WCT_SCALE_MAX_SHRINK: refused by the entries
  const size_t lds = ((size_t)fixed + (size_t)p.sr * p.sstr) * 4;
  const dim3 grid((unsigned)((oW + p.tw - 1) / p.tw), (unsigned)((oH + p.th - 1) / p.th), 3);
  if (grid.y > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(scale_weights_kernel, dim3((unsigned)((oW + oH + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, s, p);
  const int need = (p.sr * slots + SC_THREADS - 1) / SC_THREADS;   // <= SC_BATCH (SC_BATCH / 2 for the merge) by the choice of sr
#define SCALE_LAUNCH(M, N) hipLaunchKernelGGL((scale_resample_kernel<M, N>), grid, dim3(SC_THREADS), lds, s, p)
  if (b) {
    if (need <= 1) SCALE_LAUNCH(true, 1); else if (need <= 2) SCALE_LAUNCH(true, 2); else SCALE_LAUNCH(true, SC_BATCH / 2);
  } else {
    if (need <= 1) SCALE_LAUNCH(false, 1); else if (need <= 2) SCALE_LAUNCH(false, 2); else if (need <= 4) SCALE_LAUNCH(false, 4); else SCALE_LAUNCH(false, SC_BATCH);
  }
#undef SCALE_LAUNCH
  return hipGetLastError();
}
