// Spatial control: per-region whitening / colouring (wct_stylize_regions).  A uint8 label map gives every content pixel a region
// 0 .. K-1 (its own style) or 255 (unstyled).  Per region the transform is the reference's whiten_and_color
// (PytorchWCT/util_wct.py:62-131) on that region's feature columns only; every other operator of the cascade is local and unchanged.
// Three kernels, all new (the single-style path does not go through here):
//   labels_levels_kernel    the level label maps lab_L[i][j] = labels[i s + s/2][j s + s/2] (s = 2^(L-1)) of every level a cascade
//                           visits, and per-(level, label) pixel counts (+ the whole map's histogram: the call's argument check)
//   moments_labeled_kernel  per-label raw fp64 moments (n_k, sum_k, sumsq_k) of an NHWC map: the arithmetic of moments.hip
//   apply_labeled_kernel    out_p = M_lab(p) x_p + b_lab(p), labels >= K (255) copied through: one read and one write of the map
#include "wct_common.h"
#include <algorithm>

namespace {

// ---- level label maps -------------------------------------------------------------------------------------------------------
// One thread per output element of the concatenation [whole map (histogram only) | lab_5 | lab_4 | ... | lab_1]; bins are per
// workgroup in LDS (integers: any order is exact), then one atomic per non-empty bin.
struct LabLevels {
  const uint8_t* labels;
  int H, W;
  uint8_t* out[6];       // [level] (unused entries null)
  long begin[7];         // element ranges: [begin[s], begin[s + 1]) is segment s (0 = whole map, 1..5 = level 6 - s)
  int h[6], w[6], s[6];  // per segment
  unsigned* hist;        // [6][256]: segment 0 = whole map, segment L = level L
};

__global__ __launch_bounds__(256) void labels_levels_kernel(LabLevels a) {
  __shared__ unsigned bins[6][256];
  for (int e = threadIdx.x; e < 6 * 256; e += 256) (&bins[0][0])[e] = 0u;
  __syncthreads();
  const long total = a.begin[6];
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    int seg = 0;
    while (e >= a.begin[seg + 1]) ++seg;
    const long q = e - a.begin[seg];
    if (seg == 0) {
      atomicAdd(&bins[0][a.labels[q]], 1u);
    } else {
      const int level = 6 - seg, w = a.w[seg], s = a.s[seg];
      const long i = q / w, j = q - i * w;
      const uint8_t v = a.labels[(i * s + s / 2) * (long)a.W + j * s + s / 2];
      a.out[level][q] = v;
      atomicAdd(&bins[level][v], 1u);
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 6 * 256; e += 256) {
    const unsigned v = (&bins[0][0])[e];
    if (v) atomicAdd(a.hist + e, v);
  }
}

// ---- per-label moments --------------------------------------------------------------------------------------------------------
// grid = (pixel chunks, pair groups, K labels).  A workgroup (4 waves) walks its chunk in LDS tiles of MP pixels (64 for C <= 128,
// 32 for C <= 256, 16 above: 33 KB of LDS), pixels of other labels written as zeros (a 0/1 mask on an operand is exact), tiles
// without a pixel of its label skipped before their features are loaded -- a spatially coherent label map is read about once over
// all K labels.  Wave w owns the 16 x 16 tile pairs pg * 4 PW + w + 4 j of the upper triangle for the whole chunk (accumulators in
// registers, no cross-wave reduction).  Arithmetic as moments.hip: F32 = fp32 products on v_mfma_f32_16x16x4_f32 summed over a tile
// (<= 64 pixels) in fp32, tile totals in fp64; F32 = false: fp64 products on v_mfma_f64_16x16x4_f64.  Partials per (label, chunk),
// then a fixed-order reduction: bitwise reproducible.
struct MomLabArgs {
  const float* x;
  const uint8_t* lab;
  int C, T, NP, Cs, MP, PW, NPC;
  long npix, chunk;
  double* part;          // [K][NPC][NP * 256 + T * 16 + 1]
};

__device__ __forceinline__ int row_of(bool f32, int pk, int r) { return f32 ? 4 * pk + r : pk + 4 * r; }

template <int PW, bool F32>
__global__ __launch_bounds__(256, 2) void moments_labeled_kernel(MomLabArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* lds = reinterpret_cast<float*>(smem);                      // [MP][Cs]
  int* labok = reinterpret_cast<int*>(lds + (size_t)a.MP * a.Cs);   // [MP]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, pk = lane >> 4;
  const int pc = blockIdx.x, pg = blockIdx.y, k = blockIdx.z;
  const int MP = a.MP, Cs = a.Cs, c4n = a.C >> 2;
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
  unsigned npx = 0;
  const long p0 = (long)pc * a.chunk, p1 = min(a.npix, p0 + a.chunk);
  for (long pt = p0; pt < p1; pt += MP) {
    __syncthreads();                                        // previous tile consumed
    int mine = 0;
    if (tid < MP) {
      const long p = pt + tid;
      mine = p < p1 && a.lab[p] == k;
      labok[tid] = mine;
      npx += mine;
    }
    if (!__syncthreads_or(mine)) continue;                  // no pixel of this label in the tile: nothing loaded
    for (int e = tid; e < MP * c4n; e += 256) {
      const int px = e / c4n, q = e - px * c4n;
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (labok[px]) v = *reinterpret_cast<const f32x4*>(a.x + (pt + px) * a.C + 4 * q);
      *reinterpret_cast<f32x4*>(lds + px * Cs + 4 * q) = v;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PW; ++j) {
      if (j < cnt) {
        if constexpr (F32) {
          f32x4 f = f32x4{0.f, 0.f, 0.f, 0.f};
          float t = 0.f;
          for (int st = 0; st < MP; st += 4) {
            const float* row = lds + (st + pk) * Cs;
            const float av = row[offA[j]], bv = row[offB[j]];
            t += av;
            f = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, f, 0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[j][r] += (double)f[r];
          s[j] += (double)t;
        } else {
          for (int st = 0; st < MP; st += 4) {
            const float* row = lds + (st + pk) * Cs;
            const double av = (double)row[offA[j]], bv = (double)row[offB[j]];
            s[j] += av;
            acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[j], 0, 0, 0);
          }
        }
      }
    }
  }
  const long stride = (long)a.NP * 256 + a.T * 16 + 1;
  double* dst = a.part + ((size_t)k * a.NPC + pc) * stride;
#pragma unroll
  for (int j = 0; j < PW; ++j) {
    if (j < cnt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[(size_t)pidx[j] * 256 + row_of(F32, pk, r) * 16 + c] = acc[j][r];
      if (diag[j]) {                                        // the diagonal tile's owner also owns the sums of its 16 channels
        double v = s[j];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (pk == 0) dst[(size_t)a.NP * 256 + offA[j]] = v;
      }
    }
  }
  if (pg == 0) {                                            // pixel count: one wave's lanes saw every tile pixel once
    __shared__ unsigned cnt_sh;
    if (tid == 0) cnt_sh = 0u;
    __syncthreads();
    if (npx) atomicAdd(&cnt_sh, npx);
    __syncthreads();
    if (tid == 0) dst[stride - 1] = (double)cnt_sh;
  }
}

// partials -> n[K], sum[K][C], sumsq[K][C][C] in a fixed order (16 slices of the chunk index, then the slices in order)
__global__ __launch_bounds__(256) void moments_labeled_reduce_kernel(MomLabArgs a, double* n, double* sum, double* sumsq) {
  __shared__ double red[16][17];
  const int el = threadIdx.x & 15, sl = threadIdx.x >> 4, k = blockIdx.y;
  const long e = (long)blockIdx.x * 16 + el;
  const long nsq = (long)a.NP * 256, stride = nsq + a.T * 16 + 1;
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
    const int ra = I * 16 + r, cb = J * 16 + cc;
    if (ra < a.C && cb < a.C) {
      sumsq[k * C * C + (size_t)ra * C + cb] = v;
      if (I != J) sumsq[k * C * C + (size_t)cb * C + ra] = v;
    }
  } else if (e < stride - 1) {
    const int ch = (int)(e - nsq);
    if (ch < a.C) sum[k * C + ch] = v;
  } else {
    n[k] = v;
  }
}

MomLabArgs plan_labeled(int C, long npix, int K) {
  MomLabArgs a{};
  a.C = C; a.T = (C + 15) / 16; a.NP = a.T * (a.T + 1) / 2;
  a.Cs = (a.T & 1) ? a.T * 16 : a.T * 16 + 16;              // == 16 (mod 32) dwords: conflict-free operand reads
  a.MP = C <= 128 ? 64 : C <= 256 ? 32 : 16;
  a.PW = a.NP <= 8 ? 2 : 8;
  const int npg = (a.NP + 4 * a.PW - 1) / (4 * a.PW);
  a.npix = npix;
  long npc = std::max(1L, 1024L / npg);                     // ~1024 workgroups per label
  const long maxc = (npix + a.MP - 1) / a.MP;
  if (npc > maxc) npc = maxc;
  long chunk = (npix + npc - 1) / npc;
  a.chunk = (chunk + a.MP - 1) / a.MP * a.MP;
  a.NPC = (int)((npix + a.chunk - 1) / a.chunk);
  (void)K;
  return a;
}

// ---- labeled apply ----------------------------------------------------------------------------------------------------------------
// A workgroup owns PT pixels (64 for C <= 128, 32 / 16 above) staged in LDS [PT][Cs]; the (16 output channels x 16 pixels) items of
// the tile are dealt to the four waves.  Per label present in the tile (found with a 64-bit ballot; an interior tile has one):
// v_mfma_f32_16x16x4_f32 with A = M_L rows (fp32, from the fp64 map), B = the pixels, fp32 accumulation; only pixels of that label
// are written.  Channel c of a 16-channel group k0 is read in the order k0 + 4 (lane >> 4) + step by both operands (float4 loads).
struct ApplyLabArgs {
  const float* x;
  const uint8_t* lab;
  const float* Mf;       // [K][Cp][Cp] fp32, zero padded
  const float* bf;       // [K][Cp]
  float* out;
  int C, Cp, Cs, PT, K;
  long npix;
};

__global__ __launch_bounds__(256) void apply_labeled_kernel(ApplyLabArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xs = reinterpret_cast<float*>(smem);                        // [PT][Cs]
  int* labs = reinterpret_cast<int*>(xs + (size_t)a.PT * a.Cs);      // [PT]
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
  if (tid < PT) {
    int l = 255;
    if (tid < npt) { l = a.lab[p0 + tid]; if (l >= a.K) l = 255; }
    labs[tid] = l;
  }
  __syncthreads();
  const int j = lane & 15, kq = lane >> 4;
  const int nO = Cp >> 4, nP = PT >> 4, nItems = nO * nP;
  const int mylab = lane < PT ? labs[lane] : 255;
  unsigned long long pending = __ballot(mylab != 255);
  while (pending) {                                                  // wave-uniform loop over the labels present
    const int first = __builtin_ctzll(pending);
    const int L = __shfl(mylab, first);
    pending &= ~__ballot(mylab == L);
    const float* M = a.Mf + (size_t)L * Cp * Cp;
    for (int it = wave; it < nItems; it += 4) {
      const int ot = it / nP, ptile = it - ot * nP;
      const int o0 = ot * 16, px = ptile * 16 + j;
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
      const float* arow = M + (size_t)(o0 + j) * Cp + 4 * kq;
      const float* brow = xs + px * Cs + 4 * kq;
      for (int k0 = 0; k0 < Cp; k0 += 16) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(arow + k0);
        const f32x4 bv = *reinterpret_cast<const f32x4*>(brow + k0);
#pragma unroll
        for (int st = 0; st < 4; ++st) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[st], bv[st], acc, 0, 0, 0);
      }
      // D layout: column = pixel (lane & 15), rows = output channels o0 + 4 (lane >> 4) + r
      const int oc = o0 + 4 * kq;
      if (labs[px] == L && oc < C) {
        const f32x4 bb = *reinterpret_cast<const f32x4*>(a.bf + (size_t)L * Cp + oc);
        *reinterpret_cast<f32x4*>(a.out + (p0 + px) * C + oc) = acc + bb;
      }
    }
  }
  // unstyled pixels (255, and labels >= K) are copied through
  for (int e = tid; e < npt * c4n; e += 256) {
    const int px = e / c4n, q = e - px * c4n;
    if (labs[px] == 255) *reinterpret_cast<f32x4*>(a.out + (p0 + px) * C + 4 * q) = *reinterpret_cast<const f32x4*>(xs + px * Cs + 4 * q);
  }
}

// fp64 (M, b) of K labels -> fp32, zero padded to Cp
__global__ void mb_to_f32_kernel(const double* M, const double* b, int K, int C, int Cp, float* Mf, float* bf) {
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

// M = I, b = 0 for the labels in `mask` (regions that are empty, a single pixel, or not solved)
__global__ void mb_identity_kernel(double* M, double* b, int C, unsigned mask) {
  const int k = blockIdx.y;
  if (!(mask >> k & 1u)) return;
  const long cc = (long)C * C;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < cc + C; e += (long)gridDim.x * blockDim.x) {
    if (e < cc) M[k * cc + e] = (e / C == e % C) ? 1.0 : 0.0;
    else b[(long)k * C + (e - cc)] = 0.0;
  }
}

}  // namespace

hipError_t launch_labels_levels(const uint8_t* labels, int H, int W, const int* h, const int* w, uint8_t* const* out, unsigned* hist,
                                hipStream_t s) {
  LabLevels a{};
  a.labels = labels; a.H = H; a.W = W; a.hist = hist;
  a.begin[0] = 0;
  a.begin[1] = (long)H * W;
  a.h[0] = H; a.w[0] = W; a.s[0] = 1;
  for (int seg = 1; seg <= 5; ++seg) {
    const int level = 6 - seg;
    a.out[level] = out[level];
    a.h[seg] = h[level]; a.w[seg] = w[level]; a.s[seg] = 1 << (level - 1);
    if ((long)(h[level] - 1) * a.s[seg] + a.s[seg] / 2 >= H || (long)(w[level] - 1) * a.s[seg] + a.s[seg] / 2 >= W) return hipErrorInvalidValue;
    a.begin[seg + 1] = a.begin[seg] + (long)h[level] * w[level];
  }
  hipError_t e = hipMemsetAsync(hist, 0, 6 * 256 * sizeof(unsigned), s);
  if (e != hipSuccess) return e;
  const long total = a.begin[6];
  const int grid = (int)std::min(2048L, (total + 255) / 256);
  hipLaunchKernelGGL(labels_levels_kernel, dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

size_t moments_labeled_workspace_bytes(int C, long npix, int K) {
  const MomLabArgs a = plan_labeled(C, npix, K);
  return (size_t)K * a.NPC * ((size_t)a.NP * 256 + a.T * 16 + 1) * sizeof(double);
}

hipError_t launch_moments_labeled(const float* feat, int C, long npix, const uint8_t* lab, int K, double* n, double* sum, double* sumsq,
                                  void* ws, size_t ws_bytes, hipStream_t s, bool f32_products) {
  if (C < 4 || (C & 3) || C > 512 || npix < 1 || K < 1 || K > 255) return hipErrorInvalidValue;
  if (ws_bytes < moments_labeled_workspace_bytes(C, npix, K)) return hipErrorOutOfMemory;
  MomLabArgs a = plan_labeled(C, npix, K);
  a.x = feat; a.lab = lab; a.part = reinterpret_cast<double*>(ws);
  const int npg = (a.NP + 4 * a.PW - 1) / (4 * a.PW);
  const size_t lds = (size_t)a.MP * a.Cs * sizeof(float) + a.MP * sizeof(int);
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
  if (a.PW == 2) e = f32_products ? go(moments_labeled_kernel<2, true>) : go(moments_labeled_kernel<2, false>);
  else e = f32_products ? go(moments_labeled_kernel<8, true>) : go(moments_labeled_kernel<8, false>);
  if (e != hipSuccess) return e;
  const long stride = (long)a.NP * 256 + a.T * 16 + 1;
  hipLaunchKernelGGL(moments_labeled_reduce_kernel, dim3((unsigned)((stride + 15) / 16), (unsigned)K), dim3(256), 0, s, a, n, sum, sumsq);
  return hipGetLastError();
}

size_t apply_labeled_workspace_bytes(int C, int K) {
  const size_t Cp = (size_t)(C + 15) / 16 * 16;
  return ((size_t)K * Cp * Cp + (size_t)K * Cp) * sizeof(float);
}

hipError_t launch_apply_labeled(const float* feat, int C, long npix, const uint8_t* lab, int K, const double* M, const double* b,
                                float* out, void* ws, size_t ws_bytes, hipStream_t s) {
  if (C < 4 || (C & 3) || C > 512 || npix < 1 || K < 1 || K > 255) return hipErrorInvalidValue;
  if (ws_bytes < apply_labeled_workspace_bytes(C, K)) return hipErrorOutOfMemory;
  ApplyLabArgs a{};
  a.C = C; a.Cp = (C + 15) / 16 * 16; a.Cs = a.Cp + 4; a.K = K; a.npix = npix;
  a.PT = C <= 128 ? 64 : C <= 256 ? 32 : 16;
  a.x = feat; a.lab = lab; a.out = out;
  float* Mf = reinterpret_cast<float*>(ws);
  float* bf = Mf + (size_t)K * a.Cp * a.Cp;
  a.Mf = Mf; a.bf = bf;
  const long nconv = (long)K * a.Cp * a.Cp + (long)K * a.Cp;
  hipLaunchKernelGGL(mb_to_f32_kernel, dim3((unsigned)std::min(1024L, (nconv + 255) / 256)), dim3(256), 0, s, M, b, K, C, a.Cp, Mf, bf);
  const size_t lds = (size_t)a.PT * a.Cs * sizeof(float) + a.PT * sizeof(int);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(apply_labeled_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(apply_labeled_kernel, dim3((unsigned)((npix + a.PT - 1) / a.PT)), dim3(256), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_mb_identity(double* M, double* b, int C, int K, unsigned mask, hipStream_t s) {
  if (!mask) return hipSuccess;
  hipLaunchKernelGGL(mb_identity_kernel, dim3((unsigned)std::min(256, ((C * C + C) + 255) / 256), (unsigned)K), dim3(256), 0, s, M, b, C, mask);
  return hipGetLastError();
}
