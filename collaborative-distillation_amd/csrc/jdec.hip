// The device JPEG decoder's kernels (include/wct_hip_jdec.h has the definition; api_jdec.hip the entries).  Integer arithmetic only;
// what crosses threads is an integer sum, an integer OR or a state compared for equality, so the result cannot depend on the launch.
// Every loop is bounded by a constant or by a launch argument, never by the bytes of the file.  Plain C++ and vector atomics only.
#include "wct_common.h"
#include "jdec_parse.h"

using namespace wct_jdec;

namespace {

typedef unsigned long long u64;

constexpr int S = WCT_JDEC_SUBSEQ_BITS;
constexpr int SYNC_T = WCT_JDEC_SYNC_THREADS;
constexpr int CHUNK = WCT_JDEC_CHUNK;
constexpr int DC_TILE = WCT_JDEC_DC_TILE;
constexpr int MAX_STEPS = 2 * S + 64;            // steps of one subsequence: every step but an anchor's moves p, and a symbol has at most 27 bits
constexpr unsigned FLAG_UNSYNC = 1u, FLAG_CORRUPT = 2u;
enum { META_BITS = 0, META_NSUB = 1, META_NA = 2, META_FLAGS = 3, META_WORDS = 8 };

__constant__ uint8_t d_zigzag_inv[64] = {   // natural index -> zig-zag position
    0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// exclusive prefix of one value per thread of a 256-thread workgroup; *total = the sum.  `sh` holds 256 words.
__device__ __forceinline__ unsigned scan256(unsigned v, unsigned* sh, unsigned* total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const unsigned add = t >= d ? sh[t - d] : 0u;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  const unsigned incl = sh[t];
  *total = sh[255];
  __syncthreads();
  return incl - v;
}

// ---- 1. unstuff ---------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool is_rst(unsigned x) { return x >= 0xD0u && x <= 0xD7u; }

// thread t's four bytes of chunk c: the dropped ones and the markers, as masks
__device__ __forceinline__ void classify(const uint8_t* __restrict__ raw, u64 n, u64 i0, unsigned* drop, unsigned* mark) {
  unsigned d = 0, m = 0;
  unsigned prev = i0 > 0 && i0 - 1 < n ? raw[i0 - 1] : 0u;
  unsigned x = i0 < n ? raw[i0] : 0u;
  for (int j = 0; j < 4; ++j) {
    const u64 i = i0 + j;
    const unsigned next = i + 1 < n ? raw[i + 1] : 0u;
    if (i < n) {
      const bool mk = x == 0xFFu && is_rst(next);
      if (mk) m |= 1u << j;
      if (mk || prev == 0xFFu) d |= 1u << j;
    }
    prev = x;
    x = next;
  }
  *drop = d;
  *mark = m;
}

// the chunk's two counts: integer sums in LDS, so their order cannot show
__global__ __launch_bounds__(256) void jdec_mark_kernel(const uint8_t* __restrict__ raw, u64 n, unsigned* __restrict__ drop, unsigned* __restrict__ mk) {
  __shared__ unsigned tot[2];
  if (threadIdx.x < 2) tot[threadIdx.x] = 0u;
  __syncthreads();
  unsigned d, m;
  classify(raw, n, (u64)blockIdx.x * CHUNK + threadIdx.x * 4, &d, &m);
  if (d) atomicAdd(&tot[0], (unsigned)__popc(d));
  if (m) atomicAdd(&tot[1], (unsigned)__popc(m));
  __syncthreads();
  if (threadIdx.x == 0) {
    drop[blockIdx.x] = tot[0];
    mk[blockIdx.x] = tot[1];
  }
}

// one workgroup: the exclusive prefixes of both counts over the chunks; then the stream's bits, its subsequences, the anchors' number,
// the flags of this call, and the last anchor
__global__ __launch_bounds__(256) void jdec_mark_scan_kernel(const unsigned* __restrict__ drop, const unsigned* __restrict__ mk, unsigned nch, u64 n,
                                                             unsigned expected, unsigned* __restrict__ drop_off, unsigned* __restrict__ mk_off,
                                                             unsigned* __restrict__ meta, unsigned* __restrict__ anchors) {
  __shared__ unsigned sh[256];
  unsigned cd = 0, cm = 0;
  for (unsigned base = 0; base < nch; base += 256) {
    const unsigned i = base + threadIdx.x;
    unsigned td, tm;
    const unsigned ed = scan256(i < nch ? drop[i] : 0u, sh, &td);
    const unsigned em = scan256(i < nch ? mk[i] : 0u, sh, &tm);
    if (i < nch) {
      drop_off[i] = cd + ed;
      mk_off[i] = cm + em;
    }
    cd += td;
    cm += tm;
  }
  if (threadIdx.x == 0) {
    const unsigned bits = (unsigned)(n - cd) * 8u;
    meta[META_BITS] = bits;
    meta[META_NSUB] = (bits + S - 1) / S;
    const unsigned na = min(cm, expected) + 1u;
    meta[META_NA] = na;
    meta[META_FLAGS] = cm == expected ? 0u : FLAG_CORRUPT;
    anchors[na - 1] = bits;
  }
}

__global__ __launch_bounds__(256) void jdec_compact_kernel(const uint8_t* __restrict__ raw, u64 n, const unsigned* __restrict__ drop_off,
                                                           const unsigned* __restrict__ mk_off, unsigned expected, uint8_t* __restrict__ out,
                                                           unsigned* __restrict__ anchors) {
  __shared__ unsigned sh[256];
  const u64 i0 = (u64)blockIdx.x * CHUNK + threadIdx.x * 4;
  unsigned d, m, total;
  classify(raw, n, i0, &d, &m);
  unsigned valid = 0;
  for (int j = 0; j < 4; ++j)
    if (i0 + j < n) valid |= 1u << j;
  const unsigned keep = valid & ~d;
  u64 o = (u64)blockIdx.x * CHUNK - drop_off[blockIdx.x] + scan256((unsigned)__popc(keep), sh, &total);   // kept bytes in front: <= i0 <= n
  unsigned a = mk_off[blockIdx.x] + scan256((unsigned)__popc(m), sh, &total);
  for (int j = 0; j < 4; ++j) {
    if (m >> j & 1) {
      if (a < expected) anchors[a] = (unsigned)o * 8u;
      ++a;
    }
    if (keep >> j & 1) out[o++] = raw[i0 + j];
  }
}

// ---- 2. the decoder -----------------------------------------------------------------------------------------------------------------

// per Huffman table (0, 1: DC; 2, 3: AC): lim[l] = the first 16-bit prefix beyond the codes of length <= l; a code of length l with
// prefix v has the symbol vals[off[l] + (v >> (16 - l))]; lut[v >> 8] = length << 8 | symbol for codes of at most 8 bits, else 0
struct Tables {
  uint32_t lim[4][17];
  int32_t off[4][17];
  uint16_t lut[4][256];
  uint8_t vals[4][256];
  uint8_t dct[8], act[8];   // table of block b of the MCU
};

struct Cfg {
  int bpm, nY, ri;
  unsigned nb;
};

__device__ __forceinline__ Cfg make_cfg(const wct_jdec_info& f) {
  Cfg c;
  c.nY = f.ncomp == 1 ? 1 : f.hs[0] * f.vs[0];
  c.bpm = f.ncomp == 1 ? 1 : c.nY + 2;
  c.ri = f.restart_interval;
  const int mw = 8 * (f.ncomp == 1 ? 1 : f.hs[0]), mh = 8 * (f.ncomp == 1 ? 1 : f.vs[0]);
  c.nb = (unsigned)((f.W + mw - 1) / mw) * (unsigned)((f.H + mh - 1) / mh) * (unsigned)c.bpm;
  return c;
}

__device__ void build_tables(Tables& T, const wct_jdec_info& f, const Cfg& c) {
  const int t = threadIdx.x;
  if (t < 4) {
    const uint8_t* counts = t < 2 ? f.dc_counts[t] : f.ac_counts[t - 2];
    uint32_t code = 0;
    int k = 0;
    T.lim[t][0] = 0;
    T.off[t][0] = 0;
    for (int l = 1; l <= 16; ++l) {
      T.off[t][l] = k - (int)code;
      code += counts[l - 1];
      k += counts[l - 1];
      T.lim[t][l] = code << (16 - l);
      code <<= 1;
    }
  }
  for (int i = t; i < 4 * 256; i += blockDim.x) {
    const int k = i >> 8, j = i & 255;
    T.vals[k][j] = k < 2 ? (j < 16 ? f.dc_vals[k][j] : 0) : f.ac_vals[k - 2][j];
  }
  if (t < 8) {
    const int comp = t < c.nY ? 0 : min(t - c.nY + 1, 2);
    const int cc = f.ncomp == 1 ? 0 : comp;
    T.dct[t] = (uint8_t)(f.td[cc] & 1);
    T.act[t] = (uint8_t)(2 + (f.ta[cc] & 1));
  }
  __syncthreads();
  for (int i = t; i < 4 * 256; i += blockDim.x) {
    const int k = i >> 8;
    const unsigned v = (unsigned)(i & 255) << 8;
    unsigned e = 0;
    for (int l = 1; l <= 8; ++l)
      if (v < T.lim[k][l]) {
        e = (unsigned)l << 8 | T.vals[k][(T.off[k][l] + (int)(v >> (16 - l))) & 255];
        break;
      }
    T.lut[k][i & 255] = (uint16_t)e;
  }
  __syncthreads();
}

struct State {
  unsigned p;
  int b, z;
};
__device__ __forceinline__ u64 pack(State s) { return (u64)s.p | (u64)(unsigned)s.b << 32 | (u64)(unsigned)s.z << 40; }
__device__ __forceinline__ State unpack(u64 x) { return State{(unsigned)x, (int)(x >> 32 & 255), (int)(x >> 40 & 255)}; }

// the smallest k in [0, na) with anchors[k] >= p (strict: > p); anchors[na - 1] is the stream's end, which no p passed here exceeds
__device__ __forceinline__ int anchor_bound(const unsigned* __restrict__ A, int na, unsigned p, bool strict) {
  int lo = 0, hi = na - 1;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi) >> 1;
    const unsigned a = A[mid];
    if (strict ? a > p : a >= p) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// Bytes at or beyond `cap` read as FF.  Between the stream's end and `cap` lies scratch that this call never wrote: a refill may load
// it, but every bit at or beyond the next anchor -- the stream's end is the last one -- is replaced by 1 before it is looked at, so
// what the scratch holds cannot show (the "poison" test fills it with three different bytes).
struct Reader {
  const uint8_t* __restrict__ s;
  unsigned cap, at;   // bytes that may be read; the next byte
  u64 acc;            // the bits from p on, the earliest on top
  int n;
  __device__ __forceinline__ void refill() {
#pragma unroll 1
    for (int i = 0; i < 8 && n <= 56; ++i) {
      const u64 x = at < cap ? s[at] : 0xFFu;
      ++at;
      acc |= x << (56 - n);
      n += 8;
    }
  }
  __device__ __forceinline__ void seek(unsigned p) {
    at = p >> 3;
    acc = 0;
    n = 0;
    refill();
    acc <<= p & 7;
    n -= (int)(p & 7);
  }
  __device__ __forceinline__ void consume(int k) {
    acc <<= k;
    n -= k;
  }
};

// Decode from `s` while p < stop.  *count: blocks completed; *flaws: whether the definition's FLAW was met.  WRITE: the coefficients of
// block blk0 + *count go to coef (stores bounded by c.nb), and a restart anchor away from its block index is a flaw.
template <bool WRITE>
__device__ State decode_sub(const uint8_t* __restrict__ strm, unsigned cap, const unsigned* __restrict__ A, int na, unsigned stop, State s,
                            const Tables& T, const Cfg& c, unsigned* count, bool* flaws, int16_t* __restrict__ coef, unsigned blk0) {
  unsigned p = s.p, cnt = 0;
  int b = s.b, z = s.z;
  bool flaw = false;
  if (b >= c.bpm) b = 0;   // no state this decoder makes; keeps the tables' index in range whatever the scratch held
  int k = anchor_bound(A, na, p, false);
  Reader r{strm, cap, 0, 0, 0};
  r.seek(p);
#pragma unroll 1
  for (int step = 0; step < MAX_STEPS && p < stop; ++step) {
    const unsigned a = A[k];
    if (p >= a) {   // p is an anchor (p > a cannot be)
      if (b | z) flaw = true;
      b = z = 0;
      k = anchor_bound(A, na, p, true);
      if (WRITE && (u64)(blk0 + cnt) != (u64)k * (u64)c.ri * (u64)c.bpm) flaw = true;
      continue;
    }
    const unsigned avail = a - p;
    r.refill();
    if (!(b | z) && avail < 8 && (r.acc >> (64 - avail)) == (1ull << avail) - 1ull) {
      p = a;
      r.seek(p);
      continue;
    }
    unsigned v = (unsigned)(r.acc >> 48);
    if (avail < 16) v |= 0xFFFFu >> avail;
    const int tb = z == 0 ? T.dct[b] : T.act[b];
    int len = 0, sym = 0;
    const unsigned e = T.lut[tb][v >> 8];
    if (e) {
      len = (int)(e >> 8);
      sym = (int)(e & 255);
    } else {
      for (int l = 9; l <= 16; ++l)
        if (v < T.lim[tb][l]) {
          len = l;
          sym = T.vals[tb][(T.off[tb][l] + (int)(v >> (16 - l))) & 255];
          break;
        }
    }
    if (!len) {
      flaw = true;
      p += 1;
      r.consume(1);
      continue;
    }
    const int size = sym & 15, L = len + size;
    if ((unsigned)L > avail) {
      flaw = true;
      p = a;
      b = z = 0;
      r.seek(p);
      continue;
    }
    int val = 0;
    if (size) {
      const unsigned bits = (unsigned)((r.acc << len) >> (64 - size));
      val = bits >> (size - 1) ? (int)bits : (int)bits - (1 << size) + 1;
    }
    r.consume(L);
    p += (unsigned)L;
    bool done = false;
    int at = -1;
    if (z == 0) {
      at = 0;
      z = 1;
    } else if (size == 0) {
      if ((sym >> 4) == 15) {
        z += 16;
        if (z >= 64) {
          if (z > 64) flaw = true;
          done = true;
        }
      } else {
        done = true;
      }
    } else {
      z += sym >> 4;
      if (z > 63) {
        flaw = true;
        done = true;
      } else {
        at = z++;
        done = z == 64;
      }
    }
    if (WRITE && at >= 0 && blk0 + cnt < c.nb) coef[(size_t)(blk0 + cnt) * 64 + at] = (int16_t)val;
    if (done) {
      ++cnt;
      b = b + 1 == c.bpm ? 0 : b + 1;
      z = 0;
    }
  }
  *count = cnt;
  *flaws = flaw;
  return State{p, b, z};
}

// ---- 3. synchronise -----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(SYNC_T) void jdec_sync_kernel(const uint8_t* __restrict__ strm, unsigned cap, const unsigned* __restrict__ meta,
                                                           const unsigned* __restrict__ A, wct_jdec_info f, int launch, int rounds,
                                                           const u64* __restrict__ e_prev, u64* __restrict__ e_cur, u64* __restrict__ e_in,
                                                           unsigned* __restrict__ cnt) {
  __shared__ Tables T;
  __shared__ u64 sh[SYNC_T];
  const Cfg c = make_cfg(f);
  build_tables(T, f, c);
  const unsigned total = meta[META_BITS], nsub = meta[META_NSUB];
  const int na = (int)meta[META_NA];
  const int t = threadIdx.x;
  const unsigned i = blockIdx.x * SYNC_T + t;
  const bool active = i < nsub;
  const unsigned stop = active ? min((i + 1u) * S, total) : 0u;
  u64 e = 0, in = 0;
  unsigned n = 0;
  bool fl;
  if (active) {
    if (launch == 0) {
      in = pack(State{i * S, 0, 0});
      e = pack(decode_sub<false>(strm, cap, A, na, stop, unpack(in), T, c, &n, &fl, nullptr, 0));
    } else {
      e = e_prev[i];
      in = e_in[i];
      n = cnt[i];
    }
  }
  // what the first thread of the workgroup takes as its predecessor: the true start, the previous launch's state, or nothing yet
  const bool head_known = active && t == 0 && (i == 0 || launch > 0);
  const u64 head = head_known ? (i == 0 ? pack(State{0, 0, 0}) : e_prev[i - 1]) : 0;
  sh[t] = e;
  __syncthreads();
#pragma unroll 1
  for (int r = 0; r < rounds; ++r) {
    const bool known = active && (t > 0 || head_known);
    const u64 pred = t > 0 ? sh[t - 1] : head;
    int changed = 0;
    if (known && pred != in) {
      in = pred;
      const u64 ne = pack(decode_sub<false>(strm, cap, A, na, stop, unpack(pred), T, c, &n, &fl, nullptr, 0));
      changed = ne != e;
      e = ne;
    }
    const int any = __syncthreads_or(changed);
    sh[t] = e;
    __syncthreads();
    if (!any) break;
  }
  if (active) {
    e_cur[i] = e;
    e_in[i] = in;
    cnt[i] = n;
  }
}

// ---- 4. count, scan, write ----------------------------------------------------------------------------------------------------------

// off[i] = the blocks in front of subsequence i; a total other than the geometry's is CORRUPT
__global__ __launch_bounds__(256) void jdec_count_scan_kernel(const unsigned* __restrict__ cnt, unsigned nsub_max, unsigned nb, unsigned* __restrict__ off,
                                                              unsigned* __restrict__ meta) {
  __shared__ unsigned sh[256];
  const unsigned nsub = min(meta[META_NSUB], nsub_max);
  unsigned carry = 0;
  for (unsigned base = 0; base < nsub_max; base += 256) {
    if (base >= nsub) break;   // uniform
    const unsigned i = base + threadIdx.x;
    unsigned total;
    const unsigned ex = scan256(i < nsub ? cnt[i] : 0u, sh, &total);
    if (i < nsub) off[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0 && carry != nb) atomicOr(&meta[META_FLAGS], FLAG_CORRUPT);
}

__global__ __launch_bounds__(SYNC_T) void jdec_write_kernel(const uint8_t* __restrict__ strm, unsigned cap, unsigned* __restrict__ meta,
                                                            const unsigned* __restrict__ A, wct_jdec_info f, const u64* __restrict__ e_fin,
                                                            const u64* __restrict__ e_in, const unsigned* __restrict__ cnt,
                                                            const unsigned* __restrict__ off, int16_t* __restrict__ coef) {
  __shared__ Tables T;
  const Cfg c = make_cfg(f);
  build_tables(T, f, c);
  const unsigned total = meta[META_BITS], nsub = meta[META_NSUB];
  const int na = (int)meta[META_NA];
  const unsigned i = blockIdx.x * SYNC_T + threadIdx.x;
  if (i >= nsub) return;
  const u64 start = i == 0 ? pack(State{0, 0, 0}) : e_fin[i - 1];
  unsigned flags = start != e_in[i] ? FLAG_UNSYNC : 0u;
  unsigned n;
  bool fl;
  const State x = decode_sub<true>(strm, cap, A, na, min((i + 1u) * S, total), unpack(start), T, c, &n, &fl, coef, off[i]);
  if (pack(x) != e_fin[i] || n != cnt[i]) flags |= FLAG_UNSYNC;
  if (fl) flags |= FLAG_CORRUPT;
  if (i == nsub - 1 && (x.p != total || (x.b | x.z))) flags |= FLAG_CORRUPT;
  if (flags) atomicOr(&meta[META_FLAGS], flags);
}

// ---- 5. DC --------------------------------------------------------------------------------------------------------------------------

// the differences of MCU m per component
__device__ __forceinline__ void mcu_diffs(const int16_t* __restrict__ coef, unsigned m, int nY, int bpm, int ncomp, unsigned d[3]) {
  d[0] = d[1] = d[2] = 0;
  const int16_t* p = coef + (size_t)m * bpm * 64;
  for (int j = 0; j < nY; ++j) d[0] += (unsigned)(int)p[j * 64];
  if (ncomp == 3) {
    d[1] = (unsigned)(int)p[nY * 64];
    d[2] = (unsigned)(int)p[(nY + 1) * 64];
  }
}

__global__ __launch_bounds__(DC_TILE) void jdec_dc_tile_kernel(const int16_t* __restrict__ coef, unsigned mcus, int nY, int bpm, int ncomp,
                                                               unsigned* __restrict__ x, unsigned* __restrict__ tile) {
  __shared__ unsigned sh[256];
  const unsigned m = blockIdx.x * DC_TILE + threadIdx.x;
  unsigned d[3] = {0, 0, 0};
  if (m < mcus) mcu_diffs(coef, m, nY, bpm, ncomp, d);
  for (int k = 0; k < 3; ++k) {
    unsigned total;
    const unsigned ex = scan256(d[k], sh, &total);
    if (m < mcus) x[(size_t)m * 3 + k] = ex;
    if (threadIdx.x == 0) tile[blockIdx.x * 3 + k] = total;
  }
}

__global__ __launch_bounds__(256) void jdec_dc_scan_kernel(const unsigned* __restrict__ tile, unsigned tiles, unsigned* __restrict__ tile_off) {
  __shared__ unsigned sh[256];
  for (int k = 0; k < 3; ++k) {
    unsigned carry = 0;
    for (unsigned base = 0; base < tiles; base += 256) {
      const unsigned i = base + threadIdx.x;
      unsigned total;
      const unsigned ex = scan256(i < tiles ? tile[i * 3 + k] : 0u, sh, &total);
      if (i < tiles) tile_off[i * 3 + k] = carry + ex;
      carry += total;
    }
  }
}

// the absolute DC values in place, and the status of the call
__global__ __launch_bounds__(DC_TILE) void jdec_dc_apply_kernel(int16_t* __restrict__ coef, unsigned mcus, int nY, int bpm, int ncomp, int ri,
                                                                const unsigned* __restrict__ x, const unsigned* __restrict__ tile_off,
                                                                const unsigned* __restrict__ meta, uint32_t* __restrict__ status) {
  const unsigned m = blockIdx.x * DC_TILE + threadIdx.x;
  if (m == 0) {
    const unsigned fl = meta[META_FLAGS];
    *status = fl & FLAG_UNSYNC ? WCT_JDEC_STATUS_UNSYNC : fl & FLAG_CORRUPT ? WCT_JDEC_STATUS_CORRUPT : WCT_JDEC_STATUS_OK;
  }
  if (m >= mcus) return;
  const unsigned s = ri > 0 ? m / (unsigned)ri * (unsigned)ri : 0u;
  unsigned run[3];
  for (int k = 0; k < 3; ++k) run[k] = tile_off[m / DC_TILE * 3 + k] + x[(size_t)m * 3 + k] - tile_off[s / DC_TILE * 3 + k] - x[(size_t)s * 3 + k];
  int16_t* p = coef + (size_t)m * bpm * 64;
  for (int j = 0; j < nY; ++j) {
    run[0] += (unsigned)(int)p[j * 64];
    p[j * 64] = (int16_t)run[0];
  }
  if (ncomp == 3)
    for (int k = 1; k < 3; ++k) {
      run[k] += (unsigned)(int)p[(nY + k - 1) * 64];
      p[(nY + k - 1) * 64] = (int16_t)run[k];
    }
}

// ---- the pixels ---------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int sar(unsigned x, int n) { return (int)x >> n; }

// jidctint's one-dimensional pass on 8 values, wrapping; descaled by n
__device__ __forceinline__ void idct8(unsigned (&v)[8], int n) {
  const unsigned r = 1u << (n - 1);
  unsigned z2 = v[2], z3 = v[6];
  unsigned z1 = (z2 + z3) * 4433u;
  const unsigned t2 = z1 - z3 * 15137u, t3 = z1 + z2 * 6270u;
  const unsigned t0 = (v[0] + v[4]) << 13, t1 = (v[0] - v[4]) << 13;
  const unsigned t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  unsigned a0 = v[7], a1 = v[5], a2 = v[3], a3 = v[1];
  z1 = a0 + a3;
  z2 = a1 + a2;
  z3 = a0 + a2;
  unsigned z4 = a1 + a3;
  const unsigned z5 = (z3 + z4) * 9633u;
  a0 *= 2446u;
  a1 *= 16819u;
  a2 *= 25172u;
  a3 *= 12299u;
  z1 *= (unsigned)-7373;
  z2 *= (unsigned)-20995;
  z3 = z3 * (unsigned)-16069 + z5;
  z4 = z4 * (unsigned)-3196 + z5;
  a0 += z1 + z3;
  a1 += z2 + z4;
  a2 += z2 + z3;
  a3 += z1 + z4;
  v[0] = (unsigned)sar(t10 + a3 + r, n);
  v[7] = (unsigned)sar(t10 - a3 + r, n);
  v[1] = (unsigned)sar(t11 + a2 + r, n);
  v[6] = (unsigned)sar(t11 - a2 + r, n);
  v[2] = (unsigned)sar(t12 + a1 + r, n);
  v[5] = (unsigned)sar(t12 - a1 + r, n);
  v[3] = (unsigned)sar(t13 + a0 + r, n);
  v[4] = (unsigned)sar(t13 - a0 + r, n);
}

struct Quant {
  uint8_t t[3][64];   // per component, natural order
};

constexpr int IDCT_BLOCKS = 32;   // blocks per workgroup, 8 threads each

// planes: Y [MH mcu_h][MW mcu_w], then Cb and Cr [MH 8][MW 8] each
__global__ __launch_bounds__(IDCT_BLOCKS * 8) void jdec_idct_kernel(const int16_t* __restrict__ coef, unsigned nb, int nY, int bpm, int hs, int MW, int MH,
                                                                     Quant q, uint8_t* __restrict__ planes) {
  __shared__ int work[IDCT_BLOCKS * 72];
  __shared__ uint8_t zinv[64];
  const int tid = threadIdx.x, blk = tid >> 3, lane = tid & 7;
  if (tid < 64) zinv[tid] = d_zigzag_inv[tid];
  __syncthreads();
  const unsigned B = blockIdx.x * IDCT_BLOCKS + blk;
  const bool on = B < nb;
  const unsigned m = on ? B / (unsigned)bpm : 0u;
  const int j = on ? (int)(B % (unsigned)bpm) : 0;
  const int comp = j < nY ? 0 : j - nY + 1;
  unsigned v[8];
  if (on) {
    const int16_t* p = coef + (size_t)B * 64;
    for (int r = 0; r < 8; ++r) v[r] = (unsigned)((int)p[zinv[r * 8 + lane]] * (int)q.t[comp][r * 8 + lane]);   // column `lane`
    idct8(v, 11);
    for (int r = 0; r < 8; ++r) work[blk * 72 + r * 8 + lane] = (int)v[r];
  }
  __syncthreads();
  if (!on) return;
  for (int i = 0; i < 8; ++i) v[i] = (unsigned)work[blk * 72 + lane * 8 + i];   // row `lane`
  idct8(v, 18);
  const int mx = (int)(m % (unsigned)MW), my = (int)(m / (unsigned)MW);
  const int vs = nY / hs;
  size_t base, stride;
  if (comp == 0) {
    stride = (size_t)MW * 8 * hs;
    base = ((size_t)(my * vs + j / hs) * 8 + lane) * stride + (size_t)(mx * hs + j % hs) * 8;
  } else {
    stride = (size_t)MW * 8;
    base = (size_t)MW * 8 * hs * MH * 8 * vs + (size_t)(comp - 1) * stride * MH * 8 + ((size_t)my * 8 + lane) * stride + (size_t)mx * 8;
  }
  for (int i = 0; i < 8; ++i) planes[base + i] = (uint8_t)min(max((int)v[i] + 128, 0), 255);
}

__global__ __launch_bounds__(256) void jdec_colour_kernel(const uint8_t* __restrict__ planes, int H, int W, int ncomp, int hs, int vs, int MW, int MH,
                                                          uint8_t* __restrict__ out) {
  const u64 idx = (u64)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (u64)H * W) return;
  const int y = (int)(idx / (unsigned)W), x = (int)(idx % (unsigned)W);
  const size_t ys = (size_t)MW * 8 * hs;
  const int Y = planes[(size_t)y * ys + x];
  int R = Y, G = Y, B = Y;
  if (ncomp == 3) {
    const size_t cs = (size_t)MW * 8, csize = cs * MH * 8;
    const uint8_t* pc = planes + ys * MH * 8 * vs;
    const int ch = (H + vs - 1) / vs, cw = (W + hs - 1) / hs;
    int c[2];
    for (int k = 0; k < 2; ++k) {
      const uint8_t* pl = pc + k * csize;
      if (hs == 1) {
        c[k] = pl[(size_t)y * cs + x];
      } else {
        const int cx = x >> 1, nx = min(max(x & 1 ? cx + 1 : cx - 1, 0), cw - 1);
        if (vs == 1) {
          const uint8_t* row = pl + (size_t)y * cs;
          c[k] = (3 * row[cx] + row[nx] + (x & 1 ? 2 : 1)) >> 2;
        } else {
          const int cy = y >> 1, ny = min(max(y & 1 ? cy + 1 : cy - 1, 0), ch - 1);
          const uint8_t *r0 = pl + (size_t)cy * cs, *r1 = pl + (size_t)ny * cs;
          const int s0 = 3 * r0[cx] + r1[cx], s1 = 3 * r0[nx] + r1[nx];
          c[k] = (3 * s0 + s1 + (x & 1 ? 7 : 8)) >> 4;
        }
      }
    }
    const int cb = c[0] - 128, cr = c[1] - 128;
    R = min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
    G = min(max(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
    B = min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
  }
  uint8_t* o = out + idx * 3;
  o[0] = (uint8_t)R;
  o[1] = (uint8_t)G;
  o[2] = (uint8_t)B;
}

// [e0 nsub | e1 nsub | e_in nsub] u64, then u32: [meta | drop nch | mk nch | drop_off nch | mk_off nch | anchors expected + 1 | cnt nsub |
// off nsub | x 3 mcus | tile 3 tiles | tile_off 3 tiles]
struct JdecWs {
  u64 *e[2], *e_in;
  unsigned *meta, *drop, *mk, *drop_off, *mk_off, *anchors, *cnt, *off, *x, *tile, *tile_off;
  unsigned nch, nsub, expected, tiles;
  size_t bytes;
};

JdecWs jdec_carve(void* ws, size_t n, const wct_jdec_info& f) {
  const Geometry g = geometry(f);
  JdecWs w{};
  w.nch = (unsigned)((n + CHUNK - 1) / CHUNK);
  if (w.nch == 0) w.nch = 1;
  w.nsub = (unsigned)((n * 8 + S - 1) / S);
  if (w.nsub == 0) w.nsub = 1;
  w.expected = f.restart_interval > 0 ? (unsigned)((g.mcus + f.restart_interval - 1) / f.restart_interval - 1) : 0u;
  w.tiles = (unsigned)((g.mcus + DC_TILE - 1) / DC_TILE);
  w.e[0] = reinterpret_cast<u64*>(ws);
  w.e[1] = w.e[0] + w.nsub;
  w.e_in = w.e[1] + w.nsub;
  w.meta = reinterpret_cast<unsigned*>(w.e_in + w.nsub);
  w.drop = w.meta + META_WORDS;
  w.mk = w.drop + w.nch;
  w.drop_off = w.mk + w.nch;
  w.mk_off = w.drop_off + w.nch;
  w.anchors = w.mk_off + w.nch;
  w.cnt = w.anchors + w.expected + 1;
  w.off = w.cnt + w.nsub;
  w.x = w.off + w.nsub;
  w.tile = w.x + (size_t)g.mcus * 3;
  w.tile_off = w.tile + (size_t)w.tiles * 3;
  w.bytes = (size_t)(reinterpret_cast<char*>(w.tile_off + (size_t)w.tiles * 3) - reinterpret_cast<char*>(ws));
  return w;
}

}  // namespace

// ---- launchers (declared in wct_common.h) ------------------------------------------------------------------------------------------

size_t jdec_stream_bytes(size_t n) { return n + 16; }
size_t jdec_workspace_bytes(size_t n, const wct_jdec_info& f) { return jdec_carve(nullptr, n, f).bytes; }

size_t jdec_planes_bytes(const wct_jdec_info& f) {
  const Geometry g = geometry(f);
  return (size_t)g.MW * g.mcu_w * g.MH * g.mcu_h + (f.ncomp == 3 ? 2 * (size_t)g.MW * 8 * g.MH * 8 : 0);
}

hipError_t launch_jdec_coefficients(const uint8_t* scan, const wct_jdec_info& f, int rounds, int16_t* coef, uint32_t* status, void* ws, void* stream,
                                    hipStream_t s) {
  const size_t n = (size_t)f.scan_length;
  const Geometry g = geometry(f);
  const JdecWs w = jdec_carve(ws, n, f);
  uint8_t* strm = reinterpret_cast<uint8_t*>(stream);
  const unsigned cap = (unsigned)jdec_stream_bytes(n);
  jdec_mark_kernel<<<w.nch, 256, 0, s>>>(scan, n, w.drop, w.mk);
  jdec_mark_scan_kernel<<<1, 256, 0, s>>>(w.drop, w.mk, w.nch, n, w.expected, w.drop_off, w.mk_off, w.meta, w.anchors);
  jdec_compact_kernel<<<w.nch, 256, 0, s>>>(scan, n, w.drop_off, w.mk_off, w.expected, strm, w.anchors);
  const unsigned groups = (w.nsub + SYNC_T - 1) / SYNC_T;
  for (int l = 0; l < WCT_JDEC_LAUNCHES; ++l)
    jdec_sync_kernel<<<groups, SYNC_T, 0, s>>>(strm, cap, w.meta, w.anchors, f, l, rounds, w.e[(l + 1) & 1], w.e[l & 1], w.e_in, w.cnt);
  const u64* e_fin = w.e[(WCT_JDEC_LAUNCHES - 1) & 1];
  jdec_count_scan_kernel<<<1, 256, 0, s>>>(w.cnt, w.nsub, (unsigned)g.blocks, w.off, w.meta);
  if (hipError_t e = hipMemsetAsync(coef, 0, (size_t)g.blocks * 64 * sizeof(int16_t), s)) return e;
  jdec_write_kernel<<<groups, SYNC_T, 0, s>>>(strm, cap, w.meta, w.anchors, f, e_fin, w.e_in, w.cnt, w.off, coef);
  jdec_dc_tile_kernel<<<w.tiles, DC_TILE, 0, s>>>(coef, (unsigned)g.mcus, g.nY, g.bpm, f.ncomp, w.x, w.tile);
  jdec_dc_scan_kernel<<<1, 256, 0, s>>>(w.tile, w.tiles, w.tile_off);
  jdec_dc_apply_kernel<<<w.tiles, DC_TILE, 0, s>>>(coef, (unsigned)g.mcus, g.nY, g.bpm, f.ncomp, f.restart_interval, w.x, w.tile_off, w.meta, status);
  return hipGetLastError();
}

hipError_t launch_jdec_pixels(const int16_t* coef, const wct_jdec_info& f, uint8_t* hwc, void* planes, hipStream_t s) {
  const Geometry g = geometry(f);
  Quant q{};
  for (int c = 0; c < f.ncomp; ++c)
    for (int i = 0; i < 64; ++i) q.t[c][i] = f.qt[f.tq[c]][i];
  const int hs = f.ncomp == 1 ? 1 : f.hs[0], vs = f.ncomp == 1 ? 1 : f.vs[0];
  uint8_t* pl = reinterpret_cast<uint8_t*>(planes);
  jdec_idct_kernel<<<(unsigned)((g.blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS), IDCT_BLOCKS * 8, 0, s>>>(coef, (unsigned)g.blocks, g.nY, g.bpm, hs, g.MW, g.MH, q, pl);
  const size_t px = (size_t)f.H * f.W;
  jdec_colour_kernel<<<(unsigned)((px + 255) / 256), 256, 0, s>>>(pl, f.H, f.W, f.ncomp, hs, vs, g.MW, g.MH, hwc);
  return hipGetLastError();
}
