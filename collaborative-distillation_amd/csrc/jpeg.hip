// The device JPEG encoder's kernels (include/wct_hip_jpeg.h has the definition; api_jpeg.hip the entries).  Integer arithmetic only; what
// crosses threads is an integer sum or an integer OR, so the bytes cannot depend on the launch.  Plain C++ and vector atomics only.
#include "wct_common.h"
#include "jpeg_tables.h"
#include "../../include/wct_hip_jpeg.h"

using namespace wct_jpeg;

namespace {

__constant__ HuffCodes d_huff = make_codes();
__constant__ uint8_t d_zigzag_inv[64] = {   // natural index -> zig-zag position
    0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

typedef unsigned long long u64;

constexpr int SEG = WCT_JPEG_SEG_MCUS;           // MCUs per workgroup of the blocks kernel
constexpr int SEG_W = SEG * 16;                  // its pixel columns
constexpr int BLK_THREADS = SEG * 6 * 8;         // 8 threads per block
constexpr int WORK_STRIDE = 72;                  // words per block between the two DCT passes: 64 + 8, so that four blocks' columns fall on 32 banks
constexpr int TILE = WCT_JPEG_SCAN_TILE;
constexpr int SPAN = WCT_JPEG_PACK_SPAN;
constexpr int SPAN_WORDS = SPAN * WCT_JPEG_BLOCK_MAX_BITS / 32 + 2;
constexpr int CHUNK = WCT_JPEG_STUFF_CHUNK;

// jfdctint's one-dimensional pass on 8 values; first: the row pass (outputs scaled up by PASS1_BITS), else the column pass
__device__ __forceinline__ void fdct8(int (&v)[8], bool first) {
  const int t0 = v[0] + v[7], t7 = v[0] - v[7], t1 = v[1] + v[6], t6 = v[1] - v[6];
  const int t2 = v[2] + v[5], t5 = v[2] - v[5], t3 = v[3] + v[4], t4 = v[3] - v[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  const int n = first ? 11 : 15, r = 1 << (n - 1);
  if (first) {
    v[0] = (t10 + t11) << 2;
    v[4] = (t10 - t11) << 2;
  } else {
    v[0] = (t10 + t11 + 2) >> 2;
    v[4] = (t10 - t11 + 2) >> 2;
  }
  int z1 = (t12 + t13) * 4433;
  v[2] = (z1 + t13 * 6270 + r) >> n;
  v[6] = (z1 - t12 * 15137 + r) >> n;
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  v[7] = (a4 + z1 + z3 + r) >> n;
  v[5] = (a5 + z2 + z4 + r) >> n;
  v[3] = (a6 + z2 + z3 + r) >> n;
  v[1] = (a7 + z1 + z4 + r) >> n;
}

// One workgroup: SEG MCUs of MCU row blockIdx.y.  The 16 pixel rows of the segment are read as whole row pieces into LDS (rows and
// columns clamped to the image), converted, and every block's DCT is done by 8 threads: a row each, then a column each.
__global__ __launch_bounds__(BLK_THREADS) void jpeg_blocks_kernel(const uint8_t* __restrict__ img, int H, int W, int MW, QuantTables qt,
                                                                   int16_t* __restrict__ coef) {
  __shared__ uint8_t rgb[16][SEG_W * 3];
  __shared__ int16_t ys[16][SEG_W];
  __shared__ int16_t cs[2][8][SEG_W / 2];
  __shared__ int work[SEG * 6 * WORK_STRIDE];
  __shared__ __attribute__((aligned(4))) int16_t zz[SEG * 6 * 64];
  __shared__ uint16_t q[2][64];
  __shared__ uint8_t zinv[64];
  const int tid = threadIdx.x, my = blockIdx.y, mx0 = blockIdx.x * SEG;
  const int nm = min(SEG, MW - mx0);
  if (tid < 128) q[tid >> 6][tid & 63] = qt.t[tid >> 6][tid & 63];
  if (tid < 64) zinv[tid] = d_zigzag_inv[tid];
  // stage: thread t takes byte t of every row piece (SEG_W * 3 == BLK_THREADS bytes)
  {
    const int col = min(mx0 * 16 + tid / 3, W - 1), ch = tid % 3;
    for (int r = 0; r < 16; ++r) {
      const int row = min(my * 16 + r, H - 1);
      rgb[r][tid] = img[((size_t)row * W + col) * 3 + ch];
    }
  }
  __syncthreads();
  for (int i = tid; i < 16 * SEG_W; i += BLK_THREADS) {
    const int r = i / SEG_W, c = i % SEG_W;
    const int R = rgb[r][c * 3], G = rgb[r][c * 3 + 1], B = rgb[r][c * 3 + 2];
    ys[r][c] = (int16_t)(((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128);
  }
  const int chh = (H + 1) / 2;
  for (int i = tid; i < 2 * 8 * (SEG_W / 2); i += BLK_THREADS) {
    const int comp = i / (8 * (SEG_W / 2)), y = i / (SEG_W / 2) % 8, x = i % (SEG_W / 2);
    const int cy = min(my * 8 + y, chh - 1);                  // a chroma row past the image takes the last DOWNSAMPLED row
    const int ra = 2 * cy - my * 16, rb = min(2 * cy + 1, H - 1) - my * 16;
    int s = 0;
    for (int k = 0; k < 4; ++k) {
      const int r = k < 2 ? ra : rb, c = 2 * x + (k & 1);
      const int R = rgb[r][c * 3], G = rgb[r][c * 3 + 1], B = rgb[r][c * 3 + 2];
      s += comp == 0 ? (-11059 * R - 21709 * G + 32768 * B + 8388608 + 32767) >> 16 : (32768 * R - 27439 * G - 5329 * B + 8388608 + 32767) >> 16;
    }
    cs[comp][y][x] = (int16_t)(((s + 1 + (x & 1)) >> 2) - 128);
  }
  __syncthreads();
  const int blk = tid >> 3, lane = tid & 7, m = blk / 6, k = blk % 6;
  int v[8];
  if (k < 4) {
    const int16_t* p = &ys[(k >> 1) * 8 + lane][m * 16 + (k & 1) * 8];
    for (int i = 0; i < 8; ++i) v[i] = p[i];
  } else {
    const int16_t* p = &cs[k - 4][lane][m * 8];
    for (int i = 0; i < 8; ++i) v[i] = p[i];
  }
  fdct8(v, true);
  for (int i = 0; i < 8; ++i) work[blk * WORK_STRIDE + lane * 8 + i] = v[i];
  __syncthreads();
  for (int i = 0; i < 8; ++i) v[i] = work[blk * WORK_STRIDE + i * 8 + lane];
  fdct8(v, false);
  // a Y block outside the image's ceil(W / 8) x ceil(H / 8) blocks is a dummy
  const bool dummy = k < 4 && ((mx0 + m) * 2 + (k & 1) >= (W + 7) / 8 || my * 2 + (k >> 1) >= (H + 7) / 8);
  for (int i = 0; i < 8; ++i) {
    const int n = i * 8 + lane;
    const unsigned t = q[k >= 4][n];
    const unsigned a = (unsigned)abs(v[i]);
    const int c = (int)((a + 4 * t) / (8 * t));
    zz[blk * 64 + zinv[n]] = dummy ? (int16_t)0 : (int16_t)(v[i] < 0 ? -c : c);
  }
  __syncthreads();
  if (tid < SEG) {   // a dummy's DC: the quantised DC of the preceding Y block of its MCU, in order
    const int gx = (mx0 + tid) * 2, gy = my * 2;
    for (int b = 1; b < 4; ++b)
      if (gx + (b & 1) >= (W + 7) / 8 || gy + (b >> 1) >= (H + 7) / 8) zz[(tid * 6 + b) * 64] = zz[(tid * 6 + b - 1) * 64];
  }
  __syncthreads();
  uint32_t* dst = reinterpret_cast<uint32_t*>(coef + ((size_t)my * MW + mx0) * 384);
  const uint32_t* src = reinterpret_cast<const uint32_t*>(zz);
  for (int i = tid; i < nm * 192; i += BLK_THREADS) dst[i] = src[i];
}

__device__ __forceinline__ int bit_length(unsigned a) { return 32 - __clz((int)a); }

// where the DC predictor of block b lives: the preceding block of the same component in scan order, -1 for none
__device__ __forceinline__ long pred_block(long b) {
  const long m = b / 6;
  const int k = (int)(b % 6);
  if (k >= 1 && k <= 3) return b - 1;
  if (m == 0) return -1;
  return k == 0 ? (m - 1) * 6 + 3 : b - 6;
}

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

// A thread walks one block.  EMIT(code, length) receives every code with its value bits appended, in order.
template <typename EMIT>
__device__ __forceinline__ void walk_block(const int16_t* __restrict__ coef, long b, const uint32_t* huff /* LDS: [2][HUFF_WORDS] */, EMIT&& emit) {
  const uint4* p = reinterpret_cast<const uint4*>(coef + b * 64);
  uint4 c[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) c[i] = p[i];
  const long pb = pred_block(b);
  const int pred = pb < 0 ? 0 : coef[pb * 64];
  const uint32_t* h = huff + ((b % 6) >= 4 ? HUFF_WORDS : 0);
  int run = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t w[4] = {c[i].x, c[i].y, c[i].z, c[i].w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int v = (int)(int16_t)(w[j >> 1] >> ((j & 1) * 16));
      if (i == 0 && j == 0) {
        v -= pred;
        const int n = min(bit_length((unsigned)abs(v)), 11);   // 11 and 10: all that baseline JPEG has codes for; keeps any input within WCT_JPEG_BLOCK_MAX_BITS
        const uint32_t e = h[n];
        const uint32_t bits = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u);
        emit(((e & 0xFFFFu) << n) | bits, (int)(e >> 16) + n);
      } else if (v == 0) {
        ++run;
      } else {
        for (; run > 15; run -= 16) emit(h[16 + 0xF0] & 0xFFFFu, (int)(h[16 + 0xF0] >> 16));
        const int n = min(bit_length((unsigned)abs(v)), 10);
        const uint32_t e = h[16 + (run << 4 | n)];
        const uint32_t bits = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u);
        emit(((e & 0xFFFFu) << n) | bits, (int)(e >> 16) + n);
        run = 0;
      }
    }
  }
  if (run > 0) emit(h[16] & 0xFFFFu, (int)(h[16] >> 16));
}

__device__ __forceinline__ void load_huff(uint32_t* huff, int nthreads) {
  for (int i = threadIdx.x; i < 2 * HUFF_WORDS; i += nthreads) huff[i] = d_huff.w[i / HUFF_WORDS][i % HUFF_WORDS];
  __syncthreads();
}

// pre[b] = the bits of the blocks of b's tile in front of b; tile_bits[tile] = the tile's bits
__global__ __launch_bounds__(TILE) void jpeg_count_kernel(const int16_t* __restrict__ coef, long nb, unsigned* __restrict__ pre,
                                                          unsigned* __restrict__ tile_bits) {
  __shared__ uint32_t huff[2 * HUFF_WORDS];
  __shared__ unsigned sh[TILE];
  load_huff(huff, TILE);
  const long b = (long)blockIdx.x * TILE + threadIdx.x;
  unsigned bits = 0;
  if (b < nb) walk_block(coef, b, huff, [&](uint32_t, int len) { bits += (unsigned)len; });
  unsigned total;
  const unsigned ex = scan256(bits, sh, &total);
  if (b < nb) pre[b] = ex;
  if (threadIdx.x == 0) tile_bits[blockIdx.x] = total;
}

// off[i] = the sum of v[0 .. i), i = 0 .. n; one workgroup, WCT_JPEG_SCAN_CHUNK values per step.  n is n_host, or *n_dev when that is
// not null.  bits_to_bytes (the scan of the tiles' bits): meta[0] = the stream's bits, meta[1] = its bytes, padded, meta[2] = its
// stuffing chunks.
__global__ __launch_bounds__(WCT_JPEG_SCAN_CHUNK) void jpeg_scan_kernel(const unsigned* __restrict__ v, u64 n_host, const u64* __restrict__ n_dev,
                                                                         u64* __restrict__ off, u64* __restrict__ meta) {
  __shared__ unsigned sh[WCT_JPEG_SCAN_CHUNK];
  const u64 n = n_dev ? *n_dev : n_host;
  u64 carry = 0;
  for (u64 base = 0; base < n; base += WCT_JPEG_SCAN_CHUNK) {
    const u64 i = base + threadIdx.x;
    const unsigned x = i < n ? v[i] : 0u;
    unsigned total;
    const unsigned ex = scan256(x, sh, &total);
    if (i < n) off[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    off[n] = carry;
    if (meta) {
      meta[0] = carry;
      meta[1] = (carry + 7) / 8;
      meta[2] = ((carry + 7) / 8 + CHUNK - 1) / CHUNK;
    }
  }
}

// the words of the stream that the pack ORs into, and one more
__global__ __launch_bounds__(256) void jpeg_zero_kernel(uint32_t* __restrict__ stream, const u64* __restrict__ meta) {
  const u64 words = (meta[0] + 31) / 32 + 1;
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i < words) stream[i] = 0u;
}

// One workgroup (a wave): the bits of SPAN blocks, assembled in LDS in words whose bit 31 is the earliest bit, then stored byte-swapped.
// Only the first and the last word of the span can be shared with a neighbour: those two are ORed into the zeroed stream.
__global__ __launch_bounds__(SPAN) void jpeg_pack_kernel(const int16_t* __restrict__ coef, long nb, const unsigned* __restrict__ pre,
                                                         const u64* __restrict__ tile_off, uint32_t* __restrict__ stream) {
  __shared__ uint32_t huff[2 * HUFF_WORDS];
  __shared__ uint32_t words[SPAN_WORDS];
  load_huff(huff, SPAN);
  const long b0 = (long)blockIdx.x * SPAN, b = b0 + threadIdx.x, b1 = min(b0 + SPAN, nb);
  const u64 start = tile_off[b0 / TILE] + pre[b0];
  const u64 end = b1 < nb ? tile_off[b1 / TILE] + pre[b1] : tile_off[(nb + TILE - 1) / TILE];
  const u64 w0 = start >> 5;
  const int nw = (int)(((end + 31) >> 5) - w0);   // <= SPAN_WORDS: a block has at most WCT_JPEG_BLOCK_MAX_BITS bits
  for (int i = threadIdx.x; i < nw; i += SPAN) words[i] = 0u;
  __syncthreads();
  if (b < nb) {
    const u64 at = tile_off[b / TILE] + pre[b] - (w0 << 5);
    int wi = (int)(at >> 5), nacc = (int)(at & 31);
    u64 acc = 0;
    walk_block(coef, b, huff, [&](uint32_t code, int len) {
      acc = acc << len | code;
      nacc += len;
      if (nacc >= 32) {
        nacc -= 32;
        atomicOr(&words[wi++], (uint32_t)(acc >> nacc));
        acc &= (1ull << nacc) - 1ull;
      }
    });
    if (nacc > 0) atomicOr(&words[wi], (uint32_t)(acc << (32 - nacc)));
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nw; i += SPAN) {
    const uint32_t x = __builtin_bswap32(words[i]);
    if (i == 0 || i == nw - 1) atomicOr(&stream[w0 + i], x);
    else stream[w0 + i] = x;
  }
}

// byte i of the padded stream (i < bytes): the last byte's free bits are ones
__device__ __forceinline__ unsigned stream_byte(const uint8_t* __restrict__ stream, u64 i, u64 bits, u64 bytes) {
  unsigned x = stream[i];
  if (i == bytes - 1 && (bits & 7)) x |= 0xFFu >> (bits & 7);
  return x;
}

// the FF bytes among thread t's four bytes of chunk c, as a mask
__device__ __forceinline__ unsigned ff_mask(const uint8_t* __restrict__ stream, u64 i0, u64 bits, u64 bytes) {
  unsigned m = 0;
  for (int j = 0; j < 4; ++j)
    if (i0 + j < bytes && stream_byte(stream, i0 + j, bits, bytes) == 0xFFu) m |= 1u << j;
  return m;
}

__global__ __launch_bounds__(256) void jpeg_ffcount_kernel(const uint8_t* __restrict__ stream, const u64* __restrict__ meta, unsigned* __restrict__ ff) {
  __shared__ unsigned sh[256];
  if (blockIdx.x >= meta[2]) return;
  const u64 i0 = (u64)blockIdx.x * CHUNK + threadIdx.x * 4;
  unsigned total;
  (void)scan256((unsigned)__popc(ff_mask(stream, i0, meta[0], meta[1])), sh, &total);
  if (threadIdx.x == 0) ff[blockIdx.x] = total;
}

// out[head + i + (FF bytes in front of i)] = byte i, 00 behind every FF; FF D9 and the length by the first thread.  Nothing at or
// beyond `capacity` is written.
__global__ __launch_bounds__(256) void jpeg_scatter_kernel(const uint8_t* __restrict__ stream, const u64* __restrict__ meta, const u64* __restrict__ ff_off,
                                                           uint8_t* __restrict__ out, u64 head, u64 capacity, u64* __restrict__ len) {
  __shared__ unsigned sh[256];
  const u64 chunks = meta[2];
  if (blockIdx.x >= chunks) return;
  const u64 bits = meta[0], bytes = meta[1];
  const u64 i0 = (u64)blockIdx.x * CHUNK + threadIdx.x * 4;
  const unsigned m = ff_mask(stream, i0, bits, bytes);
  unsigned total;
  u64 o = head + i0 + ff_off[blockIdx.x] + scan256((unsigned)__popc(m), sh, &total);
  for (int j = 0; j < 4; ++j)
    if (i0 + j < bytes) {
      if (o < capacity) out[o] = (uint8_t)stream_byte(stream, i0 + j, bits, bytes);
      ++o;
      if (m >> j & 1) {
        if (o < capacity) out[o] = 0;
        ++o;
      }
    }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const u64 e = head + bytes + ff_off[chunks];
    if (e < capacity) out[e] = 0xFF;
    if (e + 1 < capacity) out[e + 1] = 0xD9;
    *len = e + 2 <= capacity ? e + 2 : WCT_JPEG_OVERFLOW;
  }
}

__global__ __launch_bounds__(256) void jpeg_head_kernel(Header h, uint8_t* __restrict__ out, u64 capacity) {
  for (int i = threadIdx.x; i < WCT_JPEG_HEADER_BYTES; i += 256)
    if ((u64)i < capacity) out[i] = h.b[i];
}

}  // namespace

// ---- launchers (declared in wct_common.h) ------------------------------------------------------------------------------------------

long jpeg_num_blocks(int H, int W) { return (long)((H + 15) / 16) * ((W + 15) / 16) * 6; }
size_t jpeg_stream_bytes(long nb) { return (size_t)nb * (WCT_JPEG_BLOCK_MAX_BITS / 8) + 16; }

// [meta 4 | tile_off tiles + 1 | ff_off chunks + 1] u64, then [pre nb | tile_bits tiles | ff chunks] u32
namespace {
struct JpegWs {
  u64 *meta, *tile_off, *ff_off;
  unsigned *pre, *tile_bits, *ff;
  size_t tiles, chunks, bytes;
};
JpegWs jpeg_carve(void* ws, long nb) {
  JpegWs w{};
  w.tiles = (size_t)(nb + TILE - 1) / TILE;
  w.chunks = (jpeg_stream_bytes(nb) + CHUNK - 1) / CHUNK;
  w.meta = reinterpret_cast<u64*>(ws);
  w.tile_off = w.meta + 4;
  w.ff_off = w.tile_off + w.tiles + 1;
  w.pre = reinterpret_cast<unsigned*>(w.ff_off + w.chunks + 1);
  w.tile_bits = w.pre + nb;
  w.ff = w.tile_bits + w.tiles;
  w.bytes = (size_t)(reinterpret_cast<char*>(w.ff + w.chunks) - reinterpret_cast<char*>(ws));
  return w;
}
}  // namespace

size_t jpeg_workspace_bytes(long nb) { return jpeg_carve(nullptr, nb).bytes; }

hipError_t launch_jpeg_blocks(const uint8_t* hwc, int H, int W, int quality, int16_t* coef, hipStream_t s) {
  const int MH = (H + 15) / 16, MW = (W + 15) / 16;
  jpeg_blocks_kernel<<<dim3((MW + SEG - 1) / SEG, MH), BLK_THREADS, 0, s>>>(hwc, H, W, MW, make_quant(quality), coef);
  return hipGetLastError();
}

hipError_t launch_jpeg_pack(const int16_t* coef, int H, int W, const uint8_t* header, uint8_t* out, uint64_t capacity, uint64_t* len, void* ws,
                            void* stream, hipStream_t s) {
  const long nb = jpeg_num_blocks(H, W);
  const JpegWs w = jpeg_carve(ws, nb);
  u64* dlen = reinterpret_cast<u64*>(len);
  uint64_t head = 0;
  if (header) {
    Header h{};
    for (int i = 0; i < WCT_JPEG_HEADER_BYTES; ++i) h.b[i] = header[i];
    jpeg_head_kernel<<<1, 256, 0, s>>>(h, out, capacity);
    head = WCT_JPEG_HEADER_BYTES;
  }
  jpeg_count_kernel<<<(unsigned)w.tiles, TILE, 0, s>>>(coef, nb, w.pre, w.tile_bits);
  jpeg_scan_kernel<<<1, WCT_JPEG_SCAN_CHUNK, 0, s>>>(w.tile_bits, w.tiles, nullptr, w.tile_off, w.meta);
  const size_t words = jpeg_stream_bytes(nb) / 4;
  jpeg_zero_kernel<<<(unsigned)((words + 255) / 256), 256, 0, s>>>(reinterpret_cast<uint32_t*>(stream), w.meta);
  jpeg_pack_kernel<<<(unsigned)((nb + SPAN - 1) / SPAN), SPAN, 0, s>>>(coef, nb, w.pre, w.tile_off, reinterpret_cast<uint32_t*>(stream));
  jpeg_ffcount_kernel<<<(unsigned)w.chunks, 256, 0, s>>>(reinterpret_cast<const uint8_t*>(stream), w.meta, w.ff);
  jpeg_scan_kernel<<<1, WCT_JPEG_SCAN_CHUNK, 0, s>>>(w.ff, 0, w.meta + 2, w.ff_off, nullptr);
  jpeg_scatter_kernel<<<(unsigned)w.chunks, 256, 0, s>>>(reinterpret_cast<const uint8_t*>(stream), w.meta, w.ff_off, out, head, capacity, dlen);
  return hipGetLastError();
}
